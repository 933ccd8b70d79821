"""The fused step of the pure-gauge inner loop of a two-scale integrator (qmg_hmc_gauge_step, csrc/qmg_hmc.hip) against the two launches it
replaces, at 64^2 (a lattice Schwinger-model HMC actually runs: launch-bound), 2048^2 and 4096^2 (bandwidth-bound):
  (i)  fused:    qmg_hmc_gauge_step, ping-ponging between two link fields -- 128 B per site: pi read and written (32), theta read and written (32),
                 two complex<double> links read (32) and two written (32); the neighbours' links are expected from cache;
  (ii) composed: qmg_hmc_momentum_update with QMG_HMC_GAUGE_ONLY (64 B per site) followed by qmg_hmc_link_update (80 B per site), in place.
Model ratio 128 / 144 = 0.89 where bandwidth binds; where launches bind the fused step saves one of two.  The two legs give the same bits
(tests/test_gpu_md_schemes.py), each runs on its own copy of the same fields.
HIP events around STEPS steps back to back (so that a window is not a single launch), the legs alternating within each of ROUNDS rounds after
WARMUP warm-up rounds; reported per step: median [min .. max] over the rounds.  Copy ceiling: 6.2 TB/s (profiles/r01_membw_ceiling.txt).
    python tools/hmc_gauge_step_bench.py   (GPU box; everything is allocated before the first timed region)"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
qmg = importlib.import_module("quantum-mg_amd")
WARMUP, ROUNDS = 3, 7
COPY_CEILING_GBS = 6205.4
BETA, DT = 6.0, 1e-3
STEPS = {64: 400, 2048: 40, 4096: 20}      # an even number each: the fused leg ends in the field it started from


def main():
    qmg.init(0)
    timer = qmg.Timer()
    for L in (64, 2048, 4096):
        V, steps = L * L, STEPS[L]
        fields = []
        for _ in range(2):                                                 # one set per leg, the same numbers in both
            gauge, other = qmg.DeviceArray(2 * V), qmg.DeviceArray(2 * V)
            theta, pi = qmg.DeviceArray(2 * V, np.float64), qmg.DeviceArray(2 * V, np.float64)
            qmg.u1_gauss_gauge(gauge, L, L, BETA, 1337)
            qmg.u1_gauge_to_phase(theta, gauge, 2 * V)
            qmg.copy_vector(other, gauge, 2 * V)
            qmg.hmc_momentum_refresh(pi, 2 * V, 7, 0)
            fields.append((theta, pi, gauge, other))

        def fused():
            theta, pi, gauge, other = fields[0]
            for _ in range(steps // 2):
                qmg.hmc_gauge_step(theta, other, gauge, pi, L, L, BETA, DT, DT)
                qmg.hmc_gauge_step(theta, gauge, other, pi, L, L, BETA, DT, DT)

        def composed():
            theta, pi, gauge, _ = fields[1]
            for _ in range(steps):
                qmg.hmc_momentum_update(pi, gauge, None, None, L, L, BETA, DT, qmg.HMC_GAUGE_ONLY)
                qmg.hmc_link_update(theta, gauge, pi, 2 * V, DT)

        runs = {"fused step": (128.0, fused), "kick + link update": (144.0, composed)}
        t = {k: [] for k in runs}
        for rep in range(WARMUP + ROUNDS):
            for k, (_, call) in runs.items():
                timer.start(); call(); ms = timer.stop_ms()
                if rep >= WARMUP:
                    t[k].append(ms / steps)
        med = {k: float(np.median(v)) for k, v in t.items()}
        for k, (bytes_per_site, _) in runs.items():
            mb = bytes_per_site * V / 1e6                                  # MB per step; MB / ms = GB/s
            print("%d^2 %-19s %.5f ms per step [%.5f .. %.5f] = %.0f GB/s on the %.0f B/site model, %.1f %% of the %.0f GB/s copy ceiling" % (
                L, k + ":", med[k], min(t[k]), max(t[k]), mb / med[k], bytes_per_site, 100.0 * mb / med[k] / COPY_CEILING_GBS, COPY_CEILING_GBS), flush=True)
        ratio = med["fused step"] / med["kick + link update"]
        print("%d^2 fused / composed: %.3f (model 128 / 144 = 0.889) -- %s" % (L, ratio, "fused is not slower" if ratio <= 1.0 else "FUSED IS SLOWER"), flush=True)
        same = all(np.array_equal(a.to_host().view(np.uint64), b.to_host().view(np.uint64)) for a, b in zip(fields[0][:3], fields[1][:3]))
        print("%d^2 both legs after %d steps each: %s" % (L, (WARMUP + ROUNDS) * steps, "the same bits" if same else "DIFFERENT BITS"), flush=True)
        for f in fields:
            for d in f:
                d.free()


if __name__ == "__main__":
    main()
