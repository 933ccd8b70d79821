"""The Wilson-flow stage kernel (qmg_u1_flow_stage, csrc/qmg_flow.hip) and the Wilson-loop call (qmg_u1_wilson_loops): milliseconds per call at
2048^2 and 4096^2 against their byte models, this part's copy ceiling and the same stage composed from the entries that existed before it.
Byte model of a fused stage: 128 B per site -- the phases read and written (32), the accumulator read and written (32; stage 1 only writes it),
two complex<double> links read (32) and two written (32); the neighbours' links are expected from cache.
Composed stage (stage 2 of the scheme): qmg_hmc_momentum_update with QMG_HMC_GAUGE_ONLY, beta = 1, dt = eps on a zeroed field (Z = -eps dS/dtheta; 64 B
per site, the zeroing not timed), qmg_caxpby on the accumulator viewed as complex (A = 8/9 Z - 17/36 A; 48 B per site), qmg_hmc_link_update
(theta += A, U = exp(i theta); 80 B per site): 192 B per site in three launches, model ratio 128 / 192 = 0.67.
Wilson loops: time per (R, T) pair of an r_max x t_max = 4 x 4 table against the model of four 16-byte reads per site and pair (64 B per site);
the call also extends one line product per pair (48 B per site), which the model does not count.
Copy ceiling: 6.2 TB/s (profiles/r01_membw_ceiling.txt, read + write, 262 144 blocks); a device-to-device copy of the link field through
qmg_copy_vector, the ceiling of the day, is timed alongside.  HIP events around single calls, 3 warm-up rounds, medians of 10.
    python tools/u1_flow_bench.py   (GPU box; everything is allocated before the first timed region)"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
qmg = importlib.import_module("quantum-mg_amd")
WARMUP, REPEAT = 3, 10
COPY_CEILING_GBS = 6205.4
EPS = 0.01
R_MAX = T_MAX = 4


def main():
    qmg.init(0)
    timer = qmg.Timer()
    for L in (2048, 4096):
        V = L * L
        gauge, other, Z = qmg.DeviceArray(2 * V), qmg.DeviceArray(2 * V), qmg.DeviceArray(2 * V)
        theta, acc, z = qmg.DeviceArray(2 * V, np.float64), qmg.DeviceArray.zeros(2 * V, np.float64), qmg.DeviceArray.zeros(2 * V, np.float64)
        qmg.u1_gauss_gauge(gauge, L, L, 6.0, 1337)
        qmg.u1_gauge_to_phase(theta, gauge, 2 * V)
        qmg.copy_vector(other, gauge, 2 * V)
        qmg.u1_wilson_loops(gauge, L, L, 1, 1)                             # the scratch of the loops is allocated here, not in a timed call

        def composed():
            qmg.hmc_momentum_update(z, gauge, None, None, L, L, 1.0, EPS, qmg.HMC_GAUGE_ONLY)
            qmg.caxpby(8.0 / 9.0, z, -17.0 / 36.0, acc, V)             # 2 V doubles = V complex numbers
            qmg.hmc_link_update(theta, gauge, acc, 2 * V, 1.0)

        runs = {
            "flow stage 1, fused": (112.0, 1, lambda: qmg.u1_flow_stage(theta, acc, other, gauge, L, L, EPS, 1)),
            "flow stage 2, fused": (128.0, 1, lambda: qmg.u1_flow_stage(theta, acc, other, gauge, L, L, EPS, 2)),
            "flow stage 3, fused": (128.0, 1, lambda: qmg.u1_flow_stage(theta, acc, other, gauge, L, L, EPS, 3)),
            "flow stage 2, composed": (192.0, 1, composed),
            "wilson loops 4 x 4, per pair": (64.0, R_MAX * T_MAX, lambda: qmg.u1_wilson_loops(gauge, L, L, R_MAX, T_MAX)),
            "copy of the link field": (64.0, 1, lambda: qmg.copy_vector(Z, gauge, 2 * V)),
        }
        t = {k: [] for k in runs}
        for rep in range(WARMUP + REPEAT):
            for k, (_, per, call) in runs.items():
                if k == "flow stage 2, composed":
                    qmg.zero_vector(z, V)                                  # Z starts from zero; not timed
                timer.start(); call(); ms = timer.stop_ms()
                if rep >= WARMUP:
                    t[k].append(ms / per)
        med = {k: float(np.median(v)) for k, v in t.items()}
        for k, (bytes_per_site, _, _) in runs.items():
            mb = bytes_per_site * V / 1e6                                  # MB per call; MB / ms = GB/s
            print("%d^2 %-29s %.4f ms (min %.4f max %.4f) = %.0f GB/s on the %.0f B/site model, %.1f %% of the %.0f GB/s copy ceiling" % (
                L, k + ":", med[k], min(t[k]), max(t[k]), mb / med[k], bytes_per_site, 100.0 * mb / med[k] / COPY_CEILING_GBS, COPY_CEILING_GBS), flush=True)
        ratio = med["flow stage 2, fused"] / med["flow stage 2, composed"]
        print("%d^2 fused / composed stage 2: %.3f (model 128 / 192 = 0.667) -- %s" % (L, ratio, "fused is faster" if ratio < 1.0 else "FUSED IS NOT FASTER"), flush=True)
        for d in (gauge, other, Z, theta, acc, z):
            d.free()


if __name__ == "__main__":
    main()
