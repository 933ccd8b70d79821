"""The staggered pole kick (qmg_hmc_momentum_update_staggered, csrc/qmg_hmc.hip) at 2048^2 and 4096^2: pure gauge, n = 1 (two tastes) and
n = 8 (rooted RHMC).  Fused: pi -= dt (Fg + sum_j w_j Fs(W_j)) in one pass.  Composed: n single-pole calls, the first with the gauge force,
the rest with beta = 0, each of which reads and writes the momenta and reads the links again.
Byte model: fused 64 + 16 n B per site (momenta read and written 32, two complex<double> links 32, one complex<double> W_j per pole);
composed 80 n.  The model ratio is (64 + 16 n) / (80 n): 1.0 at n = 1, 0.30 at n = 8.  A qmg_copy_vector of the momenta-sized field (32 B per
site moved) of the same run is the yardstick for the bandwidth.
HIP events around whole kicks, 3 warm-up rounds, medians of 10, the variants alternating.
    python tools/stag_force_bench.py   (GPU box; everything is allocated before the first timed region)"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
qmg = importlib.import_module("quantum-mg_amd")
WARMUP, REPEAT = 3, 10


def main():
    qmg.init(0)
    timer = qmg.Timer()
    for L in (2048, 4096):
        V = L * L
        gauge = qmg.DeviceArray(2 * V)
        pi = qmg.DeviceArray(2 * V, np.float64)
        src, dst = qmg.DeviceArray(V), qmg.DeviceArray(V)
        qmg.u1_gauss_gauge(gauge, L, L, 6.0, 1337)
        qmg.hmc_momentum_refresh(pi, 2 * V, 3, 0)
        qmg.gaussian(src, V, 5)
        W = []
        for j in range(8):
            W.append(qmg.DeviceArray(V))
            qmg.gaussian(W[-1], V, 10 + j)
        dt = 1e-3
        for n in (0, 1, 8):
            w = [0.1 + 0.05 * j for j in range(n)]

            def fused():
                qmg.hmc_momentum_update_staggered(pi, gauge, W[:n], w, L, L, 6.0, dt, 0)

            def composed():
                for j in range(n):
                    qmg.hmc_momentum_update_staggered(pi, gauge, [W[j]], [w[j]], L, L, 6.0 if j == 0 else 0.0, dt, 0)

            def copy():
                qmg.copy_vector(dst, src, V)

            calls = [("fused", fused), ("copy", copy)] + ([("composed", composed)] if n else [])
            t = {k: [] for k, _ in calls}
            for rep in range(WARMUP + REPEAT):
                for k, call in calls:
                    timer.start(); call(); ms = timer.stop_ms()
                    if rep >= WARMUP:
                        t[k].append(ms)
            med = {k: float(np.median(v)) for k, v in t.items()}
            copy_gbs = 32.0 * V / 1e6 / med["copy"]
            bf = 64.0 + 16.0 * n
            print("%d^2 n=%d fused    %.4f ms (min %.4f max %.4f) = %.0f GB/s on the %.0f B/site model; copy_vector %.4f ms = %.0f GB/s, the kick is at %.1f %% of it" % (
                L, n, med["fused"], min(t["fused"]), max(t["fused"]), bf * V / 1e6 / med["fused"], bf, med["copy"], copy_gbs, 100.0 * bf * V / 1e6 / med["fused"] / copy_gbs))
            if n:
                bc = 80.0 * n
                print("%d^2 n=%d composed %.4f ms (min %.4f max %.4f) = %.0f GB/s on the %.0f B/site model; time ratio fused / composed %.3f, byte-model ratio %.3f" % (
                    L, n, med["composed"], min(t["composed"]), max(t["composed"]), bc * V / 1e6 / med["composed"], bc, med["fused"] / med["composed"], bf / bc), flush=True)
        for d in [gauge, pi, src, dst] + W:
            d.free()


if __name__ == "__main__":
    main()
