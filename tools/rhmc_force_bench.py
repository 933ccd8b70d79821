"""The RHMC pole kick (qmg_hmc_momentum_update_poles, csrc/qmg_hmc.hip) against the composition it replaces, at 2048^2 and 4096^2 for n = 4, 8
and 12 poles.  Fused: pi -= dt (Fg + sum_j w_j Ff(X_j, Y_j)) in one pass.  Composed: one gauge-only call of qmg_hmc_momentum_update plus n
calls of it with beta = 0 and dt w_j, each of which reads and writes the momenta and reads the links again.
Byte model: fused 64 + 64 n B per site (momenta read and written 32, two complex<double> links 32, X_j and Y_j at two spin components each
64 per pole); composed 64 + 128 n.  The model ratio is (64 + 64 n) / (64 + 128 n): 0.556, 0.529, 0.520 at n = 4, 8, 12.
HIP events around whole kicks, 3 warm-up rounds, medians of 10, fused and composed alternating.
    python tools/rhmc_force_bench.py   (GPU box; everything is allocated before the first timed region)"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
qmg = importlib.import_module("quantum-mg_amd")
WARMUP, REPEAT = 3, 10
COPY_CEILING_GBS = 6205.4


def main():
    qmg.init(0)
    timer = qmg.Timer()
    for L in (2048, 4096):
        V = L * L
        gauge = qmg.DeviceArray(2 * V)
        pi = qmg.DeviceArray(2 * V, np.float64)
        qmg.u1_gauss_gauge(gauge, L, L, 6.0, 1337)
        qmg.hmc_momentum_refresh(pi, 2 * V, 3, 0)
        X, Y = [], []
        for n in (4, 8, 12):
            while len(X) < n:
                X.append(qmg.DeviceArray(2 * V)); Y.append(qmg.DeviceArray(2 * V))
                qmg.gaussian(X[-1], 2 * V, 10 + 2 * len(X))
                qmg.gaussian(Y[-1], 2 * V, 11 + 2 * len(X))
            w = [0.1 + 0.05 * j for j in range(n)]
            dt = 1e-3

            def fused():
                qmg.hmc_momentum_update_poles(pi, gauge, X[:n], Y[:n], w, L, L, 6.0, dt, 0)

            def composed():
                qmg.hmc_momentum_update(pi, gauge, None, None, L, L, 6.0, dt, qmg.HMC_GAUGE_ONLY)
                for j in range(n):
                    qmg.hmc_momentum_update(pi, gauge, X[j], Y[j], L, L, 0.0, dt * w[j], 0)

            t = {"fused": [], "composed": []}
            for rep in range(WARMUP + REPEAT):
                for k, call in (("fused", fused), ("composed", composed)):
                    timer.start(); call(); ms = timer.stop_ms()
                    if rep >= WARMUP:
                        t[k].append(ms)
            mf, mc = float(np.median(t["fused"])), float(np.median(t["composed"]))
            bf, bc = 64.0 + 64.0 * n, 64.0 + 128.0 * n
            print("%d^2 n=%2d fused    %.4f ms (min %.4f max %.4f) = %.0f GB/s on the %.0f B/site model, %.1f %% of the %.0f GB/s copy ceiling" % (
                L, n, mf, min(t["fused"]), max(t["fused"]), bf * V / 1e6 / mf, bf, 100.0 * bf * V / 1e6 / mf / COPY_CEILING_GBS, COPY_CEILING_GBS))
            print("%d^2 n=%2d composed %.4f ms (min %.4f max %.4f) = %.0f GB/s on the %.0f B/site model" % (L, n, mc, min(t["composed"]), max(t["composed"]), bc * V / 1e6 / mc, bc))
            print("%d^2 n=%2d time ratio fused / composed %.3f (spread of the fused median's samples %.1f %%, composed %.1f %%); byte-model ratio %.3f" % (
                L, n, mf / mc, 100.0 * (max(t["fused"]) - min(t["fused"])) / mf, 100.0 * (max(t["composed"]) - min(t["composed"])) / mc, bf / bc), flush=True)
        for d in [gauge, pi] + X + Y:
            d.free()


if __name__ == "__main__":
    main()
