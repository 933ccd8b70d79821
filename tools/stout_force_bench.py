"""The stout kernels (csrc/qmg_stout.hip): milliseconds per call at 2048^2 and 4096^2 against their byte models and this part's copy ceiling.
Byte models, per site (the neighbours' links and forces are expected from cache):
  fused kick (qmg_hmc_momentum_update_stout)   80 B -- the momenta read and written (32), two complex<double> links (32), F_in (16)
  level kernel (qmg_u1_stout_force_level)      64 B -- two links (32), F_in (16), F_out (16)
  force bilinear (qmg_hmc_fermion_force)       48 + 64 n B -- two links (32), F written (16), per pole X_j and Y_j (64); timed at n = 1 and n = 8
  smear level (qmg_u1_stout_smear, one level)  64 B -- two links read (32), two written (32)
and the composition the fused kick replaces, timed in the same run: the level kernel (64), the gauge-only qmg_hmc_momentum_update (64) and
pi -= dt F as a qmg_caxpy over the momenta viewed as complex numbers (48) -- 176 B against 80, so the models say 0.45 for fused over composed.
Copy ceiling: 6.2 TB/s (profiles/r01_membw_ceiling.txt, read + write, 262 144 blocks).  HIP events around single calls (around the three
calls of the composition), 3 warm-up rounds, medians of 10.
    python tools/stout_force_bench.py   (GPU box; everything is allocated before the first timed region)"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
qmg = importlib.import_module("quantum-mg_amd")
WARMUP, REPEAT = 3, 10
COPY_CEILING_GBS = 6205.4
RHO, BETA, DT = 0.1, 6.0, 1e-3
POLES = 8


def main():
    qmg.init(0)
    timer = qmg.Timer()
    for L in (2048, 4096):
        V = L * L
        gauge, fat = qmg.DeviceArray(2 * V), qmg.DeviceArray(2 * V)
        X = [qmg.DeviceArray(2 * V) for _ in range(POLES)]
        Y = [qmg.DeviceArray(2 * V) for _ in range(POLES)]
        pi, Fa, Fb = (qmg.DeviceArray(2 * V, np.float64) for _ in range(3))
        qmg.u1_gauss_gauge(gauge, L, L, 6.0, 1337)
        for j in range(POLES):
            qmg.gaussian(X[j], 2 * V, 1 + 2 * j)
            qmg.gaussian(Y[j], 2 * V, 2 + 2 * j)
        qmg.hmc_momentum_refresh(pi, 2 * V, 3, 0)
        qmg.hmc_momentum_refresh(Fa, 2 * V, 4, 0)
        w = [1.0 / POLES] * POLES

        def composed():
            qmg.u1_stout_force_level(Fb, Fa, gauge, L, L, RHO)
            qmg.hmc_momentum_update(pi, gauge, None, None, L, L, BETA, DT, qmg.HMC_GAUGE_ONLY)
            qmg.caxpy(-DT, Fb, pi, V)

        runs = {
            "fused kick": (80.0, lambda: qmg.hmc_momentum_update_stout(pi, gauge, Fa, L, L, BETA, RHO, DT)),
            "level + gauge kick + axpy": (176.0, composed),
            "level kernel": (64.0, lambda: qmg.u1_stout_force_level(Fb, Fa, gauge, L, L, RHO)),
            "gauge-only kick": (64.0, lambda: qmg.hmc_momentum_update(pi, gauge, None, None, L, L, BETA, DT, qmg.HMC_GAUGE_ONLY)),
            "axpy of F": (48.0, lambda: qmg.caxpy(-DT, Fb, pi, V)),
            "force bilinear, 1 pole": (48.0 + 64.0, lambda: qmg.hmc_fermion_force(Fb, gauge, X[:1], Y[:1], [1.0], L, L)),
            "force bilinear, %d poles" % POLES: (48.0 + 64.0 * POLES, lambda: qmg.hmc_fermion_force(Fb, gauge, X, Y, w, L, L)),
            "smear level": (64.0, lambda: qmg.u1_stout_smear(fat, gauge, L, L, RHO, 1)),
        }
        t = {k: [] for k in runs}
        for rep in range(WARMUP + REPEAT):
            for k, (_, call) in runs.items():
                timer.start(); call(); ms = timer.stop_ms()
                if rep >= WARMUP:
                    t[k].append(ms)
        for k, (bytes_per_site, _) in runs.items():
            med = float(np.median(t[k]))
            mb = bytes_per_site * V / 1e6                              # MB per call; MB / ms = GB/s
            print("%d^2 %-26s %.4f ms (min %.4f max %.4f) = %.0f GB/s on the %.0f B/site model, %.1f %% of the %.0f GB/s copy ceiling" % (
                L, k + ":", med, min(t[k]), max(t[k]), mb / med, bytes_per_site, 100.0 * mb / med / COPY_CEILING_GBS, COPY_CEILING_GBS), flush=True)
        fused, comp = float(np.median(t["fused kick"])), float(np.median(t["level + gauge kick + axpy"]))
        print("%d^2 fused over composed: %.3f (byte models: %.3f)" % (L, fused / comp, 80.0 / 176.0), flush=True)
        for d in [gauge, fat, pi, Fa, Fb] + X + Y:
            d.free()


if __name__ == "__main__":
    main()
