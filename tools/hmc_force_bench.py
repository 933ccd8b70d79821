"""The HMC force kernel (qmg_hmc_momentum_update, csrc/qmg_hmc.hip): milliseconds per call at 2048^2 and 4096^2 against the byte model and this
part's copy ceiling.  Byte model: 128 B per site -- the momenta read and written (32), two complex<double> links (32), X and Y at two spin
components each (64); the neighbours' links and spinors are expected from cache.  Pure gauge (QMG_HMC_GAUGE_ONLY): 64 B per site.
Copy ceiling: 6.2 TB/s (profiles/r01_membw_ceiling.txt, read + write, 262 144 blocks).  The link update (qmg_hmc_link_update: 40 B per link -- phase
read and written, momentum read, complex link written -- 80 B per site) and a device-to-device copy of a spinor through qmg_copy_vector, the ceiling of the day, are timed alongside.
HIP events around single calls, 3 warm-up rounds, medians of 10.
    python tools/hmc_force_bench.py   (GPU box; everything is allocated before the first timed region)"""
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
        gauge, X, Y, Z = qmg.DeviceArray(2 * V), qmg.DeviceArray(2 * V), qmg.DeviceArray(2 * V), qmg.DeviceArray(2 * V)
        pi, theta = qmg.DeviceArray(2 * V, np.float64), qmg.DeviceArray.zeros(2 * V, np.float64)
        qmg.u1_gauss_gauge(gauge, L, L, 6.0, 1337)
        qmg.gaussian(X, 2 * V, 1)
        qmg.gaussian(Y, 2 * V, 2)
        qmg.hmc_momentum_refresh(pi, 2 * V, 3, 0)
        runs = {
            "force, two flavours": (128.0, lambda: qmg.hmc_momentum_update(pi, gauge, X, Y, L, L, 6.0, 1e-3, 0)),
            "force, pure gauge": (64.0, lambda: qmg.hmc_momentum_update(pi, gauge, None, None, L, L, 6.0, 1e-3, qmg.HMC_GAUGE_ONLY)),
            "link update": (80.0, lambda: qmg.hmc_link_update(theta, gauge, pi, 2 * V, 1e-3)),
            "copy of a spinor": (64.0, lambda: qmg.copy_vector(Z, X, 2 * V)),
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
            print("%d^2 %-20s %.4f ms (min %.4f max %.4f) = %.0f GB/s on the %.0f B/site model, %.1f %% of the %.0f GB/s copy ceiling" % (
                L, k + ":", med, min(t[k]), max(t[k]), mb / med, bytes_per_site, 100.0 * mb / med / COPY_CEILING_GBS, COPY_CEILING_GBS), flush=True)
        for d in (gauge, X, Y, Z, pi, theta):
            d.free()


if __name__ == "__main__":
    main()
