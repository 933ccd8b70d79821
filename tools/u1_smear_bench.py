"""APE smearing (qmg_u1_ape_smear, csrc/qmg_u1.hip): milliseconds per iteration at 2048^2 and 4096^2 against the byte model and this part's
copy ceiling.  Byte model: 64 B per site and iteration -- two complex<double> links read, two written; the neighbours' links (13 more
loads per pair of sites) are expected from cache.  Copy ceiling: 6.2 TB/s (profiles/r01_membw_ceiling.txt, read + write, 262 144 blocks).
The cost of one iteration is the slope between two out-of-place calls of n_iter = 1 and n_iter = 21 (both odd, so both end in `smeared`), which
takes the call's own overhead out; HIP events, 3 warm-up rounds, medians of 10.
A device-to-device copy of the same field through qmg_copy_vector is timed alongside as the ceiling of the day.
    python tools/u1_smear_bench.py   (GPU box; everything is allocated before the first timed region)"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
qmg = importlib.import_module("quantum-mg_amd")
WARMUP, REPEAT = 3, 10
N_LO, N_HI = 1, 21
COPY_CEILING_GBS = 6205.4


def main():
    qmg.init(0)
    timer = qmg.Timer()
    for L in (2048, 4096):
        V = L * L
        gauge, smeared = qmg.DeviceArray(2 * V), qmg.DeviceArray(2 * V)
        qmg.u1_gauss_gauge(gauge, L, L, 6.0, 1337)
        t = {N_LO: [], N_HI: [], "copy": []}
        for rep in range(WARMUP + REPEAT):
            for n in (N_LO, N_HI):
                timer.start(); qmg.u1_ape_smear(smeared, gauge, L, L, 0.5, n); ms = timer.stop_ms()
                if rep >= WARMUP:
                    t[n].append(ms)
            timer.start(); qmg.copy_vector(smeared, gauge, 2 * V); ms = timer.stop_ms()
            if rep >= WARMUP:
                t["copy"].append(ms)
        lo, hi, cp = float(np.median(t[N_LO])), float(np.median(t[N_HI])), float(np.median(t["copy"]))
        per_iter = (hi - lo) / (N_HI - N_LO)
        mb = 64.0 * V / 1e6                                            # MB per iteration; MB / ms = GB/s
        print("%d^2: n_iter=1 %.4f ms (min %.4f max %.4f) | n_iter=21 %.4f ms (min %.4f max %.4f) | per iteration %.4f ms = %.0f GB/s on the 64 B/site model, "
              "%.1f %% of the %.0f GB/s copy ceiling | copy of the same field %.4f ms = %.0f GB/s" % (
                  L, lo, min(t[N_LO]), max(t[N_LO]), hi, min(t[N_HI]), max(t[N_HI]), per_iter, mb / per_iter, 100.0 * mb / per_iter / COPY_CEILING_GBS,
                  COPY_CEILING_GBS, cp, mb / cp), flush=True)
        qmg.u1_ape_smear(smeared, gauge, L, L, 0.5, N_HI)
        print("%d^2: plaquette %.6f, after %d iterations %.6f" % (L, qmg.u1_plaquette(gauge, L, L)[0].real, N_HI, qmg.u1_plaquette(smeared, L, L)[0].real), flush=True)
        gauge.free(); smeared.free()


if __name__ == "__main__":
    main()
