"""The Moebius domain-wall applies straight from the links (csrc/qmg_mobius.hip) at 2048^2, Ls = 8, in fp64 and fp32:
  (i)   qmg_mobius_apply_direct op 0, D          (the hop source mixed along s on the load)
  (ii)  qmg_mobius_apply_direct op 1, D^dagger   (the hop sum mixed along s through LDS)
  (iii) qmg_dwf_apply_direct, the Shamir full operator on the same lattice (kernel D2)
  (iv)  a device copy of one five-dimensional vector (qmg_memcpy_d2d)
The bar: (i) and (ii) each take no longer than (iii) + (iv) -- the floor of the alternative design, a separate mixing pass in front of or
behind a Shamir-shaped apply, which has to read and write the vector once more.  (iii) and (iv) are not code of csrc/qmg_mobius.hip.  The
ratios (i) / (iii) and (ii) / (iii) are reported and not gated: the byte model is the same, 64 Ls + 32 B/site in fp64.
Device events around `--iters` calls per timing; the legs alternate inside one process for `--rounds` rounds after a warm-up of every leg;
median [min .. max].  The exit status is 1 when a leg misses the bar by more than the run-to-run spread of the legs compared.

    python tools/mobius_bench.py [--L 2048] [--Ls 8] [--iters 20] [--rounds 7] [--out profiles/mobius_apply_bench.txt]
"""
import argparse
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

qmg = importlib.import_module("quantum-mg_amd")
COPY_CEILING_GBS = 6205.4      # profiles/r01_membw_ceiling.txt: streaming copy at 262 144 blocks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=2048)
    ap.add_argument("--Ls", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    qmg.init(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    timer = qmg.Timer()

    def timed(fn):
        qmg.sync()
        timer.start()
        for _ in range(a.iters):
            fn()
        return timer.stop_ms() / a.iters

    FULL = qmg.P_ALL | qmg.P_ZERO
    L, Ls, nc = a.L, a.Ls, 2 * a.Ls
    vol = L * L
    mass, M5, b5, c5 = 0.05, -1.0, 1.5, 0.5
    rng = np.random.default_rng(1)
    g = qmg.DeviceArray.from_host(np.exp(1j * 0.4 * rng.standard_normal(2 * vol)))
    g32 = qmg.DeviceArray(2 * vol, np.complex64)
    qmg.convert(g32, qmg.C32, g, qmg.C64, 2 * vol)
    say("# Moebius domain-wall apply from the links at %d^2, Ls = %d, b5 = %g, c5 = %g: (i) D, (ii) D^dagger, (iii) Shamir kernel D2, (iv) copy of one vector"
        % (L, Ls, b5, c5))
    say("# %d calls per timing, %d alternating rounds; median [min .. max] ms" % (a.iters, a.rounds))
    failed = False
    for prec, dt, npt, esz in (("fp64", qmg.C64, np.complex128, 16), ("fp32", qmg.C32, np.complex64, 8)):
        gauge = g if dt == qmg.C64 else g32
        r, l = qmg.DeviceArray(vol * nc, npt), qmg.DeviceArray(vol * nc, npt)
        tmp = qmg.DeviceArray(vol * nc)
        qmg.gaussian(tmp, vol * nc, 5)
        qmg.convert(r, dt, tmp, qmg.C64, vol * nc)
        del tmp
        d0 = qmg.make_desc(L, L, nc, None, None)
        ds = qmg.make_desc(L, L, nc, None, None, M5)

        def leg_d():
            qmg.mobius_apply_direct(dt, d0, gauge, Ls, mass, l, r, FULL, 1.0, M5, b5, c5, 0)

        def leg_dagger():
            qmg.mobius_apply_direct(dt, d0, gauge, Ls, mass, l, r, FULL, 1.0, M5, b5, c5, 1)

        def leg_shamir():
            qmg.dwf_apply_direct(dt, ds, gauge, Ls, mass, l, r, FULL, 1.0)

        def leg_copy():
            qmg.memcpy_d2d(l, r, r.nbytes)

        legs = (("i", leg_d), ("ii", leg_dagger), ("iii", leg_shamir), ("iv", leg_copy))
        for _, fn in legs:                      # warm-up: code objects, clocks
            for _ in range(3):
                fn()
        times = {name: [] for name, _ in legs}
        for _ in range(a.rounds):
            for name, fn in legs:
                times[name].append(timed(fn))
        med = {k: float(np.median(v)) for k, v in times.items()}
        spread = {k: float(np.max(v) - np.min(v)) for k, v in times.items()}
        model = (4 * esz * Ls + 2 * esz) * vol                      # vector in, vector out, the links: (64 Ls + 32) B/site in fp64
        cmodel = 2 * esz * nc * vol
        names = {"i": "Moebius D (op 0)       ", "ii": "Moebius D^dagger (op 1)", "iii": "Shamir kernel D2       "}
        for k in ("i", "ii", "iii"):
            gbs = model / med[k] / 1e6
            say("%s %-5s %s %.4f [%.4f .. %.4f] ms  %7.1f GB/s on %d B/site  %.3f of the %.1f TB/s copy ceiling"
                % (prec, "(%s)" % k, names[k], med[k], min(times[k]), max(times[k]), gbs, model // vol, gbs / COPY_CEILING_GBS, COPY_CEILING_GBS / 1e3))
        say("%s (iv)  copy of one vector      %.4f [%.4f .. %.4f] ms  %7.1f GB/s on %d B/site"
            % (prec, med["iv"], min(times["iv"]), max(times["iv"]), cmodel / med["iv"] / 1e6, cmodel // vol))
        floor = med["iii"] + med["iv"]
        for k in ("i", "ii"):
            margin = max(spread[k], spread["iii"], spread["iv"])
            ok = med[k] <= floor + margin
            failed = failed or not ok
            say("%s (%s) / (iii) = %.3f (byte model: 1.000);  (%s) %.4f against (iii) + (iv) = %.4f ms; run-to-run spread (%s) %.4f, (iii) %.4f, (iv) %.4f ms: %s"
                % (prec, k, med[k] / med["iii"], k, med[k], floor, k, spread[k], spread["iii"], spread["iv"], "PASS" if ok else "FAIL"))
        del r, l
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
