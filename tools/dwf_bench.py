"""Kernel D2 (the Shamir domain-wall operator straight from the links, csrc/qmg_dwf.hip) at 2048^2, Ls = 8, in fp64 and fp32, against
  (ii)  Ls calls of qmg_wilson_apply_direct on the same lattice (kernel W2 on Ls distinct vector pairs: 96 Ls B/site in fp64 against
        kernel D's 64 Ls + 32), and
  (iii) the stored route (qmg_dwf_fill + qmg_stencil_apply on the nc = 2 Ls stencil), at 512^2 so that its matrices (5.5 GB) fit easily.
The vectors of the direct legs are 1 GiB each in fp64, far past the Infinity Cache.  Device events around `--iters` calls per timing; the
legs alternate inside one process for `--rounds` rounds after a warm-up of every leg, and the spread over the rounds is printed next to
the median.  Acceptance: leg (i) takes no longer than leg (ii) in both precisions, with no margin beyond the measured spread of the two
legs; the exit status is 1 otherwise.

    python tools/dwf_bench.py [--L 2048] [--Ls 8] [--Lstored 512] [--iters 20] [--rounds 7] [--out profiles/dwf_apply_bench.txt]
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
    ap.add_argument("--Lstored", type=int, default=512)
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
    mass, M5 = 0.05, -1.0
    rng = np.random.default_rng(1)
    g = qmg.DeviceArray.from_host(np.exp(1j * 0.4 * rng.standard_normal(2 * vol)))
    g32 = qmg.DeviceArray(2 * vol, np.complex64)
    qmg.convert(g32, qmg.C32, g, qmg.C64, 2 * vol)
    # the stored stencil on the small lattice
    Lp = a.Lstored
    volp = Lp * Lp
    gp = qmg.DeviceArray.from_host(np.exp(1j * 0.4 * rng.standard_normal(2 * volp)))
    cl, hp = qmg.DeviceArray(volp * nc * nc), qmg.DeviceArray(4 * volp * nc * nc)
    qmg.dwf_fill(cl, hp, gp, Lp, Lp, Ls, mass, 1.0)
    say("# domain-wall apply, Ls = %d: (i) kernel D2 from the links and (ii) %d x kernel W2 at %d^2; (iii) stored nc = %d stencil at %d^2" % (Ls, Ls, L, nc, Lp))
    say("# %d calls per timing, %d alternating rounds; median [min .. max] ms" % (a.iters, a.rounds))
    failed = False
    per_site = {}
    for prec, dt, npt, esz in (("fp64", qmg.C64, np.complex128, 16), ("fp32", qmg.C32, np.complex64, 8)):
        gauge = g if dt == qmg.C64 else g32
        r, l = qmg.DeviceArray(vol * nc, npt), qmg.DeviceArray(vol * nc, npt)
        tmp = qmg.DeviceArray(vol * nc)
        qmg.gaussian(tmp, vol * nc, 5)
        qmg.convert(r, dt, tmp, qmg.C64, vol * nc)
        del tmp
        d = qmg.make_desc(L, L, nc, None, None, M5)
        dw = qmg.make_desc(L, L, 2, None, None, mass)
        rp, lp = qmg.DeviceArray(volp * nc, npt), qmg.DeviceArray(volp * nc, npt)
        qmg.convert(rp, dt, qmg.DeviceArray.from_host(rng.standard_normal(volp * nc) + 1j * rng.standard_normal(volp * nc)), qmg.C64, volp * nc)
        if dt == qmg.C64:
            ds = qmg.make_desc(Lp, Lp, nc, cl, hp, M5)
        else:
            cl32, hp32 = qmg.DeviceArray(cl.n, np.complex64), qmg.DeviceArray(hp.n, np.complex64)
            qmg.convert(cl32, qmg.C32, cl, qmg.C64, cl.n)
            qmg.convert(hp32, qmg.C32, hp, qmg.C64, hp.n)
            ds = qmg.make_desc(Lp, Lp, nc, cl32, hp32, M5)

        def leg_direct():
            qmg.dwf_apply_direct(dt, d, gauge, Ls, mass, l, r, FULL, 1.0)

        def leg_wilson():   # Ls Wilson applies on Ls distinct vector pairs: slices of the same two arrays
            for s in range(Ls):
                qmg.wilson_apply_direct(dt, dw, gauge, l.offset(2 * vol * s), r.offset(2 * vol * s), FULL)

        def leg_stored():
            qmg.stencil_apply_t(dt, ds, lp, rp, FULL)

        legs = (("i", leg_direct), ("ii", leg_wilson), ("iii", leg_stored))
        for _, fn in legs:                      # warm-up: code objects, clocks
            for _ in range(3):
                fn()
        times = {name: [] for name, _ in legs}
        for _ in range(a.rounds):
            for name, fn in legs:
                times[name].append(timed(fn))
        med = {k: float(np.median(v)) for k, v in times.items()}
        spread = {k: float(np.max(v) - np.min(v)) for k, v in times.items()}
        model = (4 * esz * Ls + 2 * esz) * vol                      # vector in, vector out, four links of two sites' worth: (64 Ls + 32) B/site in fp64
        wmodel = 6 * esz * Ls * vol                                 # 96 Ls B/site in fp64
        smodel = (5 * nc * nc + 2 * nc) * esz * volp
        gbs = model / med["i"] / 1e6
        say("%s (i)   kernel D2             %.4f [%.4f .. %.4f] ms  %7.1f GB/s on %d B/site  %.3f of the %.1f TB/s copy ceiling"
            % (prec, med["i"], min(times["i"]), max(times["i"]), gbs, model // vol, gbs / COPY_CEILING_GBS, COPY_CEILING_GBS / 1e3))
        say("%s (ii)  %d x kernel W2         %.4f [%.4f .. %.4f] ms  %7.1f GB/s on %d B/site"
            % (prec, Ls, med["ii"], min(times["ii"]), max(times["ii"]), wmodel / med["ii"] / 1e6, wmodel // vol))
        say("%s (iii) stored stencil %d^2   %.4f [%.4f .. %.4f] ms  %7.1f GB/s on %d B/site"
            % (prec, Lp, med["iii"], min(times["iii"]), max(times["iii"]), smodel / med["iii"] / 1e6, smodel // volp))
        ratio = med["i"] / med["ii"]
        margin = max(spread["i"], spread["ii"])
        ok = med["i"] <= med["ii"] + margin
        failed = failed or not ok
        per_site[prec] = (med["iii"] / volp) / (med["i"] / vol)
        say("%s (i) / (ii) = %.3f (byte model: %.3f); run-to-run spread (i) %.4f ms, (ii) %.4f ms: %s"
            % (prec, ratio, model / wmodel, spread["i"], spread["ii"], "PASS" if ok else "FAIL"))
        say("%s stored / direct per site = %.1f" % (prec, per_site[prec]))
        del r, l, rp, lp
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
