"""The domain-wall slice norms (qmg_dwf_slice_norms, csrc/qmg_dwf_meas.hip) against the per-timeslice norm the project had before it.

The comparison leg is qmg_norm2sq_cv_timeslice on the same vector with nc = 2 Ls: the same bytes read, Ly numbers written instead of
2 Ls Ly.  It exists for complex<double> only, so the fp32 entry is held to the fp64 leg's time on the fp64 vector (twice its bytes).
Device events around `--iters` calls per timing; the legs alternate inside one process for `--rounds` rounds after a warm-up of every leg;
median [min .. max].  Bar: the new kernel's median is not above the leg's median by more than the larger min .. max spread of the two legs;
the exit status is 1 otherwise.  The wall source and the projections are reported on their byte models, without a bar.

    python tools/dwf_meas_bench.py [--L 2048] [--Ls 8] [--iters 20] [--rounds 7] [--out profiles/dwf_meas_bench.txt]
"""
import argparse
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

qmg = importlib.import_module("quantum-mg_amd")

COPY_CEILING = 6.2   # TB/s, profiles/r01_membw_ceiling.txt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=2048)
    ap.add_argument("--Ls", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    fmt = lambda v: "%.4f [%.4f .. %.4f]" % (float(np.median(v)), min(v), max(v))
    med = lambda v: float(np.median(v))
    spread = lambda v: max(v) - min(v)

    qmg.init(0)
    timer = qmg.Timer()

    def timed(fn):
        qmg.sync()
        timer.start()
        for _ in range(a.iters):
            fn()
        return timer.stop_ms() / a.iters

    L, Ls, nc = a.L, a.Ls, 2 * a.Ls
    vol, dims = L * L, (L, L)
    n5, n4 = vol * nc, vol * 2
    x64 = qmg.DeviceArray(n5)
    qmg.gaussian(x64, n5, 5)
    x32 = qmg.DeviceArray(n5, np.complex64)
    qmg.convert(x32, qmg.C32, x64, qmg.C64, n5)
    out_new = qmg.DeviceArray(L * nc, np.float64)
    out_old = qmg.DeviceArray(L, np.float64)
    C = qmg.C
    dptr = lambda d: C.cast(C.c_void_p(d.ptr), C.POINTER(C.c_double))

    def old():
        qmg.check(qmg.lib().qmg_norm2sq_cv_timeslice(C.c_void_p(x64.ptr), L, L, nc, dptr(out_old), None, None), "qmg_norm2sq_cv_timeslice")

    legs = (("new64", lambda: qmg.check(qmg.dwf_slice_norms_status(qmg.C64, dims, Ls, x64, 1, 0, out_new, None), "qmg_dwf_slice_norms")),
            ("old64", old),
            ("new32", lambda: qmg.check(qmg.dwf_slice_norms_status(qmg.C32, dims, Ls, x32, 1, 0, out_new, None), "qmg_dwf_slice_norms")))
    for _, fn in legs:
        for _ in range(3):
            fn()
    times = {name: [] for name, _ in legs}
    for _ in range(a.rounds):
        for name, fn in legs:
            times[name].append(timed(fn))
    plan = qmg.dwf_meas_plan(qmg.C64, dims, Ls, qmg.DMK_NORMS)
    say("# qmg_dwf_slice_norms (2 Ls Ly = %d numbers) against qmg_norm2sq_cv_timeslice with nc = %d (Ly = %d numbers) on the same vector at %d^2, Ls = %d"
        % (nc * L, nc, L, L, Ls))
    say("# %d calls per timing, %d alternating rounds, device events; median [min .. max] ms; plan (family, lps, block, gx, gy, pbr, lds, nk) = %s" % (a.iters, a.rounds, plan))
    failed = False
    for name, what, esz in (("new64", "fp64 qmg_dwf_slice_norms     ", 16), ("old64", "fp64 qmg_norm2sq_cv_timeslice", 16), ("new32", "fp32 qmg_dwf_slice_norms     ", 8)):
        tb = esz * nc * vol / med(times[name]) / 1e9
        say("%s  %s ms  %6.3f TB/s on %d B/site (%.0f %% of the %.1f TB/s copy ceiling)" % (what, fmt(times[name]), tb, esz * nc, 100 * tb / COPY_CEILING, COPY_CEILING))
    for name, prec in (("new64", "fp64"), ("new32", "fp32")):
        margin = max(spread(times[name]), spread(times["old64"]))
        ok = med(times[name]) <= med(times["old64"]) + margin
        failed = failed or not ok
        say("%s new / old = %.3f (bar: new <= old + %.4f ms, the larger min .. max spread): %s" % (prec, med(times[name]) / med(times["old64"]), margin, "PASS" if ok else "FAIL"))

    # the wall source and the projections on their byte models (reported)
    e64 = qmg.DeviceArray(n4)
    qmg.gaussian(e64, n4, 6)
    q64 = qmg.DeviceArray(n4)
    small = (("wall source    ", lambda: qmg.dwf_wall_source(qmg.C64, dims, Ls, x64, e64), 16 * nc + 32),
             ("wall projection", lambda: qmg.dwf_wall_project(qmg.C64, dims, Ls, q64, x64, 0), 64),
             ("midpoint proj. ", lambda: qmg.dwf_wall_project(qmg.C64, dims, Ls, q64, x64, 1), 64))
    if Ls % 2:
        small = small[:2]
    # the projections first: the source overwrites the vector they read
    for what, fn, bytes_site in small[1:] + small[:1]:
        for _ in range(3):
            fn()
        t = [timed(fn) for _ in range(a.rounds)]
        say("fp64 %s  %s ms  %6.3f TB/s on %d B/site" % (what, fmt(t), bytes_site * vol / med(t) / 1e9, bytes_site))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
