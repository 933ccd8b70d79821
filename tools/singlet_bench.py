"""The fused flavour-singlet loops kernel (qmg_loops_timeslice_batch, csrc/qmg_singlet.hip) against the same numbers composed from the
entries the project had before it, and against a copy.

Legs, on `--nsys` systems of an L x L lattice with nc = 2 (fp64; the fused kernel also in fp32), spin and even-odd dilution with nt = 4:
  (i)   the fused kernel: one launch for the batch, 16 nc B/site per system (8 nc in fp32), 5 Ly doubles per system written
  (ii)  per system: qmg_caxy_pattern for gamma5 psi, two qmg_dot_cv_timeslice against a STORED diluted source (with psi and with
        gamma5 psi), one qmg_norm2sq_cv_timeslice -- seven vector passes and four launches per system; complex<double> only
  (iii) qmg_copy_vector of the batch: the same bytes read, and as many written
Device events around `--iters` calls per timing; the legs alternate inside one process for `--rounds` rounds after a warm-up of every leg;
median [min .. max].  Bar: (i) <= (ii) in fp64, beyond the larger min .. max spread of the two; the exit status is 1 otherwise.  The ratio
and (i)'s fraction of the copy ceiling are reported.

    python tools/singlet_bench.py [--L 2048] [--nsys 8] [--iters 10] [--rounds 7] [--out profiles/singlet_loops_bench.txt]
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
    ap.add_argument("--nsys", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
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

    L, K, nc = a.L, a.nsys, 2
    dims, dil, seed = (L, L), (4, 1, 1), 7
    n = L * L * nc
    C = qmg.C
    dptr = lambda d, off=0: C.cast(C.c_void_p(d.ptr + 8 * off), C.POINTER(C.c_double))
    x64 = qmg.DeviceArray(K * n)
    qmg.gaussian(x64, K * n, 5)
    x32 = qmg.DeviceArray(K * n, np.complex64)
    qmg.convert(x32, qmg.C32, x64, qmg.C64, K * n)
    src = qmg.DeviceArray(K * n)
    qmg.noise_dilute_batch(qmg.C64, src, dims, nc, dil, 0, seed, K, n)
    tmp = qmg.DeviceArray(n)
    cpy = qmg.DeviceArray(K * n)
    out_new = qmg.DeviceArray(K * L * 5, np.float64)
    out_old = qmg.DeviceArray(K * L * 5, np.float64)

    def fused(dtype, x):
        return lambda: qmg.check(qmg.loops_timeslice_batch_status(dtype, x, dims, nc, dil, 0, seed, 0, K, n, None, out_new, None), "qmg_loops_timeslice_batch")

    def composed():
        lib = qmg.lib()
        for k in range(K):
            qmg.caxy_pattern([1.0, -1.0], [0, 1], x64.offset(k * n), tmp, L * L)
            xk, sk = C.c_void_p(x64.offset(k * n)), C.c_void_p(src.offset(k * n))
            qmg.check(lib.qmg_dot_cv_timeslice(sk, xk, L, L, nc, dptr(out_old, k * L * 5), None, None), "qmg_dot_cv_timeslice")
            qmg.check(lib.qmg_dot_cv_timeslice(sk, C.c_void_p(tmp.ptr), L, L, nc, dptr(out_old, k * L * 5 + 2 * L), None, None), "qmg_dot_cv_timeslice")
            qmg.check(lib.qmg_norm2sq_cv_timeslice(xk, L, L, nc, dptr(out_old, k * L * 5 + 4 * L), None, None), "qmg_norm2sq_cv_timeslice")

    legs = (("fused64", fused(qmg.C64, x64)), ("composed64", composed), ("fused32", fused(qmg.C32, x32)), ("copy64", lambda: qmg.copy_vector(cpy, x64, K * n)))
    for _, fn in legs:
        for _ in range(3):
            fn()
    # the two fp64 legs hold the same numbers: S, P, N of every system and row, to the summation-order gate of the tests
    qmg.check(qmg.loops_timeslice_batch_status(qmg.C64, x64, dims, nc, dil, 0, seed, 0, K, n, None, out_new, None))
    new = out_new.to_host().reshape(K, L, 5)
    old = out_old.to_host().reshape(K, 5 * L)
    old = np.concatenate([old[:, :2 * L].reshape(K, L, 2), old[:, 2 * L:4 * L].reshape(K, L, 2), old[:, 4 * L:].reshape(K, L, 1)], axis=2)
    agree = float(np.abs(new - old).max() / np.sqrt(new[:, :, 4].max() * L * nc))
    times = {name: [] for name, _ in legs}
    for _ in range(a.rounds):
        for name, fn in legs:
            times[name].append(timed(fn))
    plan = qmg.singlet_plan(dims, nc, dil, 0, K)
    say("# qmg_loops_timeslice_batch against its composition from qmg_caxy_pattern + 2 qmg_dot_cv_timeslice + qmg_norm2sq_cv_timeslice per system, and a copy:")
    say("# %d systems of %d^2, nc = %d, dilution (nt, spin, eo) = %s; %d calls per timing, %d alternating rounds, device events; median [min .. max] ms" % (K, L, nc, dil, a.iters, a.rounds))
    say("# plan (family, block, gx, gy, walk, lds, doubles, dgx, dgy, dwalk, nk, classes) = %s; the two fp64 legs agree to %.1e of sqrt(N_row x row length)" % (plan, agree))
    rows = (("fused64", "(i)   fp64 fused loops kernel      ", 16 * nc, 1), ("composed64", "(ii)  fp64 composition, 7 passes    ", 16 * nc, 7),
            ("fused32", "(i)   fp32 fused loops kernel      ", 8 * nc, 1), ("copy64", "(iii) fp64 qmg_copy_vector         ", 32 * nc, 1))
    for name, what, bytes_site, passes in rows:
        tb = bytes_site * passes * L * L * K / med(times[name]) / 1e9
        say("%s %s ms  %6.3f TB/s on %d B/site/system%s (%.0f %% of the %.1f TB/s copy ceiling)"
            % (what, fmt(times[name]), tb, bytes_site * passes, " moved" if passes > 1 or name == "copy64" else "", 100 * tb / COPY_CEILING, COPY_CEILING))
    margin = max(spread(times["fused64"]), spread(times["composed64"]))
    ok = med(times["fused64"]) <= med(times["composed64"]) + margin
    say("fp64 (i) / (ii) = %.3f (bar: (i) <= (ii) + %.4f ms, the larger min .. max spread): %s" % (med(times["fused64"]) / med(times["composed64"]), margin, "PASS" if ok else "FAIL"))
    say("fp32 (i) / fp64 (i) = %.3f ; fp64 (i) / (iii) = %.3f" % (med(times["fused32"]) / med(times["fused64"]), med(times["fused64"]) / med(times["copy64"])))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
