"""The even-odd Moebius applies and solve (csrc/qmg_mobius_eo.hip, MobiusBase) against what the project had before them.

  1. The solve: drivers/mobius_eo_selftest <Lsolve> <Ls> 0.05 7 <rounds> at 1024^2 (gated) and 256^2 (reported) -- minv_mobius_eo_cg against the
     parent's minv_mobius_cg (CG on D^dagger D, both applies from the links) on the same right-hand side, the latter's eps set so that its true
     residual on D lies within [1/2, 1] of the even-odd solve's; timed alternately in one process, wall clock.  The bar: the even-odd solve is
     faster (ratio below 1).  The expectation written beside the ratio, about 0.42, is the iteration ratio of about 0.59 (CPU, dense numpy) times a
     per-iteration byte model of about 0.71: 160 Ls for M^dagger M plus about 160 Ls of half-length CG vectors, against 128 Ls plus 320 Ls.
     Each driver runs under a time limit; if one fails, times out or prints no timings the tool stops there with exit status 1.
  2. The applies at 2048^2, Ls = 8, b5 = 1.5, c5 = 0.5, in fp64 and fp32:
       (i)   qmg_mobius_schur_apply op 0, M            (ii)  qmg_mobius_schur_apply op 1, M^dagger
       (iii) qmg_dwf_schur_apply, the Shamir Schur complement on the same lattice (the same bytes: 160 Ls + 64 per site of the system in fp64)
       (iv)  a device copy of one half five-dimensional vector (qmg_memcpy_d2d)
     The bar: (i) and (ii) each take no longer than (iii) + 2 (iv) -- the floor of doing the two B mixings as separate passes.  The ratios to
     (iii) (byte model 1.0) and the TB/s on the byte model are reported and not gated.  Device events around `--iters` calls per timing; the
     legs alternate inside one process for `--rounds` rounds after a warm-up of every leg; median [min .. max].  A leg misses the bar when it is
     over it by more than the run-to-run spread of the legs compared.

    python tools/mobius_eo_bench.py [--L 2048] [--Ls 8] [--Lsolve 1024] [--Lsmall 256] [--iters 20] [--rounds 7] [--out profiles/mobius_eo_bench.txt]
"""
import argparse
import importlib
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

qmg = importlib.import_module("quantum-mg_amd")
EXPECTED_RATIO = 0.42


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=2048)
    ap.add_argument("--Ls", type=int, default=8)
    ap.add_argument("--Lsolve", type=int, default=1024)
    ap.add_argument("--Lsmall", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--solve-timeout", type=int, default=300, help="seconds one solve driver may take")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    fmt = lambda v: "%.4f [%.4f .. %.4f]" % (float(np.median(v)), min(v), max(v))
    failed = False

    # ---- 1. the solves, each in a process of its own (run first: the apply legs below hold 3 GiB)
    exe = os.path.join(qmg.HERE, "drivers", "mobius_eo_selftest")
    for Lsolve, gated in ((a.Lsolve, True), (a.Lsmall, False)):
        # the child gets a time limit sized to its work; if it fails, times out or prints no timings, nothing more is started on the GPU
        try:
            child = subprocess.run([exe, str(Lsolve), str(a.Ls), "0.05", "7", str(a.rounds)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                   universal_newlines=True, timeout=a.solve_timeout)
        except subprocess.TimeoutExpired as e:
            print("mobius_eo_selftest did not finish within %d s; stopping before any further GPU work\n%s" % (a.solve_timeout, e.stdout or ""), flush=True)
            return 1
        out = child.stdout
        if child.returncode != 0 or "[QMG-MOBIUS-EO-BENCH] " not in out:
            print("mobius_eo_selftest returned %d%s; stopping before any further GPU work\n%s"
                  % (child.returncode, "" if "[QMG-MOBIUS-EO-BENCH] " in out else " and printed no timing lines", out), flush=True)
            return 1
        checks, eo_ms, full_ms = {}, [], []
        for ln in out.splitlines():
            w = ln.split()
            if ln.startswith("[QMG-MOBIUS-EO] "):
                checks[w[1]] = (float(w[2]), w[3])
            elif ln.startswith("[QMG-MOBIUS-EO-BENCH] "):
                eo_ms.append(float(w[4])); full_ms.append(float(w[6]))
        say("# solve D x = b at %d^2, Ls = %d, b5 = 1.5, c5 = 0.5, m = 0.05, Gaussian links of width 0.4: CG on M^dagger M of the even-odd Schur complement"
            % (Lsolve, a.Ls))
        say("# (minv_mobius_eo_cg) against CG on D^dagger D (minv_mobius_cg), everything from the links; %d alternating rounds, wall clock%s"
            % (a.rounds, "" if gated else "; reported, not gated"))
        failed = failed or any(v[1] != "PASS" for v in checks.values())
        for name in ("eo_iterations", "full_iterations", "eo_true_residual", "full_true_residual", "eo_vs_full_solution"):
            if name in checks:
                say("%-22s %.6g %s" % (name, checks[name][0], checks[name][1]))
        ratio = float(np.median(eo_ms)) / float(np.median(full_ms))
        ok = ratio < 1.0
        say("even-odd solve   %s ms" % fmt(eo_ms))
        say("full solve       %s ms" % fmt(full_ms))
        if gated:
            failed = failed or not ok
            say("even-odd / full = %.3f (bar: < 1; expected from the iteration ratio and the byte model: about %.2f): %s" % (ratio, EXPECTED_RATIO, "PASS" if ok else "FAIL"))
        else:
            say("even-odd / full = %.3f (not gated: four launches per iteration of M^dagger M against two of D^dagger D)" % ratio)
        if "eo_iterations" in checks and "full_iterations" in checks:
            ei, fi = checks["eo_iterations"][0], checks["full_iterations"][0]
            say("iterations even-odd / full = %.3f; per iteration: even-odd %.4f ms, full %.4f ms, ratio %.3f"
                % (ei / fi, float(np.median(eo_ms)) / ei, float(np.median(full_ms)) / fi, (float(np.median(eo_ms)) / ei) / (float(np.median(full_ms)) / fi)))

    # ---- 2. the applies
    qmg.init(0)
    timer = qmg.Timer()

    def timed(fn):
        qmg.sync()
        timer.start()
        for _ in range(a.iters):
            fn()
        return timer.stop_ms() / a.iters

    L, Ls, nc = a.L, a.Ls, 2 * a.Ls
    vol = L * L
    mass, M5, b5, c5 = 0.05, -1.0, 1.5, 0.5
    rng = np.random.default_rng(1)
    g = qmg.DeviceArray.from_host(np.exp(1j * 0.4 * rng.standard_normal(2 * vol)))
    g32 = qmg.DeviceArray(2 * vol, np.complex64)
    qmg.convert(g32, qmg.C32, g, qmg.C64, 2 * vol)
    say("# Schur-complement applies from the links at %d^2, Ls = %d, b5 = %g, c5 = %g: (i) Moebius M, (ii) Moebius M^dagger, (iii) Shamir M, (iv) copy of one half vector"
        % (L, Ls, b5, c5))
    say("# %d calls per timing, %d alternating rounds; median [min .. max] ms" % (a.iters, a.rounds))
    for prec, dt, npt, esz in (("fp64", qmg.C64, np.complex128, 16), ("fp32", qmg.C32, np.complex64, 8)):
        gauge = g if dt == qmg.C64 else g32
        r, l, t = (qmg.DeviceArray(vol * nc, npt) for _ in range(3))
        tmp = qmg.DeviceArray(vol * nc)
        qmg.gaussian(tmp, vol * nc, 5)
        qmg.convert(r, dt, tmp, qmg.C64, vol * nc)
        del tmp
        d0 = qmg.make_desc(L, L, nc, None, None)
        ds = qmg.make_desc(L, L, nc, None, None, M5)
        half_bytes = r.nbytes // 2
        legs = (("i", lambda: qmg.mobius_schur_apply(dt, d0, gauge, Ls, mass, l, r, t, 0, 0, 1.0, M5, b5, c5)),
                ("ii", lambda: qmg.mobius_schur_apply(dt, d0, gauge, Ls, mass, l, r, t, 0, 1, 1.0, M5, b5, c5)),
                ("iii", lambda: qmg.dwf_schur_apply(dt, ds, gauge, Ls, mass, l, r, t, 0, 0, 1.0)),
                ("iv", lambda: qmg.memcpy_d2d(l, r, half_bytes)))
        for _, fn in legs:                      # warm-up: code objects, clocks
            for _ in range(3):
                fn()
        times = {name: [] for name, _ in legs}
        for _ in range(a.rounds):
            for name, fn in legs:
                times[name].append(timed(fn))
        med = {k: float(np.median(v)) for k, v in times.items()}
        spread = {k: float(np.max(v) - np.min(v)) for k, v in times.items()}
        model = (10 * esz * Ls + 4 * esz) * (vol // 2)             # per site of the system, both launches: (160 Ls + 64) B in fp64
        cmodel = 2 * esz * nc * (vol // 2)
        names = {"i": "Moebius M (op 0)       ", "ii": "Moebius M^dagger (op 1)", "iii": "Shamir M               "}
        for k in ("i", "ii", "iii"):
            say("%s %-5s %s %s ms  %6.3f TB/s on %d B per site of the system" % (prec, "(%s)" % k, names[k], fmt(times[k]), model / med[k] / 1e9, 2 * model // vol))
        say("%s (iv)  copy of one half vector  %s ms  %6.3f TB/s on %d B per site of the system" % (prec, fmt(times["iv"]), cmodel / med["iv"] / 1e9, 2 * cmodel // vol))
        floor = med["iii"] + 2.0 * med["iv"]
        for k in ("i", "ii"):
            margin = max(spread[k], spread["iii"], spread["iv"])
            ok = med[k] <= floor + margin
            failed = failed or not ok
            say("%s (%s) / (iii) = %.3f (byte model: 1.000);  (%s) %.4f against (iii) + 2 (iv) = %.4f ms; run-to-run spread (%s) %.4f, (iii) %.4f, (iv) %.4f ms: %s"
                % (prec, k, med[k] / med["iii"], k, med[k], floor, k, spread[k], spread["iii"], spread["iv"], "PASS" if ok else "FAIL"))
        del r, l, t
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
