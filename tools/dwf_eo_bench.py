"""The even-odd domain-wall kernels and solve (csrc/qmg_dwf_eo.hip, DwfBase) against what the project had before them.

  1. Kernel K (qmg_dwf_hops_inv5, QMG_P_EO | QMG_P_ZERO_E) against kernel D on the same pieces (qmg_dwf_apply_direct: the same bytes without the
     exchange along s) at 2048^2, Ls = 8, in fp64 and fp32.  Reported, not a gate.  Device events around `--iters` calls per timing; the legs
     alternate inside one process for `--rounds` rounds after a warm-up of every leg; median [min .. max].
  2. The solve: drivers/dwf_eo_selftest 256 8 0.05 7 <rounds> -- minv_dwf_eo_cg against the parent's minv_vector_cg on apply_stencil_2D_M_dagger_M
     on the same right-hand side to the same true residual on D, timed alternately in one process (wall clock, the dagger stencil and D^dagger b
     made before the clock starts).  Acceptance: the even-odd solve takes at most a quarter of the parent's time; the exit status is 1 otherwise.
     The driver runs under a time limit; if it fails, times out or prints no timings the tool stops there with exit status 1.

    python tools/dwf_eo_bench.py [--L 2048] [--Ls 8] [--Lsolve 256] [--iters 20] [--rounds 7] [--out profiles/dwf_eo_bench.txt]
"""
import argparse
import importlib
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

qmg = importlib.import_module("quantum-mg_amd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=2048)
    ap.add_argument("--Ls", type=int, default=8)
    ap.add_argument("--Lsolve", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--solve-timeout", type=int, default=300, help="seconds the solve driver may take")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    fmt = lambda v: "%.4f [%.4f .. %.4f]" % (float(np.median(v)), min(v), max(v))

    # ---- 2. the solve, in a process of its own (run first: the kernel legs below hold 3 GiB)
    exe = os.path.join(qmg.HERE, "drivers", "dwf_eo_selftest")
    # the child gets a time limit sized to its work (about 10 s at the defaults); if it fails, times out or prints no timings, nothing
    # more is started on the GPU
    try:
        child = subprocess.run([exe, str(a.Lsolve), str(a.Ls), "0.05", "7", str(a.rounds)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True,
                               timeout=a.solve_timeout)
    except subprocess.TimeoutExpired as e:
        print("dwf_eo_selftest did not finish within %d s; stopping before any further GPU work\n%s" % (a.solve_timeout, e.stdout or ""), flush=True)
        return 1
    out = child.stdout
    if child.returncode != 0 or "[QMG-DWF-EO-BENCH] " not in out:
        print("dwf_eo_selftest returned %d%s; stopping before any further GPU work\n%s"
              % (child.returncode, "" if "[QMG-DWF-EO-BENCH] " in out else " and printed no timing lines", out), flush=True)
        return 1
    checks, eo_ms, full_ms = {}, [], []
    for ln in out.splitlines():
        w = ln.split()
        if ln.startswith("[QMG-DWF-EO] "):
            checks[w[1]] = (float(w[2]), w[3])
        elif ln.startswith("[QMG-DWF-EO-BENCH] "):
            eo_ms.append(float(w[4])); full_ms.append(float(w[6]))
    say("# solve D x = b at %d^2, Ls = %d, m = 0.05, Gaussian links of width 0.4: CG on M^dagger M of the even-odd Schur complement from the links" % (a.Lsolve, a.Ls))
    say("# (minv_dwf_eo_cg) against CG on D^dagger D through the stored dagger stencil (minv_vector_cg on apply_stencil_2D_M_dagger_M); %d alternating rounds, wall clock" % a.rounds)
    failed = any(v[1] != "PASS" for v in checks.values())
    for name in ("eo_iterations", "full_iterations", "eo_true_residual", "full_true_residual", "eo_vs_full_solution"):
        if name in checks:
            say("%-22s %.6g %s" % (name, checks[name][0], checks[name][1]))
    factor = float(np.median(full_ms)) / float(np.median(eo_ms))
    ok = 4.0 * float(np.median(eo_ms)) <= float(np.median(full_ms))
    failed = failed or not ok
    say("even-odd solve   %s ms" % fmt(eo_ms))
    say("full solve       %s ms" % fmt(full_ms))
    say("full / even-odd = %.2f (bar: >= 4): %s" % (factor, "PASS" if ok else "FAIL"))
    if "eo_iterations" in checks and "full_iterations" in checks:
        say("per iteration: even-odd %.4f ms, full %.4f ms" % (float(np.median(eo_ms)) / checks["eo_iterations"][0], float(np.median(full_ms)) / checks["full_iterations"][0]))

    # ---- 1. kernel K against kernel D
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
    mass, M5 = 0.05, -1.0
    pieces = qmg.P_EO | qmg.P_ZERO_E
    rng = np.random.default_rng(1)
    g = qmg.DeviceArray.from_host(np.exp(1j * 0.4 * rng.standard_normal(2 * vol)))
    g32 = qmg.DeviceArray(2 * vol, np.complex64)
    qmg.convert(g32, qmg.C32, g, qmg.C64, 2 * vol)
    say("# kernel K (hops + A^-1, one parity) against kernel D (hops, one parity) at %d^2, Ls = %d; %d calls per timing, %d alternating rounds; median [min .. max] ms" % (L, Ls, a.iters, a.rounds))
    for prec, dt, npt, esz in (("fp64", qmg.C64, np.complex128, 16), ("fp32", qmg.C32, np.complex64, 8)):
        gauge = g if dt == qmg.C64 else g32
        r, l = qmg.DeviceArray(vol * nc, npt), qmg.DeviceArray(vol * nc, npt)
        tmp = qmg.DeviceArray(vol * nc)
        qmg.gaussian(tmp, vol * nc, 5)
        qmg.convert(r, dt, tmp, qmg.C64, vol * nc)
        del tmp
        d = qmg.make_desc(L, L, nc, None, None, M5)
        legs = (("K", lambda: qmg.dwf_hops_inv5(dt, d, gauge, Ls, mass, l, r, pieces, 1.0, 0, 1.0)),
                ("D", lambda: qmg.dwf_apply_direct(dt, d, gauge, Ls, mass, l, r, pieces, 1.0)),
                ("I", lambda: qmg.dwf_inv5(dt, d, Ls, mass, l, r, qmg.P_CLOVER_E, 1.0, 1.0)))
        for _, fn in legs:
            for _ in range(3):
                fn()
        times = {name: [] for name, _ in legs}
        for _ in range(a.rounds):
            for name, fn in legs:
                times[name].append(timed(fn))
        model = (2 * esz * Ls + esz) * vol          # per even site: vector in (four neighbours' chunks, each read once over the lattice), out, links
        for name, what in (("K", "kernel K"), ("D", "kernel D"), ("I", "kernel I")):
            mdl = model if name != "I" else 2 * esz * Ls * vol
            say("%s %s  %s ms  %7.1f GB/s on %d B per processed site" % (prec, what, fmt(times[name]), mdl / float(np.median(times[name])) / 1e6, 2 * mdl // vol))
        say("%s K / D = %.3f (byte model: 1.000)" % (prec, float(np.median(times["K"])) / float(np.median(times["D"]))))
        del r, l
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
