"""The domain-wall kick (qmg_hmc_momentum_update_dwf, csrc/qmg_hmc.hip) at 2048^2, Ls = 8, two pairs, against what the library could do
without it:
  (i)   the fused kernel on two pairs of five-dimensional vectors (interleaved slices, c = 2 s + sigma): 64 + 64 Ls n = 1088 B/site;
  (ii)  qmg_hmc_momentum_update_poles on 2 Ls = 16 separate nc = 2 vector pairs: the same 1088 B/site, in one launch;
  (iii) qmg_copy_vector of the four five-dimensional vectors: the least that a slice-unpacking pass in front of (ii) would cost.
Device events around `--iters` calls per timing; the legs alternate inside one process for `--rounds` rounds after a warm-up of every leg, and the
spread over the rounds is printed next to the median.  Acceptance: (i) <= (ii) + (iii); the exit status is 1 otherwise.  (i) / (ii) is reported
without a gate.  Then one trajectory's kernels at 32^2 (--Lsmall), Ls = 8: the operator applies of the solves, the odd-half fills and the kicks.

    python tools/dwf_hmc_force_bench.py [--L 2048] [--Ls 8] [--iters 10] [--rounds 7] [--out profiles/dwf_hmc_force_bench.txt]
"""
import argparse
import importlib
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

qmg = importlib.import_module("quantum-mg_amd")
COPY_CEILING_GBS = 6205.4      # profiles/r01_membw_ceiling.txt: streaming copy at 262 144 blocks
DRIVERS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "quantum-mg_amd", "drivers")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=2048)
    ap.add_argument("--Ls", type=int, default=8)
    ap.add_argument("--Lsmall", type=int, default=32)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    qmg.init(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    timer = qmg.Timer()

    def timed(fn, iters):
        qmg.sync()
        timer.start()
        for _ in range(iters):
            fn()
        return timer.stop_ms() / iters

    L, Ls, n = a.L, a.Ls, 2
    vol, cv5 = L * L, 2 * a.Ls * L * L
    rng = np.random.default_rng(1)
    g = qmg.DeviceArray.from_host(np.exp(1j * 0.4 * rng.standard_normal(2 * vol)))
    pi = qmg.DeviceArray(2 * vol, np.float64)
    qmg.hmc_momentum_refresh(pi, 2 * vol, 3, 0)
    vec = [qmg.DeviceArray(cv5) for _ in range(4)]       # X[0], X[1], Y[0], Y[1]: as five-dimensional vectors, or as Ls nc = 2 vectors each
    dst = [qmg.DeviceArray(cv5) for _ in range(4)]
    for k, v in enumerate(vec):
        qmg.gaussian(v, cv5, 10 + k)
    w = [1.0, -1.0]
    xs = [vec[j].offset(2 * vol * s) for j in range(n) for s in range(Ls)]
    ys = [vec[2 + j].offset(2 * vol * s) for j in range(n) for s in range(Ls)]
    ws = [w[j] for j in range(n) for s in range(Ls)]

    def leg_fused():
        qmg.hmc_momentum_update_dwf(pi, g, vec[:2], vec[2:], w, Ls, L, L, 6.0, 1e-3, qmg.HMC_DWF_G5_Y)

    def leg_poles():
        qmg.hmc_momentum_update_poles(pi, g, xs, ys, ws, L, L, 6.0, 1e-3)

    def leg_copy():
        for k in range(4):
            qmg.copy_vector(dst[k], vec[k], cv5)

    say("# domain-wall kick at %d^2, Ls = %d, %d pairs: (i) the fused kernel, (ii) %d poles of nc = 2 through qmg_hmc_momentum_update_poles, (iii) copy of the 4 vectors"
        % (L, Ls, n, n * Ls))
    say("# %d calls per timing, %d alternating rounds; median [min .. max] ms" % (a.iters, a.rounds))
    legs = (("i", leg_fused), ("ii", leg_poles), ("iii", leg_copy))
    for _, fn in legs:
        for _ in range(3):
            fn()
    times = {name: [] for name, _ in legs}
    for _ in range(a.rounds):
        for name, fn in legs:
            times[name].append(timed(fn, a.iters))
    med = {k: float(np.median(v)) for k, v in times.items()}
    model = (64 + 64 * Ls * n) * vol
    cmodel = 2 * 4 * 16 * cv5
    for name, what, bytes_ in (("i", "fused kernel", model), ("ii", "%d poles" % (n * Ls), model), ("iii", "copy of 4 vectors", cmodel)):
        gbs = bytes_ / med[name] / 1e6
        say("(%s) %-18s %.4f [%.4f .. %.4f] ms  %7.1f GB/s on %d B/site  %.3f of the %.1f TB/s copy ceiling"
            % (name, what, med[name], min(times[name]), max(times[name]), gbs, bytes_ // vol, gbs / COPY_CEILING_GBS, COPY_CEILING_GBS / 1e3))
    ok = med["i"] <= med["ii"] + med["iii"]
    say("(i) <= (ii) + (iii): %.4f <= %.4f ms: %s" % (med["i"], med["ii"] + med["iii"], "PASS" if ok else "FAIL"))
    say("(i) / (ii) = %.3f (reported, no gate)" % (med["i"] / med["ii"]))
    for d in vec + dst + [g, pi]:
        d.free()

    # ---- one trajectory at Lsmall^2: the launches of the solves' operator, of the odd-half fills and of the kicks ----
    Lp = a.Lsmall
    volp, cvp = Lp * Lp, 2 * Ls * Lp * Lp
    steps, mass = 10, 0.2
    gp = qmg.DeviceArray.from_host(np.exp(1j * 0.4 * rng.standard_normal(2 * volp)))
    pip = qmg.DeviceArray(2 * volp, np.float64)
    qmg.hmc_momentum_refresh(pip, 2 * volp, 3, 0)
    v = [qmg.DeviceArray(cvp) for _ in range(6)]
    for k in range(6):
        qmg.gaussian(v[k], cvp, 20 + k)
    d = qmg.make_desc(Lp, Lp, 2 * Ls, None, None, -1.0)

    def mdag_m():
        qmg.dwf_schur_apply(qmg.C64, d, gp, Ls, mass, v[1], v[0], v[5], 0, 0)
        qmg.dwf_schur_apply(qmg.C64, d, gp, Ls, mass, v[2], v[1], v[5], 0, qmg.DWF_G5_IN | qmg.DWF_G5_OUT)

    def fills():
        for k in range(4):
            qmg.dwf_hops_inv5(qmg.C64, d, gp, Ls, mass if k < 2 else 1.0, v[k], v[k], qmg.P_OE | qmg.P_ZERO_O, -1.0)

    def kick():
        qmg.hmc_momentum_update_dwf(pip, gp, [v[0], v[2]], [v[1], v[3]], w, Ls, Lp, Lp, 2.0, 1e-3, qmg.HMC_DWF_G5_Y)

    for fn in (mdag_m, fills, kick):
        for _ in range(3):
            fn()
    t_op, t_fill, t_kick = (float(np.median([timed(fn, 50) for _ in range(a.rounds)])) for fn in (mdag_m, fills, kick))
    run = subprocess.run([os.path.join(DRIVERS, "dwf_hmc")] + [str(x) for x in (Lp, Ls, 2.0, mass, 2, 4, 2, steps, 7)], stdout=subprocess.PIPE, universal_newlines=True)
    cg = [int(m.group(1)) for m in re.finditer(r"\[HMC\] \d+ dH \S+ acc \d plaq \S+ Q \S+ cg (\d+)", run.stdout)][2:]
    if cg:
        it = float(np.mean(cg))
        # md_evolve: a solve at the start and one per step (the last one is the end point's action), a kick after each: steps + 1 of either
        parts = (("solves: M^dag M applies of the CG", it * t_op), ("odd-half fills (4 per force)", (steps + 1) * t_fill), ("kicks", (steps + 1) * t_kick))
        total = sum(p[1] for p in parts)
        say("# one trajectory at %d^2, Ls = %d, m = %.1f, %d steps: %.0f CG iterations (mean of %d trajectories through dwf_hmc); device time of the launches, per call %.4f / %.4f / %.4f ms"
            % (Lp, Ls, mass, steps, it, len(cg), t_op, t_fill, t_kick))
        for what, ms in parts:
            say("%-40s %8.3f ms  %5.1f %%" % (what, ms, 100.0 * ms / total))
        say("# the CG's vector updates and reductions are not in this split")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
