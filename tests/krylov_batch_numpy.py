"""The independent reference of the lock-step Krylov cores on UNEVEN batches (numpy only; drivers/krylov_batch_parity.cpp runs
the cores, tests/test_host_krylov_batch.py pins this module, tests/test_gpu_krylov_batch.py holds the device to it).

Operators: dense matrices built column by column from coordspace.wilson_apply / laplace_apply on U(1) links drawn here, in the
even-odd storage order of the device vectors.  The smallest shapes the project uses where a row is shorter than a wavefront and Lx != Ly:
  wilson16      16 x 16, nc = 2, n = 512   M,         cond_2 <= 10  (so that the normal operator below keeps cond_2 <= 100); BiCGStab(L)
  wilson16f     the same operator with another guess for slot 5 (GUESS5); GCR
  normal16      the same lattice           M^dag M,   cond_2 <= 100 (CG wants a Hermitian positive definite operator)
  laplace34x10  34 x 10, nc = 1, n = 340   Laplace + m^2, Hermitian positive definite, cond_2 <= 100

The six systems of a batch (`rhs_sets`): slot 0 gaussian; 1 identically zero; 2 gaussian (masked out in the 0x3B runs); 3 A v with v as
initial guess in the guess runs (converged at iteration 0) and the sum of the four eigenvectors of largest |lambda| in the zero-guess runs (a
Krylov space of dimension 4: done within a few iterations; a point source makes BiCGStab break down at once on the Wilson operator, whose
forward and backward hops carry orthogonal spin projectors); 4 = 2^-40 times slot 0 with 2^-40 times its guess (exact scale covariance); 5 a
gaussian vector with its left singular components weighted by (sigma / sigma_min)^-4, started in the guess runs from a guess far from the
solution (GUESS5; the slow system: a relative criterion cannot be made much slower than on a gaussian vector by the shape of b alone, so the
zero-guess runs are slower by a few iterations and the guess runs by many; on wilson16 the guess is a head start instead, see GUESS5).
MR(0.85) has to converge within its 60 iterations, so it runs on the same links at a heavier mass (wilson16h, cond_2 = 3).

Two bars, neither from a measured number:
  true residual   |b - A x| <= 1.5 eps |b|            for every system reported `success` (the bar of tests/test_gpu_krylov.py)
  error           |x - x_ref| <= (1 + 1e-6) |b - A x| / sigma_min     from x - x_ref = A^-1 r; 1e-6 covers the rounding of the numpy
                                                                      residual itself (n <= 512 in complex128) and of x_ref
                  plus the floor n 2^-53 |A| |x| / sigma_min: the absolute rounding of that residual, which a factor cannot cover where
                  r itself is at rounding level (slot 3 from its exact guess); ~1e-11 here, three orders under the bar of any iterated system
"""
import os
import re
from collections import namedtuple

import numpy as np

import coordspace as cs

NRHS = 6
FULL, PARTIAL = 0x3F, 0x3B      # every run under both: 0x3B masks slot 2 out
STRIDE_PAD = 37                 # second pass: systems n + 37 complex numbers apart (odd: complex<float> systems on 8-byte boundaries)
EPS = {"f64": 1e-9, "f32": 1e-3}
UNIT = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
COND_MAX = 100.0
SCALE = 2.0 ** -40
OMEGA = 0.85
NP_DTYPE = {"f64": np.complex128, "f32": np.complex64}

Operator = namedtuple("Operator", "name kind Lx Ly nc n mass phases A smin smax hermitian")

WILSON_MASS, WILSON_HEAVY_MASS, LAPLACE_MSQ, LINK_SPREAD = 0.2, 0.7, 0.12, 0.6
LOW_MODE_POWER, FAST_VECTORS = 4, 4
# slot 5 in the guess runs.  "far": G times a gaussian vector, the opening residual hundreds of times |b| (many more iterations).  "head": the
# dense solution of b - G |b| g/|g|, the opening residual G |b| (a head start).  BiCGStab(6) in float loses the true residual when x starts
# hundreds of times larger than the solution (no true-residual confirmation, unlike GCR and restarted CG), and a guess small enough for it
# leaves slot 5 where slot 0 stops; so its operator takes the head start.  Every G keeps 2^-24 |A| |x0| / |b| <= 0.05 eps (FP32_PREMISE).
GUESS5 = {"wilson16": ("head", 0.03), "wilson16f": ("far", 10.0), "wilson16h": ("far", 10.0), "laplace34x10": ("far", 10.0), "normal16": ("far", 1.5)}
FP32_PREMISE = 0.05


def draw_phases(Lx, Ly, seed):
    """U(1) link phases, file order x outer, y, mu inner (tests/golden/*.dat)."""
    return LINK_SPREAD * np.random.default_rng(seed).standard_normal(2 * Lx * Ly)


def dense_from_apply(apply, Lx, Ly, nc):
    """A[:, j] = apply(e_j), both sides in the even-odd order of the device vectors."""
    n = Lx * Ly * nc
    A = np.zeros((n, n), dtype=np.complex128)
    e = np.zeros(n, dtype=np.complex128)
    for j in range(n):
        e[j] = 1.0
        A[:, j] = cs.grid_to_eo(apply(cs.eo_to_grid(e, Lx, Ly, nc)), Lx, Ly, nc)
        e[j] = 0.0
    return A


_OPS = {}


def operators():
    """name -> Operator, built once."""
    if _OPS:
        return _OPS
    ph = draw_phases(16, 16, 1601)
    Ux, Uy = cs.phases_to_links(ph, 16, 16)
    M = dense_from_apply(lambda psi: cs.wilson_apply(psi, Ux, Uy, WILSON_MASS), 16, 16, 2)
    s = np.linalg.svd(M, compute_uv=False)
    _OPS["wilson16"] = Operator("wilson16", "wilson", 16, 16, 2, 512, WILSON_MASS, ph, M, s[-1], s[0], False)
    _OPS["wilson16f"] = _OPS["wilson16"]._replace(name="wilson16f")   # the same operator; its slot 5 starts from a far guess (GUESS5)
    Mh = dense_from_apply(lambda psi: cs.wilson_apply(psi, Ux, Uy, WILSON_HEAVY_MASS), 16, 16, 2)
    sh = np.linalg.svd(Mh, compute_uv=False)
    _OPS["wilson16h"] = Operator("wilson16h", "wilson", 16, 16, 2, 512, WILSON_HEAVY_MASS, ph, Mh, sh[-1], sh[0], False)
    N = M.conj().T @ M
    _OPS["normal16"] = Operator("normal16", "normal", 16, 16, 2, 512, WILSON_MASS, ph, N, s[-1] ** 2, s[0] ** 2, True)
    ph = draw_phases(34, 10, 3410)
    Ux, Uy = cs.phases_to_links(ph, 34, 10)
    Lp = dense_from_apply(lambda psi: cs.laplace_apply(psi, Ux, Uy, LAPLACE_MSQ), 34, 10, 1)
    s = np.linalg.svd(Lp, compute_uv=False)
    _OPS["laplace34x10"] = Operator("laplace34x10", "laplace", 34, 10, 1, 340, LAPLACE_MSQ, ph, Lp, s[-1], s[0], True)
    return _OPS


_SETS = {}


def rhs_sets(op, seed=77):
    """(b0, bg, g): right-hand sides of the zero-guess runs, of the guess runs, and the guesses; each NRHS x n.  Built once: read-only."""
    if (op.name, seed) not in _SETS:
        _SETS[(op.name, seed)] = _rhs_sets(op, seed)
        for a in _SETS[(op.name, seed)]:
            a.setflags(write=False)
    return _SETS[(op.name, seed)]


def _rhs_sets(op, seed):
    n = op.n
    rng = np.random.default_rng(seed + n)
    gauss = lambda: rng.standard_normal(n) + 1j * rng.standard_normal(n)
    b0 = np.zeros((NRHS, n), dtype=np.complex128)
    b0[0], b0[2] = gauss(), gauss()
    lam, V = np.linalg.eig(op.A)
    b0[3] = V[:, np.argsort(-np.abs(lam))[:FAST_VECTORS]].sum(axis=1)
    gauss()   # (one draw skipped, so that the later slots do not depend on how slot 3 is built)
    u, sv = np.linalg.svd(op.A)[:2]
    b0[5] = u @ ((sv / sv[-1]) ** -LOW_MODE_POWER * (u.conj().T @ gauss()))
    b0[4] = SCALE * b0[0]
    bg = b0.copy()
    g = np.zeros_like(b0)
    g[0], g[1], g[2] = gauss(), gauss(), gauss()
    g[3] = gauss()
    bg[3] = op.A @ g[3]
    g[4] = SCALE * g[0]
    kind, G = GUESS5[op.name]
    g[5] = G * gauss()
    if kind == "head":
        g[5] = dense_solution(op.A, b0[5] - G * np.linalg.norm(b0[5]) * g[5] / np.linalg.norm(g[5]))
    return b0, bg, g


def dense_solution(A, b):
    """np.linalg.solve and two refinement steps whose residuals are formed in extended precision."""
    x = np.linalg.solve(A, b)
    Al, bl = A.astype(np.clongdouble), b.astype(np.clongdouble)
    for _ in range(2):
        r = (bl - Al @ x.astype(np.clongdouble)).astype(np.complex128)
        x = x + np.linalg.solve(A, r)
    return x


def residual_norm(A, x, b):
    return float(np.linalg.norm(b - A @ x))


def check_bars(op, x, b, eps, x_ref=None):
    """the two derived bars for a system reported `success`; returns (relative residual, error, error bound)"""
    bn = float(np.linalg.norm(b))
    r = residual_norm(op.A, x, b)
    assert r <= 1.5 * eps * bn, ("true residual", r / bn, 1.5 * eps)
    x_ref = dense_solution(op.A, b) if x_ref is None else x_ref
    err = float(np.linalg.norm(x - x_ref))
    floor = op.n * UNIT["f64"] * op.smax * float(np.linalg.norm(x)) / op.smin
    assert err <= (1.0 + 1e-6) * r / op.smin + floor, ("error", err, r / op.smin, floor)
    return r / max(bn, 1e-300), err, r / op.smin


# ---------------------------------------------------------------------------------------------------------------------
# numpy twins of the two solver forms the CPU oracle has no twin for (dense A, one system): restarted CG and flexible GCR
# with 4 MR(omega) steps as preconditioner.  Textbook statements; they serve iteration counts and the unevenness condition.
# ---------------------------------------------------------------------------------------------------------------------
def cg_restart_dense(A, b, x0, max_iter, tol, restart):
    x = np.zeros_like(b) if x0 is None else x0.copy()
    bn = np.linalg.norm(b)
    if bn == 0.0:
        return True, 0, np.zeros_like(b), 0.0
    k, conv, rsq = 0, False, 0.0
    while k < max_iter or k == 0:
        chunk = min(restart, max_iter - k) if restart > 0 else max_iter - k
        r = b - A @ x
        p = r.copy()
        rsq = np.vdot(r, r).real
        conv = np.sqrt(rsq) < tol * bn
        j = 0
        while not conv and j < chunk:
            Ap = A @ p
            alpha = rsq / np.vdot(p, Ap).real
            x += alpha * p
            r -= alpha * Ap
            rn = np.vdot(r, r).real
            j += 1
            if np.sqrt(rn) < tol * bn:
                rsq, conv = rn, True
                break
            p = r + (rn / rsq) * p
            rsq = rn
        k += j
        if conv or j == 0:
            break
    return conv, k, x, rsq


def mr_dense(A, b, iters, omega):
    x, r = np.zeros_like(b), b.copy()
    for _ in range(iters):
        p = A @ r
        pp = np.vdot(p, p).real
        if pp == 0.0:
            break
        alpha = omega * np.vdot(p, r) / pp
        x += alpha * r
        r = r - alpha * p
    return x


def fgcr_dense(A, b, x0, max_iter, tol, restart, precond):
    x = np.zeros_like(b) if x0 is None else x0.copy()
    bn = np.linalg.norm(b)
    if bn == 0.0:
        return True, 0, np.zeros_like(b), 0.0
    r = b - A @ x
    rsq = np.vdot(r, r).real
    conv = np.sqrt(rsq) < tol * bn
    basis_max = restart if restart > 0 else max_iter
    Z, W, k = [], [], 0
    while not conv and k < max_iter:
        z = precond(r)
        w = A @ z
        for zi, wi in zip(Z, W):
            beta = np.vdot(wi, w) / np.vdot(wi, wi).real
            w = w - beta * wi
            z = z - beta * zi
        ww = np.vdot(w, w).real
        if ww == 0.0:
            break
        alpha = np.vdot(w, r) / ww
        x += alpha * z
        r = r - alpha * w
        rsq = np.vdot(r, r).real
        Z.append(z); W.append(w)
        k += 1
        if np.sqrt(rsq) < tol * bn:
            conv = True
            break
        if len(Z) == basis_max:
            r = b - A @ x
            rsq = np.vdot(r, r).real
            Z, W = [], []
            if np.sqrt(rsq) < tol * bn:
                conv = True
    return conv, k, x, rsq


# ---------------------------------------------------------------------------------------------------------------------
# The cases.  core: mr | bicg | gcr | cg; op: the operator solved; guess: from the guesses or from zero; pi: L (bicg) or restart
# (gcr, cg; -1 none); flags: "pre" flexible GCR, "eps" per-system tolerances, "fixed" eps = 1e-30.  slack: iteration slack against
# the twins and against the systems alone (the slacks of tests/test_gpu_krylov.py).  max_iter < 0: filled in by `cases()`
# with the twin's iteration count of slot 0 (the CUT cases: slot 3 converges, slot 5 is cut).
# ---------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name core op guess max_iter pi pre eps_ps fixed slack converging")
EPS_FACTORS = [1.0, 1.0, 1.0, 1e2, 1.0, 1e-2]


def _case(name, core, op, guess, max_iter, pi=-1, pre=False, eps_ps=False, fixed=False, slack=1, converging=True):
    return Case(name, core, op, guess, max_iter, pi, pre, eps_ps, fixed, slack, converging)


def case_table():
    t = []
    for g in (0, 1):
        sfx = "_x0" if g else ""
        t.append(_case("mr" + sfx, "mr", "wilson16h", g, 60))
        for L in (1, 2, 6):
            t.append(_case("bicg%d%s" % (L, sfx), "bicg", "wilson16", g, 120, pi=L, slack=max(L, 1)))
        t.append(_case("gcr" + sfx, "gcr", "wilson16f", g, 120))
        t.append(_case("gcr8" + sfx, "gcr", "wilson16f", g, 200, pi=8))
        t.append(_case("gcr8eps" + sfx, "gcr", "wilson16f", g, 200, pi=8, eps_ps=True))
        t.append(_case("fgcr8" + sfx, "gcr", "wilson16f", g, 200, pi=8, pre=True))
    for op, tag, slack in (("laplace34x10", "lap", 1), ("normal16", "nrm", 2)):
        for pi in (-1, 16):
            for e in (False, True):
                t.append(_case("cg%s_%s%s" % ("" if pi < 0 else "16", tag, "eps" if e else ""), "cg", op, 0, 400, pi=pi, eps_ps=e, slack=slack))
        t.append(_case("cg16_%s_x0" % tag, "cg", op, 1, 400, pi=16, slack=slack))
    t.append(_case("mr_fixed6", "mr", "wilson16h", 0, 6, fixed=True, converging=False))
    # cut at the twin's iteration count of slot 0, and max_iter = 0, once per core
    t.append(_case("mr_cut", "mr", "wilson16h", 0, -1, converging=False))
    t.append(_case("bicg2_cut", "bicg", "wilson16", 0, -1, pi=2, slack=2, converging=False))
    t.append(_case("gcr8_cut", "gcr", "wilson16f", 0, -1, pi=8, converging=False))
    t.append(_case("cg16_lapeps_cut", "cg", "laplace34x10", 0, -1, pi=16, eps_ps=True, converging=False))
    t.append(_case("mr_zero", "mr", "wilson16h", 1, 0, converging=False))
    t.append(_case("bicg2_zero", "bicg", "wilson16", 1, 0, pi=2, slack=2, converging=False))
    t.append(_case("gcr8_zero", "gcr", "wilson16f", 1, 0, pi=8, converging=False))
    t.append(_case("cg16_lap_zero", "cg", "laplace34x10", 1, 0, pi=16, converging=False))
    return t


def case_eps(case, prec, k):
    if case.fixed:
        return 1e-30
    return EPS[prec] * (EPS_FACTORS[k] if case.eps_ps else 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# The driver's inputs and outputs (drivers/krylov_batch_parity.cpp)
# ---------------------------------------------------------------------------------------------------------------------
def write_case_dir(path, resolved):
    """resolved: [(Case, max_iter in double, max_iter in float)].  Links as text in the format of tests/golden/*.dat, vectors as complex128."""
    ops = operators()
    np.savetxt(os.path.join(path, "links_16x16.dat"), ops["wilson16"].phases, fmt="%.17g")
    np.savetxt(os.path.join(path, "links_34x10.dat"), ops["laplace34x10"].phases, fmt="%.17g")
    for name, op in ops.items():
        b0, bg, g = rhs_sets(op)
        for tag, a in (("rhs0", b0), ("rhsg", bg), ("guess", g)):
            np.ascontiguousarray(a, dtype=np.complex128).tofile(os.path.join(path, "%s_%s.bin" % (tag, name)))
    with open(os.path.join(path, "cases.txt"), "w") as f:
        f.write("masses %.17g %.17g %.17g\n" % (WILSON_MASS, WILSON_HEAVY_MASS, LAPLACE_MSQ))
        for c, m64, m32 in resolved:
            f.write("%s %s %s %d %d %d %d %d %d %d %d\n" % (c.name, c.core, c.op, c.guess, m64, m32, c.pi, int(c.pre), int(c.eps_ps), int(c.fixed), int(c.converging)))


Sys = namedtuple("Sys", "k slot success iter ops res_sq")


def parse_output(text):
    """tag -> {"sys": [Sys], "ops": [mask], "pre": [mask], "rhs": 0 | 1}"""
    runs = {}
    for line in text.splitlines():
        m = re.match(r"\[(SYS|OPS|PRE|RHS)\] (\S+)(.*)", line)
        if not m:
            continue
        run = runs.setdefault(m.group(2), {"sys": [], "ops": [], "pre": [], "rhs": None})
        rest = m.group(3).split()
        if m.group(1) == "SYS":
            run["sys"].append(Sys(int(rest[0]), int(rest[1]), bool(int(rest[2])), int(rest[3]), int(rest[4]), float(rest[5])))
        elif m.group(1) == "RHS":
            run["rhs"] = int(rest[1])
        else:
            run[m.group(1).lower()] = [int(w, 16) for w in rest]
    return runs


def nan_fill(count, dtype):
    a = np.empty(count, dtype=dtype)
    a.real, a.imag = np.nan, np.nan
    return a
