"""CPU-side checks of the scalar recurrence of the multi-shift CG (qmg::cgm_coefficients, include/qmg/krylov.hpp), compiled with g++
against the header (tests/host/multishift_host.cpp) and driven on a dense Hermitian positive definite matrix, against numpy.linalg.solve
and against the true residuals of every shift at every iteration.  The bars come from a pure-numpy twin of the same recurrence, written
here independently in Jegerlehner's notation (hep-lat/9612014: beta_n = -alpha_CG, alpha_n = beta_CG), run on the same inputs."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, EPS, MAX_ITER = 40, 1e-12, 400
SHIFTS = [0.0, 0.01, 0.1, 1.0, 10.0]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("multishift") / "multishift_host")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-o", out, os.path.join(ROOT, "tests", "host", "multishift_host.cpp")])
    return out


def system(seed, shifts):
    """dense Hermitian positive definite A with condition number 1e3 (eigenvalues log-spaced in [1e-3, 1] x 5), gaussian b"""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N)))
    lam = 5.0 * np.logspace(-3, 0, N)
    A = (Q * lam[None, :]) @ Q.conj().T
    A = 0.5 * (A + A.conj().T)
    b = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    return A, b, np.asarray(shifts, dtype=np.float64)


def run_host(exe, tmp_path, A, b, shifts):
    ns = len(shifts)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([N, ns, MAX_ITER], dtype=np.int32).tobytes())
        f.write(np.float64(EPS).tobytes())
        f.write(shifts.tobytes())
        f.write(np.ascontiguousarray(A, dtype=np.complex128).tobytes())
        f.write(np.ascontiguousarray(b, dtype=np.complex128).tobytes())
    subprocess.check_call([exe, fin, fout], timeout=120)
    raw = open(fout, "rb").read()
    iters = int(np.frombuffer(raw, dtype=np.int32, count=1)[0])
    rec = 4 + 8 * ns + 16 * N + 16 * N * ns
    assert len(raw) == 4 + iters * rec
    steps = []
    for it in range(iters):
        o = 4 + it * rec
        mask = int(np.frombuffer(raw, dtype=np.uint32, count=1, offset=o)[0])
        zeta = np.frombuffer(raw, dtype=np.float64, count=ns, offset=o + 4)
        r = np.frombuffer(raw, dtype=np.complex128, count=N, offset=o + 4 + 8 * ns)
        x = np.frombuffer(raw, dtype=np.complex128, count=N * ns, offset=o + 4 + 8 * ns + 16 * N).reshape(ns, N)
        steps.append((mask, zeta, r, x))
    return steps


def numpy_twin(A, b, shifts):
    """the same algorithm in Jegerlehner's variables; same record per iteration as the host program writes"""
    ns = len(shifts)
    base = int(np.argmin(shifts))
    s0 = shifts[base]
    xs = [np.zeros_like(b) for _ in range(ns)]
    ps = [b.copy() for _ in range(ns)]
    r = b.copy()
    rs = np.vdot(r, r).real
    bn = np.sqrt(rs)
    z_old, z, b_old, a_old = np.ones(ns), np.ones(ns), 1.0, 0.0
    live = [True] * ns
    steps = []
    while len(steps) < MAX_ITER and live[base]:
        p = ps[base]
        Ap = A @ p + s0 * p
        be = -rs / np.vdot(p, Ap).real
        zn, bes = z.copy(), np.zeros(ns)
        mask = sum(1 << s for s in range(ns) if live[s])
        for s in range(ns):
            if live[s]:
                ds = shifts[s] - s0
                zn[s] = z[s] * z_old[s] * b_old / (be * a_old * (z_old[s] - z[s]) + z_old[s] * b_old * (1.0 - ds * be))
                bes[s] = be * zn[s] / z[s]
                xs[s] = xs[s] - bes[s] * ps[s]
        r = r + be * Ap
        rn = np.vdot(r, r).real
        al = rn / rs
        for s in range(ns):
            if live[s]:
                ps[s] = zn[s] * r + al * zn[s] * bes[s] / (z[s] * be) * ps[s]
        z_old = np.where(live, z, z_old)
        z = zn
        b_old, a_old, rs = be, al, rn
        for s in range(ns):
            if live[s] and abs(z[s]) * np.sqrt(rs) < EPS * bn:
                live[s] = False
        steps.append((mask, z.copy(), r.copy(), np.array(xs)))
    return steps


def errors(A, b, shifts, steps):
    """(worst relative distance of the final iterates from numpy.linalg.solve, worst |zeta_s r - (b - (A + sigma_s) x_s)| / |b| over every
    iteration and every shift iterated in it, the iteration at which each shift stopped)"""
    ns, bn = len(shifts), np.linalg.norm(b)
    res, stopped = 0.0, [0] * ns
    for it, (mask, zeta, r, x) in enumerate(steps):
        for s in range(ns):
            if (mask >> s) & 1:
                stopped[s] = it + 1
                true = b - (A @ x[s] + shifts[s] * x[s])
                res = max(res, np.linalg.norm(zeta[s] * r - true) / bn)
    final = steps[-1][3]
    sol = 0.0
    for s in range(ns):
        want = np.linalg.solve(A + shifts[s] * np.eye(N), b)
        sol = max(sol, np.linalg.norm(final[s] - want) / np.linalg.norm(want))
    return sol, res, stopped


@pytest.mark.parametrize("seed,shifts", [(11, SHIFTS), (12, SHIFTS[::-1]), (13, [1.0, 0.0, 10.0, 0.01, 0.1])])
def test_multishift_recurrence_against_solve_and_true_residuals(exe, tmp_path, seed, shifts):
    """Bars: 10x what the numpy twin of the recurrence reaches on the same system (the reduction order differs between numpy and the C++
    loops).  Measured for the twin (seeds 11 / 12 / 13): distance from numpy.linalg.solve 5.7e-13 / 5.5e-13 / 6.2e-13,
    recurrence-vs-true residual 2.6e-14 / 5.7e-14 / 4.0e-14; the C++ recurrence: 6.0e-13 / 5.7e-13 / 6.2e-13 and 2.9e-14 / 6.1e-14 / 2.7e-14.
    (The smallest shift needs about 80 iterations at n = 40: CG is past its exact-arithmetic termination, so the iteration at which a shift
    stops moves by a few between the two implementations and is not compared.)"""
    A, b, sig = system(seed, shifts)
    host = run_host(exe, tmp_path, A, b, sig)
    twin = numpy_twin(A, b, sig)
    sol_h, res_h, stop_h = errors(A, b, sig, host)
    sol_t, res_t, stop_t = errors(A, b, sig, twin)
    print("twin: solve %.3e residual %.3e stopped %s | host: solve %.3e residual %.3e stopped %s" % (sol_t, res_t, stop_t, sol_h, res_h, stop_h))
    assert len(host) < MAX_ITER and all(s > 0 for s in stop_h)                 # every shift converged
    order = np.argsort(sig)
    assert all(stop_h[order[i]] >= stop_h[order[i + 1]] for i in range(len(sig) - 1))   # larger shifts freeze no later
    assert sol_h <= 10.0 * sol_t
    assert res_h <= 10.0 * res_t


def test_single_shift_is_plain_cg(exe, tmp_path):
    """one shift: zeta stays exactly 1 and the iterates are those of CG on A + sigma"""
    A, b, sig = system(21, [0.3])
    host = run_host(exe, tmp_path, A, b, sig)
    assert all(z[0] == 1.0 for _, z, _, _ in host)
    M = A + 0.3 * np.eye(N)
    x, r = np.zeros_like(b), b.copy()
    p, rs = r.copy(), np.vdot(b, b).real
    for _, _, rh, xh in host:
        Ap = M @ p
        a = rs / np.vdot(p, Ap).real
        x, r = x + a * p, r - a * Ap
        rn = np.vdot(r, r).real
        p, rs = r + rn / rs * p, rn
    assert np.linalg.norm(host[-1][3][0] - x) <= 1e-10 * np.linalg.norm(x)
    want = np.linalg.solve(M, b)
    assert np.linalg.norm(host[-1][3][0] - want) <= 1e-10 * np.linalg.norm(want)


def test_frozen_shift_is_left_alone(exe, tmp_path):
    """after a shift has frozen its iterate does not change again (its zeta stays where it was)"""
    A, b, sig = system(31, SHIFTS)
    host = run_host(exe, tmp_path, A, b, sig)
    for s in range(len(sig)):
        last = max(it for it, (mask, _, _, _) in enumerate(host) if (mask >> s) & 1)
        for it in range(last + 1, len(host)):
            assert np.array_equal(host[it][3][s], host[last][3][s]) and host[it][1][s] == host[last][1][s]


def test_cgm_update_symbol_is_declared_bound_and_exported():
    """qmg_batch_cgm_update_t: in include/qmg_hip.h, in the binding's symbol list, and exported by the cross-compiled library"""
    import importlib
    qmg = importlib.import_module("quantum-mg_amd")
    header = open(os.path.join(ROOT, "include", "qmg_hip.h")).read()
    assert "int qmg_batch_cgm_update_t(" in header
    assert "qmg_batch_cgm_update_t" in qmg.ABI_SYMBOLS
    qmg.build()
    assert hasattr(qmg.lib(), "qmg_batch_cgm_update_t")
