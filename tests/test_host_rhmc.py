"""CPU side of one-flavour RHMC: (i) the C++ coefficients (qmg::zolotarev_inv_sqrt, include/qmg/rational.hpp, own AGM / Landen elliptic
functions, compiled alone through tests/host/rhmc_host.cpp) against the scipy twin tests/rhmc_numpy.py and against what defines them
(equioscillation, the partial fractions, a table computed independently); (ii) the twin's dense statements -- r(Q^2) against (Q^2)^(-1/2)
from an eigendecomposition, the heatbath identity, force = derivative of the action, reversibility, the dt^2 law, the range check -- before
it judges the device in test_gpu_rhmc.py; (iii) the drop-in boundary of the new entry point."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import hmc_numpy as hn
import rhmc_numpy as rn

qmg = importlib.import_module("quantum-mg_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETA, MASS = 3.0, 0.1
RB = 4.1
GRID = 200001


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rhmc") / "rhmc_host")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-o", out, os.path.join(ROOT, "tests", "host", "rhmc_host.cpp")])
    return out


def run_host(exe, n, ra, rb):
    out = subprocess.run([exe, str(n), repr(float(ra)), repr(float(rb))], stdout=subprocess.PIPE, universal_newlines=True, timeout=60)
    kv = {}
    for line in out.stdout.splitlines():
        w = line.split()
        if w and not w[0].startswith("["):
            kv[w[0]] = np.array([float(x) for x in w[1:]])
    return out, kv


def host_rational(exe, n, ra, rb):
    out, kv = run_host(exe, n, ra, rb)
    assert out.returncode == 0 and kv["ok"][0] == 1, out.stdout
    return rn.from_coefficients(n, ra, rb, kv["c0"][0], kv["delta"][0], kv["mu2"], kv["nu2"], kv["rho"], kv["s"])


@pytest.mark.parametrize("n,eps,A,delta", rn.TABLE)
def test_cpp_coefficients_against_scipy_and_their_definition(exe, n, eps, A, delta):
    """The five (n, eps) rows of the table, rb = 4.1.  Coefficient by coefficient against scipy's ellipj / ellipk: measured over the five rows,
    the worst relative difference of any mu_j^2, nu_j^2, rho_j, s_j or c0 is 1.9e-13 (rho at n = 10; the products of up to 2n differences of
    nearby numbers amplify the last bit of the elliptic functions); the gate is ten times that, 1.9e-12.  delta is a difference of two nearly
    equal end-point values (relative 3.6e-6 at delta = 4.6e-9) and is held to the table within 1 % like the grid value."""
    rb = RB
    ra = rb * np.sqrt(eps)
    z, t = host_rational(exe, n, ra, rb), rn.zolotarev(n, ra, rb, GRID)
    worst = max(float(np.abs(getattr(z, k) / getattr(t, k) - 1.0).max()) for k in ("mu2", "nu2", "rho", "s"))
    worst = max(worst, abs(z.c0 / t.c0 - 1.0))
    y = np.exp(np.linspace(np.log(eps), 0.0, GRID))                      # the scaled variable
    err = np.sqrt(y) * rb * rn.r_product(z, rb * rb * y) - 1.0         # sqrt(y) r0(y) - 1 with the C++ numbers
    d_grid = float(np.abs(err).max())
    mismatch = float(np.abs(rb * rn.r_product(z, rb * rb * y) - rb * rn.r_poles(z, rb * rb * y)).max())
    print("n %d eps %g: A %.6f delta C++ %.4e grid %.4e twin %.4e; worst coefficient %.2e; partial fractions %.1e" % (n, eps, z.A, z.delta, d_grid, t.delta, worst, mismatch))
    assert abs(z.A / A - 1.0) < 1e-5                                     # the table has six digits
    assert abs(d_grid / delta - 1.0) < 0.01 and abs(z.delta / delta - 1.0) < 0.01 and abs(t.delta / delta - 1.0) < 0.01
    assert worst <= 1.9e-12
    assert np.all(z.rho > 0) and np.all(np.diff(z.a) < 0)               # positive residues; a_r decreasing
    assert mismatch <= 1e-12
    # equioscillation: +-delta alternately at 2n + 2 points.  The error changes sign 2n + 1 times; in each of the 2n + 2 runs of one sign its
    # peak is +-delta (a 200001-point grid misses an extremum by O(h^2), and at delta ~ 1e-9 rounding of the product adds 1e-16 / delta).
    runs = np.split(err, np.nonzero(np.diff(np.sign(err)))[0] + 1)
    assert len(runs) == 2 * n + 2
    peaks = np.array([r[np.argmax(np.abs(r))] for r in runs])
    assert np.all(np.abs(np.abs(peaks) / d_grid - 1.0) < 1e-3)
    assert np.all(np.sign(peaks[1:]) == -np.sign(peaks[:-1]))


def test_swapped_roles_are_the_classic_mistake():
    """odd and even a_r exchanged: delta of order 1, so the 1 % gates above cannot pass by accident"""
    a = rn.zolotarev_a(6, 1e-3)
    y = np.exp(np.linspace(np.log(1e-3), 0.0, 20001))
    f = np.sqrt(y) * np.prod((y[:, None] + a[1::2]) / (y[:, None] + a[0::2]), axis=-1)
    assert np.abs(2.0 / (f.max() + f.min()) * f - 1.0).max() > 0.5


def test_cpp_refuses_bad_arguments(exe):
    for n, ra, rb in ((0, 0.1, 4.0), (17, 0.1, 4.0), (4, 0.0, 4.0), (4, -1.0, 4.0), (4, 4.0, 4.0), (4, 5.0, 4.0)):
        out, kv = run_host(exe, n, ra, rb)
        assert out.returncode == 1 and kv["ok"][0] == 0 and "[QMG-ERROR]" in out.stdout, (n, ra, rb)
    out, kv = run_host(exe, 16, 0.05, 4.1)
    assert out.returncode == 0 and kv["ok"][0] == 1 and kv["mu2"].size == 16 and np.all(kv["rho"] > 0)


# ---- dense: the twin's statements on 6 x 4 and 4 x 6 ----
def setup(Lx, Ly, seed):
    rng = np.random.default_rng(seed)
    th = (0.5 * rng.standard_normal((Lx, Ly)), 0.5 * rng.standard_normal((Lx, Ly)))
    pi = (rng.standard_normal((Lx, Ly)), rng.standard_normal((Lx, Ly)))
    eta = (rng.standard_normal((Lx, Ly, 2)) + 1j * rng.standard_normal((Lx, Ly, 2))) / np.sqrt(2.0)
    lam, vec = rn.spectrum_Q2(th, MASS)
    z = rn.zolotarev(6, np.sqrt(lam[0]), np.sqrt(lam[-1]))           # ra, rb from the dense spectrum
    return th, pi, eta, z, lam, vec


@pytest.mark.parametrize("Lx,Ly", [(6, 4), (4, 6)])
def test_rational_action_is_the_inverse_square_root(Lx, Ly):
    th, _, eta, z, lam, vec = setup(Lx, Ly, 21)
    phi = rn.heatbath(z, th, eta, MASS)
    c = vec.conj().T @ phi.reshape(-1)
    exact = float(np.sum(np.abs(c) ** 2 / np.sqrt(lam)))               # phi^dag (Q^2)^(-1/2) phi
    got = rn.pf_action(z, th, phi, MASS)
    dense = float(np.vdot(phi.reshape(-1), rn.dense_r(z, th, MASS) @ phi.reshape(-1)).real)
    print("%dx%d: S_pf %.12f exact %.12f rel %.2e (delta %.2e); poles against product form %.1e" % (Lx, Ly, got, exact, abs(got - exact) / exact, z.delta, abs(got - dense) / dense))
    assert abs(got - exact) <= z.delta * exact
    assert abs(got - dense) <= 1e-11 * dense


@pytest.mark.parametrize("Lx,Ly", [(6, 4), (4, 6)])
def test_heatbath_gives_the_gaussian_weight(Lx, Ly):
    """phi = B eta with B B^dag = r^-1, so phi^dag r phi = eta^dag eta, to rounding of dense solves"""
    th, _, eta, z, _, _ = setup(Lx, Ly, 22)
    phi = rn.heatbath(z, th, eta, MASS)
    e2 = np.vdot(eta, eta).real
    got = rn.pf_action(z, th, phi, MASS)
    print("%dx%d: |S_pf - eta^2| / eta^2 = %.2e" % (Lx, Ly, abs(got - e2) / e2))
    assert abs(got - e2) <= 1e-11 * e2


@pytest.mark.parametrize("Lx,Ly", [(6, 4), (4, 6)])
def test_force_is_the_derivative_of_the_action(Lx, Ly):
    """Central differences at h = 1e-4 on every link, the 1e-6 absolute gate of test_host_hmc.py"""
    th, _, eta, z, _, _ = setup(Lx, Ly, 23)
    phi = rn.heatbath(z, th, eta, MASS)
    f = rn.force(z, th, BETA, phi, MASS)
    h, worst = 1e-4, 0.0
    for mu in range(2):
        for x in range(Lx):
            for y in range(Ly):
                up = (th[0].copy(), th[1].copy())
                dn = (th[0].copy(), th[1].copy())
                up[mu][x, y] += h
                dn[mu][x, y] -= h
                fd = (rn.action(z, up, BETA, phi, MASS) - rn.action(z, dn, BETA, phi, MASS)) / (2 * h)
                worst = max(worst, abs(fd - f[mu][x, y]))
    g = rn.pf_force(z, th, phi, MASS)
    print("%dx%d: max |F - FD| = %.2e, max |F| = %.2f, max |F_pf| = %.2f" % (Lx, Ly, worst, max(np.abs(f[0]).max(), np.abs(f[1]).max()), max(np.abs(g[0]).max(), np.abs(g[1]).max())))
    assert max(np.abs(g[0]).max(), np.abs(g[1]).max()) > 0.1
    assert worst < 1e-6


def test_leapfrog_is_reversible_and_follows_the_dt_squared_law():
    th, pi, eta, z, _, _ = setup(6, 4, 24)
    phi = rn.heatbath(z, th, eta, MASS)
    th1, pi1 = rn.leapfrog(z, th, pi, BETA, 1.0, 20, phi, MASS)
    th2, pi2 = rn.leapfrog(z, th1, (-pi1[0], -pi1[1]), BETA, 1.0, 20, phi, MASS)
    d = max(np.abs(th2[0] - th[0]).max(), np.abs(th2[1] - th[1]).max())
    dp = max(np.abs(pi2[0] + pi[0]).max(), np.abs(pi2[1] + pi[1]).max())
    dH = {n: rn.md_dH(z, th, pi, BETA, 1.0, n, phi, MASS)[2] for n in (10, 20, 40)}
    print("forward-back: phases %.2e momenta %.2e; dH over tau = 1:" % (d, dp), dH)
    assert np.abs(th1[0] - th[0]).max() > 0.1
    assert d < 1e-13 and dp < 1e-13
    assert 0.2 <= dH[40] / dH[20] <= 0.3
    assert abs(dH[20]) < abs(dH[10])


def test_multishift_cg_twin_agrees_with_the_dense_solves():
    """the solver the device comparison uses (rn.make_cg_m) against LU, every shift: relative 1e-10 at eps 1e-12"""
    th, _, eta, z, _, _ = setup(6, 4, 25)
    it = []
    a, b = rn.make_cg_m(1e-12, iters=it)(eta, th, MASS, z.mu2), rn.solve_shifts_dense(eta, th, MASS, z.mu2)
    assert it[0] > 5
    for x, y in zip(a, b):
        assert np.linalg.norm(x - y) < 1e-10 * np.linalg.norm(y)


@pytest.mark.parametrize("Lx,Ly", [(6, 4), (4, 6)])
def test_range_check_holds_inside_and_proves_a_spectrum_outside(Lx, Ly):
    """With the true ra the ratio is below 2 delta + delta^2 for any xi.  With ra^2 ten times the smallest eigenvalue, xi = the lowest
    eigenvector plus 1e-3 of noise makes the violation certain, not likely: on that eigenvector the form is v = lambda_0 r(lambda_0)^2 - 1,
    a number of the rational function alone (a few per cent here, r extrapolates smoothly below its interval) against a bound below 1e-8;
    the noise, of norm 1e-3 in a form whose eigenvalues are all at most |v| in size, moves the ratio by less than 3e-3 |v|."""
    th, _, eta, z, lam, vec = setup(Lx, Ly, 26)
    ratio, bound = rn.range_check(z, th, eta, MASS)
    print("%dx%d inside: ratio %.3e bound %.3e" % (Lx, Ly, ratio, bound))
    assert ratio <= bound * (1.0 + 1e-6) + 1e-13
    bad = rn.zolotarev(6, np.sqrt(10.0 * lam[0]), np.sqrt(lam[-1]))
    xi = vec[:, 0].reshape(Lx, Ly, 2) + 1e-3 * eta / np.linalg.norm(eta)
    ratio, bound = rn.range_check(bad, th, xi, MASS)
    v = abs(lam[0] * rn.r_product(bad, lam[0]) ** 2 - 1.0)
    print("%dx%d outside: ratio %.3e bound %.3e; lambda_0 r(lambda_0)^2 - 1 = %.3e" % (Lx, Ly, ratio, bound, v))
    assert np.abs(lam * rn.r_product(bad, lam) ** 2 - 1.0).max() <= v * (1.0 + 1e-9)
    assert bound < 1e-8 and v > 1e-2 and abs(ratio - v) <= 3e-3 * v


def test_new_entry_point_is_exported_declared_and_bound():
    qmg.build()
    lib = qmg.lib()
    header = open(os.path.join(ROOT, "include", "qmg_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in rn.NEW_SYMBOLS:
        assert hasattr(lib, name), "libqmg_hip.so does not export %s" % name
        assert re.search(r"\b%s\s*\(" % name, header), "include/qmg_hip.h does not declare %s" % name
        assert name in qmg.ABI_SYMBOLS
    for name in rn.NEW_BINDINGS:
        assert callable(getattr(qmg, name, None)), "the Python module does not bind %s" % name
