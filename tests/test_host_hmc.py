"""CPU side of the Schwinger-model HMC: (i) the numpy twin tests/hmc_numpy.py is pinned by what any correct statement must obey -- its
forces are the derivative of its action (central finite differences), action and force are gauge invariant / covariant, leapfrog is
reversible and its energy error falls as dt^2 -- before it judges the device in test_gpu_hmc.py; (ii) the drop-in boundary: every new entry
point is exported by libqmg_hip.so, declared in include/qmg_hip.h and bound in Python."""
import importlib
import os
import re

import numpy as np
import pytest

import hmc_numpy as hn

qmg = importlib.import_module("quantum-mg_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETA, MASS = 3.0, 0.1


def setup(Lx, Ly, seed, fermions=True):
    rng = np.random.default_rng(seed)
    th = (0.5 * rng.standard_normal((Lx, Ly)), 0.5 * rng.standard_normal((Lx, Ly)))
    pi = (rng.standard_normal((Lx, Ly)), rng.standard_normal((Lx, Ly)))
    phi = None
    if fermions:
        eta = (rng.standard_normal((Lx, Ly, 2)) + 1j * rng.standard_normal((Lx, Ly, 2))) / np.sqrt(2.0)
        phi = hn.Ddag(eta, th, MASS)
    return th, pi, phi


@pytest.mark.parametrize("Lx,Ly", [(6, 4), (4, 6)])
@pytest.mark.parametrize("fermions", [False, True])
def test_force_is_the_derivative_of_the_action(Lx, Ly, fermions):
    """Central differences at h = 1e-4 on every link: the O(h^2) error is h^2/6 |S'''| ~ 1e-8 for |S'''| of a few; agreement 1e-6 absolute."""
    th, _, phi = setup(Lx, Ly, 11, fermions)
    f = hn.force(th, BETA, phi, MASS)
    h, worst = 1e-4, 0.0
    for mu in range(2):
        for x in range(Lx):
            for y in range(Ly):
                up = (th[0].copy(), th[1].copy())
                dn = (th[0].copy(), th[1].copy())
                up[mu][x, y] += h
                dn[mu][x, y] -= h
                fd = (hn.action(up, BETA, phi, MASS) - hn.action(dn, BETA, phi, MASS)) / (2 * h)
                worst = max(worst, abs(fd - f[mu][x, y]))
    fmax = max(np.abs(f[0]).max(), np.abs(f[1]).max())
    print("%dx%d fermions=%s: max |F - FD| = %.2e, max |F| = %.2f" % (Lx, Ly, fermions, worst, fmax))
    assert fmax > 1.0
    assert worst < 1e-6


@pytest.mark.parametrize("Lx,Ly", [(6, 4), (4, 6)])
def test_action_is_gauge_invariant_and_the_force_covariant(Lx, Ly):
    """theta_mu(x) += a(x) - a(x+mu), phi(x) -> exp(i a(x)) phi(x): the action keeps its value, and the force -- a derivative with respect
    to the phase of a link -- its value link by link.  Rounding only: a dense solve of condition ~1e2 on O(10) numbers."""
    th, _, phi = setup(Lx, Ly, 12)
    a = np.random.default_rng(13).uniform(-np.pi, np.pi, size=(Lx, Ly))
    th2, phi2 = hn.gauge_shift(th, a), np.exp(1j * a)[:, :, None] * phi
    s0, s1 = hn.action(th, BETA, phi, MASS), hn.action(th2, BETA, phi2, MASS)
    f0, f1 = hn.force(th, BETA, phi, MASS), hn.force(th2, BETA, phi2, MASS)
    d = max(np.abs(f0[0] - f1[0]).max(), np.abs(f0[1] - f1[1]).max())
    print("%dx%d: action moved %.2e of %.2f, force moved %.2e" % (Lx, Ly, abs(s1 - s0), s0, d))
    assert abs(s1 - s0) < 1e-11 * abs(s0)
    assert d < 1e-11


def test_leapfrog_is_reversible():
    th, pi, phi = setup(6, 4, 14)
    th1, pi1 = hn.leapfrog(th, pi, BETA, 1.0, 20, phi, MASS)
    th2, pi2 = hn.leapfrog(th1, (-pi1[0], -pi1[1]), BETA, 1.0, 20, phi, MASS)
    d = max(np.abs(th2[0] - th[0]).max(), np.abs(th2[1] - th[1]).max())
    dp = max(np.abs(pi2[0] + pi[0]).max(), np.abs(pi2[1] + pi[1]).max())
    print("forward-back: phases %.2e momenta %.2e" % (d, dp))
    assert np.abs(th1[0] - th[0]).max() > 0.1          # it went somewhere
    assert d < 1e-13 and dp < 1e-13


def test_leapfrog_energy_error_follows_the_dt_squared_law():
    th, pi, phi = setup(6, 4, 14)
    dH = {n: hn.md_dH(th, pi, BETA, 1.0, n, phi, MASS)[2] for n in (10, 20, 40)}
    print("dH over tau = 1:", dH)
    assert 0.2 <= dH[40] / dH[20] <= 0.3
    assert abs(dH[20]) < abs(dH[10])


def test_twin_pure_gauge_hmc_gives_the_exact_plaquette():
    """16^2, beta 2, tau 1, 10 steps, cold start, 100 + 300 trajectories -- the run the device is held to: <cos P> = I1(2)/I0(2) = 0.697775
    within 0.014 (five standard deviations of this run's mean over seeds, 0.00276), acceptance in (0.8, 1)."""
    plaq, acc = hn.hmc_pure_gauge(16, 2.0, 1.0, 10, 100, 300, 1)
    print("twin pure gauge: <plaq> %.6f acceptance %.3f" % (plaq, acc))
    assert abs(plaq - 0.697775) <= 0.014 and 0.8 < acc < 1.0


def test_cg_twin_agrees_with_the_dense_solve():
    """the CG the device comparison uses (hn.make_cg) against LU: relative 1e-10 at eps 1e-12 (condition number ~1e2)"""
    th, _, phi = setup(6, 4, 15)
    a, b = hn.make_cg(1e-12)(phi, th, MASS), hn.solve_dense(phi, th, MASS)
    assert np.linalg.norm(a - b) < 1e-10 * np.linalg.norm(b)


def test_layout_round_trip():
    th, _, _ = setup(6, 4, 16)
    back = hn.eo_to_field(hn.field_to_eo(th), 6, 4)
    assert np.array_equal(back[0], th[0]) and np.array_equal(back[1], th[1])


def test_new_entry_points_are_exported_declared_and_bound():
    qmg.build()
    lib = qmg.lib()
    header = open(os.path.join(ROOT, "include", "qmg_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in hn.NEW_SYMBOLS:
        assert hasattr(lib, name), "libqmg_hip.so does not export %s" % name
        assert re.search(r"\b%s\s*\(" % name, header), "include/qmg_hip.h does not declare %s" % name
        assert name in qmg.ABI_SYMBOLS
    for name in hn.NEW_BINDINGS:
        assert callable(getattr(qmg, name, None)), "the Python module does not bind %s" % name
    assert qmg.HMC_GAUGE_ONLY == 1 and re.search(r"QMG_HMC_GAUGE_ONLY\s*=\s*1u", header)
