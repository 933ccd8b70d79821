"""CPU side of the integrators of HmcCore::set_integrator: the numpy twin tests/md_schemes_numpy.py is pinned by what any correct statement of
the schemes must obey -- its single-scale leapfrog is hmc_numpy's, every scheme is reversible, its energy error falls as dt^2, and nesting
without fermions is a pure-gauge run of the inner steps -- before it judges the device in test_gpu_md_schemes.py; and the drop-in boundary of
the new entry point."""
import importlib
import os
import re

import numpy as np
import pytest

import hmc_numpy as hn
import md_schemes_numpy as ms

qmg = importlib.import_module("quantum-mg_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETA, MASS = 4.0, 0.1
COMBOS = [(scheme, n_gauge) for scheme in (ms.LEAPFROG, ms.OMELYAN) for n_gauge in (0, 3, 4)]


def setup(Lx, Ly, seed):
    """uniform phases in +-1, Gaussian momenta, phi = D^dag eta"""
    rng = np.random.default_rng(seed)
    th = (rng.uniform(-1.0, 1.0, (Lx, Ly)), rng.uniform(-1.0, 1.0, (Lx, Ly)))
    pi = (rng.standard_normal((Lx, Ly)), rng.standard_normal((Lx, Ly)))
    eta = (rng.standard_normal((Lx, Ly, 2)) + 1j * rng.standard_normal((Lx, Ly, 2))) / np.sqrt(2.0)
    return th, pi, hn.Ddag(eta, th, MASS)


def forces(phi, solve=hn.solve_dense):
    return (lambda th: hn.gauge_force(th, BETA)), (lambda th: hn.fermion_force(th, phi, MASS, solve))


def dist(a, b):
    return max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max())


def test_kick_counts():
    """n steps cost n + 1 fermion forces (leapfrog) and 2 n + 1 (Omelyan); the steps of a list add up to the trajectory"""
    for n in (1, 2, 7):
        assert ms.n_fermion_forces(ms.LEAPFROG, n) == n + 1 and ms.n_fermion_forces(ms.OMELYAN, n) == 2 * n + 1
        for scheme in (ms.LEAPFROG, ms.OMELYAN):
            ops = ms.sequence(scheme, n, 1.0 / n)
            assert ops[0][0] == "K" and ops[-1][0] == "K" and all(a[0] != b[0] for a, b in zip(ops, ops[1:]))
            for kind in "KD":
                assert abs(sum(e for k, e in ops if k == kind) - 1.0) < 1e-15 * len(ops)


def test_single_scale_leapfrog_is_hmc_numpys():
    th, pi, phi = setup(6, 4, 21)
    fg, ff = forces(phi)
    a = ms.integrate(th, pi, fg, ff, 1.0, 20, ms.LEAPFROG, 0)
    b = hn.leapfrog(th, pi, BETA, 1.0, 20, phi, MASS)
    d, dp = dist(a[0], b[0]), dist(a[1], b[1])
    print("against hn.leapfrog: phases %.2e momenta %.2e" % (d, dp))
    assert d <= 1e-14 and dp <= 1e-14
    c = ms.integrate(th, pi, fg, None, 1.0, 20, ms.LEAPFROG, 0)
    e = hn.leapfrog(th, pi, BETA, 1.0, 20)
    assert dist(c[0], e[0]) <= 1e-14 and dist(c[1], e[1]) <= 1e-14


@pytest.mark.parametrize("scheme,n_gauge", COMBOS)
def test_every_scheme_is_reversible(scheme, n_gauge):
    th, pi, phi = setup(6, 4, 22)
    fg, ff = forces(phi)
    th1, pi1 = ms.integrate(th, pi, fg, ff, 1.0, 10, scheme, n_gauge)
    th2, pi2 = ms.integrate(th1, (-pi1[0], -pi1[1]), fg, ff, 1.0, 10, scheme, n_gauge)
    d, dp = dist(th2, th), dist(pi2, (-pi[0], -pi[1]))
    print("%s n_gauge %d forward-back: phases %.2e momenta %.2e" % (scheme, n_gauge, d, dp))
    assert np.abs(th1[0] - th[0]).max() > 0.1          # it went somewhere
    assert d <= 1e-13 and dp <= 1e-13


@pytest.mark.parametrize("scheme,n_gauge", [(ms.LEAPFROG, 0), (ms.LEAPFROG, 4), (ms.OMELYAN, 0), (ms.OMELYAN, 4)])
def test_energy_error_follows_the_dt_squared_law(scheme, n_gauge):
    """8 x 8, beta 4, m 0.1, tau 1, dense solves: both schemes are of second order, on one scale and on two, so halving the step divides dH by
    4 up to the next order: the ratio lies in [3, 5]."""
    th, pi, phi = setup(8, 8, 23)
    fg, ff = forces(phi)
    ham = lambda t, p: hn.hamiltonian(t, p, BETA, phi, MASS)
    n = 20 if scheme == ms.LEAPFROG else 10
    dH = {k: ms.md_dH(th, pi, ham, fg, ff, 1.0, k, scheme, n_gauge)[2] for k in (n, 2 * n)}
    print("%s n_gauge %d: dH %s ratio %.3f" % (scheme, n_gauge, dH, abs(dH[n] / dH[2 * n])))
    assert 3.0 <= abs(dH[n]) / abs(dH[2 * n]) <= 5.0


@pytest.mark.parametrize("scheme", [ms.LEAPFROG, ms.OMELYAN])
def test_nesting_without_fermions_is_a_pure_gauge_run_of_the_inner_steps(scheme):
    """Without the fermion force the kicks of the outer list are absent and the blocks follow each other: n_gauge steps of the scheme under the
    gauge force for every drift of the outer list -- n_steps n_gauge equal steps for leapfrog (one drift per step), 2 n_steps n_gauge for
    Omelyan (two drifts of h/2 per step) -- except that the kicks where two blocks meet are two (each half the merged one).  Rounding only:
    up to 81 kicks and drifts of O(1) numbers at half an ulp each, grown by at most exp(tau sqrt(4 beta)) = 55: 1e-12 with room."""
    th, pi, _ = setup(6, 4, 24)
    fg = lambda t: hn.gauge_force(t, BETA)
    drifts = sum(1 for kind, _ in ms.sequence(scheme, 5, 0.2) if kind == "D")
    assert drifts == (5 if scheme == ms.LEAPFROG else 10)
    a = ms.integrate(th, pi, fg, None, 1.0, 5, scheme, 4)
    b = ms.integrate(th, pi, fg, None, 1.0, drifts * 4, scheme, 0)
    d, dp = dist(a[0], b[0]), dist(a[1], b[1])
    print("%s: nested 5 x 4 against %d plain: phases %.2e momenta %.2e" % (scheme, drifts * 4, d, dp))
    assert np.abs(a[0][0] - th[0]).max() > 0.1
    assert d <= 1e-12 and dp <= 1e-12


def test_cg_twin_on_the_fixture_size_runs_a_nested_step(golden_dir):
    """32^2 with hn.make_cg (never a dense solve there): one nested Omelyan step is reversible"""
    L = 32
    th = hn.file_phases(os.path.join(golden_dir, "l32t32b60_heatbath.dat"), L, L)
    rng = np.random.default_rng(2024)
    pi = (rng.standard_normal((L, L)), rng.standard_normal((L, L)))
    eta = (rng.standard_normal((L, L, 2)) + 1j * rng.standard_normal((L, L, 2))) / np.sqrt(2.0)
    phi = hn.Ddag(eta, th, MASS)
    fg, ff = (lambda t: hn.gauge_force(t, 6.0)), (lambda t: hn.fermion_force(t, phi, MASS, hn.make_cg(1e-13)))
    th1, pi1 = ms.integrate(th, pi, fg, ff, 0.1, 1, ms.OMELYAN, 4)
    th2, _ = ms.integrate(th1, (-pi1[0], -pi1[1]), fg, ff, 0.1, 1, ms.OMELYAN, 4)
    assert dist(th2, th) <= 1e-13


def test_new_entry_point_is_exported_declared_and_bound():
    qmg.build()
    lib = qmg.lib()
    header = open(os.path.join(ROOT, "include", "qmg_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ms.NEW_SYMBOLS:
        assert hasattr(lib, name), "libqmg_hip.so does not export %s" % name
        assert re.search(r"\b%s\s*\(" % name, header), "include/qmg_hip.h does not declare %s" % name
        assert name in qmg.ABI_SYMBOLS
    for name in ms.NEW_BINDINGS:
        assert callable(getattr(qmg, name, None)), "the Python module does not bind %s" % name
