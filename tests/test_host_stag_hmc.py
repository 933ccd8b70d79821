"""CPU side of staggered HMC / rooted RHMC: the numpy twin tests/stag_hmc_numpy.py is pinned here -- its D against the CPU oracle's staggered
apply (which fixes the overall sign of the hopping term), its force against finite differences of its own dense action, gauge invariance and
covariance, reversibility and the dt^2 law of leapfrog, both heatbath identities, the spectral interval -- before tests/test_gpu_stag_hmc.py
judges the device by it; and the drop-in boundary of the new entry point."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import coordspace as cs
import hmc_numpy as hn
import oracle_lib as ol
import stag_hmc_numpy as sn

qmg = importlib.import_module("quantum-mg_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVERS = os.path.join(ROOT, "quantum-mg_amd", "drivers")
BETA, MASS = 3.0, 0.1
SHAPES = [(6, 4), (4, 6), (2, 2)]


def setup(Lx, Ly, seed):
    """random phases, momenta, a pseudofermion on the even sites, a full-lattice eta"""
    rng = np.random.default_rng(seed)
    th = (rng.uniform(-np.pi, np.pi, (Lx, Ly)), rng.uniform(-np.pi, np.pi, (Lx, Ly)))
    pi = (rng.standard_normal((Lx, Ly)), rng.standard_normal((Lx, Ly)))
    eta = (rng.standard_normal((Lx, Ly)) + 1j * rng.standard_normal((Lx, Ly))) / np.sqrt(2.0)
    phi = np.where(sn.even(Lx, Ly), rng.standard_normal((Lx, Ly)) + 1j * rng.standard_normal((Lx, Ly)), 0.0)
    return th, pi, phi, eta


@pytest.mark.parametrize("Lx,Ly", [(6, 4), (2, 2)])
def test_twin_D_is_the_oracles_staggered_apply(Lx, Ly):
    """fixes SIGN: the oracle applies the reference's -0.5 U / +0.5 U^dag fill"""
    ol.build()
    th, _, _, _ = setup(Lx, Ly, 10 + Lx)
    rng = np.random.default_rng(3)
    psi = rng.standard_normal((Lx, Ly)) + 1j * rng.standard_normal((Lx, Ly))
    Ux, Uy = hn.links(th)
    hopping = ol.staggered_fill(cs.links_to_eo_gauge(Ux, Uy, Lx, Ly), Lx, Ly)
    want = ol.stencil_apply(ol.make_desc(Lx, Ly, 1, None, hopping, MASS), sn.grid_to_eo(psi))
    got = sn.grid_to_eo(sn.D(psi, th, MASS))
    assert np.abs(got - want).max() <= 1e-14
    assert np.abs(sn.grid_to_eo(sn.D(psi, th, MASS, -sn.SIGN)) - want).max() > 0.1      # the other sign is another operator
    assert np.abs(got - cs.grid_to_eo(cs.staggered_apply(psi[:, :, None], Ux, Uy, MASS), Lx, Ly, 1)).max() <= 1e-14


@pytest.mark.parametrize("Lx,Ly", SHAPES)
def test_hopping_term_is_antihermitian_odd_and_bounded(Lx, Ly):
    th, _, _, _ = setup(Lx, Ly, 20 + Lx)
    Hm = sn.dense(lambda v: sn.H(v, th), Lx, Ly)
    assert np.abs(Hm + Hm.conj().T).max() <= 1e-15
    ev = sn.even(Lx, Ly).reshape(-1)
    assert np.abs(Hm[np.ix_(ev, ev)]).max() == 0.0 and np.abs(Hm[np.ix_(~ev, ~ev)]).max() == 0.0
    assert np.linalg.norm(Hm, 2) <= 2.0 + 1e-12
    # det A_ee = det D
    Dm = sn.dense(lambda v: sn.D(v, th, MASS), Lx, Ly)
    assert abs(np.linalg.det(sn.dense_A_ee(th, MASS)) / np.linalg.det(Dm) - 1.0) <= 1e-10


def fd_force(th, phi, z, sign, h=1e-5):
    out = (np.zeros(th[0].shape), np.zeros(th[0].shape))
    for mu in range(2):
        for idx in np.ndindex(*th[0].shape):
            tp = [t.copy() for t in th]
            tm = [t.copy() for t in th]
            tp[mu][idx] += h
            tm[mu][idx] -= h
            out[mu][idx] = (sn.action(tuple(tp), BETA, phi, MASS, z, sign=sign) - sn.action(tuple(tm), BETA, phi, MASS, z, sign=sign)) / (2 * h)
    return out


@pytest.mark.parametrize("Lx,Ly", SHAPES)
@pytest.mark.parametrize("rooted", [False, True])
@pytest.mark.parametrize("sign", [-1.0, 1.0])
def test_force_is_the_derivative_of_the_dense_action(Lx, Ly, rooted, sign):
    """central differences at h = 1e-5: truncation h^2 |S'''| / 6 ~ 1e-10 |F|, rounding ~ 1e-16 |S| / h ~ 1e-9; gate 1e-6"""
    th, _, phi, _ = setup(Lx, Ly, 30 + 7 * Lx + Ly)
    z = sn.rational(4, MASS) if rooted else None
    f = sn.force(th, BETA, phi, MASS, z, sign=sign)
    fd = fd_force(th, phi, z, sign)
    err = max(np.abs(f[0] - fd[0]).max(), np.abs(f[1] - fd[1]).max())
    print("%dx%d rooted=%s sign=%+.0f: max |F - FD| = %.2e, max |F| = %.2f" % (Lx, Ly, rooted, sign, err, max(np.abs(f[0]).max(), np.abs(f[1]).max())))
    assert err <= 1e-6
    g = hn.gauge_force(th, BETA)
    assert max(np.abs(f[0] - g[0]).max(), np.abs(f[1] - g[1]).max()) > 1e-3       # the fermions contribute


@pytest.mark.parametrize("rooted", [False, True])
def test_action_is_gauge_invariant_and_force_covariant(rooted):
    Lx, Ly = 6, 4
    th, _, phi, _ = setup(Lx, Ly, 41)
    z = sn.rational(4, MASS) if rooted else None
    a = np.random.default_rng(5).uniform(-np.pi, np.pi, (Lx, Ly))
    th_g, phi_g = hn.gauge_shift(th, a), np.exp(1j * a) * phi
    s0, s1 = sn.action(th, BETA, phi, MASS, z), sn.action(th_g, BETA, phi_g, MASS, z)
    assert abs(s1 - s0) <= 1e-11 * abs(s0)
    f0, f1 = sn.force(th, BETA, phi, MASS, z), sn.force(th_g, BETA, phi_g, MASS, z)
    assert max(np.abs(f0[0] - f1[0]).max(), np.abs(f0[1] - f1[1]).max()) <= 1e-11 * max(np.abs(f0[0]).max(), np.abs(f0[1]).max())
    # the bilinear alone, for any W
    W = np.random.default_rng(6).standard_normal((Lx, Ly)) + 1j * np.random.default_rng(7).standard_normal((Lx, Ly))
    g0, g1 = sn.force_W(th, W), sn.force_W(th_g, np.exp(1j * a) * W)
    assert max(np.abs(g0[0] - g1[0]).max(), np.abs(g0[1] - g1[1]).max()) <= 1e-13


@pytest.mark.parametrize("rooted", [False, True])
def test_leapfrog_is_reversible_and_dH_scales_as_dt_squared(rooted):
    Lx, Ly = 6, 4
    th, pi, phi, _ = setup(Lx, Ly, 51)
    z = sn.rational(4, MASS) if rooted else None
    th1, pi1 = sn.leapfrog(th, pi, BETA, 0.5, 10, phi, MASS, z)
    th2, pi2 = sn.leapfrog(th1, (-pi1[0], -pi1[1]), BETA, 0.5, 10, phi, MASS, z)
    assert max(np.abs(th2[0] - th[0]).max(), np.abs(th2[1] - th[1]).max()) <= 1e-11
    assert max(np.abs(pi2[0] + pi[0]).max(), np.abs(pi2[1] + pi[1]).max()) <= 1e-11
    dH = [abs(sn.md_dH(th, pi, BETA, 0.5, n, phi, MASS, z)[2]) for n in (20, 40, 80)]
    print("dH at 20, 40, 80 steps: %.3e %.3e %.3e" % tuple(dH))
    assert 3.0 < dH[0] / dH[1] < 5.0 and 3.0 < dH[1] / dH[2] < 5.0


@pytest.mark.parametrize("Lx,Ly", SHAPES)
def test_two_taste_heatbath_squares_to_A_ee(Lx, Ly):
    """phi_e = M eta with M = (D^dag)_{e, all}: M M^dag = A_ee, so phi_e^dag A_ee^-1 phi_e is distributed as eta^dag eta"""
    th, _, _, _ = setup(Lx, Ly, 61)
    ev = sn.even(Lx, Ly).reshape(-1)
    M = sn.dense(lambda v: sn.heatbath_two(th, v, MASS), Lx, Ly)[ev, :]
    assert np.abs(M @ M.conj().T - sn.dense_A_ee(th, MASS)).max() <= 1e-14
    Dm = sn.dense(lambda v: sn.D(v, th, MASS), Lx, Ly)
    assert np.abs(M - Dm.conj().T[ev, :]).max() <= 1e-15


@pytest.mark.parametrize("Lx,Ly,n", [(6, 4, 4), (4, 6, 8), (2, 2, 4)])
def test_rooted_heatbath_B_Bdag_r_is_one(Lx, Ly, n):
    """B B^dag r(A) = 1 on the full lattice, dense, to 10 delta: B B^dag = r(A)^-1 exactly in exact arithmetic, and the partial fractions of
    B lose digits to the spread of the poles.  r(A) itself is within delta of A^(-1/2)."""
    th, _, _, _ = setup(Lx, Ly, 71)
    z = sn.rational(n, MASS)
    B = sn.dense_B(z, th, MASS)
    r = sn.dense_r_full(z, th, MASS)
    err = np.abs(B @ B.conj().T @ r - np.eye(Lx * Ly)).max()
    Am = sn.dense(lambda v: sn.A(v, th, MASS), Lx, Ly)
    lam, vec = np.linalg.eigh(0.5 * (Am + Am.conj().T))
    err_r = np.abs((vec * np.sqrt(lam)[None, :]) @ vec.conj().T @ r - np.eye(Lx * Ly)).max()
    print("%dx%d n=%d: |B B^dag r - 1| = %.2e, |A^(1/2) r - 1| = %.2e, delta = %.2e" % (Lx, Ly, n, err, err_r, z.delta))
    assert err <= 10.0 * z.delta
    assert err_r <= 1.01 * z.delta
    # block diagonal: the even block of B B^dag is r(A_ee)^-1, what the even half of B eta is distributed by
    ev = sn.even(Lx, Ly).reshape(-1)
    BB = B @ B.conj().T
    assert np.abs(BB[np.ix_(ev, ~ev)]).max() <= 10.0 * z.delta
    # apply_rational is r(A_ee)
    v = np.where(sn.even(Lx, Ly), np.random.default_rng(8).standard_normal((Lx, Ly)) + 0j, 0.0)
    assert np.abs(sn.apply_rational(z, v, th, MASS).reshape(-1) - r @ v.reshape(-1)).max() <= 1e-12


def test_cg_twins_agree_with_the_dense_solves():
    Lx, Ly = 6, 4
    th, _, phi, eta = setup(Lx, Ly, 81)
    z = sn.rational(4, MASS)
    for a, b in zip(sn.make_cg(1e-13)(phi, th, MASS, z.mu2), sn.solve_dense(phi, th, MASS, z.mu2)):
        assert np.abs(a - b).max() <= 1e-11
    assert np.abs(sn.make_cg(1e-13)(phi, th, MASS)[0] - sn.solve_dense(phi, th, MASS)[0]).max() <= 1e-10
    a = sn.heatbath_one(z, th, eta, MASS, sn.make_cg_K2(1e-13))
    assert np.abs(a - sn.heatbath_one(z, th, eta, MASS)).max() <= 1e-11


def test_spectrum_of_A_ee_is_inside_the_interval_on_the_fixture(golden_dir):
    L = 32
    th = hn.file_phases(os.path.join(golden_dir, "l32t32b60_heatbath.dat"), L, L)
    lam = np.linalg.eigvalsh(sn.dense_A_ee(th, MASS))
    print("spectrum of A_ee on the 32^2 fixture at m = %.2f: [%.6f, %.6f]" % (MASS, lam[0], lam[-1]))
    assert lam[0] >= MASS ** 2 * (1 - 1e-10) and lam[-1] <= MASS ** 2 + 4.0


def test_library_exports_the_entry_point_and_the_driver_builds():
    """fails without the feature"""
    qmg.build()
    for name in sn.NEW_SYMBOLS:
        assert name in qmg.ABI_SYMBOLS and hasattr(qmg.lib(), name)
    for name in sn.NEW_BINDINGS:
        assert callable(getattr(qmg, name))
    subprocess.check_call(["make", "-C", DRIVERS, "-j4", "stag_hmc_parity", "schwinger_hmc"], stdout=subprocess.DEVNULL)
    assert os.path.exists(os.path.join(DRIVERS, "stag_hmc_parity"))
    text = open(os.path.join(ROOT, "quantum-mg_amd", "include", "qmg", "hmc_staggered.hpp")).read()
    assert "class StaggeredSchwingerHMC" in text
