"""CPU side of two-flavour domain-wall HMC: the numpy twin tests/dwf_hmc_numpy.py is pinned here -- its operator against dwf_numpy's dense D, the
determinant identity, its force against finite differences of its own dense action, the heatbath identity, zero force at m = 1, gauge
invariance and covariance, reversibility and the dt^2 law of leapfrog -- before tests/test_gpu_dwf_hmc.py judges the device by it; the launch
geometry of the kick through qmg_hmc_dwf_plan; and the drop-in boundary of the new entry points."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import coordspace as cs
import dwf_hmc_numpy as dh
import dwf_numpy as dn
import hmc_numpy as hn

qmg = importlib.import_module("quantum-mg_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVERS = os.path.join(ROOT, "quantum-mg_amd", "drivers")
BETA = 3.0
SHAPES = [(4, 4, 2, 0.1), (6, 4, 3, 0.05), (4, 6, 4, 0.2)]      # Lx, Ly, Ls, m


def setup(Lx, Ly, Ls, seed, width=1.5):
    """uniform random phases in +-width, momenta, a pseudofermion and an eta on the even sites"""
    rng = np.random.default_rng(seed)
    th = (rng.uniform(-width, width, (Lx, Ly)), rng.uniform(-width, width, (Lx, Ly)))
    pi = (rng.standard_normal((Lx, Ly)), rng.standard_normal((Lx, Ly)))
    field = lambda: dh.keep((rng.standard_normal((Lx, Ly, Ls, 2)) + 1j * rng.standard_normal((Lx, Ly, Ls, 2))) / np.sqrt(2.0), 0)
    return th, pi, field(), field()


@pytest.mark.parametrize("Lx,Ly,Ls,m", SHAPES)
def test_twin_operator_is_dwf_numpys_and_the_determinant_factorises(Lx, Ly, Ls, m):
    th, _, _, _ = setup(Lx, Ly, Ls, 10 + Lx)
    Ux, Uy = hn.links(th)
    want, g5 = dn.dense(Lx, Ly, Ls, cs.links_to_eo_gauge(Ux, Uy, Lx, Ly), m, 1.0, dh.M5)
    got = dh.dense(lambda v: dh.D(v, th, m), Lx, Ly, Ls)
    assert np.abs(got - want).max() <= 1e-14
    # A^-1 A = 1, Gamma5 D Gamma5 = D^dag, M^dag = Gamma5 M Gamma5 on the even sites
    eye = np.eye(got.shape[0])
    assert np.abs(dh.dense(lambda v: dh.apply_A_inv(dh.apply_A(v, m), m), Lx, Ly, Ls) - eye).max() <= 1e-14
    assert np.abs(g5 @ got @ g5 - got.conj().T).max() <= 1e-14
    ev = dh.even_index(Lx, Ly, Ls)
    Mm = dh.dense_M(th, m, Ls)
    assert np.abs(dh.dense(lambda v: dh.Mdag(v, th, m), Lx, Ly, Ls)[np.ix_(ev, ev)] - Mm.conj().T).max() <= 1e-13
    a, b = dh.logdets(th, m, Ls)
    print("%dx%d Ls=%d: log|det D| = %.12f, log|det A_oo| + log|det M| = %.12f" % (Lx, Ly, Ls, a, b))
    assert abs(a - b) <= 1e-12 * max(1.0, abs(a))


def fd_force(th, phi, m, h=1e-4):
    out = (np.zeros(th[0].shape), np.zeros(th[0].shape))
    for mu in range(2):
        for idx in np.ndindex(*th[0].shape):
            tp = [t.copy() for t in th]
            tm = [t.copy() for t in th]
            tp[mu][idx] += h
            tm[mu][idx] -= h
            out[mu][idx] = (dh.action(tuple(tp), BETA, phi, m) - dh.action(tuple(tm), BETA, phi, m)) / (2 * h)
    return out


@pytest.mark.parametrize("Lx,Ly,Ls,m", SHAPES)
def test_force_is_the_derivative_of_the_dense_action(Lx, Ly, Ls, m):
    """central differences at h = 1e-4 with uniform random phases in +-1.5: gate 1e-6, the project's finite-difference gate"""
    th, _, phi, _ = setup(Lx, Ly, Ls, 30 + 7 * Lx + Ly)
    f = dh.force(th, BETA, phi, m)
    fd = fd_force(th, phi, m)
    err = max(np.abs(f[0] - fd[0]).max(), np.abs(f[1] - fd[1]).max())
    print("%dx%d Ls=%d m=%.2f: max |F - FD| = %.2e, max |F| = %.2f" % (Lx, Ly, Ls, m, err, max(np.abs(f[0]).max(), np.abs(f[1]).max())))
    assert err <= 1e-6
    g = hn.gauge_force(th, BETA)
    assert max(np.abs(f[0] - g[0]).max(), np.abs(f[1] - g[1]).max()) > 1e-3       # the fermions contribute


@pytest.mark.parametrize("Lx,Ly,Ls,m", SHAPES)
def test_heatbath_identity_and_zero_force_at_unit_mass(Lx, Ly, Ls, m):
    th, _, phi, eta = setup(Lx, Ly, Ls, 50 + Lx)
    p = dh.heatbath(th, eta, m)
    e2 = np.vdot(eta, eta).real
    assert np.abs(dh.keep(p, 1)).max() == 0.0
    assert abs(dh.fermion_action(th, p, m) - e2) <= 1e-11 * e2
    # m = 1: M = P, S_f = phi^dag phi and the two pairs of the force cancel
    assert abs(dh.fermion_action(th, phi, 1.0) - np.vdot(phi, phi).real) <= 1e-11 * np.vdot(phi, phi).real
    f = dh.fermion_force(th, phi, 1.0)
    fm = dh.fermion_force(th, phi, m)
    assert max(np.abs(f[0]).max(), np.abs(f[1]).max()) <= 1e-12 * max(np.abs(fm[0]).max(), np.abs(fm[1]).max())


def test_action_is_gauge_invariant_and_force_covariant():
    Lx, Ly, Ls, m = 6, 4, 3, 0.1
    th, _, phi, _ = setup(Lx, Ly, Ls, 41)
    a = np.random.default_rng(5).uniform(-np.pi, np.pi, (Lx, Ly))
    th_g, phi_g = hn.gauge_shift(th, a), dh.gauge_rotate(phi, a)
    s0, s1 = dh.action(th, BETA, phi, m), dh.action(th_g, BETA, phi_g, m)
    assert abs(s1 - s0) <= 1e-11 * abs(s0)
    f0, f1 = dh.force(th, BETA, phi, m), dh.force(th_g, BETA, phi_g, m)
    assert max(np.abs(f0[0] - f1[0]).max(), np.abs(f0[1] - f1[1]).max()) <= 1e-11 * max(np.abs(f0[0]).max(), np.abs(f0[1]).max())
    # the bilinear alone, for any X and Y, with and without Gamma5 on Y
    rng = np.random.default_rng(6)
    X, Y = (rng.standard_normal((Lx, Ly, Ls, 2)) + 1j * rng.standard_normal((Lx, Ly, Ls, 2)) for _ in range(2))
    for g5 in (False, True):
        g0 = dh.force_pairs(th, [X], [Y], [1.3], g5)
        g1 = dh.force_pairs(th_g, [dh.gauge_rotate(X, a)], [dh.gauge_rotate(Y, a)], [1.3], g5)
        assert max(np.abs(g0[0] - g1[0]).max(), np.abs(g0[1] - g1[1]).max()) <= 1e-12


def test_leapfrog_is_reversible_and_dH_scales_as_dt_squared():
    Lx, Ly, Ls, m = 4, 4, 2, 0.2
    th, pi, phi, _ = setup(Lx, Ly, Ls, 51, width=0.5)
    th1, pi1 = dh.leapfrog(th, pi, BETA, 0.5, 10, phi, m)
    th2, pi2 = dh.leapfrog(th1, (-pi1[0], -pi1[1]), BETA, 0.5, 10, phi, m)
    assert max(np.abs(th2[0] - th[0]).max(), np.abs(th2[1] - th[1]).max()) <= 1e-11
    assert max(np.abs(pi2[0] + pi[0]).max(), np.abs(pi2[1] + pi[1]).max()) <= 1e-11
    dH = [abs(dh.md_dH(th, pi, BETA, 0.5, n, phi, m)[2]) for n in (10, 20, 40)]
    print("dH at 10, 20, 40 steps: %.3e %.3e %.3e" % tuple(dH))
    assert 3.0 < dH[0] / dH[1] < 5.0 and 3.0 < dH[1] / dH[2] < 5.0


def test_cg_twin_agrees_with_the_dense_solve_and_layouts_round_trip():
    Lx, Ly, Ls, m = 6, 4, 3, 0.1
    th, _, phi, eta = setup(Lx, Ly, Ls, 81)
    assert np.abs(dh.make_cg(1e-13)(phi, th, m) - dh.solve_dense(phi, th, m)).max() <= 1e-10
    assert np.abs(dh.heatbath(th, eta, m, dh.make_cg(1e-13)) - dh.heatbath(th, eta, m)).max() <= 1e-10
    full = np.random.default_rng(2).standard_normal((Lx, Ly, Ls, 2)) + 0j
    assert np.array_equal(dh.eo_to_grid(dh.grid_to_eo(full), Lx, Ly, Ls), full)
    assert np.array_equal(dh.half_to_even(dh.even_to_half(phi), Lx, Ly, Ls), phi)
    # a slice of the nc = 2 Ls vector is the nc = 2 vector of that slice
    flat = dh.grid_to_eo(full).reshape(Lx * Ly, Ls, 2)
    for s, v in enumerate(dh.slices_to_eo(full)):
        assert np.array_equal(v.reshape(Lx * Ly, 2), flat[:, s])


# ---- the launch geometry of the kick, without a GPU ----
@pytest.mark.parametrize("Ls", [2, 3, 6, 8, 12, 32])
@pytest.mark.parametrize("Lx,Ly", [(2, 2), (4, 6), (130, 2), (16, 8), (2048, 2048), (2, 32770)])
def test_plan_never_splits_a_site_across_the_reduction_unit(Lx, Ly, Ls):
    """the sum over s is in the LDS of one block: a block is a whole number of sites, the blocks of a row cover its lanes, the rows are walked"""
    qmg.build()
    for n in (1, 2, 3, 4, 5, 9):
        for flags in (0, qmg.HMC_DWF_G5_Y):
            family, lps, block, gx, gy, lds, launches, per_launch = qmg.hmc_dwf_plan((Lx, Ly), Ls, n, flags)
            assert family == qmg.HDF_FUSED and lps == Ls
            assert block % Ls == 0 and 0 < block <= 256 and block + Ls > 256      # whole sites, and as many as fit
            lanes = (Lx // 2) * Ls
            assert (gx - 1) * block < lanes <= gx * block
            assert gy == min(2 * Ly, 65535)
            assert lds == 2 * 256 * 16 and lds >= 2 * block * 16
            assert per_launch == 4 and launches == -(-n // per_launch)
    for n, flags in ((0, 0), (0, qmg.HMC_DWF_G5_Y), (2, qmg.HMC_GAUGE_ONLY), (2, qmg.HMC_GAUGE_ONLY | qmg.HMC_DWF_G5_Y)):
        plan = qmg.hmc_dwf_plan((Lx, Ly), Ls, n, flags)
        assert plan[0] == qmg.HDF_GAUGE and plan[1] == 0 and plan[5] == 0 and plan[6] == 1


def test_plan_refusals():
    qmg.build()
    invalid = 1
    bad = [((3, 4), 4, 2, 0), ((4, 5), 4, 2, 0), ((0, 4), 4, 2, 0), ((4, -2), 4, 2, 0),          # odd or non-positive extents
           ((4, 4), 1, 2, 0), ((4, 4), 33, 2, 0), ((4, 4), 0, 0, qmg.HMC_GAUGE_ONLY),            # Ls out of range, with and without fermions
           ((4, 4), 4, -1, 0), ((4, 4), 4, 2, 4), ((4, 4), 4, 2, 8 | qmg.HMC_DWF_G5_Y),          # negative count, unknown flags
           ((1 << 23, 2), 32, 1, 0)]                                                              # a half row past 32-bit byte offsets
    for dims, Ls, n, flags in bad:
        rc, plan = qmg.hmc_dwf_plan_status(dims, Ls, n, flags)
        assert rc == 0 and plan[0] == qmg.HDF_INVALID, (dims, Ls, n, flags, plan)
        assert qmg.hmc_momentum_update_dwf_status(None, None, None, None, None, Ls, dims[0], dims[1], 1.0, 0.1, flags, n_pairs=n) == invalid
    out = (qmg.C.c_int * 4)()
    assert qmg.lib().qmg_hmc_dwf_plan(4, 4, 4, 2, 0, out, 4) == invalid             # a short output array
    assert qmg.lib().qmg_hmc_dwf_plan(4, 4, 4, 2, 0, None, 8) == invalid


def test_library_exports_the_entry_points_and_the_drivers_build():
    """fails without the feature"""
    qmg.build()
    for name in dh.NEW_SYMBOLS:
        assert name in qmg.ABI_SYMBOLS and hasattr(qmg.lib(), name)
    for name in dh.NEW_BINDINGS:
        assert callable(getattr(qmg, name))
    assert qmg.HMC_DWF_G5_Y == 2
    subprocess.check_call(["make", "-C", DRIVERS, "-j4", "dwf_hmc", "dwf_hmc_parity"], stdout=subprocess.DEVNULL)
    assert os.path.exists(os.path.join(DRIVERS, "dwf_hmc")) and os.path.exists(os.path.join(DRIVERS, "dwf_hmc_parity"))
    text = open(os.path.join(ROOT, "quantum-mg_amd", "include", "qmg", "hmc_dwf.hpp")).read()
    assert "class DomainWallSchwingerHMC" in text
    assert "qmg_dwf_fill" not in text and "update_links" not in text       # no stored domain-wall stencil in the HMC class
    header = open(os.path.join(ROOT, "include", "qmg_hip.h")).read()
    assert "QMG_HMC_DWF_G5_Y = 2u" in header
