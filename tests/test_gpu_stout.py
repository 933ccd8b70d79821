"""Stout-smeared Wilson fermions in the Schwinger-model HMC on the device (csrc/qmg_stout.hip, include/qmg/stout.hpp and hmc.hpp, the drivers
hmc_parity, rhmc_parity and schwinger_hmc).

The yardstick is the numpy twin tests/stout_numpy.py (np.roll on (x, y) grids; pinned in test_host_stout.py by finite differences of its own
smeared action, the symmetry of its Jacobian, gauge covariance, reversibility and the dt^2 law), never the code under test:
  * the four kernels against the twin with RANDOM links, forces and spinors (no solver enters).  The one-pass kernels are sums of fewer than
    40 O(1) fp64 products per component: relative l2 <= 1e-12, the gate of the kicks in test_gpu_hmc.py; the smeared links max abs 1e-13;
  * the whole chain (smear, force bilinear, levels, fused kick) against the twin and under a gauge transformation;
  * SchwingerHMC::md_evolve with stout levels, two flavours and one, on the 32^2 beta-6.0 fixture against the twin's leapfrog;
  * a smeared two-flavour run through the driver, plain and under QMG_MALLOC_POISON."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import coordspace as cs
import hmc_numpy as hn
import rhmc_numpy as rn
import stout_numpy as sn
import u1_numpy as un

qmg = importlib.import_module("quantum-mg_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVERS = os.path.join(ROOT, "quantum-mg_amd", "drivers")
SIZES = [(2, 2), (2, 6), (6, 2), (6, 4), (34, 10), (64, 64)]   # (2, 6): xl == xr == xh with distinct rows; (6, 2): yp == ym with distinct columns
BETA, RHO = 3.0, 0.1
FIX = "l32t32b60_heatbath.dat"


@pytest.fixture(scope="module", autouse=True)
def _device():
    qmg.build()
    subprocess.check_call(["make", "-C", DRIVERS, "-j4"], stdout=subprocess.DEVNULL)
    qmg.init(0)
    yield
    qmg.sync()


def rel_l2(a, b):
    return float(np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(np.ravel(b)))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def random_setup(Lx, Ly, seed, n_poles=1):
    rng = np.random.default_rng(seed)
    th = (rng.uniform(-np.pi, np.pi, (Lx, Ly)), rng.uniform(-np.pi, np.pi, (Lx, Ly)))
    pi = (rng.standard_normal((Lx, Ly)), rng.standard_normal((Lx, Ly)))
    F = (rng.standard_normal((Lx, Ly)), rng.standard_normal((Lx, Ly)))
    G = (rng.standard_normal((Lx, Ly)), rng.standard_normal((Lx, Ly)))
    X = [rng.standard_normal((Lx, Ly, 2)) + 1j * rng.standard_normal((Lx, Ly, 2)) for _ in range(n_poles)]
    Y = [rng.standard_normal((Lx, Ly, 2)) + 1j * rng.standard_normal((Lx, Ly, 2)) for _ in range(n_poles)]
    w = rng.uniform(0.05, 2.0, n_poles)
    return th, pi, F, G, X, Y, w


def up_links(links, Lx, Ly):
    return qmg.DeviceArray.from_host(cs.links_to_eo_gauge(links[0], links[1], Lx, Ly))


def up_field(F):
    return qmg.DeviceArray.from_host(hn.field_to_eo(F))


def up_spinors(X, Lx, Ly):
    return [qmg.DeviceArray.from_host(cs.grid_to_eo(x, Lx, Ly, 2)) for x in X]


def nan_field(n, dtype=np.float64):
    return qmg.DeviceArray.from_host(np.full(n, complex(np.nan, np.nan) if np.dtype(dtype).kind == "c" else np.nan, dtype=dtype))


def weighted_force(th, X, Y, w):
    fx, fy = np.zeros(th[0].shape), np.zeros(th[0].shape)
    for x, y, wj in zip(X, Y, w):
        g = hn.fermion_force_xy(th, x, y)
        fx, fy = fx + wj * g[0], fy + wj * g[1]
    return fx, fy


# ---- smearing ----
@pytest.mark.parametrize("Lx,Ly", SIZES)
def test_smear_levels_match_the_twin(Lx, Ly):
    """Four levels at rho = 0.1 from random phases, every level against exp(i theta^(k)) of the twin.  A level multiplies a unit number by a
    (cos, sin) pair: each costs a few 1e-16 in the link and in its modulus, and the error of level k enters the sines of level k + 1 with a
    factor of at most 1 + 4 rho: max abs 1e-13, | |U| - 1 | 1e-14."""
    th = random_setup(Lx, Ly, 400 + 7 * Lx + Ly)[0]
    n, n_levels = 2 * Lx * Ly, 4
    g0 = cs.links_to_eo_gauge(*hn.links(th), Lx, Ly)
    dg, dl = qmg.DeviceArray.from_host(g0), nan_field(n_levels * n, np.complex128)
    qmg.u1_stout_smear(dl, dg, Lx, Ly, RHO, n_levels)
    got, want = dl.to_host(), sn.levels(th, RHO, n_levels)
    worst = 0.0
    for k in range(n_levels):
        Ux, Uy = un.eo_gauge_to_links(got[k * n:(k + 1) * n], Lx, Ly)
        worst = max(worst, np.abs(Ux - np.exp(1j * want[k + 1][0])).max(), np.abs(Uy - np.exp(1j * want[k + 1][1])).max())
    mod = np.abs(np.abs(got) - 1.0).max()
    print("%dx%d: levels against the twin %.2e, | |U| - 1 | %.2e" % (Lx, Ly, worst, mod))
    assert max(np.abs(want[4][0] - th[0]).max(), np.abs(want[4][1] - th[1]).max()) > 0.1      # the smearing moved the links
    assert worst <= 1e-13 and mod <= 1e-14
    assert np.array_equal(bits(dg.to_host()), bits(g0))
    # no levels: nothing is touched
    dn = nan_field(n, np.complex128)
    qmg.u1_stout_smear(dn, dg, Lx, Ly, RHO, 0)
    assert np.isnan(dn.to_host().view(np.float64)).all() and np.array_equal(bits(dg.to_host()), bits(g0))


# ---- the force bilinear as a link field ----
@pytest.mark.parametrize("Lx,Ly", SIZES)
@pytest.mark.parametrize("n_poles", [1, 3, 17])
def test_fermion_force_matches_the_twin(Lx, Ly, n_poles):
    """F = sum_j w_j Ff(X_j, Y_j) into a NaN-prefilled field; 17 poles take a second launch that adds.  Relative l2 1e-12, the gate of the pole
    kick (a component is a sum of fewer than 20 n O(1) products)."""
    th, _, _, _, X, Y, w = random_setup(Lx, Ly, 500 + 11 * Lx + Ly + n_poles, n_poles)
    dg, dF = up_links(hn.links(th), Lx, Ly), nan_field(2 * Lx * Ly)
    qmg.hmc_fermion_force(dF, dg, up_spinors(X, Lx, Ly), up_spinors(Y, Lx, Ly), list(w), Lx, Ly)
    e = rel_l2(dF.to_host(), hn.field_to_eo(weighted_force(th, X, Y, w)))
    print("%dx%d n=%d: rel l2 of the force field %.2e" % (Lx, Ly, n_poles, e))
    assert e <= 1e-12


@pytest.mark.parametrize("Lx,Ly", SIZES)
def test_fermion_force_is_what_the_fused_kick_adds(Lx, Ly):
    """one pole of weight 1: pi - dt F on the host against pi + (two-flavour kick - gauge-only kick) of qmg_hmc_momentum_update, 1e-12"""
    th, pi, _, _, X, Y, _ = random_setup(Lx, Ly, 600 + Lx + Ly)
    dt = 0.37
    dg, dX, dY = up_links(hn.links(th), Lx, Ly), up_spinors(X, Lx, Ly), up_spinors(Y, Lx, Ly)
    dF, full, gauge_only = nan_field(2 * Lx * Ly), up_field(pi), up_field(pi)
    qmg.hmc_fermion_force(dF, dg, dX, dY, [1.0], Lx, Ly)
    qmg.hmc_momentum_update(full, dg, dX[0], dY[0], Lx, Ly, BETA, dt, 0)
    qmg.hmc_momentum_update(gauge_only, dg, None, None, Lx, Ly, BETA, dt, qmg.HMC_GAUGE_ONLY)
    p0 = hn.field_to_eo(pi)
    e = rel_l2(p0 - dt * dF.to_host(), p0 + (full.to_host() - gauge_only.to_host()))
    print("%dx%d: %.2e" % (Lx, Ly, e))
    assert e <= 1e-12


# ---- one level of the chain rule ----
@pytest.mark.parametrize("Lx,Ly", SIZES)
def test_level_kernel_matches_the_twin_and_is_symmetric(Lx, Ly):
    """F_out = J F_in into a NaN-prefilled field, relative l2 1e-12; <G, J F> = <J G, F> on the device's outputs to 1e-13 of |G| |J F| (the two
    sums of 2 Lx Ly products agree to rounding because J is symmetric term by term); F_in keeps its bits."""
    th, _, F, G, _, _, _ = random_setup(Lx, Ly, 700 + 13 * Lx + Ly)
    n = 2 * Lx * Ly
    dg, dF, dG, dJF, dJG = up_links(hn.links(th), Lx, Ly), up_field(F), up_field(G), nan_field(n), nan_field(n)
    qmg.u1_stout_force_level(dJF, dF, dg, Lx, Ly, RHO)
    qmg.u1_stout_force_level(dJG, dG, dg, Lx, Ly, RHO)
    JF, JG, f, g = dJF.to_host(), dJG.to_host(), hn.field_to_eo(F), hn.field_to_eo(G)
    e = rel_l2(JF, hn.field_to_eo(sn.jacobian_apply(th, F, RHO)))
    sym = abs(np.dot(g, JF) - np.dot(JG, f)) / (np.linalg.norm(g) * np.linalg.norm(JF))
    print("%dx%d: rel l2 %.2e, symmetry %.2e, |J F - F| / |F| = %.2f" % (Lx, Ly, e, sym, rel_l2(JF, f)))
    assert rel_l2(JF, f) > 0.01            # J is not the identity
    assert e <= 1e-12 and sym <= 1e-13
    assert np.array_equal(bits(dF.to_host()), bits(f))


# ---- the fused kick ----
@pytest.mark.parametrize("Lx,Ly", SIZES)
def test_fused_kick_matches_the_twin(Lx, Ly):
    """pi - dt (gauge force + J_0 F) in the momenta and in the implied force, 1e-12, as test_momentum_update_matches_the_twin_force; dt = 0
    returns the bits; rho = 0 is the gauge-only kick followed by pi -= dt F on the host."""
    th, pi, F, _, _, _, _ = random_setup(Lx, Ly, 800 + 17 * Lx + Ly)
    dt = 0.37
    fg, jf = hn.gauge_force(th, BETA), sn.jacobian_apply(th, F, RHO)
    f = (fg[0] + jf[0], fg[1] + jf[1])
    want, p0 = hn.field_to_eo((pi[0] - dt * f[0], pi[1] - dt * f[1])), hn.field_to_eo(pi)
    dg, dF, dp = up_links(hn.links(th), Lx, Ly), up_field(F), up_field(pi)
    qmg.hmc_momentum_update_stout(dp, dg, dF, Lx, Ly, BETA, RHO, dt)
    got = dp.to_host()
    e_pi, e_f = rel_l2(got, want), rel_l2((p0 - got) / dt, hn.field_to_eo(f))
    print("%dx%d: rel l2 of the new momenta %.2e, of the force %.2e" % (Lx, Ly, e_pi, e_f))
    assert e_pi <= 1e-12 and e_f <= 1e-12
    assert np.array_equal(bits(dF.to_host()), bits(hn.field_to_eo(F)))
    same = up_field(pi)
    qmg.hmc_momentum_update_stout(same, dg, dF, Lx, Ly, BETA, RHO, 0.0)
    assert np.array_equal(bits(same.to_host()), bits(p0))
    plain, thin = up_field(pi), up_field(pi)
    qmg.hmc_momentum_update_stout(plain, dg, dF, Lx, Ly, BETA, 0.0, dt)
    qmg.hmc_momentum_update(thin, dg, None, None, Lx, Ly, BETA, dt, qmg.HMC_GAUGE_ONLY)
    e0 = rel_l2(plain.to_host(), thin.to_host() - dt * hn.field_to_eo(F))
    print("%dx%d: rho = 0 against the gauge-only kick and an axpy %.2e" % (Lx, Ly, e0))
    assert e0 <= 1e-12


def device_chain(dg, pi, dX, dY, w, Lx, Ly, rho, n_levels, beta, dt):
    """StoutLinks::kick (include/qmg/stout.hpp) call by call: smear, the bilinear on the top level, n_levels - 1 level calls, the fused kick"""
    n = 2 * Lx * Ly
    dl, Fa, Fb, dp = nan_field(n_levels * n, np.complex128), nan_field(n), nan_field(n), up_field(pi)
    qmg.u1_stout_smear(dl, dg, Lx, Ly, rho, n_levels)
    qmg.hmc_fermion_force(Fa, dl.offset((n_levels - 1) * n), dX, dY, list(w), Lx, Ly)
    for k in range(n_levels - 1, 0, -1):
        qmg.u1_stout_force_level(Fb, Fa, dl.offset((k - 1) * n), Lx, Ly, rho)
        Fa, Fb = Fb, Fa
    qmg.hmc_momentum_update_stout(dp, dg, Fa, Lx, Ly, beta, rho, dt)
    return dp.to_host()


@pytest.mark.parametrize("Lx,Ly", [(6, 4), (34, 10), (64, 64)])
def test_the_whole_chain_matches_the_twin_and_is_gauge_covariant(Lx, Ly):
    """Three levels, three poles: the kick assembled as the facade assembles it against the twin's pull-back of the force on the fat links, and
    against itself with U -> g U g^dag, X -> g X, Y -> g Y (qmg_u1_gauge_transform): the momenta must not move.  1e-12 both."""
    n_levels, dt = 3, 0.37
    th, pi, _, _, X, Y, w = random_setup(Lx, Ly, 900 + Lx, 3)
    lv = sn.levels(th, RHO, n_levels)
    fg, ff = hn.gauge_force(th, BETA), sn.pull_back(lv, weighted_force(lv[-1], X, Y, w), RHO)
    want = hn.field_to_eo((pi[0] - dt * (fg[0] + ff[0]), pi[1] - dt * (fg[1] + ff[1])))
    dg = up_links(hn.links(th), Lx, Ly)
    plain = device_chain(dg, pi, up_spinors(X, Lx, Ly), up_spinors(Y, Lx, Ly), w, Lx, Ly, RHO, n_levels, BETA, dt)
    g = un.random_transform(Lx, Ly, 31)
    qmg.u1_gauge_transform(dg, qmg.DeviceArray.from_host(cs.grid_to_eo(g[:, :, None], Lx, Ly, 1)), Lx, Ly)
    moved = device_chain(dg, pi, up_spinors([g[:, :, None] * x for x in X], Lx, Ly), up_spinors([g[:, :, None] * y for y in Y], Lx, Ly), w, Lx, Ly, RHO, n_levels, BETA, dt)
    thin = hn.field_to_eo(weighted_force(th, X, Y, w))
    e, c = rel_l2(plain, want), rel_l2(moved, plain)
    print("%dx%d: chain against the twin %.2e, transformed against plain %.2e; smeared force against thin %.2f" % (Lx, Ly, e, c, rel_l2(hn.field_to_eo(ff), thin)))
    assert rel_l2(hn.field_to_eo(ff), thin) > 0.1      # an unsmeared force would not pass
    assert e <= 1e-12 and c <= 1e-12


def test_argument_checks():
    """every refusal raises and leaves the outputs as they were"""
    Lx = Ly = 4
    n = 2 * Lx * Ly
    th, pi, F, _, X, Y, w = random_setup(Lx, Ly, 5, 2)
    dg, dF, dp, dX, dY = up_links(hn.links(th), Lx, Ly), up_field(F), up_field(pi), up_spinors(X, Lx, Ly), up_spinors(Y, Lx, Ly)
    dl, dout = nan_field(2 * n, np.complex128), nan_field(n)
    nan, inf = float("nan"), float("inf")
    bad = [
        lambda: qmg.u1_stout_smear(dl, dg, 3, Ly, RHO, 2),                    # odd extent
        lambda: qmg.u1_stout_smear(dl, dg, Lx, 0, RHO, 2),                    # no extent
        lambda: qmg.u1_stout_smear(None, dg, Lx, Ly, RHO, 2),                 # no levels
        lambda: qmg.u1_stout_smear(dl, None, Lx, Ly, RHO, 2),                 # no links
        lambda: qmg.u1_stout_smear(dl, dg, Lx, Ly, RHO, -1),                  # negative count
        lambda: qmg.u1_stout_smear(dl, dg, Lx, Ly, nan, 2),                   # rho not a number
        lambda: qmg.u1_stout_smear(dl, dg, Lx, Ly, inf, 2),                   # rho not finite
        lambda: qmg.u1_stout_smear(dg, dg, Lx, Ly, RHO, 1),                   # levels on the links
        lambda: qmg.hmc_fermion_force(dout, dg, dX, dY, list(w), 3, Ly),      # odd extent
        lambda: qmg.hmc_fermion_force(None, dg, dX, dY, list(w), Lx, Ly),     # no force field
        lambda: qmg.hmc_fermion_force(dout, None, dX, dY, list(w), Lx, Ly),   # no links
        lambda: qmg.hmc_fermion_force(dout, dg, None, dY, list(w), Lx, Ly),   # poles without X
        lambda: qmg.hmc_fermion_force(dout, dg, dX, [dY[0], None], list(w), Lx, Ly),    # a null spinor in the list
        lambda: qmg.hmc_fermion_force(dout, dg, dX, dY, None, Lx, Ly, n_poles=2),       # no weights
        lambda: qmg.hmc_fermion_force(dout, dg, dX, dY, list(w), Lx, Ly, n_poles=-1),   # negative count
        lambda: qmg.u1_stout_force_level(dout, dF, dg, Lx, 5, RHO),           # odd extent
        lambda: qmg.u1_stout_force_level(None, dF, dg, Lx, Ly, RHO),
        lambda: qmg.u1_stout_force_level(dout, None, dg, Lx, Ly, RHO),
        lambda: qmg.u1_stout_force_level(dout, dF, None, Lx, Ly, RHO),
        lambda: qmg.u1_stout_force_level(dout, dF, dg, Lx, Ly, nan),
        lambda: qmg.u1_stout_force_level(dF, dF, dg, Lx, Ly, RHO),            # in place
        lambda: qmg.hmc_momentum_update_stout(dp, dg, dF, -4, Ly, BETA, RHO, 0.1),
        lambda: qmg.hmc_momentum_update_stout(None, dg, dF, Lx, Ly, BETA, RHO, 0.1),
        lambda: qmg.hmc_momentum_update_stout(dp, None, dF, Lx, Ly, BETA, RHO, 0.1),
        lambda: qmg.hmc_momentum_update_stout(dp, dg, None, Lx, Ly, BETA, RHO, 0.1),
        lambda: qmg.hmc_momentum_update_stout(dp, dg, dF, Lx, Ly, BETA, inf, 0.1),
        lambda: qmg.hmc_momentum_update_stout(dp, dg, dF, Lx, Ly, BETA, RHO, nan),
        lambda: qmg.hmc_momentum_update_stout(dp, dg, dp, Lx, Ly, BETA, RHO, 0.1),      # the force on the momenta
    ]
    for call in bad:
        with pytest.raises(qmg.QmgError):
            call()
    assert np.isnan(dl.to_host().view(np.float64)).all() and np.isnan(dout.to_host()).all()
    assert np.array_equal(bits(dp.to_host()), bits(hn.field_to_eo(pi))) and np.array_equal(bits(dF.to_host()), bits(hn.field_to_eo(F)))
    assert np.array_equal(bits(dg.to_host()), bits(cs.links_to_eo_gauge(*hn.links(th), Lx, Ly)))


# ---- the facade on the 32^2 fixture ----
def fixture_setup(golden_dir):
    """test_gpu_hmc.fixture_setup's fields"""
    L = 32
    th = hn.file_phases(os.path.join(golden_dir, FIX), L, L)
    rng = np.random.default_rng(2024)
    pi = (rng.standard_normal((L, L)), rng.standard_normal((L, L)))
    eta = (rng.standard_normal((L, L, 2)) + 1j * rng.standard_normal((L, L, 2))) / np.sqrt(2.0)
    return L, th, pi, eta


def parity_fields(tmp_path, L, stdout):
    legs = {m.group(1): (float(m.group(2)), int(m.group(3)), int(m.group(4))) for m in re.finditer(r"\[MD\] (\w+)\s+dH (\S+) cg (\d+) converged (\d)", stdout)}
    fields = {k: hn.eo_to_field(np.fromfile(str(tmp_path / (k + ".bin"))), L, L) for k in ("theta_fwd", "pi_fwd", "theta_back", "pi_back")}
    return legs, fields


def run_hmc_parity(tmp_path, golden_dir, pi, phi, L, stout):
    """32^2 beta-6.0 fixture, m = 0.1, two flavours, tau = 1, 20 steps, CG 1e-12; stout: the trailing arguments, or none"""
    os.makedirs(str(tmp_path), exist_ok=True)
    hn.field_to_eo(pi).astype(np.float64).tofile(str(tmp_path / "pi.bin"))
    cs.grid_to_eo(phi, L, L, 2).tofile(str(tmp_path / "phi.bin"))
    out = subprocess.run([os.path.join(DRIVERS, "hmc_parity"), str(L), os.path.join(golden_dir, FIX), str(tmp_path), "6.0", "0.1", "2", "1.0", "20", "1e-12"] + list(stout),
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    return parity_fields(tmp_path, L, out.stdout)


def max_abs(a, b):
    return max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max())


def test_md_evolve_with_stout_levels_matches_the_twin_and_is_reversible(tmp_path, golden_dir):
    """32^2 beta-6.0 fixture, m = 0.1, tau = 1, 20 steps, two levels at rho = 0.1, device CG eps 1e-12; the twin runs its own CG to 1e-13.

    Gates, fixed on the CPU before the device was run, by the rule of test_md_evolve_matches_the_twin_and_is_reversible: the twin at CG eps 1e-12
    against the twin at 1e-13 on these inputs differs by 4.1e-12 in the end phases (max abs; they move by up to 2.76) and by 2.7e-11 in dH
    (dH = 0.051705444741) -- solver error alone.  The device CG stops at another iterate, so the gates are ten times that: 4.1e-11 on the
    phases and 2.7e-10 on dH.  Forward, momenta negated, back: the twin at eps 1e-12 returns to its start within 7.9e-14 (max abs over the
    phases); the device gate is ten times that, 7.9e-13.  The twin's smeared end phases differ from its unsmeared ones by 0.42.
    Measured on an MI355X: end phases 4.1e-12, dH 2.1e-11, forward-back 2.0e-14 (6662 CG iterations per leg; 6035 on the thin links)."""
    L, th, pi, eta = fixture_setup(golden_dir)
    phi = hn.Ddag(eta, th, 0.1)
    legs, f = run_hmc_parity(tmp_path / "stout", golden_dir, pi, phi, L, ["2", "0.1"])
    thin_legs, thin = run_hmc_parity(tmp_path / "thin", golden_dir, pi, phi, L, [])
    assert legs["forward"][2] == 1 and legs["back"][2] == 1
    th1, pi1, dH = sn.md_dH(th, pi, 6.0, 1.0, 20, phi, 0.1, 0.1, 2, None, hn.make_cg(1e-13))
    d_th, d_pi, d_back = max_abs(f["theta_fwd"], th1), max_abs(f["pi_fwd"], pi1), max_abs(f["theta_back"], th)
    apart = max_abs(f["theta_fwd"], thin["theta_fwd"])
    print("md_evolve vs twin: end phases %.2e, end momenta %.2e, dH device %.12f twin %.12f (diff %.2e); forward-back %.2e; CG iterations %d (thin links: %d); "
          "end phases against the thin-link run %.3f" % (d_th, d_pi, legs["forward"][0], dH, abs(legs["forward"][0] - dH), d_back, legs["forward"][1], thin_legs["forward"][1], apart))
    assert np.abs(th1[0] - th[0]).max() > 1.0
    assert apart > 1e-3
    assert d_th <= 4.1e-11
    assert abs(legs["forward"][0] - dH) <= 2.7e-10
    assert d_back <= 7.9e-13
    assert abs(legs["back"][0] + legs["forward"][0]) <= 2 * 2.7e-10      # the way back undoes the energy change


def test_zero_levels_passed_explicitly_reproduce_the_thin_run_bit_for_bit(tmp_path, golden_dir):
    L, th, pi, eta = fixture_setup(golden_dir)
    phi = hn.Ddag(eta, th, 0.1)
    run_hmc_parity(tmp_path / "none", golden_dir, pi, phi, L, [])
    run_hmc_parity(tmp_path / "zero", golden_dir, pi, phi, L, ["0", "0.1"])
    for name in ("theta_fwd", "pi_fwd", "theta_back", "pi_back"):
        a, b = (tmp_path / "none" / (name + ".bin")).read_bytes(), (tmp_path / "zero" / (name + ".bin")).read_bytes()
        assert len(a) == 8 * 2 * L * L and a == b, name


def test_md_evolve_one_flavour_with_a_stout_level_matches_the_twin(tmp_path, golden_dir):
    """The shape of test_md_evolve_one_flavour_matches_the_twin_and_is_reversible (32^2 beta-6.0 fixture, m = 0.1, tau = 1, 20 steps, n = 8 on
    [0.152, 4.1], device multi-shift CG at 1e-12, the twin's at 1e-13) with one level at rho = 0.1.

    Gates, fixed on the CPU before the device was run, by the same rule: the twin at 1e-12 against the twin at 1e-13 differs by 8.5e-13 in the
    end phases (they move by up to 2.49) and by 3.5e-11 in dH (dH = 0.053088716786); the device gates are ten times that, 8.5e-12 and 3.5e-10.
    Forward-back of the twin at 1e-12: 5.7e-15, device gate 5.7e-14.  The twin's smeared end phases differ from its unsmeared ones by 0.09.
    Measured on an MI355X: end phases 8.5e-13, dH 3.5e-11, forward-back 7.1e-15 (6504 multi-shift iterations per leg)."""
    L, th, pi, eta = fixture_setup(golden_dir)
    z = rn.zolotarev(8, 0.152, 4.1)
    phi = rn.heatbath(z, th, eta, 0.1, rn.make_cg_m(1e-13))
    hn.field_to_eo(pi).astype(np.float64).tofile(str(tmp_path / "pi.bin"))
    cs.grid_to_eo(phi, L, L, 2).tofile(str(tmp_path / "phi.bin"))
    out = subprocess.run([os.path.join(DRIVERS, "rhmc_parity"), "md", str(L), os.path.join(golden_dir, FIX), str(tmp_path), "6.0", "0.1", "1.0", "20", "1e-12", "8", "0.152", "0",
                          "1", "0.1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    legs, f = parity_fields(tmp_path, L, out.stdout)
    assert legs["forward"][2] == 1 and legs["back"][2] == 1
    th1, pi1, dH = sn.md_dH(th, pi, 6.0, 1.0, 20, phi, 0.1, 0.1, 1, z, rn.make_cg_m(1e-13))
    d_th, d_pi, d_back = max_abs(f["theta_fwd"], th1), max_abs(f["pi_fwd"], pi1), max_abs(f["theta_back"], th)
    print("md_evolve vs twin: end phases %.2e, end momenta %.2e, dH device %.12f twin %.12f (diff %.2e); forward-back %.2e; multi-shift iterations %d"
          % (d_th, d_pi, legs["forward"][0], dH, abs(legs["forward"][0] - dH), d_back, legs["forward"][1]))
    assert np.abs(th1[0] - th[0]).max() > 1.0
    assert d_th <= 8.5e-12
    assert abs(legs["forward"][0] - dH) <= 3.5e-10
    assert d_back <= 5.7e-14
    assert abs(legs["back"][0] + legs["forward"][0]) <= 2 * 3.5e-10


# ---- the driver ----
def run_driver(args, poison=False):
    env = dict(os.environ)
    env.pop("QMG_MALLOC_POISON", None)
    if poison:
        env["QMG_MALLOC_POISON"] = "1"
    out = subprocess.run([os.path.join(DRIVERS, "schwinger_hmc")] + [str(a) for a in args], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                         timeout=300)
    rows = [(int(m.group(1)), float(m.group(2)), int(m.group(3)), float(m.group(4)), float(m.group(5)), int(m.group(6)))
            for m in re.finditer(r"\[HMC\] (\d+) dH (\S+) acc (\d) plaq (\S+) Q (\S+) cg (\d+)", out.stdout)]
    return out, rows


def test_smeared_two_flavour_run_through_the_driver(tmp_path):
    """16^2, beta 4, m 0.1, 20 steps, 10 trajectories from a heatbath start with two levels at rho = 0.1; once more under QMG_MALLOC_POISON=1
    (DESIGN 10.12), which must print the same lines; and the thin-link run beside it for the CG counts, which are printed, not gated.  The
    written smeared links are stout_smear_u1's: they are held to the device kernel's top level and to the twin's on the written thin links.
    Measured on an MI355X: acceptance 0.9, plaquette 0.8578 thin and 0.9656 smeared, 3211 .. 3369 CG iterations per trajectory against
    3155 .. 3297 of the thin-link run from the same start (the smeared run takes 2 % more, not fewer, at this mass and size)."""
    line = [16, 4.0, 0.1, 2, 10, 0, 20, 99]
    out, rows = run_driver(line + [tmp_path / "out.dat", "heatbath", "stout", 2, 0.1])
    print(out.stdout[-2500:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    assert "[QMG-ERROR]" not in out.stdout and not re.search(r"(?<![a-z])nan(?![a-z])", out.stdout, re.I)
    assert len(rows) == 10 and re.search(r"unconverged 0\b", out.stdout) and all(r[5] > 0 for r in rows)
    assert float(np.mean([r[2] for r in rows])) > 0.5
    head = re.search(r"^\[STOUT\] levels (\d+) rho (\S+)$", out.stdout, re.M)
    assert head and int(head.group(1)) == 2 and float(head.group(2)) == 0.1
    back = re.search(r"^\[STOUT-READBACK\] plaq (\S+) fat (\S+)$", out.stdout, re.M)
    assert back and abs(float(back.group(1)) - rows[-1][3]) < 1e-9
    assert float(back.group(2)) > float(back.group(1))
    # the written links: thin and smeared
    L, n = 16, 2 * 16 * 16
    th = hn.file_phases(str(tmp_path / "out.dat"), L, L)
    fat = hn.file_phases(str(tmp_path / "out.dat.stout"), L, L)
    V = sn.smear(th, 0.1, 2)
    d_twin = max(np.abs(np.exp(1j * fat[k]) - np.exp(1j * V[k])).max() for k in range(2))
    dl = nan_field(2 * n, np.complex128)
    qmg.u1_stout_smear(dl, up_links(hn.links(th), L, L), L, L, 0.1, 2)
    Ux, Uy = un.eo_gauge_to_links(dl.to_host()[n:], L, L)
    d_dev = max(np.abs(np.exp(1j * fat[0]) - Ux).max(), np.abs(np.exp(1j * fat[1]) - Uy).max())
    print("smeared links written by the driver: against the twin %.2e, against the kernel's top level %.2e; fat plaquette %.6f (twin %.6f), thin %.6f"
          % (d_twin, d_dev, float(back.group(2)), np.cos(hn.plaquette_angle(V)).mean(), float(back.group(1))))
    assert d_twin <= 1e-13 and d_dev <= 1e-13
    assert abs(np.cos(hn.plaquette_angle(V)).mean() - float(back.group(2))) < 1e-9
    # under the poison key: the same lines
    pout, prows = run_driver(line + [tmp_path / "poison.dat", "heatbath", "stout", 2, 0.1], poison=True)
    assert pout.returncode == 0, pout.stdout[-2000:] + pout.stderr
    keep = lambda s: re.findall(r"^\[(?:HMC|HMC-FINAL|HMC-READBACK|STOUT|STOUT-READBACK)\] .*$", s, re.M)
    assert keep(out.stdout) == keep(pout.stdout) and len(keep(out.stdout)) == 14
    assert (tmp_path / "out.dat").read_bytes() == (tmp_path / "poison.dat").read_bytes()
    # the thin-link run, for the record
    tout, trows = run_driver(line + [tmp_path / "thin.dat", "heatbath"])
    assert tout.returncode == 0 and len(trows) == 10
    print("CG iterations per trajectory, smeared: %s\n                               thin:    %s" % ([r[5] for r in rows], [r[5] for r in trows]))


def test_the_driver_refuses_what_the_smearing_cannot_take(tmp_path):
    for tail, code in ((["staggered", "stout", 2, 0.1], None), (["stout", 9, 0.1], 3), (["stout", -1, 0.1], 3), (["stout", 2, -0.1], 3), (["stout", 2, "nan"], 3)):
        out, rows = run_driver([8, 4.0, 0.2, 2, 1, 0, 4, 99, tmp_path / "a.dat", "heatbath"] + tail)
        assert out.returncode != 0 and not rows and out.stdout.count("[QMG-ERROR]") == 1, out.stdout[-1000:]
        if code is not None:
            assert out.returncode == code
