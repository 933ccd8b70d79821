"""Two-flavour Wilson HMC for the Schwinger model on the device (csrc/qmg_hmc.hip, include/qmg/hmc.hpp, drivers/schwinger_hmc.cpp).

The yardstick is the numpy twin tests/hmc_numpy.py (np.roll on (x, y) grids; pinned by finite differences of its own action, gauge covariance,
reversibility and the dt^2 law in test_host_hmc.py), never the code under test:
  * the force kernel against the twin force with RANDOM spinors X, Y (no solver tolerance enters), relative l2 <= 1e-12: a component is a sum of
    fewer than 20 O(1) fp64 products, and the one-pass U(1) kernels are held to 5e-16 .. 1e-13;
  * the link update against `theta + dt * pi` to 1e-15, |U| = 1 to 1e-15;
  * SchwingerHMC::md_evolve on the 32^2 beta-6.0 fixture against the twin's leapfrog on the same momenta and pseudofermion;
  * reversibility, gauge covariance, the exact pure-gauge plaquette <cos P> = I1(beta)/I0(beta), and a two-flavour run through the driver."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import coordspace as cs
import hmc_numpy as hn
import u1_numpy as un

qmg = importlib.import_module("quantum-mg_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVERS = os.path.join(ROOT, "quantum-mg_amd", "drivers")
SIZES = [(2, 2), (2, 6), (6, 2), (6, 4), (34, 10), (64, 64)]   # (2, 6): xl == xr == xh with distinct rows; (6, 2): yp == ym with distinct columns
BETA, MASS = 3.0, 0.1


@pytest.fixture(scope="module", autouse=True)
def _device():
    qmg.build()
    subprocess.check_call(["make", "-C", DRIVERS, "-j4"], stdout=subprocess.DEVNULL)
    qmg.init(0)
    yield
    qmg.sync()


def rel_l2(a, b):
    return float(np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(np.ravel(b)))


def random_setup(Lx, Ly, seed):
    rng = np.random.default_rng(seed)
    th = (rng.uniform(-np.pi, np.pi, (Lx, Ly)), rng.uniform(-np.pi, np.pi, (Lx, Ly)))
    pi = (rng.standard_normal((Lx, Ly)), rng.standard_normal((Lx, Ly)))
    X = rng.standard_normal((Lx, Ly, 2)) + 1j * rng.standard_normal((Lx, Ly, 2))
    Y = rng.standard_normal((Lx, Ly, 2)) + 1j * rng.standard_normal((Lx, Ly, 2))
    return th, pi, X, Y


def device_kick(th_links, pi, X, Y, Lx, Ly, beta, dt, flags):
    """qmg_hmc_momentum_update on uploaded grids; returns the new momenta as device-layout doubles"""
    Ux, Uy = th_links
    dg = qmg.DeviceArray.from_host(cs.links_to_eo_gauge(Ux, Uy, Lx, Ly))
    dp = qmg.DeviceArray.from_host(hn.field_to_eo(pi))
    dX = None if X is None else qmg.DeviceArray.from_host(cs.grid_to_eo(X, Lx, Ly, 2))
    dY = None if Y is None else qmg.DeviceArray.from_host(cs.grid_to_eo(Y, Lx, Ly, 2))
    qmg.hmc_momentum_update(dp, dg, dX, dY, Lx, Ly, beta, dt, flags)
    return dp.to_host()


@pytest.mark.parametrize("Lx,Ly", SIZES)
@pytest.mark.parametrize("fermions", [False, True])
def test_momentum_update_matches_the_twin_force(Lx, Ly, fermions):
    th, pi, X, Y = random_setup(Lx, Ly, 100 + Lx + Ly)
    dt = 0.37
    f = hn.gauge_force(th, BETA)
    if fermions:
        g = hn.fermion_force_xy(th, X, Y)
        f = (f[0] + g[0], f[1] + g[1])
    want = hn.field_to_eo((pi[0] - dt * f[0], pi[1] - dt * f[1]))
    pi0 = hn.field_to_eo(pi)
    got = device_kick(hn.links(th), pi, X if fermions else None, Y if fermions else None, Lx, Ly, BETA, dt, 0 if fermions else qmg.HMC_GAUGE_ONLY)
    e_pi, e_f = rel_l2(got, want), rel_l2((pi0 - got) / dt, hn.field_to_eo(f))
    print("%dx%d fermions=%s: rel l2 of the new momenta %.2e, of the force %.2e" % (Lx, Ly, fermions, e_pi, e_f))
    assert e_pi <= 1e-12 and e_f <= 1e-12
    # dt = 0 leaves the momenta bit-identical
    same = device_kick(hn.links(th), pi, X if fermions else None, Y if fermions else None, Lx, Ly, BETA, 0.0, 0 if fermions else qmg.HMC_GAUGE_ONLY)
    assert np.array_equal(same.view(np.uint64), pi0.view(np.uint64))


def test_momentum_update_argument_checks():
    Lx = Ly = 4
    th, pi, X, Y = random_setup(Lx, Ly, 5)
    dg = qmg.DeviceArray.from_host(cs.links_to_eo_gauge(*hn.links(th), Lx, Ly))
    dp = qmg.DeviceArray.from_host(hn.field_to_eo(pi))
    with pytest.raises(qmg.QmgError):       # the full form needs X and Y
        qmg.hmc_momentum_update(dp, dg, None, None, Lx, Ly, BETA, 0.1, 0)
    with pytest.raises(qmg.QmgError):       # odd extent
        qmg.hmc_momentum_update(dp, dg, None, None, 3, Ly, BETA, 0.1, qmg.HMC_GAUGE_ONLY)
    with pytest.raises(qmg.QmgError):       # unknown flag
        qmg.hmc_momentum_update(dp, dg, None, None, Lx, Ly, BETA, 0.1, 2)
    assert np.array_equal(dp.to_host(), hn.field_to_eo(pi))


@pytest.mark.parametrize("Lx,Ly", SIZES)
def test_link_update_matches_the_twin(Lx, Ly):
    th, pi, _, _ = random_setup(Lx, Ly, 200 + Lx)
    dt = 0.05
    n = 2 * Lx * Ly
    dth, dpi, dg = qmg.DeviceArray.from_host(hn.field_to_eo(th)), qmg.DeviceArray.from_host(hn.field_to_eo(pi)), qmg.DeviceArray(n)
    qmg.hmc_link_update(dth, dg, dpi, n, dt)
    want = hn.field_to_eo((th[0] + dt * pi[0], th[1] + dt * pi[1]))
    got, U = dth.to_host(), dg.to_host()
    d_th, d_mod, d_u = np.abs(got - want).max(), np.abs(np.abs(U) - 1.0).max(), np.abs(U - np.exp(1j * want)).max()
    print("%dx%d: phases %.2e, | |U| - 1 | %.2e, U - exp(i theta) %.2e" % (Lx, Ly, d_th, d_mod, d_u))
    assert d_th <= 1e-15 and d_mod <= 1e-15 and d_u <= 1e-15
    assert np.array_equal(dpi.to_host(), hn.field_to_eo(pi))


def test_momentum_refresh_is_unit_gaussian_and_keyed_by_seed_and_trajectory():
    """qmg_gaussian on the field viewed as complex: unit variance in EACH real component (mean within 5 sigma, variance within 5 sigma of
    sqrt(2/n)), a function of (seed, trajectory) alone."""
    n = 2 * 256 * 256
    a, b, c, d = (qmg.DeviceArray(n, np.float64) for _ in range(4))
    qmg.hmc_momentum_refresh(a, n, 7, 3)
    qmg.hmc_momentum_refresh(b, n, 7, 3)
    qmg.hmc_momentum_refresh(c, n, 7, 4)
    qmg.hmc_momentum_refresh(d, n, 8, 3)
    ha, hb, hc, hd = a.to_host(), b.to_host(), c.to_host(), d.to_host()
    assert np.array_equal(ha, hb) and not np.array_equal(ha, hc) and not np.array_equal(ha, hd)
    for part in (ha[0::2], ha[1::2]):
        m = part.size
        assert abs(part.mean()) < 5.0 / np.sqrt(m) and abs(part.var() - 1.0) < 5.0 * np.sqrt(2.0 / m)
    assert abs(np.corrcoef(ha, hc)[0, 1]) < 5.0 / np.sqrt(n)
    assert abs(qmg.norm2sq(a, n // 2) - np.sum(ha ** 2)) < 1e-12 * n      # the kinetic energy's reduction on the same view


def run_parity(tmp_path, golden_dir, th_name, pi, phi, L, beta, mass, nf, tau, n_steps, eps):
    hn.field_to_eo(pi).astype(np.float64).tofile(str(tmp_path / "pi.bin"))
    cs.grid_to_eo(phi, L, L, 2).tofile(str(tmp_path / "phi.bin"))
    out = subprocess.run([os.path.join(DRIVERS, "hmc_parity"), str(L), os.path.join(golden_dir, th_name), str(tmp_path), repr(beta), repr(mass), str(nf), repr(tau),
                          str(n_steps), repr(eps)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    legs = {m.group(1): (float(m.group(2)), int(m.group(3)), int(m.group(4))) for m in re.finditer(r"\[MD\] (\w+)\s+dH (\S+) cg (\d+) converged (\d)", out.stdout)}
    fields = {k: hn.eo_to_field(np.fromfile(str(tmp_path / (k + ".bin"))), L, L) for k in ("theta_fwd", "pi_fwd", "theta_back", "pi_back")}
    return legs, fields


def fixture_setup(golden_dir):
    L = 32
    th = hn.file_phases(os.path.join(golden_dir, "l32t32b60_heatbath.dat"), L, L)
    rng = np.random.default_rng(2024)
    pi = (rng.standard_normal((L, L)), rng.standard_normal((L, L)))
    eta = (rng.standard_normal((L, L, 2)) + 1j * rng.standard_normal((L, L, 2))) / np.sqrt(2.0)
    return L, th, pi, hn.Ddag(eta, th, 0.1)


def test_md_evolve_matches_the_twin_and_is_reversible(tmp_path, golden_dir):
    """32^2 beta-6.0 fixture, m = 0.1, tau = 1, 20 steps, device CG eps 1e-12; the twin runs its own CG to 1e-13.

    Gates, fixed before the device was run: the twin at CG eps 1e-12 against the twin at 1e-13 on these inputs differs by 5.3e-12 in the end
    phases (max abs; they move by up to 2.8) and by 8.6e-12 in dH (dH = -0.25243) -- solver error alone.  The device CG stops at another
    iterate, so the gates are ten times that: 5.3e-11 on the phases and 8.6e-11 on dH.  Forward, momenta negated, back: the twin at eps 1e-12
    returns to its start within 7.1e-15 (max abs over the phases); the device gate is ten times that, 7.1e-14.
    Measured on an MI355X: end phases 5.3e-12, dH 6.8e-12, forward-back 1.1e-14."""
    L, th, pi, phi = fixture_setup(golden_dir)
    legs, f = run_parity(tmp_path, golden_dir, "l32t32b60_heatbath.dat", pi, phi, L, 6.0, 0.1, 2, 1.0, 20, 1e-12)
    assert legs["forward"][2] == 1 and legs["back"][2] == 1
    th1, pi1, dH = hn.md_dH(th, pi, 6.0, 1.0, 20, phi, 0.1, hn.make_cg(1e-13))
    d_th = max(np.abs(f["theta_fwd"][0] - th1[0]).max(), np.abs(f["theta_fwd"][1] - th1[1]).max())
    d_pi = max(np.abs(f["pi_fwd"][0] - pi1[0]).max(), np.abs(f["pi_fwd"][1] - pi1[1]).max())
    d_back = max(np.abs(f["theta_back"][0] - th[0]).max(), np.abs(f["theta_back"][1] - th[1]).max())
    print("md_evolve vs twin: end phases %.2e, end momenta %.2e, dH device %.12f twin %.12f (diff %.2e); forward-back %.2e; CG iterations %d"
          % (d_th, d_pi, legs["forward"][0], dH, abs(legs["forward"][0] - dH), d_back, legs["forward"][1]))
    assert np.abs(th1[0] - th[0]).max() > 1.0
    assert d_th <= 5.3e-11
    assert abs(legs["forward"][0] - dH) <= 8.6e-11
    assert d_back <= 7.1e-14
    assert abs(legs["back"][0] + legs["forward"][0]) <= 2 * 8.6e-11      # the way back undoes the energy change


def test_pure_gauge_md_evolve_matches_the_twin(tmp_path, golden_dir):
    """No solver at all: the device leapfrog against the twin's, to rounding.  Each of the 40 link updates rounds a phase of magnitude up to 8 by
    half an ulp (4.4e-16), 1.8e-14 in the linear worst case, in two independent runs; a perturbation grows along the trajectory by at most
    exp(tau sqrt(4 beta)) = 130 (four plaquette terms of curvature beta per link): 5e-12."""
    L, th, pi, phi = fixture_setup(golden_dir)
    legs, f = run_parity(tmp_path, golden_dir, "l32t32b60_heatbath.dat", pi, phi, L, 6.0, 0.1, 0, 1.0, 40, 1e-12)
    th1, pi1, dH = hn.md_dH(th, pi, 6.0, 1.0, 40)
    d_th = max(np.abs(f["theta_fwd"][0] - th1[0]).max(), np.abs(f["theta_fwd"][1] - th1[1]).max())
    d_back = max(np.abs(f["theta_back"][0] - th[0]).max(), np.abs(f["theta_back"][1] - th[1]).max())
    print("pure gauge: end phases %.2e, dH device %.12f twin %.12f, forward-back %.2e" % (d_th, legs["forward"][0], dH, d_back))
    assert d_th <= 5e-12 and d_back <= 5e-12
    assert abs(legs["forward"][0] - dH) <= 1e-9        # differences of sums of 2048 O(1) terms of size ~1e3


@pytest.mark.parametrize("Lx,Ly", [(6, 4), (34, 10), (64, 64)])
def test_force_is_gauge_covariant_on_the_device(Lx, Ly):
    th, pi, X, Y = random_setup(Lx, Ly, 300 + Lx)
    Ux, Uy = hn.links(th)
    g = un.random_transform(Lx, Ly, 31)
    dg = qmg.DeviceArray.from_host(cs.links_to_eo_gauge(Ux, Uy, Lx, Ly))
    qmg.u1_gauge_transform(dg, qmg.DeviceArray.from_host(cs.grid_to_eo(g[:, :, None], Lx, Ly, 1)), Lx, Ly)
    dp = qmg.DeviceArray.from_host(hn.field_to_eo(pi))
    qmg.hmc_momentum_update(dp, dg, qmg.DeviceArray.from_host(cs.grid_to_eo(g[:, :, None] * X, Lx, Ly, 2)),
                            qmg.DeviceArray.from_host(cs.grid_to_eo(g[:, :, None] * Y, Lx, Ly, 2)), Lx, Ly, BETA, 0.37, 0)
    plain = device_kick((Ux, Uy), pi, X, Y, Lx, Ly, BETA, 0.37, 0)
    e = rel_l2(dp.to_host(), plain)
    print("%dx%d: transformed against plain %.2e" % (Lx, Ly, e))
    assert e <= 1e-12


def run_driver(args, timeout):
    out = subprocess.run([os.path.join(DRIVERS, "schwinger_hmc")] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=timeout)
    rows = [(int(m.group(1)), float(m.group(2)), int(m.group(3)), float(m.group(4)), float(m.group(5)), int(m.group(6)))
            for m in re.finditer(r"\[HMC\] (\d+) dH (\S+) acc (\d) plaq (\S+) Q (\S+) cg (\d+)", out.stdout)]
    return out, rows


def test_pure_gauge_plaquette_is_the_exact_one(tmp_path):
    """16^2, beta 2, tau 1, 10 steps, cold start, 100 + 300 trajectories: <cos P> = I1(2)/I0(2) = 0.697775 in two dimensions.  The twin's mean over
    exactly this run has a standard deviation of 0.00276 over 12 seeds; the gate is five of those, 0.014.  Acceptance: the twin gives 0.92."""
    out, rows = run_driver([16, 2.0, 0.0, 0, 300, 100, 10, 4242, tmp_path / "pg.dat", "cold"], 300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    assert len(rows) == 400
    meas = rows[100:]
    plaq, acc = float(np.mean([r[3] for r in meas])), float(np.mean([r[2] for r in meas]))
    print("pure gauge 16^2 beta 2: <plaq> = %.6f (exact 0.697775), acceptance %.3f" % (plaq, acc))
    assert abs(plaq - 0.697775) <= 0.014
    assert 0.8 < acc < 1.0


def test_two_flavour_run_through_the_driver(tmp_path):
    """16^2, beta 4, m 0.1, 20 steps, 30 trajectories from a heatbath start"""
    cfg = tmp_path / "nf2.dat"
    out, rows = run_driver([16, 4.0, 0.1, 2, 30, 0, 20, 99, cfg], 390)
    print(out.stdout[-3000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    assert len(rows) == 30 and re.search(r"unconverged 0\b", out.stdout)
    assert all(r[5] > 0 for r in rows)
    acc = float(np.mean([r[2] for r in rows]))
    w = np.exp(-np.array([r[1] for r in rows]))
    n = w.size
    jk = (w.sum() - w) / (n - 1)
    err = float(np.sqrt((n - 1) / n * np.sum((jk - w.mean()) ** 2)))
    print("two flavours: acceptance %.3f, <exp(-dH)> = %.4f +/- %.4f" % (acc, w.mean(), err))
    assert acc > 0.5
    assert abs(w.mean() - 1.0) <= 4.0 * err
    # the written file: numpy's plaquette of it, and the driver's own read_gauge_u1 of it, are the last printed plaquette
    Ux, Uy = cs.phases_to_links(np.loadtxt(str(cfg)), 16, 16)
    assert abs(un.plaquette(Ux, Uy)[0].real - rows[-1][3]) < 1e-9
    back = re.search(r"\[HMC-READBACK\] plaq (\S+)", out.stdout)
    assert back and abs(float(back.group(1)) - rows[-1][3]) < 1e-9


# 8^2, beta 4, 4 steps, 3 trajectories from a heatbath start: Wilson 0, 2 and 1 flavours (degree 8 on [0.1, default]), staggered 2 and 1 tastes
SEEDED_LEGS = {
    "wilson-0": [0.1, 0, 3, 0, 4, "SEED", "CFG", "heatbath"],
    "wilson-2": [0.1, 2, 3, 0, 4, "SEED", "CFG", "heatbath"],
    "wilson-1": [0.1, 1, 3, 0, 4, "SEED", "CFG", "heatbath", 8, 0.1],
    "staggered-2": [0.2, 2, 3, 0, 4, "SEED", "CFG", "heatbath", "staggered"],
    "staggered-1": [0.2, 1, 3, 0, 4, "SEED", "CFG", "heatbath", 8, "staggered"],
}


@pytest.mark.parametrize("leg", sorted(SEEDED_LEGS))
def test_trajectories_are_a_function_of_the_seed(tmp_path, leg):
    """The shared trajectory() (hmc_core.hpp) draws every random field from (seed, trajectory, field) alone and starts every solve from zero:
    two runs with one seed print the same [HMC] lines to the last digit, another seed prints others."""
    def lines(seed, name):
        args = [8, 4.0] + [seed if a == "SEED" else (tmp_path / name if a == "CFG" else a) for a in SEEDED_LEGS[leg]]
        out, rows = run_driver(args, 120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr
        assert len(rows) == 3
        return re.findall(r"^\[HMC\] .*$", out.stdout, re.M)
    first, again, other = lines(99, "a.dat"), lines(99, "b.dat"), lines(100, "c.dat")
    print("\n".join(first))
    assert len(first) == 3 and first == again
    assert first != other
    assert (tmp_path / "a.dat").read_bytes() == (tmp_path / "b.dat").read_bytes()
