"""One-flavour RHMC for the Schwinger model on the device (qmg_hmc_momentum_update_poles in csrc/qmg_hmc.hip, include/qmg/rational.hpp and
hmc.hpp, drivers/rhmc_parity.cpp and schwinger_hmc.cpp).

The yardstick is the numpy / scipy twin tests/rhmc_numpy.py (pinned in test_host_rhmc.py), never the code under test:
  * the pole kernel against the twin's force with RANDOM spinors and weights (no solver enters), relative l2 <= 1e-12, the gate of the
    two-flavour kernel; its two bit-for-bit contracts; gauge covariance; argument checks;
  * apply_rational twice against (Q^2)^-1, the heatbath identity, md_evolve against the twin's leapfrog on the 32^2 beta-6.0 fixture;
  * a one-flavour run through the driver.

The fixture's spectrum, from the twin's dense Q on the CPU (rn.spectrum_Q2, 7 s, not repeated here): Q^2 in [0.0288746, 16.5951] at m = 0.1.
Hence ra = 0.152 (ra^2 = 0.0231, 0.8 of the smallest eigenvalue), rb = the default |2 + m| + 2 = 4.1 (rb^2 = 16.81), eps = 1.37e-3, and
n = 8 gives delta = 6.6e-8."""
import importlib
import os
import re
import subprocess
import time

import numpy as np
import pytest

import coordspace as cs
import hmc_numpy as hn
import rhmc_numpy as rn
import u1_numpy as un

qmg = importlib.import_module("quantum-mg_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVERS = os.path.join(ROOT, "quantum-mg_amd", "drivers")
SIZES = [(2, 2), (2, 6), (6, 2), (6, 4), (34, 10), (64, 64)]   # (2, 6): xl == xr == xh with distinct rows; (6, 2): yp == ym with distinct columns
POLES = [1, 5, 8, 16, 17]
BETA, MASS = 3.0, 0.1
FIX = "l32t32b60_heatbath.dat"
FIX_N, FIX_RA, FIX_RB = 8, 0.152, 4.1


@pytest.fixture(scope="module", autouse=True)
def _device():
    qmg.build()
    subprocess.check_call(["make", "-C", DRIVERS, "-j4"], stdout=subprocess.DEVNULL)
    qmg.init(0)
    yield
    qmg.sync()


def rel_l2(a, b):
    return float(np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(np.ravel(b)))


def random_setup(Lx, Ly, n, seed):
    rng = np.random.default_rng(seed)
    th = (rng.uniform(-np.pi, np.pi, (Lx, Ly)), rng.uniform(-np.pi, np.pi, (Lx, Ly)))
    pi = (rng.standard_normal((Lx, Ly)), rng.standard_normal((Lx, Ly)))
    X = [rng.standard_normal((Lx, Ly, 2)) + 1j * rng.standard_normal((Lx, Ly, 2)) for _ in range(n)]
    Y = [rng.standard_normal((Lx, Ly, 2)) + 1j * rng.standard_normal((Lx, Ly, 2)) for _ in range(n)]
    w = rng.uniform(0.05, 2.0, n)
    return th, pi, X, Y, w


def upload(th_links, pi, X, Y, Lx, Ly):
    dg = qmg.DeviceArray.from_host(cs.links_to_eo_gauge(th_links[0], th_links[1], Lx, Ly))
    dp = qmg.DeviceArray.from_host(hn.field_to_eo(pi))
    dX = [qmg.DeviceArray.from_host(cs.grid_to_eo(x, Lx, Ly, 2)) for x in X]
    dY = [qmg.DeviceArray.from_host(cs.grid_to_eo(y, Lx, Ly, 2)) for y in Y]
    return dg, dp, dX, dY


def pole_kick(th_links, pi, X, Y, w, Lx, Ly, beta, dt, flags=0):
    dg, dp, dX, dY = upload(th_links, pi, X, Y, Lx, Ly)
    qmg.hmc_momentum_update_poles(dp, dg, dX, dY, list(w), Lx, Ly, beta, dt, flags)
    return dp.to_host()


@pytest.mark.parametrize("Lx,Ly", SIZES)
@pytest.mark.parametrize("n", POLES)
def test_pole_kernel_matches_the_twin_force(Lx, Ly, n):
    """pi - dt (Fg + sum_j w_j Ff(X_j, Y_j)) with random positive weights; n = 17 takes a second launch without the gauge force.  A
    component is a sum of fewer than 20 n O(1) fp64 products: 1e-12 relative l2, the gate of the two-flavour kernel."""
    th, pi, X, Y, w = random_setup(Lx, Ly, n, 1000 + 17 * Lx + Ly + n)
    dt = 0.37
    f = hn.gauge_force(th, BETA)
    for j in range(n):
        g = hn.fermion_force_xy(th, X[j], Y[j])
        f = (f[0] + w[j] * g[0], f[1] + w[j] * g[1])
    want = hn.field_to_eo((pi[0] - dt * f[0], pi[1] - dt * f[1]))
    pi0 = hn.field_to_eo(pi)
    got = pole_kick(hn.links(th), pi, X, Y, w, Lx, Ly, BETA, dt)
    e_pi, e_f = rel_l2(got, want), rel_l2((pi0 - got) / dt, hn.field_to_eo(f))
    print("%dx%d n=%d: rel l2 of the new momenta %.2e, of the force %.2e" % (Lx, Ly, n, e_pi, e_f))
    assert e_pi <= 1e-12 and e_f <= 1e-12
    # dt = 0 returns the momenta bit for bit
    same = pole_kick(hn.links(th), pi, X, Y, w, Lx, Ly, BETA, 0.0)
    assert np.array_equal(same.view(np.uint64), pi0.view(np.uint64))


@pytest.mark.parametrize("Lx,Ly", SIZES)
def test_one_pole_of_weight_one_is_the_two_flavour_kernel_bit_for_bit(Lx, Ly):
    th, pi, X, Y, _ = random_setup(Lx, Ly, 1, 2000 + Lx)
    got = pole_kick(hn.links(th), pi, X, Y, [1.0], Lx, Ly, BETA, 0.37)
    dg, dp, dX, dY = upload(hn.links(th), pi, X, Y, Lx, Ly)
    qmg.hmc_momentum_update(dp, dg, dX[0], dY[0], Lx, Ly, BETA, 0.37, 0)
    assert np.array_equal(got.view(np.uint64), dp.to_host().view(np.uint64))
    assert not np.array_equal(got, hn.field_to_eo(pi))


@pytest.mark.parametrize("Lx,Ly", [(6, 4), (34, 10)])
def test_gauge_only_and_zero_poles_are_the_pure_gauge_kick(Lx, Ly):
    th, pi, X, Y, w = random_setup(Lx, Ly, 2, 2100 + Lx)
    dg, dp, _, _ = upload(hn.links(th), pi, [], [], Lx, Ly)
    qmg.hmc_momentum_update(dp, dg, None, None, Lx, Ly, BETA, 0.37, qmg.HMC_GAUGE_ONLY)
    want = dp.to_host()
    a = pole_kick(hn.links(th), pi, X, Y, w, Lx, Ly, BETA, 0.37, qmg.HMC_GAUGE_ONLY)
    dg, dp, _, _ = upload(hn.links(th), pi, [], [], Lx, Ly)
    qmg.hmc_momentum_update_poles(dp, dg, None, None, None, Lx, Ly, BETA, 0.37, 0)       # n_poles = 0, null lists
    assert np.array_equal(a.view(np.uint64), want.view(np.uint64)) and np.array_equal(dp.to_host().view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize("Lx,Ly", [(6, 4), (34, 10), (64, 64)])
def test_pole_force_is_gauge_covariant(Lx, Ly):
    n = 5
    th, pi, X, Y, w = random_setup(Lx, Ly, n, 3000 + Lx)
    Ux, Uy = hn.links(th)
    g = un.random_transform(Lx, Ly, 31)
    dg, dp, dX, dY = upload((Ux, Uy), pi, [g[:, :, None] * x for x in X], [g[:, :, None] * y for y in Y], Lx, Ly)
    qmg.u1_gauge_transform(dg, qmg.DeviceArray.from_host(cs.grid_to_eo(g[:, :, None], Lx, Ly, 1)), Lx, Ly)
    qmg.hmc_momentum_update_poles(dp, dg, dX, dY, list(w), Lx, Ly, BETA, 0.37, 0)
    plain = pole_kick((Ux, Uy), pi, X, Y, w, Lx, Ly, BETA, 0.37)
    e = rel_l2(dp.to_host(), plain)
    print("%dx%d: transformed against plain %.2e" % (Lx, Ly, e))
    assert e <= 1e-12


def test_pole_kernel_argument_checks():
    Lx = Ly = 4
    th, pi, X, Y, w = random_setup(Lx, Ly, 2, 5)
    dg, dp, dX, dY = upload(hn.links(th), pi, X, Y, Lx, Ly)
    bad = [
        lambda: qmg.hmc_momentum_update_poles(dp, dg, None, dY, list(w), Lx, Ly, BETA, 0.1),                 # poles without X
        lambda: qmg.hmc_momentum_update_poles(dp, dg, dX, None, list(w), Lx, Ly, BETA, 0.1),                 # ... without Y
        lambda: qmg.hmc_momentum_update_poles(dp, dg, dX, dY, None, Lx, Ly, BETA, 0.1, n_poles=2),           # ... without weights
        lambda: qmg.hmc_momentum_update_poles(dp, dg, [dX[0], None], dY, list(w), Lx, Ly, BETA, 0.1),        # a null spinor in the list
        lambda: qmg.hmc_momentum_update_poles(dp, dg, dX, dY, list(w), Lx, Ly, BETA, 0.1, n_poles=-1),       # negative count
        lambda: qmg.hmc_momentum_update_poles(dp, dg, dX, dY, list(w), 3, Ly, BETA, 0.1),                    # odd extent
        lambda: qmg.hmc_momentum_update_poles(dp, dg, dX, dY, list(w), Lx, Ly, BETA, 0.1, 2),                # unknown flag
        lambda: qmg.hmc_momentum_update_poles(None, dg, dX, dY, list(w), Lx, Ly, BETA, 0.1),                 # no momenta
        lambda: qmg.hmc_momentum_update_poles(dp, None, dX, dY, list(w), Lx, Ly, BETA, 0.1),                 # no links
        lambda: qmg.hmc_momentum_update_poles(dp, dg, dX, dY, [1.0, float("nan")], Lx, Ly, BETA, 0.1),       # a weight that is not a number
    ]
    for call in bad:
        with pytest.raises(qmg.QmgError):
            call()
    assert np.array_equal(dp.to_host(), hn.field_to_eo(pi))


# ---- the facade on the 32^2 fixture ----
@pytest.fixture(scope="module")
def fixture32(golden_dir):
    """phases, momenta, eta, the twin's rational function and its heatbath phi (multi-shift CG at 1e-13), computed once"""
    L = 32
    th = hn.file_phases(os.path.join(golden_dir, FIX), L, L)
    rng = np.random.default_rng(2024)
    pi = (rng.standard_normal((L, L)), rng.standard_normal((L, L)))
    eta = (rng.standard_normal((L, L, 2)) + 1j * rng.standard_normal((L, L, 2))) / np.sqrt(2.0)
    z = rn.zolotarev(FIX_N, FIX_RA, FIX_RB)
    phi = rn.heatbath(z, th, eta, 0.1, rn.make_cg_m(1e-13))
    return L, th, pi, eta, z, phi


def run_parity(mode, tmp_path, golden_dir, L, files, beta=6.0, tau=1.0, n_steps=20, eps=1e-12, ra=FIX_RA):
    for name, arr in files.items():
        arr.tofile(str(tmp_path / name))
    out = subprocess.run([os.path.join(DRIVERS, "rhmc_parity"), mode, str(L), os.path.join(golden_dir, FIX), str(tmp_path), repr(beta), "0.1", repr(tau), str(n_steps),
                          repr(eps), str(FIX_N), repr(ra), "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    print(out.stdout)
    return out


def test_coefficients_of_the_facade_are_the_twins(tmp_path, golden_dir, fixture32):
    L, th, pi, eta, z, phi = fixture32
    out = run_parity("check", tmp_path, golden_dir, L, {})
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"\[RHMC\] n (\d+) ra (\S+) rb (\S+) c0 (\S+) delta (\S+)", out.stdout)
    assert m and int(m.group(1)) == FIX_N and float(m.group(2)) == FIX_RA and abs(float(m.group(3)) - FIX_RB) < 1e-15      # the default rb = |2 + m| + 2
    assert abs(float(m.group(4)) / z.c0 - 1.0) < 1.9e-12 and abs(float(m.group(5)) / z.delta - 1.0) < 0.01
    c = re.search(r"\[RHMC-CHECK\] ratio (\S+) bound (\S+) ok (\d)", out.stdout)
    assert c and int(c.group(3)) == 1 and float(c.group(1)) <= float(c.group(2)) * 1.01 and abs(float(c.group(2)) / (2 * z.delta + z.delta ** 2) - 1.0) < 0.01
    # an interval that the spectrum has left (ra^2 = 0.25, nine times the smallest eigenvalue) is found out
    out = run_parity("check", tmp_path, golden_dir, L, {}, ra=0.5)
    c = re.search(r"\[RHMC-CHECK\] ratio (\S+) bound (\S+) ok (\d)", out.stdout)
    assert c and int(c.group(3)) == 0 and float(c.group(1)) > 10.0 * float(c.group(2))


def test_apply_rational_twice_is_the_inverse(tmp_path, golden_dir, fixture32):
    """|| r r v - (Q^2)^-1 v || <= (2 delta + delta^2) || (Q^2)^-1 v || plus the solvers' share: r^2 y = (1 + e)^2 / y with |e| <= delta on the
    spectrum.  (Q^2)^-1 v is the twin's CG at 1e-13: its error is at most 1e-13 cond(Q^2) = 1e-13 * 575 = 6e-11 of |x|; the device's multi-shift
    CG at 1e-12 leaves each application of r off by at most 1e-12 rb / ra = 3e-11 relative.  Together below 2e-10, a hundredth of the bound
    1.3e-7, and added to it.  Measured on an MI355X: 8.99e-8 against the bound 1.317e-7; r v against the twin's r v 8.4e-13."""
    L, th, pi, eta, z, phi = fixture32
    out = run_parity("rational", tmp_path, golden_dir, L, {"v.bin": cs.grid_to_eo(phi, L, L, 2)})
    assert out.returncode == 0 and re.search(r"\[RAT\] cg \d+ converged 1", out.stdout), out.stdout + out.stderr
    rv = cs.eo_to_grid(np.fromfile(str(tmp_path / "rv.bin"), dtype=np.complex128), L, L, 2)
    rrv = cs.eo_to_grid(np.fromfile(str(tmp_path / "rrv.bin"), dtype=np.complex128), L, L, 2)
    x = hn.make_cg(1e-13)(phi, th, 0.1)
    bound = 2 * z.delta + z.delta ** 2
    e = float(np.linalg.norm(rrv - x) / np.linalg.norm(x))
    e1 = rel_l2(rv, rn.apply_rational(z, phi, th, 0.1, rn.make_cg_m(1e-13)))
    print("|| r r v - (Q^2)^-1 v || / || (Q^2)^-1 v || = %.3e (bound %.3e); r v against the twin's %.2e" % (e, bound, e1))
    assert e <= bound + 2e-10
    assert e > 1e-3 * bound          # it is an approximation: an exact inverse here would mean the test compares a thing with itself
    assert e1 <= 1e-10


def test_heatbath_on_the_device(tmp_path, golden_dir, fixture32):
    """phi = B eta on the device, then S_pf(phi) on the device, against eta^dag eta.  Gate, fixed on the CPU before the device ran: the twin
    with its multi-shift CG at 1e-12 gives |S_pf - eta^2| / eta^2 = 1.15e-13, at 1e-13 3.2e-15, and the two S_pf differ by 1.12e-13 of eta^2
    -- solver error alone; the device CG stops at another iterate, so the gate is ten times that, 1.1e-12.  phi itself against the twin's at
    1e-13: the twins at 1e-12 and 1e-13 differ by 1.7e-12 relative l2, gate 1.7e-11.
    Measured on an MI355X: |S_pf - eta^2| / eta^2 = 1.15e-13, phi against the twin's 1.7e-12."""
    L, th, pi, eta, z, phi = fixture32
    out = run_parity("heatbath", tmp_path, golden_dir, L, {"eta.bin": cs.grid_to_eo(eta, L, L, 2)})
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"\[HB\] eta2 (\S+) spf (\S+) cg (\d+) converged (\d)", out.stdout)
    assert m and int(m.group(4)) == 1 and int(m.group(3)) > 0
    e2, spf = float(m.group(1)), float(m.group(2))
    got = cs.eo_to_grid(np.fromfile(str(tmp_path / "phi.bin"), dtype=np.complex128), L, L, 2)
    d_phi = rel_l2(got, phi)
    print("device heatbath: |S_pf - eta^2| / eta^2 = %.3e, phi against the twin's %.3e" % (abs(spf - e2) / e2, d_phi))
    assert abs(e2 - np.vdot(eta, eta).real) <= 1e-12 * e2
    assert abs(spf - e2) <= 1.1e-12 * e2
    assert d_phi <= 1.7e-11


def test_md_evolve_one_flavour_matches_the_twin_and_is_reversible(tmp_path, golden_dir, fixture32):
    """32^2 beta-6.0 fixture, m = 0.1, tau = 1, 20 steps, n = 8 on [0.152, 4.1], device multi-shift CG at 1e-12; the twin runs its own at 1e-13.

    Gates, fixed on the CPU before the device was run: the twin at 1e-12 against the twin at 1e-13 on these inputs differs by 7.6e-13 in the
    end phases (max abs; they move by up to 2.5) and by 9.1e-13 in dH (dH = -0.023977889345) -- solver error alone.  The device CG stops at
    another iterate, so the gates are ten times that: 7.6e-12 on the phases and 9.1e-12 on dH.  Forward, momenta negated, back: the twin at
    1e-12 returns to its start within 2.2e-15 (max abs over the phases); the device gate is ten times that, 2.2e-14.
    Measured on an MI355X: end phases 7.6e-13, dH 4.5e-13, forward-back 2.0e-15 (6046 multi-shift iterations per leg)."""
    L, th, pi, eta, z, phi = fixture32
    out = run_parity("md", tmp_path, golden_dir, L, {"pi.bin": hn.field_to_eo(pi).astype(np.float64), "phi.bin": cs.grid_to_eo(phi, L, L, 2)})
    assert out.returncode == 0, out.stdout + out.stderr
    legs = {m.group(1): (float(m.group(2)), int(m.group(3)), int(m.group(4))) for m in re.finditer(r"\[MD\] (\w+)\s+dH (\S+) cg (\d+) converged (\d)", out.stdout)}
    f = {k: hn.eo_to_field(np.fromfile(str(tmp_path / (k + ".bin"))), L, L) for k in ("theta_fwd", "pi_fwd", "theta_back", "pi_back")}
    assert legs["forward"][2] == 1 and legs["back"][2] == 1
    th1, pi1, dH = rn.md_dH(z, th, pi, 6.0, 1.0, 20, phi, 0.1, rn.make_cg_m(1e-13))
    d_th = max(np.abs(f["theta_fwd"][0] - th1[0]).max(), np.abs(f["theta_fwd"][1] - th1[1]).max())
    d_pi = max(np.abs(f["pi_fwd"][0] - pi1[0]).max(), np.abs(f["pi_fwd"][1] - pi1[1]).max())
    d_back = max(np.abs(f["theta_back"][0] - th[0]).max(), np.abs(f["theta_back"][1] - th[1]).max())
    print("md_evolve vs twin: end phases %.2e, end momenta %.2e, dH device %.12f twin %.12f (diff %.2e); forward-back %.2e; multi-shift iterations %d"
          % (d_th, d_pi, legs["forward"][0], dH, abs(legs["forward"][0] - dH), d_back, legs["forward"][1]))
    assert np.abs(th1[0] - th[0]).max() > 1.0
    assert d_th <= 7.6e-12
    assert abs(legs["forward"][0] - dH) <= 9.1e-12
    assert d_back <= 2.2e-14
    assert abs(legs["back"][0] + legs["forward"][0]) <= 2 * 9.1e-12


def test_one_flavour_run_through_the_driver(tmp_path):
    """16^2, beta 4, m 0.1, 20 steps, 30 trajectories from a heatbath start.  The twin's spectrum of thermalised 16^2 beta-4 fields (ten
    quenched configurations of its own HMC): the smallest eigenvalue of Q^2 ranges over 0.037 .. 0.058, the largest stays below 16.5.  ra = 0.1
    (ra^2 = 0.01, a quarter of the smallest seen, because the dynamical field is not those), rb the default 4.1, n = 10: delta = 6.0e-9 and
    det r^-1 within 3.1e-6 of det D.  The range check after the run says whether the interval held.  Measured on an MI355X: 5.2 s for the run,
    acceptance 0.90, <exp(-dH)> = 0.975 +/- 0.024, range check 2.8e-10 against 1.2e-8."""
    cfg = tmp_path / "nf1.dat"
    t0 = time.time()
    out = subprocess.run([os.path.join(DRIVERS, "schwinger_hmc")] + [str(a) for a in (16, 4.0, 0.1, 1, 30, 0, 20, 99, cfg, "heatbath", 10, 0.1)],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=390)
    print(out.stdout[-3500:])
    print("driver run: %.1f s" % (time.time() - t0))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    rows = [(int(m.group(1)), float(m.group(2)), int(m.group(3)), float(m.group(4)), float(m.group(5)), int(m.group(6)))
            for m in re.finditer(r"\[HMC\] (\d+) dH (\S+) acc (\d) plaq (\S+) Q (\S+) cg (\d+)", out.stdout)]
    assert len(rows) == 30 and re.search(r"unconverged 0\b", out.stdout)
    assert all(r[5] > 0 for r in rows)
    head = re.search(r"\[RHMC\] n (\d+) ra (\S+) rb (\S+) delta (\S+) det_bound (\S+)", out.stdout)
    assert head and int(head.group(1)) == 10 and float(head.group(2)) == 0.1 and float(head.group(4)) < 1e-8 and float(head.group(5)) < 1e-5
    checks = re.findall(r"\[RHMC-CHECK\] ratio (\S+) bound (\S+) ok (\d)", out.stdout)
    assert checks and all(c[2] == "1" for c in checks)
    acc = float(np.mean([r[2] for r in rows]))
    w = np.exp(-np.array([r[1] for r in rows]))
    n = w.size
    jk = (w.sum() - w) / (n - 1)
    err = float(np.sqrt((n - 1) / n * np.sum((jk - w.mean()) ** 2)))
    print("one flavour: acceptance %.3f, <exp(-dH)> = %.4f +/- %.4f" % (acc, w.mean(), err))
    assert acc > 0.5
    assert abs(w.mean() - 1.0) <= 4.0 * err
    Ux, Uy = cs.phases_to_links(np.loadtxt(str(cfg)), 16, 16)
    assert abs(un.plaquette(Ux, Uy)[0].real - rows[-1][3]) < 1e-9
    back = re.search(r"\[HMC-READBACK\] plaq (\S+)", out.stdout)
    assert back and abs(float(back.group(1)) - rows[-1][3]) < 1e-9
