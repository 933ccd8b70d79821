"""Staggered HMC and rooted RHMC for the Schwinger model on the device (qmg_hmc_momentum_update_staggered in csrc/qmg_hmc.hip,
include/qmg/hmc_staggered.hpp, drivers/stag_hmc_parity.cpp and schwinger_hmc.cpp ... staggered).

The yardstick is the numpy twin tests/stag_hmc_numpy.py (pinned in test_host_stag_hmc.py), never the code under test:
  * the kernel against the twin's force with RANDOM W and weights (no solver enters), relative l2 <= 1e-12, the gate of the Wilson force
    kernels; dt = 0; the pure-gauge kick against qmg.hmc_momentum_update; linearity in the weight; gauge covariance; argument checks;
  * md_evolve for two tastes and one against the twin's leapfrog on the 32^2 beta-6.0 fixture, the heatbaths, apply_rational;
  * runs through schwinger_hmc ... staggered against the twin's identical runs.
Every gate on a solver-dependent number was fixed on the CPU first (twin with CG at 1e-12 against twin at 1e-13) and is ten times that."""
import importlib
import os
import re
import subprocess
import time

import numpy as np
import pytest

import coordspace as cs
import hmc_numpy as hn
import stag_hmc_numpy as sn
import u1_numpy as un

qmg = importlib.import_module("quantum-mg_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVERS = os.path.join(ROOT, "quantum-mg_amd", "drivers")
SIZES = [(2, 2), (2, 6), (6, 2), (6, 4), (34, 10), (64, 64)]   # (2, 6): xl == xr == xh with distinct rows; (6, 2): yp == ym with distinct columns
POLES = [1, 3, 16, 17]
BETA = 3.0
FIX = "l32t32b60_heatbath.dat"
FIX_M, FIX_N = 0.1, 8


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
    W = [rng.standard_normal((Lx, Ly)) + 1j * rng.standard_normal((Lx, Ly)) for _ in range(n)]
    w = rng.uniform(0.05, 2.0, n)
    return th, pi, W, w


def upload(th_links, pi, W, Lx, Ly):
    dg = qmg.DeviceArray.from_host(cs.links_to_eo_gauge(th_links[0], th_links[1], Lx, Ly))
    dp = qmg.DeviceArray.from_host(hn.field_to_eo(pi))
    dW = [qmg.DeviceArray.from_host(sn.grid_to_eo(v)) for v in W]
    return dg, dp, dW


def kick(th_links, pi, W, w, Lx, Ly, beta, dt, flags=0):
    dg, dp, dW = upload(th_links, pi, W, Lx, Ly)
    qmg.hmc_momentum_update_staggered(dp, dg, dW, list(w), Lx, Ly, beta, dt, flags)
    return dp.to_host()


def twin_force(th, W, w, beta):
    f = hn.gauge_force(th, beta)
    for wj, v in zip(w, W):
        g = sn.force_W(th, v)
        f = (f[0] + wj * g[0], f[1] + wj * g[1])
    return f


@pytest.mark.parametrize("Lx,Ly", SIZES)
@pytest.mark.parametrize("n", POLES)
def test_kernel_matches_the_twin_force(Lx, Ly, n):
    """pi - dt (Fg + sum_j w_j Fs(W_j)) with random positive weights; n = 17 takes a second launch without the gauge force.  A component is a
    sum of fewer than 6 n O(1) fp64 products: 1e-12 relative l2, the gate of the Wilson force kernels."""
    th, pi, W, w = random_setup(Lx, Ly, n, 1000 + 17 * Lx + Ly + n)
    dt = 0.37
    f = twin_force(th, W, w, BETA)
    want = hn.field_to_eo((pi[0] - dt * f[0], pi[1] - dt * f[1]))
    pi0 = hn.field_to_eo(pi)
    got = kick(hn.links(th), pi, W, w, Lx, Ly, BETA, dt)
    e_pi, e_f = rel_l2(got, want), rel_l2((pi0 - got) / dt, hn.field_to_eo(f))
    print("%dx%d n=%d: rel l2 of the new momenta %.2e, of the force %.2e" % (Lx, Ly, n, e_pi, e_f))
    assert e_pi <= 1e-12 and e_f <= 1e-12
    # dt = 0 returns the momenta bit for bit
    same = kick(hn.links(th), pi, W, w, Lx, Ly, BETA, 0.0)
    assert np.array_equal(same.view(np.uint64), pi0.view(np.uint64))


@pytest.mark.parametrize("Lx,Ly", SIZES)
def test_pure_gauge_is_the_wilson_entry_points_pure_gauge_kick(Lx, Ly):
    """GAUGE_ONLY with poles given, and n_poles = 0 with null lists, against qmg.hmc_momentum_update(..., HMC_GAUGE_ONLY) and the twin"""
    th, pi, W, w = random_setup(Lx, Ly, 2, 2100 + Lx)
    dg, dp, _ = upload(hn.links(th), pi, [], Lx, Ly)
    qmg.hmc_momentum_update(dp, dg, None, None, Lx, Ly, BETA, 0.37, qmg.HMC_GAUGE_ONLY)
    want = dp.to_host()
    a = kick(hn.links(th), pi, W, w, Lx, Ly, BETA, 0.37, qmg.HMC_GAUGE_ONLY)
    dg, dp, _ = upload(hn.links(th), pi, [], Lx, Ly)
    qmg.hmc_momentum_update_staggered(dp, dg, None, None, Lx, Ly, BETA, 0.37, 0)
    b = dp.to_host()
    print("%dx%d: pure gauge against the Wilson entry point %.2e / %.2e, bits equal %s" % (Lx, Ly, rel_l2(a, want), rel_l2(b, want), np.array_equal(a, want)))
    assert rel_l2(a, want) <= 1e-14 and rel_l2(b, want) <= 1e-14
    f = hn.gauge_force(th, BETA)
    assert rel_l2(a, hn.field_to_eo((pi[0] - 0.37 * f[0], pi[1] - 0.37 * f[1]))) <= 1e-12
    # the gauge part inside a launch with poles is the same force: a pole of weight 0 against the pure-gauge kick
    c = kick(hn.links(th), pi, W[:1], [0.0], Lx, Ly, BETA, 0.37)
    assert rel_l2(c, want) <= 1e-14


@pytest.mark.parametrize("Lx,Ly", [(6, 4), (34, 10)])
def test_one_pole_of_weight_w_is_w_times_the_single_pole_force(Lx, Ly):
    th, pi, W, _ = random_setup(Lx, Ly, 1, 2200 + Lx)
    zero = (np.zeros((Lx, Ly)), np.zeros((Lx, Ly)))
    w = 1.7
    f1 = -kick(hn.links(th), zero, W, [1.0], Lx, Ly, 0.0, 1.0)          # beta = 0, pi = 0, dt = 1: the fermion force alone
    fw = -kick(hn.links(th), zero, W, [w], Lx, Ly, 0.0, 1.0)
    assert np.linalg.norm(f1) > 1.0
    assert rel_l2(fw, w * f1) <= 1e-14       # fma(w, f, -0) is the one rounding of w f that numpy makes of w times f


@pytest.mark.parametrize("Lx,Ly", [(6, 4), (34, 10), (64, 64)])
def test_force_is_gauge_covariant(Lx, Ly):
    n = 3
    th, pi, W, w = random_setup(Lx, Ly, n, 3000 + Lx)
    Ux, Uy = hn.links(th)
    g = un.random_transform(Lx, Ly, 31)
    dg, dp, dW = upload((Ux, Uy), pi, [g * v for v in W], Lx, Ly)
    qmg.u1_gauge_transform(dg, qmg.DeviceArray.from_host(cs.grid_to_eo(g[:, :, None], Lx, Ly, 1)), Lx, Ly)
    qmg.hmc_momentum_update_staggered(dp, dg, dW, list(w), Lx, Ly, BETA, 0.37, 0)
    plain = kick((Ux, Uy), pi, W, w, Lx, Ly, BETA, 0.37)
    e = rel_l2(dp.to_host(), plain)
    print("%dx%d: transformed against plain %.2e" % (Lx, Ly, e))
    assert e <= 1e-12


def test_argument_checks():
    Lx = Ly = 4
    th, pi, W, w = random_setup(Lx, Ly, 2, 5)
    dg, dp, dW = upload(hn.links(th), pi, W, Lx, Ly)
    bad = [
        lambda: qmg.hmc_momentum_update_staggered(dp, dg, None, list(w), Lx, Ly, BETA, 0.1),                 # poles without W
        lambda: qmg.hmc_momentum_update_staggered(dp, dg, dW, None, Lx, Ly, BETA, 0.1, n_poles=2),           # ... without weights
        lambda: qmg.hmc_momentum_update_staggered(dp, dg, [dW[0], None], list(w), Lx, Ly, BETA, 0.1),        # a null vector in the list
        lambda: qmg.hmc_momentum_update_staggered(dp, dg, dW, list(w), Lx, Ly, BETA, 0.1, n_poles=-1),       # negative count
        lambda: qmg.hmc_momentum_update_staggered(dp, dg, dW, list(w), 3, Ly, BETA, 0.1),                    # odd extent
        lambda: qmg.hmc_momentum_update_staggered(dp, dg, dW, list(w), Lx, 0, BETA, 0.1),                    # extent < 2
        lambda: qmg.hmc_momentum_update_staggered(dp, dg, dW, list(w), Lx, Ly, BETA, 0.1, 2),                # unknown flag
        lambda: qmg.hmc_momentum_update_staggered(None, dg, dW, list(w), Lx, Ly, BETA, 0.1),                 # no momenta
        lambda: qmg.hmc_momentum_update_staggered(dp, None, dW, list(w), Lx, Ly, BETA, 0.1),                 # no links
    ]
    for call in bad:
        with pytest.raises(qmg.QmgError):
            call()
    assert np.array_equal(dp.to_host(), hn.field_to_eo(pi))


# ---- the facade on the 32^2 fixture ----
@pytest.fixture(scope="module")
def fixture32(golden_dir):
    """phases, momenta, a full-lattice eta, the rational function and both pseudofermions of the twin (CG at 1e-13), computed once"""
    L = 32
    th = hn.file_phases(os.path.join(golden_dir, FIX), L, L)
    rng = np.random.default_rng(2025)
    pi = (rng.standard_normal((L, L)), rng.standard_normal((L, L)))
    eta = (rng.standard_normal((L, L)) + 1j * rng.standard_normal((L, L))) / np.sqrt(2.0)
    z = sn.rational(FIX_N, FIX_M)
    phi = {2: sn.heatbath_two(th, eta, FIX_M), 1: sn.heatbath_one(z, th, eta, FIX_M, sn.make_cg_K2(1e-13))}
    return L, th, pi, eta, z, phi


def run_parity(mode, tmp_path, golden_dir, L, n_tastes, files):
    for name, arr in files.items():
        arr.tofile(str(tmp_path / name))
    out = subprocess.run([os.path.join(DRIVERS, "stag_hmc_parity"), mode, str(L), os.path.join(golden_dir, FIX), str(tmp_path), "6.0", repr(FIX_M), "1.0", "20", "1e-12",
                          str(n_tastes), str(FIX_N)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    print(out.stdout)
    return out


# (end phases, dH, forward-back) of the twin with CG at 1e-12 against itself at 1e-13 on the fixture's inputs -- solver error alone.
# two tastes: dH = -0.200814720080, 3347 CG iterations per leg; one taste: dH = -0.119376214175, 3350 multi-shift iterations per leg.
TWIN = {2: (1.112e-12, 5.002e-12, 9.159e-14), 1: (2.420e-13, 2.728e-12, 1.377e-14)}


@pytest.mark.parametrize("n_tastes", [2, 1])
def test_md_evolve_matches_the_twin_and_is_reversible(tmp_path, golden_dir, fixture32, n_tastes):
    """32^2 beta-6.0 fixture, m = 0.1, tau = 1, 20 steps, device CG at 1e-12 (one taste: degree 8 on [0.1, sqrt(4.01)], multi-shift); the twin
    runs its own CG at 1e-13.

    Gates, fixed on the CPU before the device was run (TWIN above): the twin at 1e-12 against the twin at 1e-13 differs by 1.11e-12 (two
    tastes) / 2.42e-13 (one) in the end phases (max abs; they move by 2.50 / 2.64) and by 5.00e-12 / 2.73e-12 in dH; forward, momenta
    negated, back, the twin at 1e-12 returns to its start within 9.16e-14 / 1.38e-14.  The device CG stops at another iterate, so the gates
    are ten times those.
    Not yet measured on an MI355X."""
    L, th, pi, eta, z, phi = fixture32
    out = run_parity("md", tmp_path, golden_dir, L, n_tastes, {"pi.bin": hn.field_to_eo(pi).astype(np.float64), "phi.bin": sn.even_to_half(phi[n_tastes])})
    assert out.returncode == 0, out.stdout + out.stderr
    legs = {m.group(1): (float(m.group(2)), int(m.group(3)), int(m.group(4))) for m in re.finditer(r"\[MD\] (\w+)\s+dH (\S+) cg (\d+) converged (\d)", out.stdout)}
    f = {k: hn.eo_to_field(np.fromfile(str(tmp_path / (k + ".bin"))), L, L) for k in ("theta_fwd", "pi_fwd", "theta_back", "pi_back")}
    assert legs["forward"][2] == 1 and legs["back"][2] == 1
    th1, pi1, dH = sn.md_dH(th, pi, 6.0, 1.0, 20, phi[n_tastes], FIX_M, z if n_tastes == 1 else None, sn.make_cg(1e-13))
    mx = lambda a, b: max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max())
    d_th, d_pi, d_back = mx(f["theta_fwd"], th1), mx(f["pi_fwd"], pi1), mx(f["theta_back"], th)
    print("%d tastes, md_evolve vs twin: end phases %.2e, end momenta %.2e, dH device %.12f twin %.12f (diff %.2e); forward-back %.2e; CG iterations %d"
          % (n_tastes, d_th, d_pi, legs["forward"][0], dH, abs(legs["forward"][0] - dH), d_back, legs["forward"][1]))
    g_th, g_dH, g_back = (10.0 * v for v in TWIN[n_tastes])
    assert mx(th1, th) > 1.0
    assert d_th <= g_th
    assert abs(legs["forward"][0] - dH) <= g_dH
    assert d_back <= g_back
    assert abs(legs["back"][0] + legs["forward"][0]) <= 2 * g_dH


def test_two_taste_heatbath_on_the_device(tmp_path, golden_dir, fixture32):
    """phi_e = (D^dag eta)_e on the device against the twin's (no solver: 1e-14 relative l2, a handful of fp64 products per site), then
    S_f(phi_e) = phi_e^dag A_ee^-1 phi_e on the device against the twin's solve.  phi_e^dag A_ee^-1 phi_e equals eta^dag eta in distribution
    only: phi_e = M eta with M the V/2 x V even rows of D^dag and M M^dag = A_ee, so S_f = eta^dag P eta with P a projector of rank V/2 (on the
    fixture S_f = 497.92 against eta^dag eta = 1002.55).  The twin's S_f with CG at 1e-12 and at 1e-13 differ by 2.3e-16 relative (the error of
    the quadratic form is second order in the residual); ten times that is below the rounding of a 512-term fp64 dot product in another
    order, gamma_512 = 512 * 1.1e-16 = 5.7e-14, which is added: gate 6e-14."""
    L, th, pi, eta, z, phi = fixture32
    out = run_parity("heatbath", tmp_path, golden_dir, L, 2, {"eta.bin": sn.grid_to_eo(eta)})
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"\[HB\] eta2 (\S+) spf (\S+) cg (\d+) converged (\d)", out.stdout)
    assert m and int(m.group(4)) == 1 and int(m.group(3)) > 0
    e2, spf = float(m.group(1)), float(m.group(2))
    got = sn.half_to_even(np.fromfile(str(tmp_path / "phi.bin"), dtype=np.complex128), L, L)
    want = sn.fermion_action(th, phi[2], FIX_M, None, sn.make_cg(1e-13))
    print("two tastes: phi_e against the twin's %.2e, S_f device %.12f twin %.12f (rel %.2e), eta2 %.6f" % (rel_l2(got, phi[2]), spf, want, abs(spf - want) / want, e2))
    assert abs(e2 - np.vdot(eta, eta).real) <= 1e-12 * e2
    assert rel_l2(got, phi[2]) <= 1e-14
    assert abs(spf - want) <= 6e-14 * want


def test_rooted_heatbath_and_rational_on_the_device(tmp_path, golden_dir, fixture32):
    """phi_e = (B eta)_e on the device against the even half of the twin's B eta: the twin with its multi-shift CG on -H^2 at 1e-12 and at
    1e-13 differ by 1.10e-12 relative l2; gate 1.1e-11.  apply_rational twice against A_ee^-1 (the twin's CG at 1e-13):
    || r r v - x || <= (2 delta + delta^2) || x || = 3.89e-8 || x || plus the solvers' share -- the twin's r r v at 1e-12 and 1e-13 differ by
    9.9e-13 || x ||, ten times that is added; the twin measures 2.857e-8.  r v against the twin's: twins differ by 4.4e-13, gate 4.4e-12."""
    L, th, pi, eta, z, phi = fixture32
    out = run_parity("heatbath", tmp_path, golden_dir, L, 1, {"eta.bin": sn.grid_to_eo(eta)})
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"\[HB\] eta2 (\S+) spf (\S+) cg (\d+) converged (\d)", out.stdout)
    assert m and int(m.group(4)) == 1 and int(m.group(3)) > 0
    head = re.search(r"\[RHMC\] n (\d+) ra (\S+) rb (\S+) c0 (\S+) delta (\S+)", out.stdout)
    assert head and int(head.group(1)) == FIX_N and float(head.group(2)) == FIX_M and abs(float(head.group(3)) - np.sqrt(FIX_M ** 2 + 4.0)) < 1e-15
    assert abs(float(head.group(4)) / z.c0 - 1.0) < 1.9e-12 and abs(float(head.group(5)) / z.delta - 1.0) < 0.01
    got = sn.half_to_even(np.fromfile(str(tmp_path / "phi.bin"), dtype=np.complex128), L, L)
    d_phi = rel_l2(got, phi[1])
    want = sn.fermion_action(th, phi[1], FIX_M, z, sn.make_cg(1e-13))
    print("rooted heatbath: phi_e against the twin's %.3e; S_pf device %.12f twin %.12f" % (d_phi, float(m.group(2)), want))
    assert d_phi <= 1.1e-11
    assert abs(float(m.group(2)) - want) <= 1e-11 * want      # 1.1e-11 in phi, twice in the quadratic form, is the looser of the two statements

    out = run_parity("rational", tmp_path, golden_dir, L, 1, {"v.bin": sn.even_to_half(phi[1])})
    assert out.returncode == 0 and re.search(r"\[RAT\] cg \d+ converged 1", out.stdout), out.stdout + out.stderr
    rv = sn.half_to_even(np.fromfile(str(tmp_path / "rv.bin"), dtype=np.complex128), L, L)
    rrv = sn.half_to_even(np.fromfile(str(tmp_path / "rrv.bin"), dtype=np.complex128), L, L)
    x = sn.make_cg(1e-13)(phi[1], th, FIX_M)[0]
    bound = 2 * z.delta + z.delta ** 2
    e = float(np.linalg.norm(rrv - x) / np.linalg.norm(x))
    e1 = rel_l2(rv, sn.apply_rational(z, phi[1], th, FIX_M, sn.make_cg(1e-13)))
    print("|| r r v - A_ee^-1 v || / || A_ee^-1 v || = %.3e (bound %.3e); r v against the twin's %.2e" % (e, bound, e1))
    assert e <= bound + 1e-11
    assert e > 1e-3 * bound          # it is an approximation: an exact inverse here would mean the test compares a thing with itself
    assert e1 <= 4.4e-12


# The twin's identical runs (stag_hmc_numpy.hmc_run: 8^2, beta 2, m 0.2, 10 steps, cold start, 100 + 300 trajectories, dense solves), seeds
# 1 .. 8 on the CPU: (mean plaquette over the seeds, standard deviation of one run's mean, seeds), and their acceptance.
TWIN_RUNS = {2: (0.730498, 0.005307, 8), 1: (0.717183, 0.004550, 8)}
# acceptance over the eight seeds: two tastes 0.927 .. 0.957 (mean 0.944), one taste 0.950 .. 0.970 (mean 0.959)


@pytest.mark.parametrize("n_tastes", [2, 1])
def test_run_through_the_driver(tmp_path, n_tastes):
    """schwinger_hmc 8 2.0 0.2 <tastes> 300 100 10 <seed> cfg cold staggered.  The twin's acceptance at these ten steps is inside (0.7, 1) for every seed (TWIN_RUNS above)."""
    cfg = tmp_path / "stag.dat"
    t0 = time.time()
    out = subprocess.run([os.path.join(DRIVERS, "schwinger_hmc")] + [str(a) for a in (8, 2.0, 0.2, n_tastes, 300, 100, 10, 77, cfg, "cold", "staggered")],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=390)
    print(out.stdout[-2500:])
    print("driver run: %.1f s" % (time.time() - t0))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    rows = [(int(m.group(1)), float(m.group(2)), int(m.group(3)), float(m.group(4)), float(m.group(5)), int(m.group(6)))
            for m in re.finditer(r"\[HMC\] (\d+) dH (\S+) acc (\d) plaq (\S+) Q (\S+) cg (\d+)", out.stdout)]
    assert len(rows) == 400 and re.search(r"unconverged 0\b", out.stdout)
    assert all(r[5] > 0 for r in rows)
    if n_tastes == 1:
        head = re.search(r"\[RHMC\] n (\d+) ra (\S+) rb (\S+) delta (\S+) det_bound (\S+)", out.stdout)
        assert head and int(head.group(1)) == 8 and float(head.group(2)) == 0.2 and float(head.group(4)) < 1e-8
    fin = re.search(r"\[HMC-FINAL\] trajectories 300 acceptance (\S+) exp_mdH (\S+) \+/- (\S+) plaq (\S+) \+/- (\S+)", out.stdout)
    assert fin
    acc, w, w_err, plaq = (float(fin.group(i)) for i in (1, 2, 3, 4))
    mean, std, _ = TWIN_RUNS[n_tastes]
    print("%d tastes: acceptance %.3f, <exp(-dH)> = %.4f +/- %.4f, plaquette %.5f (twin %.5f +/- %.5f)" % (n_tastes, acc, w, w_err, plaq, mean, std))
    assert 0.7 < acc < 1.0
    assert abs(w - 1.0) <= 4.0 * w_err
    assert abs(plaq - mean) <= 5.0 * std
    assert abs(plaq - np.mean([r[3] for r in rows[100:]])) < 1e-8
    Ux, Uy = cs.phases_to_links(np.loadtxt(str(cfg)), 8, 8)
    assert abs(un.plaquette(Ux, Uy)[0].real - rows[-1][3]) < 1e-9
    back = re.search(r"\[HMC-READBACK\] plaq (\S+)", out.stdout)
    assert back and abs(float(back.group(1)) - rows[-1][3]) < 1e-9


def test_wilson_command_lines_are_unchanged_by_the_switch(tmp_path):
    """the same pure-gauge Wilson run with and without the trailing `wilson`: identical output"""
    base = [os.path.join(DRIVERS, "schwinger_hmc")] + [str(a) for a in (8, 2.0, 0.1, 2, 3, 0, 10, 5, tmp_path / "w.dat", "cold")]
    a = subprocess.run(base, stdout=subprocess.PIPE, universal_newlines=True, timeout=120)
    b = subprocess.run(base + ["wilson"], stdout=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert a.returncode == 0 and b.returncode == 0
    assert a.stdout == b.stdout and len(re.findall(r"\[HMC\] \d+ dH", a.stdout)) == 3
