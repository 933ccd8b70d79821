"""Two-flavour domain-wall HMC for the Schwinger model on the device (qmg_hmc_momentum_update_dwf in csrc/qmg_hmc.hip, include/qmg/hmc_dwf.hpp,
drivers/dwf_hmc_parity.cpp and dwf_hmc.cpp).

The yardstick is the numpy twin tests/dwf_hmc_numpy.py (pinned in test_host_dwf_hmc.py), never the code under test:
  * the kernel against the twin's force with RANDOM X, Y, momenta, links and weights of both signs (no solver enters), relative l2 <= 1e-12, the
    gate of the Wilson force kernels; dt = 0 and two runs bit for bit; the same data, slice by slice, through qmg_hmc_momentum_update_poles;
    equal pairs of weights +1 and -1 against the pure-gauge kick; argument checks;
  * md_evolve against the twin's leapfrog, the heatbath and the action through dwf_hmc_parity;
  * a short run through dwf_hmc against the twin's identical runs.
Every gate on a solver-dependent number was fixed on the CPU first (twin with CG at 1e-12 against twin at 1e-13) and is ten times that."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import coordspace as cs
import dwf_hmc_numpy as dh
import dwf_numpy as dn
import hmc_numpy as hn
import u1_numpy as un

qmg = importlib.import_module("quantum-mg_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVERS = os.path.join(ROOT, "quantum-mg_amd", "drivers")
# (2, 2): every neighbour coincides; (4, 6): distinct rows and columns; (130, 2): more than one block per half row at every Ls (65 Ls lanes);
# (16, 8): several rows per block column
SIZES = [(2, 2), (4, 6), (130, 2), (16, 8)]
LS = [2, 3, 6, 8, 12, 32]          # 3, 6, 12: a site straddles wavefronts and the block is not 256 lanes
BETA, DT = 3.0, 0.37


@pytest.fixture(scope="module", autouse=True)
def _device():
    qmg.build()
    subprocess.check_call(["make", "-C", DRIVERS, "-j4"], stdout=subprocess.DEVNULL)
    qmg.init(0)
    yield
    qmg.sync()


def rel_l2(a, b):
    return float(np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(np.ravel(b)))


def random_setup(Lx, Ly, Ls, n, seed):
    rng = np.random.default_rng(seed)
    th = (rng.uniform(-np.pi, np.pi, (Lx, Ly)), rng.uniform(-np.pi, np.pi, (Lx, Ly)))
    pi = (rng.standard_normal((Lx, Ly)), rng.standard_normal((Lx, Ly)))
    field = lambda: rng.standard_normal((Lx, Ly, Ls, 2)) + 1j * rng.standard_normal((Lx, Ly, Ls, 2))
    X, Y = [field() for _ in range(n)], [field() for _ in range(n)]
    w = rng.uniform(0.05, 2.0, n) * np.where(np.arange(n) % 2, -1.0, 1.0)     # every second weight negative
    return th, pi, X, Y, w


def upload(th, pi, X, Y):
    Lx, Ly = th[0].shape
    Ux, Uy = hn.links(th)
    dg = qmg.DeviceArray.from_host(cs.links_to_eo_gauge(Ux, Uy, Lx, Ly))
    dp = qmg.DeviceArray.from_host(hn.field_to_eo(pi))
    return dg, dp, [qmg.DeviceArray.from_host(dh.grid_to_eo(v)) for v in X], [qmg.DeviceArray.from_host(dh.grid_to_eo(v)) for v in Y]


def kick(th, pi, X, Y, w, Ls, beta, dt, flags=0):
    Lx, Ly = th[0].shape
    dg, dp, dX, dY = upload(th, pi, X, Y)
    qmg.hmc_momentum_update_dwf(dp, dg, dX, dY, list(w), Ls, Lx, Ly, beta, dt, flags)
    return dp.to_host()


def twin_kick(th, pi, X, Y, w, beta, dt, g5_y=False):
    f = hn.gauge_force(th, beta)
    g = dh.force_pairs(th, X, Y, w, g5_y)
    f = (f[0] + g[0], f[1] + g[1])
    return hn.field_to_eo((pi[0] - dt * f[0], pi[1] - dt * f[1])), hn.field_to_eo(f)


@pytest.mark.parametrize("Lx,Ly", SIZES)
@pytest.mark.parametrize("Ls", LS)
def test_kernel_matches_the_twin_force(Lx, Ly, Ls):
    """pi - dt (Fg + sum_j w_j sum_s Ff(X_j(s), Y_j(s))) for n = 1, 2, 3 and 5 pairs (5 takes a second launch without the gauge force), weights of
    both signs, with and without QMG_HMC_DWF_G5_Y.  A component is a sum of fewer than 40 Ls n O(1) fp64 products: 1e-12 relative l2, the gate
    of the Wilson force kernels.  dt = 0 returns the momenta bit for bit; a second run returns the bits of the first."""
    for n in (1, 2, 3, 5):
        th, pi, X, Y, w = random_setup(Lx, Ly, Ls, n, 1000 + 17 * Lx + Ly + 3 * Ls + n)
        pi0 = hn.field_to_eo(pi)
        for g5 in (False, True):
            flags = qmg.HMC_DWF_G5_Y if g5 else 0
            want, f = twin_kick(th, pi, X, Y, w, BETA, DT, g5)
            got = kick(th, pi, X, Y, w, Ls, BETA, DT, flags)
            e_pi, e_f = rel_l2(got, want), rel_l2((pi0 - got) / DT, f)
            print("%dx%d Ls=%d n=%d g5=%d: rel l2 of the new momenta %.2e, of the force %.2e" % (Lx, Ly, Ls, n, g5, e_pi, e_f))
            assert e_pi <= 1e-12 and e_f <= 1e-12
            again = kick(th, pi, X, Y, w, Ls, BETA, DT, flags)
            assert np.array_equal(again.view(np.uint64), got.view(np.uint64))
            same = kick(th, pi, X, Y, w, Ls, BETA, 0.0, flags)
            assert np.array_equal(same.view(np.uint64), pi0.view(np.uint64))


@pytest.mark.parametrize("Ls", [2, 3])
def test_kernel_walks_more_rows_than_the_grid_has_blocks(Ls):
    """2 x 32770: 65540 (parity, y) rows on the 65535 blocks of grid.y, so five blocks take a second row through the other LDS buffer"""
    Lx, Ly, n = 2, 32770, 2
    assert qmg.hmc_dwf_plan((Lx, Ly), Ls, n)[4] == 65535 < 2 * Ly
    th, pi, X, Y, w = random_setup(Lx, Ly, Ls, n, 2000 + Ls)
    want, f = twin_kick(th, pi, X, Y, w, BETA, DT, True)
    got = kick(th, pi, X, Y, w, Ls, BETA, DT, qmg.HMC_DWF_G5_Y)
    e_pi, e_f = rel_l2(got, want), rel_l2((hn.field_to_eo(pi) - got) / DT, f)
    print("%dx%d Ls=%d: rel l2 of the new momenta %.2e, of the force %.2e" % (Lx, Ly, Ls, e_pi, e_f))
    assert e_pi <= 1e-12 and e_f <= 1e-12
    # the rows walked second, alone: row = 2 y + parity runs from 65535 to 65539 there, i.e. y >= 32767
    tail = hn.eo_to_field(got, Lx, Ly), hn.eo_to_field(want, Lx, Ly)
    assert max(np.abs(a[:, 32767:] - b[:, 32767:]).max() for a, b in zip(*tail)) <= 1e-12 * max(np.abs(b).max() for b in tail[1])


@pytest.mark.parametrize("Lx,Ly", SIZES)
@pytest.mark.parametrize("Ls", [2, 12, 32])
def test_pure_gauge_has_the_bits_of_the_wilson_entry_point(Lx, Ly, Ls):
    """QMG_HMC_GAUGE_ONLY with pairs given (with and without the Gamma5 flag), and n_pairs = 0 with null lists, against
    qmg.hmc_momentum_update(..., HMC_GAUGE_ONLY): equal bits; and against the twin."""
    th, pi, X, Y, w = random_setup(Lx, Ly, Ls, 2, 2100 + Lx + Ls)
    dg, dp, _, _ = upload(th, pi, [], [])
    qmg.hmc_momentum_update(dp, dg, None, None, Lx, Ly, BETA, DT, qmg.HMC_GAUGE_ONLY)
    want = dp.to_host()
    a = kick(th, pi, X, Y, w, Ls, BETA, DT, qmg.HMC_GAUGE_ONLY)
    b = kick(th, pi, X, Y, w, Ls, BETA, DT, qmg.HMC_GAUGE_ONLY | qmg.HMC_DWF_G5_Y)
    dg, dp, _, _ = upload(th, pi, [], [])
    qmg.hmc_momentum_update_dwf(dp, dg, None, None, None, Ls, Lx, Ly, BETA, DT, 0)
    c = dp.to_host()
    for got in (a, b, c):
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert rel_l2(a, twin_kick(th, pi, [], [], [], BETA, DT)[0]) <= 1e-12
    # the gauge part inside a launch with pairs is the same force: a pair of weight 0 against the pure-gauge kick
    d = kick(th, pi, X[:1], Y[:1], [0.0], Ls, BETA, DT)
    assert rel_l2(d, want) <= 1e-14


@pytest.mark.parametrize("Lx,Ly", [(4, 6), (130, 2), (16, 8)])
@pytest.mark.parametrize("Ls", [3, 8, 32])
def test_kernel_against_the_pole_kernel_on_the_unpacked_slices(Lx, Ly, Ls):
    """the same data as n Ls separate nc = 2 vector pairs through qmg_hmc_momentum_update_poles (a thread per site pair, the poles walked
    in another order): 1e-12 relative l2"""
    n = 3
    th, pi, X, Y, w = random_setup(Lx, Ly, Ls, n, 2300 + Lx + Ls)
    for g5 in (False, True):
        got = kick(th, pi, X, Y, w, Ls, BETA, DT, qmg.HMC_DWF_G5_Y if g5 else 0)
        Yr = [dn.gamma5_grid(y) for y in Y] if g5 else Y
        dg, dp, _, _ = upload(th, pi, [], [])
        xs = [qmg.DeviceArray.from_host(v) for x in X for v in dh.slices_to_eo(x)]
        ys = [qmg.DeviceArray.from_host(v) for y in Yr for v in dh.slices_to_eo(y)]
        qmg.hmc_momentum_update_poles(dp, dg, xs, ys, list(np.repeat(w, Ls)), Lx, Ly, BETA, DT)
        e = rel_l2(got, dp.to_host())
        print("%dx%d Ls=%d g5=%d: fused kernel against %d poles %.2e" % (Lx, Ly, Ls, g5, n * Ls, e))
        assert e <= 1e-12


@pytest.mark.parametrize("Lx,Ly", [(4, 6), (16, 8)])
@pytest.mark.parametrize("Ls", [3, 8])
def test_equal_pairs_of_opposite_weight_leave_the_pure_gauge_kick(Lx, Ly, Ls):
    """what the kick sees at m = 1: X5 = X5', Y5 = Y5', weights {+1, -1}.  Each force component is Fg + F - F with the two F of equal bits, so what
    is left over the pure-gauge kick is rounding of the largest term alone: four roundings of dt |F| and of the momentum."""
    th, pi, X, Y, _ = random_setup(Lx, Ly, Ls, 1, 2400 + Lx + Ls)
    got = kick(th, pi, [X[0], X[0]], [Y[0], Y[0]], [1.0, -1.0], Ls, BETA, DT, qmg.HMC_DWF_G5_Y)
    pure = kick(th, pi, [], [], [], Ls, BETA, DT, qmg.HMC_GAUGE_ONLY)
    f1 = dh.force_pairs(th, X, Y, [1.0], True)
    largest = DT * max(np.abs(f1[0]).max(), np.abs(f1[1]).max()) + np.abs(pure).max()
    d = np.abs(got - pure).max()
    print("%dx%d Ls=%d: |kick - pure gauge| %.2e, largest term %.2e" % (Lx, Ly, Ls, d, largest))
    assert d <= 4 * np.finfo(np.float64).eps * largest


def test_argument_checks():
    Lx, Ly, Ls = 4, 4, 4
    th, pi, X, Y, w = random_setup(Lx, Ly, Ls, 2, 5)
    dg, dp, dX, dY = upload(th, pi, X, Y)
    f = qmg.hmc_momentum_update_dwf_status
    bad = [
        f(dp, dg, None, dY, list(w), Ls, Lx, Ly, BETA, 0.1),                 # pairs without X
        f(dp, dg, dX, None, list(w), Ls, Lx, Ly, BETA, 0.1),                 # ... without Y
        f(dp, dg, dX, dY, None, Ls, Lx, Ly, BETA, 0.1, n_pairs=2),           # ... without weights
        f(dp, dg, [dX[0], None], dY, list(w), Ls, Lx, Ly, BETA, 0.1),        # a null vector in the list
        f(dp, dg, dX, dY, list(w), Ls, Lx, Ly, BETA, 0.1, n_pairs=-1),       # negative count
        f(dp, dg, dX, dY, list(w), Ls, 3, Ly, BETA, 0.1),                    # odd extent
        f(dp, dg, dX, dY, list(w), Ls, Lx, 0, BETA, 0.1),                    # extent < 2
        f(dp, dg, dX, dY, list(w), 1, Lx, Ly, BETA, 0.1),                    # Ls below 2
        f(dp, dg, dX, dY, list(w), 33, Lx, Ly, BETA, 0.1),                   # Ls above 32
        f(dp, dg, dX, dY, list(w), Ls, Lx, Ly, BETA, 0.1, 4),                # unknown flag
        f(None, dg, dX, dY, list(w), Ls, Lx, Ly, BETA, 0.1),                 # no momenta
        f(dp, None, dX, dY, list(w), Ls, Lx, Ly, BETA, 0.1),                 # no links
        f(dp, dg, dX, dY, list(w), Ls, Lx, Ly, float("nan"), 0.1),           # beta a NaN
    ]
    assert all(rc in (1, 3) for rc in bad), bad
    assert np.array_equal(dp.to_host(), hn.field_to_eo(pi))


# ---- the facade: 8 x 8, Ls = 4, m = 0.1, beta = 4, Gaussian phases of width 0.4 ----
L8, LS8, M8, BETA8 = 8, 4, 0.1, 4.0


@pytest.fixture(scope="module")
def fields8(tmp_path_factory):
    """phases (also as a file in the reference's text format), momenta, a pseudofermion and an eta on the even sites, from one fixed seed"""
    L, Ls = L8, LS8
    rng = np.random.default_rng(20240)
    th = (0.4 * rng.standard_normal((L, L)), 0.4 * rng.standard_normal((L, L)))
    pi = (rng.standard_normal((L, L)), rng.standard_normal((L, L)))
    phi = dh.keep((rng.standard_normal((L, L, Ls, 2)) + 1j * rng.standard_normal((L, L, Ls, 2))) / np.sqrt(2), 0)
    eta = dh.keep((rng.standard_normal((L, L, Ls, 2)) + 1j * rng.standard_normal((L, L, Ls, 2))) / np.sqrt(2), 0)
    path = str(tmp_path_factory.mktemp("dwf_hmc") / "phases.dat")
    np.savetxt(path, np.stack(th, axis=2).reshape(-1), fmt="%.17e")
    return th, pi, phi, eta, path


def run_parity(mode, tmp_path, gauge_file, files, cg_eps="1e-12"):
    for name, arr in files.items():
        arr.tofile(str(tmp_path / name))
    out = subprocess.run([os.path.join(DRIVERS, "dwf_hmc_parity"), mode, str(L8), str(LS8), gauge_file, str(tmp_path), repr(BETA8), repr(M8), "0.5", "10", cg_eps, "2"],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    print(out.stdout)
    return out


# (end phases, dH, forward-back) of the twin with CG at 1e-12 against itself at 1e-13 on fields8 -- solver error alone.
# dH = -0.602160998758 (1e-13), 1338 / 1412 CG iterations per forward leg; the twin with dense solves gives dH = -0.602160998755.
TWIN_MD = (7.193e-13, 6.935e-12, 4.510e-16)


def test_md_evolve_matches_the_twin_and_is_reversible(tmp_path, fields8):
    """tau = 0.5, 10 steps, device CG at 1e-12; the twin runs its own CG at 1e-13.

    Gates, fixed on the CPU before the device was run (TWIN_MD above): the twin at 1e-12 against the twin at 1e-13 differs by 7.19e-13 in the end
    phases (max abs) and by 6.93e-12 in dH; forward, momenta negated, back, the twin at 1e-12 returns to its start within 4.51e-16.  The device
    CG stops at another iterate, so the gates are ten times those."""
    th, pi, phi, eta, gauge_file = fields8
    out = run_parity("md", tmp_path, gauge_file, {"pi.bin": hn.field_to_eo(pi).astype(np.float64), "phi.bin": dh.even_to_half(phi)})
    assert out.returncode == 0, out.stdout + out.stderr
    legs = {m.group(1): (float(m.group(2)), int(m.group(3)), int(m.group(4))) for m in re.finditer(r"\[MD\] (\w+)\s+dH (\S+) cg (\d+) converged (\d)", out.stdout)}
    f = {k: hn.eo_to_field(np.fromfile(str(tmp_path / (k + ".bin"))), L8, L8) for k in ("theta_fwd", "pi_fwd", "theta_back", "pi_back")}
    assert legs["forward"][2] == 1 and legs["back"][2] == 1
    th1, pi1, dH = dh.md_dH(th, pi, BETA8, 0.5, 10, phi, M8, dh.make_cg(1e-13))
    mx = lambda a, b: max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max())
    d_th, d_pi, d_back = mx(f["theta_fwd"], th1), mx(f["pi_fwd"], pi1), mx(f["theta_back"], th)
    print("md_evolve vs twin: end phases %.2e, end momenta %.2e, dH device %.12f twin %.12f (diff %.2e); forward-back %.2e; CG iterations %d"
          % (d_th, d_pi, legs["forward"][0], dH, abs(legs["forward"][0] - dH), d_back, legs["forward"][1]))
    g_th, g_dH, g_back = (10.0 * v for v in TWIN_MD)
    assert mx(th1, th) > 0.3
    assert d_th <= g_th
    assert abs(legs["forward"][0] - dH) <= g_dH
    assert d_back <= g_back


def test_heatbath_and_action_through_the_facade(tmp_path, fields8):
    """phi = P (P^dag P)^-1 M^dag eta on the device (CG at 1e-12) against the twin's (CG at 1e-13), and S_f(phi) on the device against |eta|^2.
    The twin at 1e-12 against itself at 1e-13: phi differs by 4.72e-13 relative l2, S_f(phi) from |eta|^2 by 4.21e-14 relative; the gates are
    ten times those."""
    th, pi, phi, eta, gauge_file = fields8
    out = run_parity("heatbath", tmp_path, gauge_file, {"eta.bin": dh.even_to_half(eta)})
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"\[HB\] eta2 (\S+) spf (\S+) cg (\d+) converged (\d)", out.stdout)
    assert m and int(m.group(4)) == 1 and int(m.group(3)) > 0
    e2, spf = float(m.group(1)), float(m.group(2))
    got = dh.half_to_even(np.fromfile(str(tmp_path / "phi.bin"), dtype=np.complex128), L8, L8, LS8)
    want = dh.heatbath(th, eta, M8, dh.make_cg(1e-13))
    print("heatbath: phi against the twin's %.2e, S_f device %.12f, eta2 %.12f (rel %.2e)" % (rel_l2(got, want), spf, e2, abs(spf - e2) / e2))
    assert abs(e2 - np.vdot(eta, eta).real) <= 1e-12 * e2
    assert rel_l2(got, want) <= 4.72e-12
    assert abs(spf - e2) <= 4.21e-13 * e2


# The twin's identical runs (dwf_hmc_numpy.hmc_run: 8^2, Ls 4, beta 2, m 0.2, 10 steps, cold start, 10 + 40 trajectories, dense solves), seeds 1 .. 5
# on the CPU: acceptance over the 40 measured trajectories 0.975, 0.975, 0.975, 0.925, 0.950 (mean plaquette 0.7484, 0.7412, 0.7569, 0.7577, 0.7374;
# <exp(-dH)> 0.9956, 1.0048, 1.0137, 0.9987, 0.9970).  The band is what the five runs span.
TWIN_ACCEPTANCE = (0.925, 0.975)


def test_short_run_through_the_driver(tmp_path):
    """dwf_hmc 8 4 2.0 0.2 2 40 10 10 <seed> cfg cold, twice: every CG converged, <exp(-dH)> within four of its jackknife errors of 1, the
    acceptance inside the twin's band, the written file reads back with the printed plaquette, and the two runs print the same lines."""
    cfg = tmp_path / "dwf.dat"
    cmd = [os.path.join(DRIVERS, "dwf_hmc")] + [str(a) for a in (8, 4, 2.0, 0.2, 2, 40, 10, 10, 77, cfg, "cold")]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    print(out.stdout[-2500:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    rows = [(int(m.group(1)), float(m.group(2)), int(m.group(3)), float(m.group(4)), float(m.group(5)), int(m.group(6)))
            for m in re.finditer(r"\[HMC\] (\d+) dH (\S+) acc (\d) plaq (\S+) Q (\S+) cg (\d+)", out.stdout)]
    assert len(rows) == 50 and re.search(r"unconverged 0\b", out.stdout)
    assert all(r[5] > 0 for r in rows)
    fin = re.search(r"\[HMC-FINAL\] trajectories 40 acceptance (\S+) exp_mdH (\S+) \+/- (\S+) plaq (\S+) \+/- (\S+)", out.stdout)
    assert fin
    acc, w, w_err, plaq = (float(fin.group(i)) for i in (1, 2, 3, 4))
    print("acceptance %.3f (twin %.3f .. %.3f), <exp(-dH)> = %.4f +/- %.4f, plaquette %.5f" % (acc, TWIN_ACCEPTANCE[0], TWIN_ACCEPTANCE[1], w, w_err, plaq))
    assert TWIN_ACCEPTANCE[0] <= acc <= TWIN_ACCEPTANCE[1]
    assert abs(w - 1.0) <= 4.0 * w_err
    assert abs(plaq - np.mean([r[3] for r in rows[10:]])) < 1e-8
    Ux, Uy = cs.phases_to_links(np.loadtxt(str(cfg)), 8, 8)
    assert abs(un.plaquette(Ux, Uy)[0].real - rows[-1][3]) < 1e-9
    back = re.search(r"\[HMC-READBACK\] plaq (\S+)", out.stdout)
    assert back and abs(float(back.group(1)) - rows[-1][3]) < 1e-9
    again = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert again.returncode == 0 and again.stdout == out.stdout
