"""U(1) field tools on the device (csrc/qmg_u1.hip, include/qmg/u1.hpp): gauge transforms, APE smearing, instantons, random fields.

Pins, strongest first:
  * deterministic: transform, smear and both instantons against the numpy twin tests/u1_numpy.py (np.roll on (x, y) grids, pinned by its
    own identities in test_host_u1_tools.py), max |difference| < 1e-12 -- the tolerance this project holds a build to against a CPU statement:
    one iteration on unit-modulus numbers rounds at ~1e-15, n_iter <= 10, and the fields are at beta >= 6 where smearing does not amplify;
  * invariants measured on the device: plaquette (1e-13) and topology (1e-9) under a transform, smear o transform = transform o smear (1e-12),
    the unit charge of an instanton on the unit field, smearing raising the plaquette;
  * gauge covariance of the operators, D[U^g] (g psi) = g D[U] psi, relative L2 < 1e-13 (the tolerance of the apply-parity tests): the one
    check of fill + apply that is not a second transcription of the same formulas;
  * random fields: on the unit circle, a function of the seed alone, and of the law they claim (8 sigma);
  * the drivers n01_u1_test and u1_make_config, and a K-cycle solve on a genuinely 64 x 64 file the latter wrote."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import coordspace as cs
import u1_numpy as un

qmg = importlib.import_module("quantum-mg_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVERS = os.path.join(ROOT, "quantum-mg_amd", "drivers")
TOL = 1e-12
STORED = [("l32t32b60", 32), ("l64t64b60", 64), ("l128t128b60", 128)]


@pytest.fixture(scope="module", autouse=True)
def _device():
    qmg.build()
    subprocess.check_call(["make", "-C", DRIVERS, "-j4"], stdout=subprocess.DEVNULL)
    qmg.init(0)
    yield
    qmg.sync()


def fields(golden_dir):
    """(name, Lx, Ly, Ux, Uy): the three stored configurations and Gaussian fields at beta = 6 on the thinnest lattices (2 x 2, 2 x 6, 6 x 2) and two rectangles"""
    out = []
    for name, L in STORED:
        Ux, Uy = cs.phases_to_links(np.loadtxt(os.path.join(golden_dir, name + "_heatbath.dat")), L, L)
        out.append((name, L, L, Ux, Uy))
    for Lx, Ly in ((2, 2), (2, 6), (6, 2), (6, 4), (34, 10)):
        Ux, Uy = un.gaussian_links(Lx, 6.0, 100 + Lx, Ly=Ly)
        out.append(("%dx%d" % (Lx, Ly), Lx, Ly, Ux, Uy))
    return out


def up(Ux, Uy):
    Lx, Ly = Ux.shape
    return qmg.DeviceArray.from_host(cs.links_to_eo_gauge(Ux, Uy, Lx, Ly))


def diff(dev, Ux, Uy):
    Lx, Ly = Ux.shape
    return float(np.abs(dev.to_host() - cs.links_to_eo_gauge(Ux, Uy, Lx, Ly)).max())


def test_gauge_transform_matches_numpy_and_keeps_plaquette_and_topology(golden_dir):
    for name, Lx, Ly, Ux, Uy in fields(golden_dir):
        g = un.random_transform(Lx, Ly, 21)
        dg = up(Ux, Uy)
        p0, q0 = qmg.u1_plaquette(dg, Lx, Ly)
        qmg.u1_gauge_transform(dg, qmg.DeviceArray.from_host(cs.grid_to_eo(g[:, :, None], Lx, Ly, 1)), Lx, Ly)
        d = diff(dg, *un.gauge_transform(Ux, Uy, g))
        p1, q1 = qmg.u1_plaquette(dg, Lx, Ly)
        print("transform %s: max diff %.2e, plaquette moved %.2e, topology moved %.2e" % (name, d, abs(p1 - p0), abs(q1 - q0)))
        assert d < TOL, name
        assert abs(p1 - p0) < 1e-13 and abs(q1 - q0) < 1e-9, name


@pytest.mark.parametrize("alpha,n_iter", [(0.5, 1), (0.5, 2), (0.1, 3), (0.5, 5), (0.7, 10), (0.5, 0), (0.0, 4)])
def test_ape_smear_matches_numpy(golden_dir, alpha, n_iter):
    for name, Lx, Ly, Ux, Uy in fields(golden_dir):
        dg, ds = up(Ux, Uy), qmg.DeviceArray(2 * Lx * Ly)
        qmg.u1_ape_smear(ds, dg, Lx, Ly, alpha, n_iter)
        want = un.ape_smear(Ux, Uy, alpha, n_iter)
        d = diff(ds, *want)
        print("smear %s alpha %.1f n_iter %d: max diff %.2e" % (name, alpha, n_iter, d))
        assert d < TOL, name
        assert diff(dg, Ux, Uy) == 0.0                                # the source is untouched
        qmg.u1_ape_smear(dg, dg, Lx, Ly, alpha, n_iter)               # in place: bit-identical to out of place
        assert np.array_equal(dg.to_host(), ds.to_host()), name
        assert np.abs(np.abs(ds.to_host()) - 1.0).max() < 1e-15


def test_ape_smear_projects_zero_to_one():
    """An exact zero: the unit field with alpha = -1/2 gives 1 - (1 + 1)/2 = 0 on every link, and P[0] = 1."""
    L = 8
    one = np.ones((L, L), dtype=complex)
    ds = qmg.DeviceArray(2 * L * L)
    qmg.u1_ape_smear(ds, up(one, one), L, L, -0.5, 1)
    assert np.array_equal(ds.to_host(), np.ones(2 * L * L, dtype=complex))
    assert np.array_equal(un.ape_iteration(one, one, -0.5)[0], one)


def test_smearing_commutes_with_a_transform_and_raises_the_plaquette(golden_dir):
    for name, Lx, Ly, Ux, Uy in fields(golden_dir):
        dt = qmg.DeviceArray(Lx * Ly)
        qmg.u1_random_trans(dt, Lx, Ly, 77)
        a, b = up(Ux, Uy), up(Ux, Uy)
        p_before = qmg.u1_plaquette(a, Lx, Ly)[0].real
        qmg.u1_ape_smear(a, a, Lx, Ly, 0.5, 5)
        p_after = qmg.u1_plaquette(a, Lx, Ly)[0].real
        qmg.u1_gauge_transform(a, dt, Lx, Ly)
        qmg.u1_gauge_transform(b, dt, Lx, Ly)
        qmg.u1_ape_smear(b, b, Lx, Ly, 0.5, 5)
        d = float(np.abs(a.to_host() - b.to_host()).max())
        print("%s: smear o transform - transform o smear = %.2e; plaquette %.6f -> %.6f" % (name, d, p_before, p_after))
        assert d < TOL, name
        assert p_after > p_before, name


@pytest.mark.parametrize("Q,x0,y0", [(1.0, None, None), (1.0, 3, 1), (-2.0, 0, 0), (1.0, -5, 70), (0.5, 1, 2)])
def test_instanton_matches_numpy(golden_dir, Q, x0, y0):
    """centred, off-centre, and centres that wrap (negative, and beyond the lattice) -- the reference's (x - L/2 + x0 + 3 L) % L"""
    for name, Lx, Ly, Ux, Uy in fields(golden_dir):
        cx, cy = (Lx // 2, Ly // 2) if x0 is None else (x0, y0)
        if cx < -2 * Lx - Lx // 2 or cy < -2 * Ly - Ly // 2:
            continue                                                   # the reference's % would see a negative argument
        dg = up(Ux, Uy)
        qmg.u1_instanton(dg, Lx, Ly, Q, cx, cy)
        d = diff(dg, *un.instanton(Ux, Uy, Q, cx, cy))
        print("instanton %s Q %.1f at (%d, %d): max diff %.2e" % (name, Q, cx, cy, d))
        assert d < TOL, name


@pytest.mark.parametrize("L,x0,y0", [(16, 8, 8), (16, 0, 0), (32, 5, 29)])
def test_unit_field_with_an_instanton_has_charge_one(L, x0, y0):
    one = np.ones((L, L), dtype=complex)
    dg = up(one, one)
    qmg.u1_instanton(dg, L, L, 1.0, x0, y0)
    assert abs(qmg.u1_plaquette(dg, L, L)[1] - 1.0) < 1e-9


def test_noncompact_instanton_matches_numpy():
    for Lx, Ly, Q in ((6, 4, 1.0), (34, 10, -3.0), (64, 64, 2.0)):
        A = np.random.default_rng(5).normal(0.0, 0.4, size=(Lx, Ly, 2))
        Ax, Ay = A[:, :, 0], A[:, :, 1]
        dph = qmg.DeviceArray.from_host(np.concatenate([un.grid_to_eo_real(Ax, Lx, Ly), un.grid_to_eo_real(Ay, Lx, Ly)]))
        qmg.u1_noncompact_instanton(dph, Lx, Ly, Q)
        Wx, Wy = un.noncompact_instanton(Ax, Ay, Q)
        d = float(np.abs(dph.to_host() - np.concatenate([un.grid_to_eo_real(Wx, Lx, Ly), un.grid_to_eo_real(Wy, Lx, Ly)])).max())
        print("non-compact instanton %dx%d: max diff %.2e" % (Lx, Ly, d))
        assert d < TOL


def _covariance(L, nc, desc_of, dg, dgt, dt, what):
    n = nc * L * L
    psi = cs.gaussian_cvec(n, 1337)
    g = np.repeat(dt.to_host(), nc)
    lhs, lhs_t = qmg.DeviceArray(n), qmg.DeviceArray(n)
    desc_of(dg)(lhs, qmg.DeviceArray.from_host(psi))
    desc_of(dgt)(lhs_t, qmg.DeviceArray.from_host(g * psi))
    err = cs.rel_l2(lhs_t.to_host(), g * lhs.to_host())
    print("gauge covariance, %s: relative L2 %.2e" % (what, err))
    assert err < 1e-13, what
    assert cs.rel_l2(lhs_t.to_host(), lhs.to_host()) > 0.1              # the transform did something


def test_operators_are_gauge_covariant(golden_dir):
    """D[U^g] (g psi) = g D[U] psi on l32t32b60 with a device random transform: the stored Wilson stencil, the Wilson kernel that reads the
    links, staggered and the gauged Laplace."""
    L = 32
    V = L * L
    Ux, Uy = cs.phases_to_links(np.loadtxt(os.path.join(golden_dir, "l32t32b60_heatbath.dat")), L, L)
    dg, dgt, dt = up(Ux, Uy), up(Ux, Uy), qmg.DeviceArray(V)
    qmg.u1_random_trans(dt, L, L, 4242)
    qmg.u1_gauge_transform(dgt, dt, L, L)

    def wilson_stored(gauge):
        dc, dh = qmg.DeviceArray(4 * V), qmg.DeviceArray(16 * V)
        qmg.wilson_fill(dc, dh, gauge, L, L, 1.0)
        desc = qmg.make_desc(L, L, 2, dc, dh, -0.07)
        return lambda lhs, rhs: qmg.stencil_apply(desc, lhs, rhs)

    def wilson_direct(gauge):
        desc = qmg.make_desc(L, L, 2, None, None, -0.07)
        return lambda lhs, rhs: qmg.wilson_apply_direct(qmg.C64, desc, gauge, lhs, rhs, qmg.P_ALL | qmg.P_ZERO)

    def staggered(gauge):
        dh = qmg.DeviceArray(4 * V)
        qmg.staggered_fill(dh, gauge, L, L)
        desc = qmg.make_desc(L, L, 1, None, dh, 0.04)
        return lambda lhs, rhs: qmg.stencil_apply(desc, lhs, rhs)

    def laplace(gauge):
        dc, dh = qmg.DeviceArray(V), qmg.DeviceArray(4 * V)
        qmg.laplace_fill(dc, dh, gauge, L, L)
        desc = qmg.make_desc(L, L, 1, dc, dh, 0.01)
        return lambda lhs, rhs: qmg.stencil_apply(desc, lhs, rhs)

    _covariance(L, 2, wilson_stored, dg, dgt, dt, "wilson_fill + stencil_apply")
    _covariance(L, 2, wilson_direct, dg, dgt, dt, "wilson_apply_direct fp64")
    _covariance(L, 1, staggered, dg, dgt, dt, "staggered_fill + stencil_apply")
    _covariance(L, 1, laplace, dg, dgt, dt, "laplace_fill + stencil_apply")


def test_random_fields_are_unit_and_a_function_of_the_seed_alone():
    Lx, Ly = 34, 10
    V = Lx * Ly
    st = qmg.stream_create()
    try:
        for fill, n in ((lambda d, seed, stream=None: qmg.u1_hot_gauge(d, Lx, Ly, seed, stream=stream), 2 * V),
                        (lambda d, seed, stream=None: qmg.u1_gauss_gauge(d, Lx, Ly, 6.0, seed, stream=stream), 2 * V),
                        (lambda d, seed, stream=None: qmg.u1_random_trans(d, Lx, Ly, seed, stream=stream), V)):
            a, b, c, s = qmg.DeviceArray(n), qmg.DeviceArray(n), qmg.DeviceArray(n), qmg.DeviceArray(n)
            fill(a, 11); fill(c, 12); fill(b, 11)
            fill(s, 11, stream=st)
            qmg.sync(st)
            ha = a.to_host()
            assert np.abs(np.abs(ha) - 1.0).max() < 1e-15
            assert np.array_equal(ha, b.to_host()) and np.array_equal(ha, s.to_host())
            assert not np.array_equal(ha, c.to_host())
            assert len(np.unique(ha)) == n                             # no two links share a draw
    finally:
        qmg.stream_destroy(st)
    # beta == 0 is the hot start; the sign of beta does not matter
    a, b = qmg.DeviceArray(2 * V), qmg.DeviceArray(2 * V)
    qmg.u1_gauss_gauge(a, Lx, Ly, 0.0, 5); qmg.u1_hot_gauge(b, Lx, Ly, 5)
    assert np.array_equal(a.to_host(), b.to_host())
    qmg.u1_gauss_gauge(a, Lx, Ly, -6.0, 5); qmg.u1_gauss_gauge(b, Lx, Ly, 6.0, 5)
    assert np.array_equal(a.to_host(), b.to_host())


def test_random_fields_follow_their_laws():
    L, beta = 256, 6.0
    V = L * L
    dg = qmg.DeviceArray(2 * V)
    qmg.u1_gauss_gauge(dg, L, L, beta, 2024)
    p = qmg.u1_plaquette(dg, L, L)[0].real
    # four independent N(0, 1/beta) phases per plaquette: <cos> = exp(-2/beta), var(cos) = (1 + e^{-8/beta})/2 - e^{-4/beta}; 8 sigma of the
    # independent-plaquette scatter, because neighbouring plaquettes share links
    sigma = np.sqrt((0.5 * (1 + np.exp(-8.0 / beta)) - np.exp(-4.0 / beta)) / V)
    print("gaussian field beta 6 256^2: plaquette %.6f, exp(-2/beta) %.6f, sigma %.2e" % (p, np.exp(-2.0 / beta), sigma))
    assert abs(p - np.exp(-2.0 / beta)) < 8 * sigma
    A = np.angle(dg.to_host())
    assert abs(A.mean()) < 8 * np.sqrt(1.0 / beta / (2 * V)) and abs(A.var() - 1.0 / beta) < 8 * np.sqrt(2.0 / (2 * V)) / beta
    qmg.u1_hot_gauge(dg, L, L, 2025)
    p = qmg.u1_plaquette(dg, L, L)[0]
    print("hot field 256^2: plaquette %.2e %+.2ei, 8/sqrt(V) = %.2e" % (p.real, p.imag, 8 / np.sqrt(V)))
    assert abs(p) < 8.0 / np.sqrt(V)
    dt = qmg.DeviceArray(V)
    qmg.u1_random_trans(dt, L, L, 2026)
    ph = np.angle(dt.to_host())
    # uniform on (-pi, pi): mean 0, variance pi^2/3, fourth moment pi^4/5
    se_mean, se_var = np.sqrt(np.pi ** 2 / 3 / V), np.sqrt((np.pi ** 4 / 5 - np.pi ** 4 / 9) / V)
    print("transform phases: mean %.2e (se %.2e), variance %.6f - pi^2/3 = %.2e (se %.2e)" % (ph.mean(), se_mean, ph.var(), ph.var() - np.pi ** 2 / 3, se_var))
    assert abs(ph.mean()) < 8 * se_mean and abs(ph.var() - np.pi ** 2 / 3) < 8 * se_var
    assert np.abs(ph).max() < np.pi


def test_invalid_arguments_are_refused():
    L = 8
    d = qmg.DeviceArray(2 * L * L)
    for call in (lambda: qmg.u1_ape_smear(d, d, L, L + 1, 0.5, 1), lambda: qmg.u1_ape_smear(d, d, L, L, 0.5, -1), lambda: qmg.u1_ape_smear(None, d, L, L, 0.5, 1),
                 lambda: qmg.u1_gauge_transform(d, None, L, L), lambda: qmg.u1_instanton(d, 7, L, 1.0, 0, 0), lambda: qmg.u1_instanton(d, L, L, 1.0, -3 * L, 0),
                 lambda: qmg.u1_hot_gauge(None, L, L, 1), lambda: qmg.u1_gauss_gauge(d, 0, L, 6.0, 1), lambda: qmg.u1_random_trans(d, L, 3, 1),
                 lambda: qmg.u1_noncompact_instanton(None, L, L, 1.0)):
        with pytest.raises(qmg.QmgError, match="invalid"):
            call()


PAIR = r"\(([-\d.]+),([-\d.]+)\) and topology ([-\d.]+)"


def test_n01_u1_test_driver(tmp_path):
    out = subprocess.run([os.path.join(DRIVERS, "n01_u1_test"), "16", str(tmp_path / "cfg16_hot.dat")], cwd=DRIVERS, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    print(out.stdout)
    unit = re.search(r"A unit gauge field has average plaquette " + PAIR, out.stdout)
    assert unit and float(unit.group(1)) == 1.0 and float(unit.group(2)) == 0.0 and float(unit.group(3)) == 0.0
    rungs = re.findall(r"A gauge field with beta ([-\d.]+) has average plaquette " + PAIR + r"\n and, after 3 iteration\(s\) of ape smearing with alpha=0.100000, has average plaquette " + PAIR, out.stdout)
    assert [r[0] for r in rungs] == ["100.000000", "10.000000", "1.000000", "0.100000", "0.010000", "0.001000", "0.000100"]   # the last product is 1.0000000000000003e-4 > 1e-4
    for r in rungs:
        assert float(r[4]) > float(r[1]), r
    loaded = re.search(r"The loaded gauge field has average plaquette (\(.*?\)) and topology", out.stdout).group(1)
    after = re.search(r"After a random gauge transform, the average plaquette is (\(.*?\)) and topology", out.stdout).group(1)
    assert loaded == after
    assert re.search(r"After adding an instanton with charge 1, the average plaquette is " + PAIR, out.stdout)
    assert np.loadtxt(str(tmp_path / "cfg16_hot.dat")).shape == (2 * 16 * 16,)


def test_u1_make_config_feeds_the_kcycle_driver(tmp_path):
    L, cfg = 64, str(tmp_path / "f.dat")
    out = subprocess.run([os.path.join(DRIVERS, "u1_make_config"), "64", "6.0", "4000", "1337", cfg, "0.5", "2"], cwd=DRIVERS, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    print(out.stdout)
    stages = re.findall(r"^\[QMG-GAUGE\]: plaq ([-\d.]+) topo ([-\d.]+) \((.*)\)$", out.stdout, re.M)
    assert [s[2] for s in stages] == ["heatbath", "ape smearing"]
    assert 0.90 < float(stages[0][0]) < 0.94                          # test_gpu_u1.py's band: beta = 6.0, exp(-1/12) = 0.9200
    assert float(stages[1][0]) > float(stages[0][0])
    Ux, Uy = cs.phases_to_links(np.loadtxt(cfg), L, L)
    got = qmg.u1_plaquette(up(Ux, Uy), L, L)[0].real
    assert abs(got - float(stages[1][0])) < 1e-6
    assert abs(got - un.plaquette(Ux, Uy)[0].real) < 1e-13
    # mass -0.01 is the reference n16's own value at 64^2; tile = L: the file is the whole lattice
    kc = subprocess.run([os.path.join(DRIVERS, "n13_wilson_kcycle"), "64", "-0.01", "6.0", "1", "8", cfg, "64"], cwd=DRIVERS, capture_output=True, text=True, timeout=300)
    print(kc.stdout[-1500:])
    assert kc.returncode == 0, kc.stdout[-3000:] + kc.stderr[-2000:]
    assert re.search(r"Multigrid converged in \d+ iterations", kc.stdout), kc.stdout[-1500:]
