"""The flavour-singlet kernels on the GPU (csrc/qmg_singlet.hip) against singlet_numpy's statement, and the facade through drivers/wilson_singlet
against a dense numpy solve on the same links (tests/test_host_singlet.py holds the twin to its own identities without a GPU).

Lattices (2, 2), (4, 6), (130, 2), (16, 8) x nc = 1, 2, 4 x every dilution (nt in {1, 2, Ly}, spin, eo) x batches of 1, 3 and 16 systems with
first_class > 0, a sparse mask and a long stride, in fp64 and fp32.  Ly = 2 rows of 2 nc elements leave most of a block idle, (130, 2) with
nc = 4 has runs of 260 elements (a second trip of the lanes), and (2, 65536) is the smallest lattice whose rows exceed one grid dimension
(qmg_singlet_plan: walk = 2).

Noise and dilution move exact values (0, +-1, +-i): bit for bit.  The loops are fp64 sums in another order than numpy's: the gate of
tests/test_gpu_reductions.py, |got - want| <= 1e-12 sum_row |psi| per entry.

End to end at 8 x 8 (phases 0.5 uniform(-pi, pi), mass 0.2: cond(D) = 6.17, ||D^-1||_2 = 1.60): with r_d the driver's true residual of class d
and delta_d = ||D^-1||_2 |r_d| + 1e-12 ||psi_d|| (the second term: links that differ in the last bit, std::polar against np.exp, and the
summation order), every S_d(y), P_d(y) lies within sqrt(|support_d(y)|) delta_d of the twin by Cauchy-Schwarz, and every N_d(y) within
(2 ||psi_d||_row(y) + delta_d) delta_d.
"""
import functools
import importlib
import itertools
import os
import subprocess

import numpy as np
import pytest

import coordspace as cs
import singlet_numpy as sn

qmg = importlib.import_module("quantum-mg_amd")
pytestmark = pytest.mark.gpu
D = qmg.DeviceArray.from_host

LATTICES = [(2, 2), (4, 6), (130, 2), (16, 8)]
IDS = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)
PREC = pytest.mark.parametrize("f32", [False, True], ids=["c64", "c32"])
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVERS = os.path.join(ROOT, "quantum-mg_amd", "drivers")
SEED = 20261020


@pytest.fixture(scope="module", autouse=True)
def _device():
    qmg.build()
    qmg.init(0)
    yield
    qmg.sync()


def cvec(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def types(f32):
    return (qmg.C32, np.complex64) if f32 else (qmg.C64, np.complex128)


def dilutions(Ly):
    return [(nt, spin, eo) for nt in sorted({1, 2, Ly}) for spin in (0, 1) for eo in (0, 1)]


def batches(nd):
    """(nrhs, first_class, mask, elements between the systems) that fit nd classes: one system, three from the top classes, sixteen under a
    sparse mask with a long stride"""
    out = [(1, nd - 1, 1, 0)]
    if nd >= 3:
        out.append((3, nd - 3, 0b111, 2))
    if nd >= 16:
        out.append((16, nd - 16, 0x8425, 70))
    return out


def cases(dims):
    Lx, Ly = dims
    for nc, dil in itertools.product((1, 2, 4), dilutions(Ly)):
        for nrhs, first, mask, extra in batches(sn.n_classes(nc, dil)):
            yield nc, dil, nrhs, first, mask, extra


def active(mask, nrhs):
    return [k for k in range(nrhs) if (mask >> k) & 1]


# ---- the noise
@pytest.mark.parametrize("n", [1, 255, 4097])
def test_noise_z4_bit_for_bit(n):
    start = np.full(n + 3, np.nan + 0j)
    d = D(start)
    qmg.noise_z4(d, n, SEED)
    got = d.to_host()
    assert got[:n].tobytes() == sn.noise_z4(SEED, n).tobytes()
    assert got[n:].tobytes() == start[n:].tobytes()
    # the largest seed: the product wraps mod 2^64 as the twin's does
    qmg.noise_z4(d, n, 2 ** 64 - 1)
    assert d.to_host()[:n].tobytes() == sn.noise_z4(2 ** 64 - 1, n).tobytes()


@PREC
@pytest.mark.parametrize("dims", LATTICES, ids=IDS)
def test_dilution_bit_for_bit_and_isolated(dims, f32):
    """Every element of an active system is the twin's diluted noise; frozen systems and the padding between the systems, pre-filled with NaN,
    come back bit for bit."""
    Lx, Ly = dims
    dt, npt = types(f32)
    for nc, dil, nrhs, first, mask, extra in cases(dims):
        n = Lx * Ly * nc
        stride = n + extra
        start = np.full(nrhs * stride, np.nan + 1j * np.nan, dtype=npt)
        out = D(start)
        qmg.noise_dilute_batch(dt, out, dims, nc, dil, first, SEED, nrhs, stride, mask)
        got = out.to_host()
        tag = (nc, dil, nrhs, first, hex(mask))
        for k in range(nrhs):
            sl = slice(k * stride, k * stride + n)
            if (mask >> k) & 1:
                assert got[sl].tobytes() == sn.diluted(SEED, Lx, Ly, nc, dil, first + k).astype(npt).tobytes(), tag + (k,)
                assert got[sl.stop:(k + 1) * stride].tobytes() == start[sl.stop:(k + 1) * stride].tobytes(), tag + (k, "padding")
            else:
                assert got[k * stride:(k + 1) * stride].tobytes() == start[k * stride:(k + 1) * stride].tobytes(), tag + (k, "frozen")


# ---- the loops
def loops_case(dims, nc, dil, nrhs, first, mask, extra, f32, g5_mode, seed=3):
    """(psi on the device, the host copy with NaN in frozen systems and padding, got[k, y, 5], stride)"""
    Lx, Ly = dims
    dt, npt = types(f32)
    n = Lx * Ly * nc
    stride = n + extra
    x = np.full(nrhs * stride, np.nan + 1j * np.nan, dtype=npt)
    for k in active(mask, nrhs):
        x[k * stride:k * stride + n] = cvec(n, seed + k).astype(npt)
    dx = D(x)
    got = qmg.loops_timeslice_batch(dt, dx, dims, nc, dil, first, SEED, g5_mode, nrhs, stride, mask, fill=-7.5)
    return dx, x, got, stride


def check_loops(dims, nc, dil, nrhs, first, mask, x, got, stride, g5_mode, tag):
    Lx, Ly = dims
    n = Lx * Ly * nc
    worst = 0.0
    for k in range(nrhs):
        if not (mask >> k) & 1:
            assert np.all(got[k] == -7.5), tag + (k, "a frozen system's entries were written")
            continue
        xk = x[k * stride:k * stride + n].astype(np.complex128)
        want = sn.loops(xk, SEED, Lx, Ly, nc, dil, first + k, g5_mode)
        gate = 1e-12 * sn.row_abs_sum(xk, Lx, Ly, nc)
        err = np.abs(got[k] - want)
        assert np.all(np.isfinite(got[k])), tag + (k, "NaN reached the output")
        assert np.all(err <= gate[:, None]), tag + (k, float((err / gate[:, None]).max()))
        worst = max(worst, float((err / gate[:, None]).max()))
        # rows outside the class hold exact zeros in S and P, and N is a sum of squares
        off = sn.support_sizes(Lx, Ly, nc, dil, first + k) == 0
        assert not np.any(got[k][off, :4]) and np.all(got[k][:, 4] > 0), tag + (k,)
    return worst


@PREC
@pytest.mark.parametrize("dims", LATTICES, ids=IDS)
def test_loops_against_the_twin(dims, f32):
    """fp64: random psi; fp32: the twin on the input rounded to complex64 (a product of two floats is exact in a double), the same gate."""
    worst = 0.0
    for nc, dil, nrhs, first, mask, extra in cases(dims):
        for g5_mode in ((0, 1) if nc % 2 == 0 else (1,)):
            dx, x, got, stride = loops_case(dims, nc, dil, nrhs, first, mask, extra, f32, g5_mode)
            worst = max(worst, check_loops(dims, nc, dil, nrhs, first, mask, x, got, stride, g5_mode, (nc, dil, nrhs, first, hex(mask), g5_mode)))
    print("loops %s %s worst err / gate %.4f" % (dims, "c32" if f32 else "c64", worst))


@PREC
@pytest.mark.parametrize("dims", LATTICES, ids=IDS)
def test_loops_are_deterministic_and_isolated(dims, f32):
    """A second run, out_dev against out_host, and every system alone at nrhs = 1: the same bits.  NaN in frozen systems and padding reaches no
    output (loops_case puts it there), and the entries of frozen systems keep their prefill on the host and on the device."""
    Lx, Ly = dims
    dt, npt = types(f32)
    for nc, dil, nrhs, first, mask, extra in cases(dims):
        g5_mode = 1 if nc % 2 else 0
        dx, x, got, stride = loops_case(dims, nc, dil, nrhs, first, mask, extra, f32, g5_mode)
        tag = (nc, dil, nrhs, first, hex(mask))
        prefill = np.full((nrhs, Ly, 5), 3.25)
        out_dev = D(prefill)
        again = qmg.loops_timeslice_batch(dt, dx, dims, nc, dil, first, SEED, g5_mode, nrhs, stride, mask, out_dev=out_dev, fill=-7.5)
        assert again.tobytes() == got.tobytes(), tag
        dev = out_dev.to_host().reshape(nrhs, Ly, 5)
        for k in range(nrhs):
            if (mask >> k) & 1:
                assert dev[k].tobytes() == got[k].tobytes(), tag + (k,)
                alone = qmg.loops_timeslice_batch(dt, dx.offset(k * stride), dims, nc, dil, first + k, SEED, g5_mode, 1, 0, 1)
                assert alone[0].tobytes() == got[k].tobytes(), tag + (k, "alone")
            else:
                assert dev[k].tobytes() == prefill[k].tobytes() and np.all(got[k] == -7.5), tag + (k, "frozen")
        assert dx.to_host().tobytes() == x.tobytes()


@PREC
def test_loops_walk_rows_beyond_the_grid_cap(f32):
    """(2, 65536): 65536 rows on 65535 blocks, block 0 takes rows 0 and 65535 (qmg_singlet_plan: walk 2); two systems under a mask of three."""
    dims, nc, dil = (2, 65536), 2, (2, 1, 1)
    plan = qmg.singlet_plan(dims, nc, dil, 1, 3, 0b101)
    assert plan[:5] == (qmg.SGF_ROWS, 256, 2, 65535, 2)
    dx, x, got, stride = loops_case(dims, nc, dil, 3, 1, 0b101, 6, f32, 0)
    worst = check_loops(dims, nc, dil, 3, 1, 0b101, x, got, stride, 0, ("walk",))
    print("walked rows worst err / gate %.4f" % worst)
    dt, npt = types(f32)
    out = D(np.full(3 * stride, np.nan + 0j, dtype=npt))
    qmg.noise_dilute_batch(dt, out, dims, nc, dil, 1, SEED, 3, stride, 0b101)
    h = out.to_host()
    for k in (0, 2):
        assert h[k * stride:k * stride + stride - 6].tobytes() == sn.diluted(SEED, dims[0], dims[1], nc, dil, 1 + k).astype(npt).tobytes()


# ---- the facade, through its driver
def parse(stdout):
    blocks, classes, loops, cur = {}, [], [], None
    for ln in stdout.splitlines():
        if ln.startswith("[QMG-BEGIN-"):
            cur = ln[len("[QMG-BEGIN-"):-1]
            blocks[cur] = []
        elif ln.startswith("[QMG-END-"):
            assert ln[len("[QMG-END-"):-1] == cur
            cur = None
        elif cur is not None:
            idx, val = ln.split()
            assert int(idx) == len(blocks[cur]) + (1 if cur.endswith("EFFMASS") else 0)
            blocks[cur].append(float(val))
        elif ln.startswith("[QMG-CLASS]: "):
            f = ln.split()[1:]
            classes.append(dict(noise=int(f[0]), d=int(f[1]), iter=int(f[2]), res=float(f[3]), src=float(f[4])))
        elif ln.startswith("[QMG-LOOPS]: "):
            f = ln.split()[1:]
            loops.append(dict(noise=int(f[0]), cond=float(f[1]), q5=float(f[2]), mq5=float(f[3]), topo=float(f[4]), iters=int(f[5]), worst=float(f[6])))
    return {k: np.array(v) for k, v in blocks.items()}, classes, loops


def run_driver(L, mass, n_refine, cfg, n_noise, dil, seed, route, dump):
    exe = os.path.join(DRIVERS, "wilson_singlet")
    assert os.path.exists(exe), "drivers/wilson_singlet is not built"
    os.makedirs(dump, exist_ok=True)
    args = [exe, str(L), repr(mass), "6.0", str(n_refine), "8", cfg, str(L), str(n_noise), str(dil[0]), str(dil[1]), str(dil[2]), str(seed), route, dump]
    out = subprocess.run(args, cwd=DRIVERS, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300, env=dict(os.environ, QMG_QUIET="1"))
    tagged = "\n".join(ln for ln in out.stdout.splitlines() if ln.startswith(("[QMG-CLASS]", "[QMG-LOOPS]", "[QMG-COND", "[QMG-TIMING]", "[QMG-ERROR]", "[QMG-INFO]")))
    print(tagged)
    assert out.returncode == 0, out.stdout[-4000:]
    blocks, classes, loops = parse(out.stdout)
    n = L * L * 2
    nd = sn.n_classes(2, dil)
    dumped = []
    for a in range(n_noise):
        t = np.loadtxt(os.path.join(dump, "loops_noise%d.txt" % a)).reshape(nd, L, 7)
        psi = np.fromfile(os.path.join(dump, "psi_noise%d.bin" % a), dtype=np.complex128).reshape(nd, n)
        dumped.append({"S": t[:, :, 2] + 1j * t[:, :, 3], "P": t[:, :, 4] + 1j * t[:, :, 5], "N": t[:, :, 6], "psi": psi})
    return blocks, classes, loops, dumped


def test_wilson_singlet_against_a_dense_solve(tmp_path):
    """8 x 8, nt = 8, spin, eo: 32 classes of four elements in two batches of 16, two noises, BiCGStab-6."""
    L, mass, dil, seed = 8, 0.2, (8, 1, 1), 4711
    ph = 0.5 * np.random.default_rng(5).uniform(-np.pi, np.pi, L * L * 2)
    cfg = tmp_path / "cfg8.dat"
    cfg.write_text("".join("%.17g\n" % p for p in ph))
    Ux, Uy = cs.phases_to_links(ph, L, L)
    Dm = sn.wilson_dense(Ux, Uy, mass)
    sv = np.linalg.svd(Dm, compute_uv=False)
    inv_norm = 1.0 / sv[-1]
    print("cond(D) = %.4f  ||D^-1||_2 = %.4f" % (sv[0] / sv[-1], inv_norm))
    blocks, classes, loops, dumped = run_driver(L, mass, 0, str(cfg), 2, dil, seed, "bicgstab", str(tmp_path / "dump"))
    nd = sn.n_classes(2, dil)
    assert len(classes) == 2 * nd and len(loops) == 2 and len(dumped) == 2
    worst = 0.0
    for a in range(2):
        want = sn.measure(Dm, seed + a, L, L, 2, dil)
        for d in range(nd):
            cl = classes[a * nd + d]
            assert (cl["noise"], cl["d"]) == (a, d) and cl["res"] < 20 * 1e-10
            supp = sn.support_sizes(L, L, 2, dil, d)
            assert abs(cl["src"] - np.sqrt(supp.sum())) < 1e-14
            psi = want["psi"][d]
            delta = inv_norm * cl["res"] * cl["src"] + 1e-12 * np.linalg.norm(psi)
            assert np.linalg.norm(dumped[a]["psi"][d] - psi) <= delta
            bound = np.sqrt(supp) * delta
            for name in ("S", "P"):
                err = np.abs(dumped[a][name][d] - want[name][d])
                assert np.all(err <= bound), (a, d, name, err.max(), bound.max())
                worst = max(worst, float((err[supp > 0] / bound[supp > 0]).max()))
            row = np.sqrt(want["N"][d])
            bound_n = (2 * row + delta) * delta
            err = np.abs(dumped[a]["N"][d] - want["N"][d])
            assert np.all(err <= bound_n), (a, d, "N", err.max())
            worst = max(worst, float((err / bound_n).max()))
    print("worst |got - twin| / bound %.3e" % worst)
    # what the driver prints is the twin's combine of what it dumped
    c = sn.combine(dumped, L, L, 2, dil)
    for tag, key in (("PION", "Cpi"), ("DISC", "Ddisc"), ("ETA", "Ceta")):
        rel = np.abs(blocks[tag] - c[key]) / np.abs(c[key])
        print("%s worst relative difference to the twin's combine %.3e" % (tag, rel.max()))
        assert blocks[tag].shape == (L,) and np.all(rel <= 1e-13), (tag, rel.max())
    for a in range(2):
        assert abs(loops[a]["q5"] - c["q5"][a]) <= 1e-13 * abs(c["q5"][a])
        assert abs(loops[a]["cond"] - c["condensate_per_noise"][a]) <= 1e-13 * abs(c["condensate_per_noise"][a])
        assert abs(loops[a]["mq5"] - mass * c["q5"][a]) <= 1e-13 * abs(mass * c["q5"][a])
    assert len(blocks["PION-EFFMASS"]) == L - 2 and len(blocks["ETA-EFFMASS"]) == L - 2


KC = dict(L=64, mass=-0.01, dil=(4, 1, 1), seed=99)


@functools.lru_cache(maxsize=None)
def _kc_run(route, dump):
    cfg = os.path.join(ROOT, "tests", "golden", "l64t64b60_heatbath.dat")
    return run_driver(KC["L"], KC["mass"], 1, cfg, 1, KC["dil"], KC["seed"], route, os.path.join(dump, route))


@pytest.fixture(scope="module")
def kc_dump(tmp_path_factory):
    return str(tmp_path_factory.mktemp("wilson_singlet"))


@pytest.mark.parametrize("route", ["kcycle", "kcycle_f32"])
def test_kcycle_route_agrees_with_bicgstab(kc_dump, route):
    """64^2 fixture, mass -0.01, one coarse level of 8 dof; nt = 4, spin, eo: 16 classes in ONE lock-step batch, one noise.  Both routes reach
    true residuals under 20 tol (the driver's exit status and its [QMG-CLASS] lines), and their loops differ by at most the Cauchy-Schwarz
    bound from the dumped solutions: |S_kc - S_bi|(d, y) <= sqrt(|support_d(y)|) ||psi_kc - psi_bi||_row(y), the same for P, and
    |N_kc - N_bi| <= (||psi_kc||_row + ||psi_bi||_row) ||psi_kc - psi_bi||_row."""
    L, dil = KC["L"], KC["dil"]
    nd = sn.n_classes(2, dil)
    assert nd == 16
    bi = _kc_run("bicgstab", kc_dump)
    kc = _kc_run(route, kc_dump)
    y = sn.coords(L, L, 2)[0]
    worst = 0.0
    for run in (bi, kc):
        assert len(run[1]) == nd and all(c["res"] < 20 * 1e-10 and c["iter"] > 0 for c in run[1])
    print("%s iterations %s ; bicgstab %s" % (route, [c["iter"] for c in kc[1]], [c["iter"] for c in bi[1]]))
    for d in range(nd):
        pk, pb = kc[3][0]["psi"][d], bi[3][0]["psi"][d]
        diff = np.sqrt(np.bincount(y, weights=np.abs(pk - pb) ** 2, minlength=L))
        supp = sn.support_sizes(L, L, 2, dil, d)
        for name in ("S", "P"):
            err = np.abs(kc[3][0][name][d] - bi[3][0][name][d])
            bound = np.sqrt(supp) * diff
            assert np.all(err <= bound), (d, name, float(err.max()), float(bound.max()))
            worst = max(worst, float((err[supp > 0] / bound[supp > 0]).max()))
        nk, nb = np.sqrt(kc[3][0]["N"][d]), np.sqrt(bi[3][0]["N"][d])
        err = np.abs(kc[3][0]["N"][d] - bi[3][0]["N"][d])
        assert np.all(err <= (nk + nb) * diff), (d, "N", float(err.max()))
    print("%s against bicgstab: worst |difference| / Cauchy-Schwarz bound %.3e" % (route, worst))
    assert abs(kc[2][0]["topo"] - bi[2][0]["topo"]) == 0.0
