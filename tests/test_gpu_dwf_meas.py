"""The domain-wall measurement kernels on the GPU (csrc/qmg_dwf_meas.hip) -- qmg_dwf_wall_source, qmg_dwf_wall_project and
qmg_dwf_slice_norms against dwf_meas_numpy's statement on coordinate grids (tests/test_host_dwf_meas.py holds it to the dense operator
without a GPU) -- and the facade on them through drivers/dwf_measure against a dense numpy solve on the same links.

Lattices and Ls are those of test_gpu_dwf_eo.py: (2, 2), (4, 6), (130, 2), (16, 8) x Ls = 2, 3, 6, 8, 12, 32.  Ls = 3, 6, 12 do not divide
the wavefront (sites straddle wavefronts, the block of the norms is 255 / 252 / 252 lanes); blocks are partial; at (130, 2) with Ls = 8,
12, 32 a half row takes 3, 4, 4 partial blocks, so the partial slab holds more than one block per row, and at Ls = 32 the lanes stride.

Source and projections move values unchanged: bit for bit.  The norms: fp64 accumulation of Lx terms re^2 + im^2 per output, held to
stencil_numpy.elementwise_bound(S = want, n = Lx + 2) = (Lx + 3) 2^-50 want in both precisions, on inputs rounded to complex64 for fp32 (a
product of two floats is exact in a double).

One statement of the issue does not hold under its own conventions and is replaced: project(source(eta)) == eta.  The source puts eta(x, 0)
on slice 0 and the projection reads sigma 0 from slice Ls-1 (for sigma 1 the other way round), so project(source(eta)) is identically zero;
what comes back is the source reflected in s, which the test checks next to the zero.

The driver on the rough quenched 32 x 32 fixture (Ls = 8, m = 0.05), measured on an MI355X: see DESIGN 19."""
import functools
import importlib
import os
import subprocess

import numpy as np
import pytest

import dwf_meas_numpy as dm
import dwf_numpy as dn
import stencil_numpy as sn

qmg = importlib.import_module("quantum-mg_amd")
pytestmark = pytest.mark.gpu
D = qmg.DeviceArray.from_host

LATTICES = [(2, 2), (4, 6), (130, 2), (16, 8)]
LS_ALL = [2, 3, 6, 8, 12, 32]
IDS = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)
PREC = pytest.mark.parametrize("f32", [False, True], ids=["c64", "c32"])
INVALID, UNSUPPORTED = 1, 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


class Batch:
    """nsys vectors of n elements `stride` apart (nsys == 1: one vector, stride 0 in the call)"""

    def __init__(self, n, nsys, extra):
        self.n, self.nsys = n, nsys
        self.stride = n + extra if nsys > 1 else n
        self.arg = self.stride if nsys > 1 else 0
        self.total = nsys * self.stride
        self.pad = np.ones(self.total, dtype=bool)
        for k in range(nsys):
            self.pad[self.sl(k)] = False

    def sl(self, k):
        return slice(k * self.stride, k * self.stride + self.n)

    def start(self, seed, npt):
        """what an output holds before the call: NaN where it is overwritten, numbers between the systems"""
        a = cvec(self.total, seed).astype(npt)
        a[~self.pad] = np.nan
        return a


BATCHES = [(1, 0, 0), (3, 4, 6)]     # (nsys, extra elements between 5D systems, between 4D systems): even, so complex<float> systems stay 16-byte aligned


# ---- the wall source and the projections
@PREC
@pytest.mark.parametrize("dims", LATTICES, ids=IDS)
@pytest.mark.parametrize("Ls", LS_ALL)
def test_wall_source_and_projections_bit_for_bit(dims, Ls, f32):
    Lx, Ly = dims
    dt, npt = types(f32)
    for nsys, e5, e4 in BATCHES:
        b5, b4 = Batch(Lx * Ly * 2 * Ls, nsys, e5), Batch(Lx * Ly * 2, nsys, e4)
        eta = cvec(b4.total, 1).astype(npt)
        start5 = b5.start(2, npt)
        psi = D(start5)
        qmg.dwf_wall_source(dt, dims, Ls, psi, D(eta), nsys, b5.arg, b4.arg)
        h = psi.to_host()
        for k in range(nsys):
            assert h[b5.sl(k)].tobytes() == dm.wall_source(eta[b4.sl(k)], Lx, Ly, Ls).tobytes(), ("source", nsys, k)
        assert h[b5.pad].tobytes() == start5[b5.pad].tobytes(), "source wrote between the systems"
        # the projections of a full 5D field
        x = cvec(b5.total, 3).astype(npt)
        dx = D(x)
        for which, name in ((0, "wall"), (1, "mid")):
            start4 = b4.start(4 + which, npt)
            q = D(start4)
            rc = qmg.dwf_wall_project_status(dt, dims, Ls, q, dx, which, nsys, b4.arg, b5.arg)
            g = q.to_host()
            if which == 1 and Ls % 2:
                assert rc == UNSUPPORTED and g.tobytes() == start4.tobytes()      # no midpoint between the walls: refused, nothing written
                continue
            assert rc == 0
            for k in range(nsys):
                assert g[b4.sl(k)].tobytes() == dm.wall_project(x[b5.sl(k)], Lx, Ly, Ls, name).tobytes(), (name, nsys, k)
            assert g[b4.pad].tobytes() == start4[b4.pad].tobytes(), "projection wrote between the systems"
        # the round trip: the projection reads the walls opposite to the source's, so it sees zeros; the source reflected in s comes back
        start4 = b4.start(6, npt)
        q = D(start4)
        qmg.dwf_wall_project(dt, dims, Ls, q, psi, 0, nsys, b4.arg, b5.arg)
        g = q.to_host()
        refl = h.copy()
        for k in range(nsys):
            assert not np.any(g[b4.sl(k)])
            refl[b5.sl(k)] = h[b5.sl(k)].reshape(Lx * Ly, Ls, 2)[:, ::-1].reshape(-1)
        qmg.dwf_wall_project(dt, dims, Ls, q, D(refl), 0, nsys, b4.arg, b5.arg)
        g = q.to_host()
        for k in range(nsys):
            assert g[b4.sl(k)].tobytes() == eta[b4.sl(k)].tobytes(), ("round trip", nsys, k)


# ---- the slice norms
@PREC
@pytest.mark.parametrize("dims", LATTICES, ids=IDS)
@pytest.mark.parametrize("Ls", LS_ALL)
def test_slice_norms_within_the_fp64_bound_and_reproducible(dims, Ls, f32):
    Lx, Ly = dims
    dt, npt = types(f32)
    for nsys, e5, _ in BATCHES:
        b5 = Batch(Lx * Ly * 2 * Ls, nsys, e5)
        x = cvec(b5.total, 5).astype(npt)
        dx = D(x)
        out_dev = qmg.DeviceArray(nsys * Ly * 2 * Ls, np.float64)
        got = qmg.dwf_slice_norms(dt, dims, Ls, dx, nsys, b5.arg, out_dev)
        assert out_dev.to_host().tobytes() == got.tobytes()                       # out_dev and out_host: the same bits
        again = qmg.dwf_slice_norms(dt, dims, Ls, dx, nsys, b5.arg)               # host only
        assert again.tobytes() == got.tobytes()                                   # two calls: the same bits
        for k in range(nsys):
            xk = x[b5.sl(k)].astype(np.complex128)
            want = dm.slice_norms(xk, Lx, Ly, Ls)
            bound = sn.elementwise_bound(want, Lx + 2)
            err = np.abs(got[k].astype(np.longdouble) - want)
            worst = float(np.max(err / bound))
            print("dwf slice_norms %s Ls=%d %s nsys=%d k=%d worst err/bound %.4f" % (dims, Ls, "c32" if f32 else "c64", nsys, k, worst))
            assert np.all(err <= bound), (nsys, k, worst)
            # summed over the slices and spins: qmg_norm2sq_cv_timeslice on the same numbers, within the same bound
            ts = qmg.norm2sq_cv_timeslice(D(xk), Lx, Ly, 2 * Ls)
            want_t = want.sum(axis=(1, 2))
            bound_t = sn.elementwise_bound(want_t, Lx + 2)
            err_t = np.abs(got[k].astype(np.longdouble).sum(axis=(1, 2)) - ts.astype(np.longdouble))
            assert np.all(err_t <= bound_t), (nsys, k, float(np.max(err_t / bound_t)))
        assert dx.to_host().tobytes() == x.tobytes()


# ---- past the cap of grid.y: the 65540 (parity, y) rows of 2 x 32770 on 65535 blocks, so five blocks take a second row.  The rows are walked
# in storage order, row = parity Ly + y: the second trip is the odd rows y = 32765 .. 32769, the last five rows of a vector
TALL = (2, 32770)
TALL_Y0 = 32765


def capped(dt, Ls, kernel, nsys):
    plan = qmg.dwf_meas_plan(dt, TALL, Ls, kernel, nsys)
    assert plan[4] == 65535 < 2 * TALL[1] == 65540 and plan[7] == nsys, plan
    return plan


@PREC
@pytest.mark.parametrize("Ls", [2, 3])
def test_source_and_projections_walk_more_rows_than_the_grid_has_blocks(Ls, f32):
    Lx, Ly = TALL
    dt, npt = types(f32)
    for nsys, e5, e4 in BATCHES:
        b5, b4 = Batch(Lx * Ly * 2 * Ls, nsys, e5), Batch(Lx * Ly * 2, nsys, e4)
        tail5, tail4 = 5 * (Lx // 2) * 2 * Ls, 5 * (Lx // 2) * 2       # the elements of the five rows walked second
        assert capped(dt, Ls, qmg.DMK_SOURCE, nsys)[0] == qmg.DMF_SOURCE
        eta = cvec(b4.total, 1).astype(npt)
        start5 = b5.start(2, npt)
        runs = []
        for _ in range(2):
            psi = D(start5)
            qmg.dwf_wall_source(dt, TALL, Ls, psi, D(eta), nsys, b5.arg, b4.arg)
            runs.append(psi.to_host())
        h = runs[0]
        assert not np.any(np.isnan(h[~b5.pad])), "source: NaN prefill survived"
        for k in range(nsys):
            want = dm.wall_source(eta[b4.sl(k)], Lx, Ly, Ls)
            assert h[b5.sl(k)].tobytes() == want.tobytes(), ("source", nsys, k)
            assert h[b5.sl(k)][-tail5:].tobytes() == want[-tail5:].tobytes() and np.any(want[-tail5:]), ("source, second trip", nsys, k)
        assert h[b5.pad].tobytes() == start5[b5.pad].tobytes(), "source wrote between the systems"
        assert runs[1].tobytes() == h.tobytes()
        x = cvec(b5.total, 3).astype(npt)
        dx = D(x)
        for which, name, kernel in ((0, "wall", qmg.DMK_PROJECT_WALL), (1, "mid", qmg.DMK_PROJECT_MID)):
            if which == 1 and Ls % 2:
                continue                                           # no midpoint between the walls: test_wall_source_and_projections_bit_for_bit holds the refusal
            assert capped(dt, Ls, kernel, nsys)[0] == qmg.DMF_PROJECT
            start4 = b4.start(4 + which, npt)
            runs = []
            for _ in range(2):
                q = D(start4)
                qmg.dwf_wall_project(dt, TALL, Ls, q, dx, which, nsys, b4.arg, b5.arg)
                runs.append(q.to_host())
            g = runs[0]
            assert not np.any(np.isnan(g[~b4.pad])), (name, "NaN prefill survived")
            for k in range(nsys):
                want = dm.wall_project(x[b5.sl(k)], Lx, Ly, Ls, name)
                assert g[b4.sl(k)].tobytes() == want.tobytes(), (name, nsys, k)
                assert g[b4.sl(k)][-tail4:].tobytes() == want[-tail4:].tobytes(), (name, "second trip", nsys, k)
            assert g[b4.pad].tobytes() == start4[b4.pad].tobytes(), "projection wrote between the systems"
            assert runs[1].tobytes() == g.tobytes()


def norms_held(dims, Ls, f32, nsys, e5, tail_from=None):
    """qmg_dwf_slice_norms into a NaN-filled device result, twice, against the twin at the file's fp64 summation bound; tail_from: the
    first y whose odd row is walked second, compared on its own too"""
    Lx, Ly = dims
    dt, npt = types(f32)
    b5 = Batch(Lx * Ly * 2 * Ls, nsys, e5)
    x = cvec(b5.total, 5).astype(npt)
    dx = D(x)
    runs = []
    for _ in range(2):
        out_dev = D(np.full(nsys * Ly * 2 * Ls, np.nan))
        got = qmg.dwf_slice_norms(dt, dims, Ls, dx, nsys, b5.arg, out_dev)
        assert out_dev.to_host().tobytes() == got.tobytes()
        runs.append(got)
    got = runs[0]
    assert np.all(np.isfinite(got)), "NaN prefill survived"
    assert runs[1].tobytes() == got.tobytes()                                     # two calls: the same bits
    for k in range(nsys):
        want = dm.slice_norms(x[b5.sl(k)].astype(np.complex128), Lx, Ly, Ls)
        bound = sn.elementwise_bound(want, Lx + 2)
        err = np.abs(got[k].astype(np.longdouble) - want)
        print("dwf slice_norms %s Ls=%d %s nsys=%d k=%d worst err/bound %.4f" % (dims, Ls, "c32" if f32 else "c64", nsys, k, float(np.max(err / bound))))
        assert np.all(err <= bound), (nsys, k, float(np.max(err / bound)))
        if tail_from is not None:
            assert np.all(err[tail_from:] <= bound[tail_from:]) and err[tail_from:].shape[0] == 5, (nsys, k, "second trip")
    assert dx.to_host().tobytes() == x.tobytes()


@PREC
@pytest.mark.parametrize("Ls", [2, 3])
def test_slice_norms_walk_more_rows_than_the_grid_has_blocks(Ls, f32):
    for nsys, e5, _ in BATCHES:
        assert capped(types(f32)[0], Ls, qmg.DMK_NORMS, nsys)[0] == qmg.DMF_NORMS
        norms_held(TALL, Ls, f32, nsys, e5, TALL_Y0)


@PREC
@pytest.mark.parametrize("dims,Ls", [((520, 2), 32), ((4800, 2), 3)], ids=IDS)
def test_slice_norms_through_the_unrolled_loop(dims, Ls, f32):
    """wide half rows: lane 0 makes two trips of the loop that holds four chunks in flight, and only part of the lanes enter the remainder
    loop after it.  (520, 2), Ls = 32: 8320 lanes, step 1024; (4800, 2), Ls = 3: 7200 lanes, step 1020 (only lanes below 60 take the second
    unrolled trip)."""
    for nsys, e5, _ in BATCHES:
        family, _, block, gx, _, pbr, _, _ = qmg.dwf_meas_plan(types(f32)[0], dims, Ls, qmg.DMK_NORMS, nsys)
        lanes, step = dims[0] // 2 * Ls, pbr * block
        assert family == qmg.DMF_NORMS and gx == pbr
        assert lanes > 7 * step and lanes % (4 * step) != 0, (lanes, step)
        norms_held(dims, Ls, f32, nsys, e5)


def test_invalid_arguments_are_refused_before_any_launch():
    dims, Ls = (16, 8), 8
    n5, n4 = 16 * 8 * 2 * Ls, 16 * 8 * 2
    x0, e0 = cvec(17 * n5, 6), cvec(17 * n4, 7)
    x, e = D(x0), D(e0)
    out0 = np.arange(3 * 8 * 2 * Ls, dtype=np.float64)
    host = out0.copy()

    def source(dtype=qmg.C64, dims=dims, Ls=Ls, psi=x, eta=e, nsys=1, s5=0, s4=0):
        return qmg.dwf_wall_source_status(dtype, dims, Ls, psi, eta, nsys, s5, s4)

    def project(dtype=qmg.C64, dims=dims, Ls=Ls, q=e, psi=x, which=0, nsys=1, s4=0, s5=0):
        return qmg.dwf_wall_project_status(dtype, dims, Ls, q, psi, which, nsys, s4, s5)

    def norms(dtype=qmg.C64, dims=dims, Ls=Ls, psi=x, nsys=1, s5=0, out_dev=None, out_host=host):
        return qmg.dwf_slice_norms_status(dtype, dims, Ls, psi, nsys, s5, out_dev, out_host)

    for f in (source, project, norms):
        assert f(dtype=2) == INVALID and f(dtype=-1) == INVALID
        for bad in [(15, 8), (16, 7), (0, 8), (16, 0)]:
            assert f(dims=bad) == INVALID, bad
        for bad in (1, 0, 33):
            assert f(Ls=bad) == INVALID, bad
        assert f(nsys=0) == INVALID and f(nsys=17, s5=n5, **({} if f is norms else {"s4": n4})) == INVALID
        assert f(psi=None) == INVALID
        assert f(psi=x.ptr + 8) == INVALID                                   # not 16-byte aligned
        assert f(nsys=2, s5=n5 - 2, **({} if f is norms else {"s4": n4})) == INVALID        # 5D systems that overlap
        assert f(dtype=qmg.C32, nsys=2, s5=2 * n5 + 1, **({} if f is norms else {"s4": 2 * n4})) == INVALID   # complex<float>: an odd stride
    for f in (source, project):
        assert f(nsys=2, s5=n5, s4=n4 - 2) == INVALID                        # 4D systems that overlap
        assert f(dtype=qmg.C32, nsys=2, s5=2 * n5, s4=2 * n4 + 1) == INVALID
    assert source(eta=None) == INVALID and source(eta=e.ptr + 8) == INVALID
    assert project(q=None) == INVALID and project(q=e.ptr + 8) == INVALID
    assert project(which=2) == INVALID and project(which=-1) == INVALID
    assert norms(out_dev=None, out_host=None) == INVALID                     # nowhere to put the result
    # nothing was written by any of them
    assert x.to_host().tobytes() == x0.tobytes() and e.to_host().tobytes() == e0.tobytes() and host.tobytes() == out0.tobytes()
    # and the same calls with valid arguments succeed
    assert norms(nsys=3, s5=n5 + 2) == 0 and not np.array_equal(host, out0)


# ---- the facade, through its driver
M, EPS = 0.05, 1e-12


def parse(stdout):
    blocks, ward, mres, cur = {}, [], None, None
    for ln in stdout.splitlines():
        if ln.startswith("[QMG-BEGIN-"):
            cur = ln[len("[QMG-BEGIN-"):-1]
            blocks[cur] = []
        elif ln.startswith("[QMG-END-"):
            assert ln[len("[QMG-END-"):-1] == cur
            cur = None
        elif cur is not None:
            idx, val = ln.split()
            assert int(idx) == len(blocks[cur]) + (1 if cur == "PION-EFFMASS" else 0)
            blocks[cur].append(float(val))
        elif ln.startswith("[QMG-WARD]: "):
            f = ln.split()[1:]
            ward.append(dict(spin=int(f[0]), iter=int(f[1]), res=float(f[2]), psi=float(f[3]), lhs=float(f[4]), rhs=float(f[5]), defect=float(f[6])))
        elif ln.startswith("[QMG-MRES]: "):
            mres = float(ln.split()[1])
    return {k: np.array(v) for k, v in blocks.items()}, ward, mres


def run_driver(L, cfg, Ls, eps):
    exe = os.path.join(qmg.HERE, "drivers", "dwf_measure")
    assert os.path.exists(exe), "drivers/dwf_measure is not built"
    out = subprocess.run([exe, str(L), cfg, repr(M), str(Ls), "-1", repr(eps)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout
    return parse(out.stdout)


def ward_within_bound(ward, Ls, L):
    """|defect| <= 2 |Psi| |r| + (N + 1) 2^-50 lhs: the residual-aware identity with a factor 2, plus the rounding of the N = 2 Ls L^2 squares
    that lhs and |Psi|^2 sum"""
    N = 2 * Ls * L * L
    assert [w["spin"] for w in ward] == [0, 1]
    for w in ward:
        bound = 2 * w["psi"] * w["res"] + (N + 1) * 2.0 ** -50 * w["lhs"]
        print("ward spin %d iterations %d |defect| %.3e bound %.3e (%.3f of it)" % (w["spin"], w["iter"], abs(w["defect"]), bound, abs(w["defect"]) / bound))
        assert abs(w["defect"]) <= bound, w
        assert w["iter"] > 0 and w["lhs"] > 0


@pytest.fixture(scope="module")
def small_cfg(tmp_path_factory):
    """the 8 x 8 file: phases 0.4 N(0, 1) in the reference's text order (x outer, y, mu inner)"""
    ph = 0.4 * np.random.default_rng(11).standard_normal(128)
    path = tmp_path_factory.mktemp("dwf_measure") / "cfg8.dat"
    path.write_text("".join("%.17g\n" % p for p in ph))
    return str(path), ph.reshape(8, 8, 2)


@functools.lru_cache(maxsize=None)
def _small_run(cfg, Ls):
    return run_driver(8, cfg, Ls, EPS)


def dense_reference(ph, Ls):
    """(N[spin][y, s, sigma], |Psi_spin|, |B - D Psi_spin|, sigma_min(D)) from a dense solve on the file's links"""
    L = 8
    n = L * L * Ls * 2
    Ux, Uy = np.exp(1j * ph[:, :, 0]), np.exp(1j * ph[:, :, 1])
    eye = np.eye(n, dtype=np.complex128).reshape(L, L, Ls, 2, n)
    Dm, _, _ = dn._core(eye, np.zeros_like(eye), Ux, Uy, M, 1.0, -1.0, 0.0, 0.0, 0xFFF | (dn.P_ZERO_E * 3), np.complex128)
    Dm = Dm.reshape(n, n)
    smin = float(np.linalg.svd(Dm, compute_uv=False)[-1])
    out = []
    for spin in (0, 1):
        eta = np.zeros((L, L, 2), dtype=np.complex128)
        eta[0, 0, spin] = 1.0
        B = dm.source_grid(eta, Ls).reshape(-1)
        psi = np.linalg.solve(Dm, B)
        out.append((dm.norms_grid(psi.reshape(L, L, Ls, 2)), float(np.linalg.norm(psi)), float(np.linalg.norm(B - Dm @ psi))))
    return out, smin


@pytest.mark.parametrize("Ls", [4, 8, 12])
def test_dwf_measure_against_a_dense_solve(small_cfg, Ls):
    cfg, ph = small_cfg
    blocks, ward, mres = _small_run(cfg, Ls)
    ref, smin = dense_reference(ph, Ls)
    print("sigma_min(D) = %.6f" % smin)
    ward_within_bound(ward, Ls, 8)
    # | |a|^2 - |b|^2 | <= (|a| + |b|) |a - b| <= (2 |Psi| + delta) delta on any subset of the elements, per source spin; delta bounds the
    # distance of the driver's solution to numpy's: both residuals, and 2^-50 |Psi| for links that differ in the last bit (std::polar against
    # np.exp), over sigma_min
    N = sum(r[0] for r in ref)
    bound = 0.0
    for (_, psi, res), w in zip(ref, ward):
        delta = (w["res"] + res + 2.0 ** -50 * psi) / smin
        bound += (2 * psi + delta) * delta
        assert abs(w["psi"] - psi) <= delta
    cpi, cmp_, prof = dm.correlators(N)
    total = float(N.sum())
    for name, got, want, b in (("PION", blocks["PION"], cpi, bound), ("MIDPOINT", blocks["MIDPOINT"], cmp_, bound),
                               # p_s = N_s / T with both within `bound`: |p~ - p| <= bound / T~ + p bound / T~ <= 2 bound / (T - bound)
                               ("SPROFILE", blocks["SPROFILE"], prof, 2 * bound / (total - bound))):
        err = np.abs(got - want.astype(np.float64))
        print("%s Ls=%d worst |got - want| %.3e bound %.3e" % (name, Ls, err.max(), b))
        assert got.shape == want.shape and np.all(err <= b), (name, err.max(), b)
    assert np.allclose(blocks["MRES"], blocks["MIDPOINT"] / blocks["PION"], rtol=1e-14, atol=0)
    assert abs(mres - blocks["MIDPOINT"].sum() / blocks["PION"].sum()) <= 1e-14 * mres
    assert len(blocks["PION-EFFMASS"]) == 6


def test_m_res_falls_with_ls(small_cfg):
    cfg, _ = small_cfg
    m = [_small_run(cfg, Ls)[2] for Ls in (4, 8, 12)]
    print("m_res at Ls = 4, 8, 12: %.4e %.4e %.4e" % tuple(m))
    assert m[0] > m[1] > m[2] > 0


def test_dwf_measure_on_the_quenched_fixture():
    L, Ls = 32, 8
    blocks, ward, mres = run_driver(L, os.path.join(ROOT, "tests", "golden", "l32t32b60_heatbath.dat"), Ls, 1e-10)
    ward_within_bound(ward, Ls, L)
    assert blocks["PION"].shape == (L,) and np.all(blocks["PION"] > 0)
    prof = blocks["SPROFILE"]
    assert prof.shape == (Ls,) and abs(prof.sum() - 1) <= 1e-14
    assert sorted(np.argsort(prof)[-2:]) == [0, Ls - 1], prof               # the two wall slices hold the most
    print("quenched 32^2 Ls=8: m_res %.6e iterations %s" % (mres, [w["iter"] for w in ward]))
