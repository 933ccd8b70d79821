"""The reductions hold their documented summation order bit for bit (the order is written out in tests/reduce_order_numpy.py).

Every case uploads inputs whose products are exact in a double, runs the entry point, and requires the BYTES of the emulation: the lane's
serial accumulation, the xor-1...32 tree, the wavefronts in index order, the partials thread-strided and through tree and wavefronts
again.  tests/test_host_reduce_order.py shows that on these inputs another order changes the bits of more than 90 % of the outputs, so a
reordered reduction cannot pass.  The cases are true of the butterfly-per-value reduction (wave_sum) and of the recursive-halving one
(wave_reduce_many) alike: that is the point.

Shapes: n in {1, 63, 64, 65, 255, 256, 257, 1000, 262147} (below, at and above a wavefront and a block; a ragged last block; 1024 blocks
with a second trip of the grid-stride loop); 1, 3 and 8 systems with masks with holes; nj in {1, 2, 3, 4, 7, 8, 9, 15, 32} (every chunking into
kernels of 8 / 4 / 2 / 1 dots), and 33 and 64 for the single-vector multidot (more than one pass takes); complex<double>, and complex<float> read one and two elements per access.  Not the full product: every n
meets every storage form and every nj, the batch shapes rotate, and n = 262147 goes with the widest shapes that stay small on the host.
"""
import ctypes as C
import importlib

import numpy as np
import pytest

import reduce_order_numpy as ro

qmg = importlib.import_module("quantum-mg_amd")

pytestmark = pytest.mark.gpu

SMALL_N = (1, 63, 64, 65, 255, 256, 257, 1000)
BIG_N = 262147
NJS = (1, 2, 3, 4, 7, 8, 9, 15, 32)
BATCHES = ((1, 0b1), (3, 0b101), (8, 0b10111101))     # (systems, mask)
FORMS = ("f64", "f32w1", "f32w2")
BIG_MULTIDOT = {("f64", 1): 2, ("f64", 8): 0, ("f64", 9): 1, ("f32w1", 2): 1, ("f32w1", 8): 0}   # (form, nj) -> batch shape at n = BIG_N


@pytest.fixture(scope="module", autouse=True)
def _device():
    qmg.build()
    qmg.init(0)
    yield
    qmg.sync()


def same_bits(got, want):
    return np.array_equal(np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(want).view(np.uint64))


def layout(form, n, nrhs):
    """(dtype code, numpy storage, mantissa bits, stride): f32w2 on even strides, f32w1 on odd ones wherever a stride is read"""
    if form == "f64":
        return qmg.C64, np.complex128, 25, n + 6
    stride = n + 6
    if form == "f32w1" and stride % 2 == 0:
        stride += 1
    if form == "f32w2" and stride % 2:
        stride += 1
    return qmg.C32, np.complex64, 23, stride


def batch_vectors(rng, n, nrhs, stride, bits, count, like=None):
    """count vectors of nrhs systems, host values (count, nrhs, stride); the padding holds values too: it must not be read"""
    return ro.cvalues(rng, (count, nrhs, stride), bits, like)


def upload(host, store):
    return [qmg.DeviceArray.from_host(v.reshape(-1).astype(store)) for v in host]


def free(*arrays):
    for a in arrays:
        a.free()


def sizes_for(form):
    return tuple(n for n in SMALL_N if form != "f32w2" or n % 2 == 0)


def check_batch_multidot(form, nj, n, nrhs, mask, seed):
    dtype, store, bits, stride = layout(form, n, nrhs)
    rng = np.random.default_rng(seed)
    xs, _ = batch_vectors(rng, n, nrhs, stride, bits, nj)
    y, _ = batch_vectors(rng, n, nrhs, stride, bits, 1)
    ro.make_cancelling(rng, xs, y, n)
    dxs, dy = upload(xs, store), upload(y, store)
    xs, y = xs[:, :, :n], y[:, :, :n]
    W = qmg.batch_plan(qmg.BE_MULTIDOT, dtype, n, stride, nrhs, mask, nj=nj)[0][1]
    if form == "f32w2":
        assert W == 2
    if form == "f32w1" and (nrhs > 1 or n % 2):
        assert W == 1
    got = qmg.batch_multidot_t(dtype, dxs, dy[0], n, nrhs, stride, mask)      # (nrhs, nj)
    free(*dxs, *dy)
    act = [k for k in range(nrhs) if (mask >> k) & 1]
    re_t, im_t = ro.dot_terms(xs[:, act], y[:, act])                            # (nj, active, n)
    want = ro.complex_sum(re_t, im_t, n, W).T                                   # (active, nj)
    assert same_bits(got[act], want), (form, nj, n, nrhs, hex(mask), W)
    assert np.all(np.isnan(got[np.array([k for k in range(nrhs) if k not in act], dtype=int)].real))   # inactive systems: left as they were
    return W


@pytest.mark.parametrize("nj", NJS)
@pytest.mark.parametrize("form", FORMS)
def test_batch_multidot_bits(form, nj):
    widths = set()
    for i, n in enumerate(sizes_for(form)):
        nrhs, mask = BATCHES[(i + NJS.index(nj)) % 3]
        widths.add(check_batch_multidot(form, nj, n, nrhs, mask, 1000 * nj + n))
    if (form, nj) in BIG_MULTIDOT:
        nrhs, mask = BATCHES[BIG_MULTIDOT[(form, nj)]]
        widths.add(check_batch_multidot(form, nj, BIG_N, nrhs, mask, 77 + nj))
    assert (widths == {2}) if form == "f32w2" else (1 in widths)


@pytest.mark.parametrize("op", (qmg.BRED_NORM2, qmg.BRED_DOT, qmg.BRED_DIFFNORM2), ids=("norm2", "dot", "diffnorm2"))
@pytest.mark.parametrize("form", FORMS)
def test_batch_reduce_bits(form, op):
    for i, n in enumerate(sizes_for(form) + (() if form == "f32w2" else (BIG_N,))):
        nrhs, mask = BATCHES[(i + op) % 3]
        dtype, store, bits, stride = layout(form, n, nrhs)
        rng = np.random.default_rng(5000 + 10 * n + op)
        x, exps = batch_vectors(rng, n, nrhs, stride, bits, 1)
        y, _ = batch_vectors(rng, n, nrhs, stride, bits, 1, exps if op == qmg.BRED_DIFFNORM2 else None)
        if op == qmg.BRED_DOT:
            ro.make_cancelling(rng, x, y, n)
        dx, dy = upload(x, store), upload(y, store)
        x, y = x[:, :, :n], y[:, :, :n]
        W = qmg.batch_plan(qmg.BE_REDUCE, dtype, n, stride, nrhs, mask, op=op)[0][1]
        got = qmg.batch_reduce_t(dtype, op, dx[0], dy[0], n, nrhs, stride, mask)
        free(*dx, *dy)
        act = [k for k in range(nrhs) if (mask >> k) & 1]
        xa, ya = x[0, act], y[0, act]
        if op == qmg.BRED_DOT:
            want = ro.complex_sum(*ro.dot_terms(xa, ya), n, W)
        else:
            want = ro.device_sum(ro.norm_terms(xa) if op == qmg.BRED_NORM2 else ro.diff_terms(xa, ya), n, W) + 0j
        assert same_bits(got[act], want), (form, op, n, nrhs, hex(mask), W)


@pytest.mark.parametrize("nj", NJS + (33, 64))      # (33, 64: more vectors than one pass of the multidot kernels takes)
def test_multidot_bits(nj):
    for n in (1000,) if nj > 32 else SMALL_N + ((BIG_N,) if nj == 8 else ()):
        rng = np.random.default_rng(9000 + 100 * nj + n)
        xs, _ = ro.cvalues(rng, (nj, n), 25)
        y, _ = ro.cvalues(rng, (n,), 25)
        ro.make_cancelling(rng, xs, y, n)
        dxs, dy = [qmg.DeviceArray.from_host(v) for v in xs], qmg.DeviceArray.from_host(y)
        got = qmg.multidot(dxs, dy, n)
        free(*dxs, dy)
        assert same_bits(got, ro.complex_sum(*ro.dot_terms(xs, y[None, :]), n)), (nj, n)


def test_single_vector_reductions_bits():
    for n in SMALL_N + (BIG_N,):
        rng = np.random.default_rng(12000 + n)
        x, exps = ro.cvalues(rng, (n,), 25)
        z, _ = ro.cvalues(rng, (n,), 25, exps)
        u, _ = ro.cvalues(rng, (n,), 25)
        y, _ = ro.cvalues(rng, (n,), 25)
        ro.make_cancelling(rng, u, y, n)
        dx, dz, du, dy = (qmg.DeviceArray.from_host(v) for v in (x, z, u, y))
        n2, d, dn, ninf = qmg.norm2sq(dx, n), qmg.dot(du, dy, n), qmg.diffnorm2sq(dx, dz, n), qmg.norminf(dx, n)
        free(dx, dz, du, dy)
        assert same_bits(np.float64(n2), ro.device_sum(ro.norm_terms(x), n)), n
        assert same_bits(np.complex128(d), ro.complex_sum(*ro.dot_terms(u, y), n)), n
        assert same_bits(np.float64(dn), ro.device_sum(ro.diff_terms(x, z), n)), n
        # a maximum has no order; |x|^2 is exact products and one rounding of their sum, the square root is held to one unit in the last place
        want = np.sqrt(np.max(x.real * x.real + x.imag * x.imag))
        assert abs(ninf - want) <= np.spacing(want), n


def _through(call, width):
    """the `width` doubles of one single-vector reduction three ways: out_host alone, out_dev alone (asynchronous: read after a
    synchronise), and both at once"""
    host, both = (C.c_double * width)(), (C.c_double * width)()
    dev, dev2 = qmg.DeviceArray.from_host(np.full(width + 1, np.nan)), qmg.DeviceArray.from_host(np.full(width + 1, np.nan))
    qmg.check(call(None, host))
    qmg.check(call(C.cast(C.c_void_p(dev.ptr), C.POINTER(C.c_double)), None))
    qmg.check(call(C.cast(C.c_void_p(dev2.ptr), C.POINTER(C.c_double)), both))
    got = np.array(host[:]), dev.to_host(), np.array(both[:]), dev2.to_host()
    free(dev, dev2)
    return got


@pytest.mark.parametrize("red", ("norm2sq", "dot", "diffnorm2sq", "norminf", "multidot"))
def test_single_vector_reductions_through_out_dev(red):
    """a result taken through the device pointer is the bytes of the one taken through the host pointer, and nothing is written behind it"""
    L = qmg.lib()
    for n in (257, 1000):
        rng = np.random.default_rng(13000 + n)
        nj = 33
        xs, _ = ro.cvalues(rng, (nj, n), 25)
        y, _ = ro.cvalues(rng, (n,), 25)
        ro.make_cancelling(rng, xs, y, n)
        dxs, dy = [qmg.DeviceArray.from_host(v) for v in xs], qmg.DeviceArray.from_host(y)
        px, py, nn = C.c_void_p(dxs[0].ptr), C.c_void_p(dy.ptr), C.c_size_t(n)
        ptrs = (C.c_void_p * nj)(*[d.ptr for d in dxs])
        call, width = {
            "norm2sq": (lambda od, oh: L.qmg_norm2sq(px, nn, od, oh, None), 1),
            "dot": (lambda od, oh: L.qmg_dot(px, py, nn, od, oh, None), 2),
            "diffnorm2sq": (lambda od, oh: L.qmg_diffnorm2sq(px, py, nn, od, oh, None), 1),
            "norminf": (lambda od, oh: L.qmg_norminf(px, nn, od, oh, None), 1),
            "multidot": (lambda od, oh: L.qmg_multidot(ptrs, nj, py, nn, od, oh, None), 2 * nj),
        }[red]
        host, dev, both, dev2 = _through(call, width)
        free(*dxs, dy)
        assert not np.any(np.isnan(host))
        for d in (dev, dev2):
            assert same_bits(d[:width], host) and np.isnan(d[width]), (red, n)
        assert same_bits(both, host), (red, n)
        if red == "dot":
            assert same_bits(host.view(np.complex128), ro.complex_sum(*ro.dot_terms(xs[0], y), n)), n
        if red == "multidot":
            assert same_bits(host.view(np.complex128), ro.complex_sum(*ro.dot_terms(xs, y[None, :]), n)), n
