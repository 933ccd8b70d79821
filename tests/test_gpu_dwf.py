"""The Shamir domain-wall operator on the GPU (csrc/qmg_dwf.hip): the stored-stencil fill and the apply straight from the gauge links
(kernel D), each against dwf_numpy's grid statement of the operator, which shares no index arithmetic with the kernels
(tests/test_host_dwf.py validates it without a GPU).

Lattices: (2, 2) every neighbour pair coincides; (4, 6) small general case; (130, 2) Lx/2 = 65 lanes and +-y coincide; (16, 8) regular.
Ls: 2, 3, 6, 8, 12 (3, 6, 12 do not divide the wavefront: sites straddle wavefronts and the last block is partial), and 32 for the direct
entry alone (nc = 64 is beyond the stored-stencil apply).

Bounds: the project's elementwise summation bound (stencil_numpy.elementwise_bound) on the term-magnitude sum S and term count n that
dwf_numpy returns -- fp64: (n + 1) 2^-50 S; fp32 arithmetic: (n + 1) 2^-21 S + 2^-23 |want|, against the grid formula on the inputs as the
kernel sees them (rounded to complex<float>)."""
import functools
import importlib
import os
import subprocess

import numpy as np
import pytest

import dwf_numpy as dn
import stencil_numpy as sn

qmg = importlib.import_module("quantum-mg_amd")
pytestmark = pytest.mark.gpu
D = qmg.DeviceArray.from_host
P = qmg

LATTICES = [(2, 2), (4, 6), (130, 2), (16, 8)]
LS_STORED = [2, 3, 6, 8, 12]
M, W = 0.05 + 0.02j, 0.9
SHIFTS = (-1.0 + 0.03j, 0.011 - 0.02j, 0.023 + 0.01j)     # shift (the domain-wall height), eo_shift, dof_shift: all three nonzero
SERVED = [P.P_ALL | P.P_ZERO, P.P_ALL, P.P_ALL | P.P_ZERO_E, P.P_CLOVER | P.P_HOPPING | P.P_ZERO, P.P_CLOVER | P.P_HOPPING,
          P.P_CLOVER_E | P.P_EO | P.P_SHIFT_E | P.P_ZERO_E, P.P_CLOVER_O | P.P_OE | P.P_SHIFT_O,
          P.P_HOPPING | P.P_ZERO, P.P_HOPPING, P.P_EO | P.P_ZERO_E, P.P_EO, P.P_OE | P.P_ZERO_O, P.P_OE]
IDS = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.fixture(scope="module", autouse=True)
def _device():
    qmg.build()
    qmg.init(0)
    yield
    qmg.sync()


def gauge(Lx, Ly, seed=11, width=0.4):
    return np.exp(1j * width * np.random.default_rng(seed).standard_normal(2 * Lx * Ly))


def cvec(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def rounded(a, f32):
    return a.astype(np.complex64).astype(np.complex128) if f32 else a


@functools.lru_cache(maxsize=None)
def case(dims, Ls, f32):
    """the inputs of one (lattice, Ls, precision) as the kernel sees them, computed once"""
    Lx, Ly = dims
    n = Lx * Ly * 2 * Ls
    return rounded(gauge(Lx, Ly), f32), rounded(cvec(n, 1), f32), rounded(cvec(n, 2), f32)


@functools.lru_cache(maxsize=None)
def reference(dims, Ls, f32, pieces):
    g, rhs, lhs0 = case(dims, Ls, f32)
    return dn.apply(dims[0], dims[1], Ls, g, M, W, *SHIFTS, pieces, rhs, lhs0)


def within(got, want, S, n, f32):
    err = np.abs(got.astype(sn.CLD) - want)
    bound = sn.elementwise_bound(S, n, want, fp32_arithmetic=True) if f32 else sn.elementwise_bound(S, n)
    worst = float(np.max(err / np.where(bound > 0, bound, 1)))
    return bool(np.all(err <= bound)), worst


def np_dtype(f32):
    return np.complex64 if f32 else np.complex128


# ---- the fill
@pytest.mark.parametrize("dims", LATTICES, ids=IDS)
@pytest.mark.parametrize("Ls", LS_STORED)
def test_fill_equals_the_numpy_fields(dims, Ls):
    Lx, Ly = dims
    nc2 = 4 * Ls * Ls
    g = gauge(Lx, Ly)
    dg = D(g)
    cl, hp = qmg.DeviceArray(Lx * Ly * nc2), qmg.DeviceArray(4 * Lx * Ly * nc2)
    # w = 1, m real: every entry is an exact product -- bit for bit
    qmg.dwf_fill(cl, hp, dg, Lx, Ly, Ls, 0.05, 1.0)
    wc, wh = dn.fields(Lx, Ly, Ls, g, 0.05, 1.0)
    assert np.array_equal(cl.to_host(), wc) and np.array_equal(hp.to_host(), wh)
    # w = 0.9, m complex: 3 w and w/2 U are rounded products on both sides -- within 1 ulp per entry
    qmg.dwf_fill(cl, hp, dg, Lx, Ly, Ls, M, W)
    wc, wh = dn.fields(Lx, Ly, Ls, g, M, W)
    for got, want in ((cl.to_host(), wc), (hp.to_host(), wh)):
        for part in (np.real, np.imag):
            assert np.all(np.abs(part(got) - part(want)) <= np.spacing(np.abs(part(want)))), (dims, Ls)
        assert np.array_equal(got == 0, want == 0)      # the zeros are zeros


# ---- the apply from the links, and the stored route beside it
@pytest.mark.parametrize("f32", [False, True], ids=["c64", "c32"])
@pytest.mark.parametrize("dims", LATTICES, ids=IDS)
@pytest.mark.parametrize("Ls", LS_STORED + [32])
def test_direct_apply_against_the_grid_formula(dims, Ls, f32):
    Lx, Ly = dims
    nc = 2 * Ls
    dt, npt = (qmg.C32 if f32 else qmg.C64), np_dtype(f32)
    g, rhs, lhs0 = case(dims, Ls, f32)
    dg, dx = D(g.astype(npt)), D(rhs.astype(npt))
    d = qmg.make_desc(Lx, Ly, nc, None, None, *SHIFTS)
    stored = None
    if Ls <= 12:
        cl, hp = qmg.DeviceArray(Lx * Ly * nc * nc), qmg.DeviceArray(4 * Lx * Ly * nc * nc)
        qmg.dwf_fill(cl, hp, D(gauge(Lx, Ly)), Lx, Ly, Ls, M, W)
        if f32:
            cl32, hp32 = qmg.DeviceArray(cl.n, np.complex64), qmg.DeviceArray(hp.n, np.complex64)
            qmg.convert(cl32, qmg.C32, cl, qmg.C64, cl.n)
            qmg.convert(hp32, qmg.C32, hp, qmg.C64, hp.n)
            cl, hp = cl32, hp32
        stored = qmg.make_desc(Lx, Ly, nc, cl, hp, *SHIFTS)
    for pieces in SERVED:
        want, S, n = reference(dims, Ls, f32, pieces)
        zeroed = [p for p in (0, 1) if pieces & (P.P_ZERO_E << p)]
        start = lhs0.copy()
        half = start.size // 2
        for p in zeroed:                                   # overwrite semantics: what ZERO clears is never read
            start[p * half:(p + 1) * half] = np.nan
        got = D(start.astype(npt))
        qmg.dwf_apply_direct(dt, d, dg, Ls, M, got, dx, pieces, W)
        h = got.to_host()
        assert np.all(np.isfinite(h)), (hex(pieces), "NaN prefill survived")
        ok, worst = within(h, want, S, n, f32)
        print("dwf direct %s Ls=%d %s pieces=%#x worst err/bound %.3f" % (dims, Ls, "c32" if f32 else "c64", pieces, worst))
        assert ok, (hex(pieces), worst)
        untouched = np.asarray(n == 0) & np.isfinite(start)
        assert np.array_equal(h[untouched], lhs0.astype(npt)[untouched]), hex(pieces)      # a parity no piece touches keeps its bits
        if stored is not None:
            gs = D(np.where(np.isfinite(start), start, 0).astype(npt))
            qmg.stencil_apply_t(dt, stored, gs, dx, pieces)
            ok, worst = within(gs.to_host(), want, S, n, f32)
            assert ok, (hex(pieces), "stored route", worst)


BATCH_CASES = [((2, 2), 3), ((4, 6), 6), ((130, 2), 12), ((16, 8), 8), ((16, 8), 32)]


@pytest.mark.parametrize("f32", [False, True], ids=["c64", "c32"])
@pytest.mark.parametrize("dims,Ls", BATCH_CASES, ids=IDS)
def test_batches_with_a_masked_system(dims, Ls, f32):
    Lx, Ly = dims
    nc = 2 * Ls
    n = Lx * Ly * nc
    stride = n + 4                                         # systems apart by more than a vector
    nrhs, mask = 3, 0b101
    dt, npt = (qmg.C32 if f32 else qmg.C64), np_dtype(f32)
    g = rounded(gauge(Lx, Ly), f32)
    xs, ls = rounded(cvec(nrhs * stride, 3), f32), rounded(cvec(nrhs * stride, 4), f32)
    d = qmg.make_desc(Lx, Ly, nc, None, None, *SHIFTS)
    dg, dx = D(g.astype(npt)), D(xs.astype(npt))
    for pieces in (P.P_ALL, P.P_HOPPING | P.P_ZERO):
        got = D(ls.astype(npt))
        qmg.dwf_apply_direct(dt, d, dg, Ls, M, got, dx, pieces, W, nrhs, stride, mask)
        h = got.to_host()
        for k in range(nrhs):
            sl = slice(k * stride, k * stride + n)
            if not (mask >> k) & 1:
                assert h[sl].tobytes() == ls.astype(npt)[sl].tobytes()              # the inactive system: byte-identical
                continue
            want, S, cnt = dn.apply(Lx, Ly, Ls, g, M, W, *SHIFTS, pieces, xs[sl], ls[sl])
            ok, worst = within(h[sl], want, S, cnt, f32)
            assert ok, (hex(pieces), k, worst)
        pad = np.ones(nrhs * stride, dtype=bool)
        for k in range(nrhs):
            pad[k * stride:k * stride + n] = False
        assert h[pad].tobytes() == ls.astype(npt)[pad].tobytes()                    # nothing between the vectors is written


@pytest.mark.parametrize("dims,Ls", BATCH_CASES, ids=IDS)
def test_hops_in_place(dims, Ls):
    """lhs == rhs: one parity written from the other by hops alone (the reference's aliased use, stencil_2d.h:1904)"""
    Lx, Ly = dims
    nc = 2 * Ls
    n = Lx * Ly * nc
    g, x = gauge(Lx, Ly), cvec(n, 5)
    d = qmg.make_desc(Lx, Ly, nc, None, None, *SHIFTS)
    for pieces, written in ((P.P_EO | P.P_ZERO_E, slice(0, n // 2)), (P.P_OE | P.P_ZERO_O, slice(n // 2, n))):
        v = D(x)
        qmg.dwf_apply_direct(qmg.C64, d, D(g), Ls, M, v, v, pieces, W)
        h = v.to_host()
        kept = np.ones(n, dtype=bool)
        kept[written] = False
        assert np.array_equal(h[kept], x[kept])
        want, S, cnt = dn.apply(Lx, Ly, Ls, g, M, W, *SHIFTS, pieces, x, x)
        ok, worst = within(h[written], want[written], S[written], cnt[written], False)
        assert ok, (hex(pieces), worst)


# ---- past the cap of grid.y: 65540 rows on 65535 blocks, so five blocks take a second row
# (name, family, lattice, pieces); kernel D walks (parity, y) rows, row = 2 y + parity on both parities and y on one; kernel D2 walks y
TALL = [("D-hops-zero", P.DF_DIRECT, (2, 32770), P.P_HOPPING | P.P_ZERO),
        ("D-hops", P.DF_DIRECT, (2, 32770), P.P_HOPPING),
        ("D-even", P.DF_DIRECT, (2, 65540), P.P_CLOVER_E | P.P_EO | P.P_SHIFT_E | P.P_ZERO_E),
        ("D2-zero", P.DF_PAIR, (2, 65540), P.P_ALL | P.P_ZERO),
        ("D2", P.DF_PAIR, (2, 65540), P.P_ALL)]
TALL_IDS = [c[0] for c in TALL]


def walked_second(plan, dims, pieces, per_site):
    """asserts from the plan that grid.y is capped below the row count, and returns the mask (over one vector of `per_site` numbers a site)
    of the rows a block reaches on its second trip: rows gy .. nrows - 1 of the kernel's own numbering, as (parity, y)"""
    Lx, Ly = dims
    family, gy = plan[0], plan[4]
    even, odd = bool(pieces & (P.P_CLOVER_E | P.P_EO)), bool(pieces & (P.P_CLOVER_O | P.P_OE))     # the parities written
    both = even and odd
    nrows = Ly if family == P.DF_PAIR or not both else 2 * Ly
    assert gy == 65535 < nrows == 65540, (plan, nrows)
    m = np.zeros((2, Ly, (Lx // 2) * per_site), dtype=bool)
    for row in range(gy, nrows):
        if family == P.DF_PAIR:
            m[:, row] = True
        elif both:
            m[row & 1, row >> 1] = True
        else:
            m[0 if even else 1, row] = True
    return m.ravel()


def held_to_the_twin(h, want, S, cnt, f32, second, tag):
    """the whole output and, on their own, the rows walked second: no NaN of the prefill left, and within the family's bound"""
    assert np.all(np.isfinite(h)), (tag, "NaN prefill survived", int(np.count_nonzero(~np.isfinite(h[second]))), "of them on the second trip")
    for name, sel in (("whole", slice(None)), ("second trip", second)):
        ok, worst = within(h[sel], np.asarray(want)[sel], np.asarray(S)[sel], np.asarray(cnt)[sel], f32)
        print("dwf tall %s %s: worst err/bound %.3f" % (tag, name, worst))
        assert ok, (tag, name, worst)


@pytest.mark.parametrize("f32", [False, True], ids=["c64", "c32"])
@pytest.mark.parametrize("Ls", [2, 3])
@pytest.mark.parametrize("name,family,dims,pieces", TALL, ids=TALL_IDS)
def test_apply_walks_more_rows_than_the_grid_has_blocks(name, family, dims, pieces, Ls, f32):
    Lx, Ly = dims
    nc = 2 * Ls
    dt, npt = (qmg.C32 if f32 else qmg.C64), np_dtype(f32)
    plan = qmg.dwf_plan(dt, dims, Ls, pieces)
    assert plan[0] == family, plan
    second = walked_second(plan, dims, pieces, nc)
    assert np.count_nonzero(second) == 5 * (Lx // 2) * nc * (2 if family == P.DF_PAIR else 1)
    g, rhs, lhs0 = case(dims, Ls, f32)
    want, S, cnt = reference(dims, Ls, f32, pieces)
    start = lhs0.copy()
    half = start.size // 2
    for p in (0, 1):
        if pieces & (P.P_ZERO_E << p):
            start[p * half:(p + 1) * half] = np.nan
    d = qmg.make_desc(Lx, Ly, nc, None, None, *SHIFTS)
    dg, dx = D(g.astype(npt)), D(rhs.astype(npt))
    runs = []
    for _ in range(2):
        got = D(start.astype(npt))
        qmg.dwf_apply_direct(dt, d, dg, Ls, M, got, dx, pieces, W)
        runs.append(got.to_host())
    h = runs[0]
    held_to_the_twin(h, want, S, cnt, f32, second, (name, Ls, "c32" if f32 else "c64"))
    untouched = np.asarray(cnt == 0) & np.isfinite(start)
    assert np.array_equal(h[untouched], lhs0.astype(npt)[untouched])
    assert runs[1].tobytes() == h.tobytes()                # a second run on the same inputs: the same bytes


@pytest.mark.parametrize("f32", [False, True], ids=["c64", "c32"])
@pytest.mark.parametrize("name,family,dims,pieces", [TALL[1], TALL[3]], ids=[TALL_IDS[1], TALL_IDS[3]])
def test_tall_batch_with_a_masked_system(name, family, dims, pieces, f32):
    """three systems, the middle one masked out, Ls = 3: the system loop runs inside the row loop, so the second row starts it again"""
    Lx, Ly = dims
    Ls, nc = 3, 6
    n = Lx * Ly * nc
    stride = n + 4
    nrhs, mask = 3, 0b101
    dt, npt = (qmg.C32 if f32 else qmg.C64), np_dtype(f32)
    plan = qmg.dwf_plan(dt, dims, Ls, pieces, 2)
    assert plan[0] == family and plan[5] & P.DPF_BATCH and plan[7] == 2, plan
    second = walked_second(plan, dims, pieces, nc)
    g = case(dims, Ls, f32)[0]
    xs, ls = rounded(cvec(nrhs * stride, 3), f32), rounded(cvec(nrhs * stride, 4), f32)
    start = ls.copy()
    if pieces & P.P_ZERO:
        for k in range(nrhs):
            if (mask >> k) & 1:
                start[k * stride:k * stride + n] = np.nan
    d = qmg.make_desc(Lx, Ly, nc, None, None, *SHIFTS)
    dg, dx = D(g.astype(npt)), D(xs.astype(npt))
    runs = []
    for _ in range(2):
        got = D(start.astype(npt))
        qmg.dwf_apply_direct(dt, d, dg, Ls, M, got, dx, pieces, W, nrhs, stride, mask)
        runs.append(got.to_host())
    h = runs[0]
    pad = np.ones(nrhs * stride, dtype=bool)
    for k in range(nrhs):
        sl = slice(k * stride, k * stride + n)
        if (mask >> k) & 1:
            pad[sl] = False
            want, S, cnt = dn.apply(Lx, Ly, Ls, g, M, W, *SHIFTS, pieces, xs[sl], ls[sl])
            held_to_the_twin(h[sl], want, S, cnt, f32, second, (name, "system", k, "c32" if f32 else "c64"))
    assert h[pad].tobytes() == ls.astype(npt)[pad].tobytes()        # the masked system and the padding: byte-identical
    assert runs[1].tobytes() == h.tobytes()


def test_refusals_leave_lhs_untouched():
    Lx, Ly, Ls = 16, 8, 8
    nc = 2 * Ls
    n = Lx * Ly * nc
    g, x, l0 = D(gauge(Lx, Ly)), D(cvec(17 * n, 6)), cvec(17 * n, 7)
    d = qmg.make_desc(Lx, Ly, nc, None, None, *SHIFTS)
    unsupported, invalid = 3, 1

    def refused(status, pieces=P.P_ALL | P.P_ZERO, desc=d, Ls=Ls, nrhs=1, stride=0, mask=1, dtype=qmg.C64, inplace=False):
        lhs = D(l0)
        rc = qmg.dwf_apply_direct_status(dtype, desc, g, Ls, M, x if inplace else lhs, x, pieces, W, nrhs, stride, mask)
        assert rc == status, (rc, status)
        assert lhs.to_host().tobytes() == l0.tobytes()

    refused(unsupported, P.P_EO_XP1 | P.P_ZERO_E)                         # a single direction: the stored stencil serves it
    refused(unsupported, P.P_CLOVER | P.P_ZERO)                           # clover without hops
    refused(invalid, desc=qmg.make_desc(Lx, Ly, nc + 2, None, None))      # nc != 2 Ls
    refused(invalid, desc=qmg.make_desc(Lx, Ly, 2, None, None), Ls=1)     # Ls = 1
    refused(invalid, desc=qmg.make_desc(Lx, Ly, 66, None, None), Ls=33)   # Ls = 33
    refused(invalid, nrhs=17, stride=n, mask=0x1FFFF)                     # nrhs = 17
    refused(invalid, nrhs=2, stride=n - 2, mask=3)                        # systems that overlap
    refused(invalid, dtype=2)
    refused(invalid, inplace=True)                                        # the full operator in place
    assert qmg.dwf_apply_direct_status(qmg.C64, d, g, Ls, M, D(l0), x, P.P_ALL | P.P_ZERO, W, 3, n, 0) == 0   # nothing active: success, nothing done


# ---- the facade, through its driver
def summation_ratio(L, Ls, mass):
    """|S| / |D x| for a Gaussian x: how much larger the term-magnitude sum is than the result it bounds"""
    g, x = gauge(L, L, 21), cvec(L * L * 2 * Ls, 22)
    want, S, n = dn.apply(L, L, Ls, g, mass, 1.0, -1.0, 0.0, 0.0, P.P_ALL | P.P_ZERO, x, np.zeros_like(x))
    return float(np.linalg.norm(S.astype(np.float64)) / np.linalg.norm(np.asarray(want).astype(np.complex128))), int(np.max(n))


@pytest.mark.parametrize("L,Ls", [(16, 8), (8, 6)])
def test_dwf_selftest_driver(L, Ls):
    exe = os.path.join(qmg.HERE, "drivers", "dwf_selftest")
    assert os.path.exists(exe), "drivers/dwf_selftest is not built"
    # (a) and (c) compare two fp64 routes that each sum the same n complex terms per element.  A complex term is two real products per
    # component, so by the standard summation bound each route is within sqrt(2) (2 n + 1) 2^-53 S of the exact result and the two differ
    # by at most 2 sqrt(2) (2 n + 1) 2^-53 |S| in l2; n and |S| / |D x| come from the grid formula: the bound stays below 1e-13
    ratio, nterms = summation_ratio(L, Ls, 0.05)
    assert nterms <= 14 and 2 * np.sqrt(2) * (2 * nterms + 1) * 2.0 ** -53 * ratio < 1e-13, (nterms, ratio)
    out = subprocess.run([exe, str(L), str(Ls), "0.05", "7"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    print(out.stdout)
    lines = {}
    for ln in out.stdout.splitlines():
        if ln.startswith("[QMG-DWF] "):
            _, name, value, verdict = ln.split()
            lines[name] = (float(value), verdict)
    assert out.returncode == 0, out.stdout
    expected = ("direct_route_on", "direct_vs_stored", "gamma5_hermiticity", "dagger_vs_gamma5", "cg_iterations", "cg_true_residual", "batch_iterations", "batch_residual")
    assert sorted(lines) == sorted(expected)
    assert all(v == "PASS" for _, v in lines.values()), lines
    assert lines["direct_vs_stored"][0] < 1e-13 and lines["dagger_vs_gamma5"][0] < 1e-13
    assert lines["gamma5_hermiticity"][0] < 1e-12
    assert lines["cg_true_residual"][0] <= 1e-9
    assert 0 < lines["cg_iterations"][0] < 1000          # condition number 32-85: a few hundred iterations at most
    assert lines["batch_iterations"][0] == 0
