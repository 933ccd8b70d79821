"""The even-odd domain-wall kernels on the GPU (csrc/qmg_dwf_eo.hip): qmg_dwf_inv5 (kernel I), qmg_dwf_hops_inv5 (kernel K) and
qmg_dwf_schur_apply (kernel K + the second stage), each against dwf_eo_numpy's long-double statement, whose A^-1 is a Gauss-Jordan inverse
and shares neither the closed form nor the index arithmetic of the kernels (tests/test_host_dwf_eo.py validates it without a GPU).

Lattices: (2, 2) every neighbour pair coincides; (4, 6) small general case; (130, 2) Lx/2 = 65 sites per half row and +-y coincide;
(16, 8) regular.  Ls: 2, 3, 6, 8, 12, 32 -- 3, 6, 12 do not divide the wavefront (sites straddle wavefronts, the block is 255 / 252 / 252
lanes and the last one is partial); at (130, 2) with Ls = 8, 12, 32 a half row takes more than one block.

Parameters: w = 0.9, m = 0.05 + 0.02i, shift = -1 + 0.03i, eo_shift = 0.011 - 0.02i (d_even != d_odd, both complex, |d| ~ 1.7).

Bounds: stencil_numpy.elementwise_bound on the S and n dwf_eo_numpy returns -- fp64: (n + 1) 2^-50 S; fp32 arithmetic: (n + 1) 2^-21 S +
2^-23 |want| on inputs rounded to complex64."""
import functools
import importlib
import os
import subprocess

import numpy as np
import pytest

import dwf_eo_numpy as de
import stencil_numpy as sn

qmg = importlib.import_module("quantum-mg_amd")
pytestmark = pytest.mark.gpu
D = qmg.DeviceArray.from_host
P = qmg

LATTICES = [(2, 2), (4, 6), (130, 2), (16, 8)]
LS_ALL = [2, 3, 6, 8, 12, 32]
M, W = 0.05 + 0.02j, 0.9
SHIFT, EO_SHIFT = -1.0 + 0.03j, 0.011 - 0.02j
ALPHA = 0.7 - 0.4j
IDS = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)
PREC = pytest.mark.parametrize("f32", [False, True], ids=["c64", "c32"])
UNSUPPORTED, INVALID = 3, 1


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
    """the inputs of one (lattice, Ls, precision) as the kernel sees them, computed once: links, rhs, lhs0, tmp0"""
    Lx, Ly = dims
    n = Lx * Ly * 2 * Ls
    return rounded(gauge(Lx, Ly), f32), rounded(cvec(n, 1), f32), rounded(cvec(n, 2), f32), rounded(cvec(n, 3), f32)


def desc(dims, Ls, shift=SHIFT, eo_shift=EO_SHIFT, dof_shift=0.0):
    return qmg.make_desc(dims[0], dims[1], 2 * Ls, None, None, shift, eo_shift, dof_shift)


def within(got, want, S, n, f32):
    err = np.abs(got.astype(sn.CLD) - want)
    bound = sn.elementwise_bound(S, n, want, fp32_arithmetic=True) if f32 else sn.elementwise_bound(S, n)
    worst = float(np.max(err / np.where(bound > 0, bound, 1)))
    return bool(np.all(err <= bound)), worst


def types(f32):
    return (qmg.C32, np.complex64) if f32 else (qmg.C64, np.complex128)


def halves(n):
    return slice(0, n // 2), slice(n // 2, n)


def prefill(lhs0, overwritten):
    """lhs0 with NaN in the halves that are overwritten: what ZERO clears is never read"""
    start = lhs0.copy()
    for p in overwritten:
        start[halves(start.size)[p]] = np.nan
    return start


# ---- kernel I
@PREC
@pytest.mark.parametrize("dims", LATTICES, ids=IDS)
@pytest.mark.parametrize("Ls", LS_ALL)
def test_inv5_against_the_gauss_jordan_inverse(dims, Ls, f32):
    Lx, Ly = dims
    dt, npt = types(f32)
    g, rhs, lhs0, _ = case(dims, Ls, f32)
    d, dx = desc(dims, Ls), D(rhs.astype(npt))
    for pieces, named in ((P.P_CLOVER_E, [0]), (P.P_CLOVER_O, [1]), (P.P_CLOVER, [0, 1])):
        want, S, n = de.inv5(Lx, Ly, Ls, M, W, SHIFT, EO_SHIFT, pieces, ALPHA, rhs, lhs0)
        start = prefill(lhs0, named)
        got = D(start.astype(npt))
        qmg.dwf_inv5(dt, d, Ls, M, got, dx, pieces, ALPHA, W)
        h = got.to_host()
        assert np.all(np.isfinite(h)), (hex(pieces), "NaN prefill survived")
        ok, worst = within(h, want, S, n, f32)
        print("dwf inv5 %s Ls=%d %s pieces=%#x worst err/bound %.3f" % (dims, Ls, "c32" if f32 else "c64", pieces, worst))
        assert ok, (hex(pieces), worst)
        for p in (0, 1):
            if p not in named:
                assert h[halves(h.size)[p]].tobytes() == lhs0.astype(npt)[halves(h.size)[p]].tobytes(), hex(pieces)
    # in place
    v = D(rhs.astype(npt))
    qmg.dwf_inv5(dt, d, Ls, M, v, v, P.P_CLOVER, ALPHA, W)
    ok, worst = within(v.to_host(), want, S, n, f32)
    assert ok, ("in place", worst)


# ---- kernel K
K_PIECES = [P.P_EO | P.P_ZERO_E, P.P_EO, P.P_OE | P.P_ZERO_O, P.P_OE, P.P_HOPPING | P.P_ZERO, P.P_HOPPING, P.P_HOPPING | P.P_ZERO_E]


@PREC
@pytest.mark.parametrize("dims", LATTICES, ids=IDS)
@pytest.mark.parametrize("Ls", LS_ALL)
def test_hops_inv5_against_the_grid_formula(dims, Ls, f32):
    Lx, Ly = dims
    dt, npt = types(f32)
    g, rhs, lhs0, _ = case(dims, Ls, f32)
    d, dg, dx = desc(dims, Ls), D(g.astype(npt)), D(rhs.astype(npt))
    for pieces in K_PIECES:
        for flags in (0, qmg.DWF_G5_IN):
            want, S, n = de.hops_inv5(Lx, Ly, Ls, g, M, W, SHIFT, EO_SHIFT, pieces, ALPHA, flags, rhs, lhs0)
            start = prefill(lhs0, [p for p in (0, 1) if pieces & (P.P_ZERO_E << p)])
            got = D(start.astype(npt))
            qmg.dwf_hops_inv5(dt, d, dg, Ls, M, got, dx, pieces, ALPHA, flags, W)
            h = got.to_host()
            assert np.all(np.isfinite(h)), (hex(pieces), flags, "NaN prefill survived")
            ok, worst = within(h, want, S, n, f32)
            print("dwf hops_inv5 %s Ls=%d %s pieces=%#x flags=%d worst err/bound %.3f" % (dims, Ls, "c32" if f32 else "c64", pieces, flags, worst))
            assert ok, (hex(pieces), flags, worst)
            untouched = np.asarray(n == 0)
            assert h[untouched].tobytes() == lhs0.astype(npt)[untouched].tobytes(), hex(pieces)      # a parity no piece touches keeps its bits


@pytest.mark.parametrize("dims,Ls", [((2, 2), 3), ((4, 6), 6), ((130, 2), 12), ((16, 8), 8), ((16, 8), 32)], ids=IDS)
def test_hops_inv5_in_place(dims, Ls):
    """lhs == rhs: one parity written from the other"""
    Lx, Ly = dims
    g, x, _, _ = case(dims, Ls, False)
    n = x.size
    for pieces, p in ((P.P_EO | P.P_ZERO_E, 0), (P.P_OE | P.P_ZERO_O, 1)):
        v = D(x)
        qmg.dwf_hops_inv5(qmg.C64, desc(dims, Ls), D(g), Ls, M, v, v, pieces, ALPHA, qmg.DWF_G5_IN, W)
        h = v.to_host()
        written, kept = halves(n)[p], halves(n)[1 - p]
        assert h[kept].tobytes() == x[kept].tobytes()
        want, S, cnt = de.hops_inv5(Lx, Ly, Ls, g, M, W, SHIFT, EO_SHIFT, pieces, ALPHA, qmg.DWF_G5_IN, x, x)
        ok, worst = within(h[written], want[written], S[written], cnt[written], False)
        assert ok, (hex(pieces), worst)


# ---- the Schur complement
@PREC
@pytest.mark.parametrize("dims", LATTICES, ids=IDS)
@pytest.mark.parametrize("Ls", LS_ALL)
def test_schur_apply_with_the_gamma5_flags(dims, Ls, f32):
    Lx, Ly = dims
    dt, npt = types(f32)
    g, rhs, lhs0, tmp0 = case(dims, Ls, f32)
    n = rhs.size
    d, dg, dx = desc(dims, Ls), D(g.astype(npt)), D(rhs.astype(npt))
    for parity in (0, 1):
        for flags in (0, qmg.DWF_G5_IN, qmg.DWF_G5_OUT, qmg.DWF_G5_IN | qmg.DWF_G5_OUT):
            want, S, cnt, wt, St, nt = de.schur(Lx, Ly, Ls, g, M, W, SHIFT, EO_SHIFT, parity, flags, rhs, lhs0, tmp0)
            got, tmp = D(prefill(lhs0, [parity]).astype(npt)), D(prefill(tmp0, [1 - parity]).astype(npt))
            qmg.dwf_schur_apply(dt, d, dg, Ls, M, got, dx, tmp, parity, flags, W)
            h, t = got.to_host(), tmp.to_host()
            assert np.all(np.isfinite(h)) and np.all(np.isfinite(t)), (parity, flags, "NaN prefill survived")
            ok, worst = within(h, want, S, cnt, f32)
            okt, worst_t = within(t, wt, St, nt, f32)
            print("dwf schur %s Ls=%d %s parity=%d flags=%d worst err/bound %.3f (tmp %.3f)" % (dims, Ls, "c32" if f32 else "c64", parity, flags, worst, worst_t))
            assert ok and okt, (parity, flags, worst, worst_t)
            p_half, o_half = halves(n)[parity], halves(n)[1 - parity]
            assert h[o_half].tobytes() == lhs0.astype(npt)[o_half].tobytes()       # the 1-p half of lhs
            assert t[p_half].tobytes() == tmp0.astype(npt)[p_half].tobytes()       # the p half of tmp
            assert dx.to_host().tobytes() == rhs.astype(npt).tobytes()             # rhs, both halves


# ---- batches
@PREC
@pytest.mark.parametrize("dims,Ls", [((2, 2), 3), ((4, 6), 6), ((130, 2), 12), ((16, 8), 8), ((16, 8), 32)], ids=IDS)
def test_batches_with_a_masked_system(dims, Ls, f32):
    Lx, Ly = dims
    n = Lx * Ly * 2 * Ls
    stride = n + 4                                         # systems apart by more than a vector
    nrhs, mask = 3, 0b101
    dt, npt = types(f32)
    g = rounded(gauge(Lx, Ly), f32)
    xs, ls, ts = (rounded(cvec(nrhs * stride, s), f32) for s in (3, 4, 5))
    d, dg, dx = desc(dims, Ls), D(g.astype(npt)), D(xs.astype(npt))
    sl = lambda k: slice(k * stride, k * stride + n)
    pad = np.ones(nrhs * stride, dtype=bool)
    for k in range(nrhs):
        pad[sl(k)] = False

    def check(h, start, ref, what):
        for k in range(nrhs):
            if not (mask >> k) & 1:
                assert h[sl(k)].tobytes() == start.astype(npt)[sl(k)].tobytes(), what       # the inactive system: byte-identical
                continue
            want, S, cnt = ref(k)
            ok, worst = within(h[sl(k)], want, S, cnt, f32)
            assert ok, (what, k, worst)
        assert h[pad].tobytes() == start.astype(npt)[pad].tobytes(), what                   # nothing between the vectors is written

    got = D(ls.astype(npt))
    qmg.dwf_inv5(dt, d, Ls, M, got, dx, P.P_CLOVER, ALPHA, W, nrhs, stride, mask)
    check(got.to_host(), ls, lambda k: de.inv5(Lx, Ly, Ls, M, W, SHIFT, EO_SHIFT, P.P_CLOVER, ALPHA, xs[sl(k)], ls[sl(k)]), "inv5")
    for pieces in (P.P_HOPPING, P.P_OE | P.P_ZERO_O):
        got = D(ls.astype(npt))
        qmg.dwf_hops_inv5(dt, d, dg, Ls, M, got, dx, pieces, ALPHA, qmg.DWF_G5_IN, W, nrhs, stride, mask)
        check(got.to_host(), ls, lambda k: de.hops_inv5(Lx, Ly, Ls, g, M, W, SHIFT, EO_SHIFT, pieces, ALPHA, qmg.DWF_G5_IN, xs[sl(k)], ls[sl(k)]), hex(pieces))
    got, tmp = D(ls.astype(npt)), D(ts.astype(npt))
    flags = qmg.DWF_G5_IN | qmg.DWF_G5_OUT
    qmg.dwf_schur_apply(dt, d, dg, Ls, M, got, dx, tmp, 1, flags, W, nrhs, stride, mask)
    ref = functools.lru_cache(maxsize=None)(lambda k: de.schur(Lx, Ly, Ls, g, M, W, SHIFT, EO_SHIFT, 1, flags, xs[sl(k)], ls[sl(k)], ts[sl(k)]))
    check(got.to_host(), ls, lambda k: ref(k)[:3], "schur lhs")
    check(tmp.to_host(), ts, lambda k: ref(k)[3:], "schur tmp")


# ---- past the cap of grid.y: 65540 rows on 65535 blocks, so five blocks take a second row (kernels K and I through the other LDS buffer
# when the number of active systems is odd)
TALL2, TALL1 = (2, 32770), (2, 65540)          # rows = (parity, y), row = 2 y + parity; rows = y of one parity
LS_TALL = [2, 3]                               # at Ls = 3 the block is 255 lanes


def walked_second(plan, dims, Ls, parity=None):
    """asserts from the plan that grid.y is capped below the row count, and returns the mask over one vector of the rows a block reaches on
    its second trip: rows gy .. nrows - 1 of the kernel's own numbering, as (parity, y).  parity: the one processed, None for both"""
    Lx, Ly = dims
    gy, nrows = plan[4], Ly * (2 if parity is None else 1)
    assert gy == 65535 < nrows == 65540, (plan, nrows)
    m = np.zeros((2, Ly, (Lx // 2) * 2 * Ls), dtype=bool)
    for row in range(gy, nrows):
        if parity is None:
            m[row & 1, row >> 1] = True
        else:
            m[parity, row] = True
    return m.ravel()


def held_to_the_twin(h, want, S, cnt, f32, second, tag):
    """the whole output and, on their own, the rows walked second: no NaN of the prefill left, and within the family's bound"""
    assert np.all(np.isfinite(h)), (tag, "NaN prefill survived", int(np.count_nonzero(~np.isfinite(h[second]))), "of them on the second trip")
    for name, sel in (("whole", slice(None)), ("second trip", second)):
        ok, worst = within(h[sel], np.asarray(want)[sel], np.asarray(S)[sel], np.asarray(cnt)[sel], f32)
        print("dwf eo tall %s %s: worst err/bound %.3f" % (tag, name, worst))
        assert ok, (tag, name, worst)


def twice(launch, start, npt):
    """the host copies of two runs from the same start"""
    out = []
    for _ in range(2):
        got = D(start.astype(npt))
        launch(got)
        out.append(got.to_host())
    return out


@PREC
@pytest.mark.parametrize("Ls", LS_TALL)
@pytest.mark.parametrize("pieces", [P.P_HOPPING | P.P_ZERO, P.P_HOPPING], ids=["zero", "add"])
def test_hops_inv5_walks_more_rows_than_the_grid_has_blocks(pieces, Ls, f32):
    dims = TALL2
    dt, npt = types(f32)
    plan = qmg.dwf_eo_plan(dt, dims, Ls, qmg.DEK_HOPS_INV5, pieces)
    assert plan[0] == qmg.DEF_HOPS_INV5 and plan[2] == Ls * (256 // Ls), plan
    second = walked_second(plan, dims, Ls)
    g, rhs, lhs0, _ = case(dims, Ls, f32)
    d, dg, dx = desc(dims, Ls), D(g.astype(npt)), D(rhs.astype(npt))
    want, S, n = de.hops_inv5(*dims, Ls, g, M, W, SHIFT, EO_SHIFT, pieces, ALPHA, qmg.DWF_G5_IN, rhs, lhs0)
    start = prefill(lhs0, [0, 1] if pieces & P.P_ZERO else [])
    h, again = twice(lambda got: qmg.dwf_hops_inv5(dt, d, dg, Ls, M, got, dx, pieces, ALPHA, qmg.DWF_G5_IN, W), start, npt)
    held_to_the_twin(h, want, S, n, f32, second, ("K", hex(pieces), Ls, f32))
    assert again.tobytes() == h.tobytes()                  # a second run on the same inputs: the same bytes


@PREC
@pytest.mark.parametrize("Ls", LS_TALL)
def test_inv5_walks_more_rows_than_the_grid_has_blocks(Ls, f32):
    dims = TALL2
    dt, npt = types(f32)
    plan = qmg.dwf_eo_plan(dt, dims, Ls, qmg.DEK_INV5, P.P_CLOVER)
    assert plan[0] == qmg.DEF_INV5 and plan[2] == Ls * (256 // Ls), plan
    second = walked_second(plan, dims, Ls)
    g, rhs, lhs0, _ = case(dims, Ls, f32)
    d, dx = desc(dims, Ls), D(rhs.astype(npt))
    want, S, n = de.inv5(*dims, Ls, M, W, SHIFT, EO_SHIFT, P.P_CLOVER, ALPHA, rhs, lhs0)
    h, again = twice(lambda got: qmg.dwf_inv5(dt, d, Ls, M, got, dx, P.P_CLOVER, ALPHA, W), prefill(lhs0, [0, 1]), npt)
    held_to_the_twin(h, want, S, n, f32, second, ("I", Ls, f32))
    assert again.tobytes() == h.tobytes()


@PREC
@pytest.mark.parametrize("Ls", LS_TALL)
@pytest.mark.parametrize("flags", [0, qmg.DWF_G5_IN, qmg.DWF_G5_OUT, qmg.DWF_G5_IN | qmg.DWF_G5_OUT])
def test_schur_apply_walks_more_rows_than_the_grid_has_blocks(flags, Ls, f32):
    """one parity of 2 x 65540: kernel K writes tmp on the other parity and the second stage lhs on this one, each over 65540 rows"""
    dims, parity = TALL1, 1
    dt, npt = types(f32)
    one = P.P_CLOVER_O | P.P_OE | P.P_SHIFT_O | P.P_ZERO_O
    plan1, plan2 = qmg.dwf_eo_plan(dt, dims, Ls, qmg.DEK_HOPS_INV5, P.P_EO | P.P_ZERO_E), qmg.dwf_eo_plan(dt, dims, Ls, qmg.DEK_SCHUR2, one)
    assert plan1[0] == qmg.DEF_HOPS_INV5 and plan2[0] == qmg.DEF_SCHUR2, (plan1, plan2)
    second_t, second = walked_second(plan1, dims, Ls, 1 - parity), walked_second(plan2, dims, Ls, parity)
    g, rhs, lhs0, tmp0 = case(dims, Ls, f32)
    n = rhs.size
    d, dg, dx = desc(dims, Ls), D(g.astype(npt)), D(rhs.astype(npt))
    want, S, cnt, wt, St, nt = de.schur(*dims, Ls, g, M, W, SHIFT, EO_SHIFT, parity, flags, rhs, lhs0, tmp0)
    runs = []
    for _ in range(2):
        got, tmp = D(prefill(lhs0, [parity]).astype(npt)), D(prefill(tmp0, [1 - parity]).astype(npt))
        qmg.dwf_schur_apply(dt, d, dg, Ls, M, got, dx, tmp, parity, flags, W)
        runs.append((got.to_host(), tmp.to_host()))
    h, t = runs[0]
    held_to_the_twin(t, wt, St, nt, f32, second_t, ("schur tmp", flags, Ls, f32))
    held_to_the_twin(h, want, S, cnt, f32, second, ("schur lhs", flags, Ls, f32))
    p_half, o_half = halves(n)[parity], halves(n)[1 - parity]
    assert h[o_half].tobytes() == lhs0.astype(npt)[o_half].tobytes() and t[p_half].tobytes() == tmp0.astype(npt)[p_half].tobytes()
    assert runs[1][0].tobytes() == h.tobytes() and runs[1][1].tobytes() == t.tobytes()


TALL_STRIDE = TALL2[0] * TALL2[1] * 6 + 4


@functools.lru_cache(maxsize=None)
def tall_batch(f32):
    """four systems of 2 x 32770 at Ls = 3, apart by more than a vector: links, rhs, lhs0"""
    return (case(TALL2, 3, f32)[0],) + tuple(rounded(cvec(4 * TALL_STRIDE, s), f32) for s in (3, 4))


@functools.lru_cache(maxsize=None)
def tall_batch_reference(kernel, f32, k):
    g, xs, ls = tall_batch(f32)
    sl = slice(k * TALL_STRIDE, k * TALL_STRIDE + TALL_STRIDE - 4)
    if kernel == "I":
        return de.inv5(*TALL2, 3, M, W, SHIFT, EO_SHIFT, P.P_CLOVER, ALPHA, xs[sl], ls[sl])
    return de.hops_inv5(*TALL2, 3, g, M, W, SHIFT, EO_SHIFT, P.P_HOPPING | P.P_ZERO, ALPHA, qmg.DWF_G5_IN, xs[sl], ls[sl])


@PREC
@pytest.mark.parametrize("nrhs,mask", [(4, 0b1101), (3, 0b101)], ids=["3of4", "2of3"])
@pytest.mark.parametrize("kernel", ["K", "I"])
def test_tall_batches_with_an_odd_and_an_even_number_of_active_systems(kernel, nrhs, mask, f32):
    """the LDS buffer flips once per system: with three active systems a block starts its second row on the other buffer than its first,
    with two on the same one"""
    dims, Ls, stride = TALL2, 3, TALL_STRIDE
    n = stride - 4
    dt, npt = types(f32)
    active = [k for k in range(nrhs) if (mask >> k) & 1]
    pieces = P.P_CLOVER if kernel == "I" else P.P_HOPPING | P.P_ZERO
    plan = qmg.dwf_eo_plan(dt, dims, Ls, qmg.DEK_INV5 if kernel == "I" else qmg.DEK_HOPS_INV5, pieces, len(active))
    assert plan[0] == (qmg.DEF_INV5 if kernel == "I" else qmg.DEF_HOPS_INV5) and plan[7] == len(active) and plan[2] == 255, plan
    second = walked_second(plan, dims, Ls)
    g, xs, ls = tall_batch(f32)
    xs, ls = xs[:nrhs * stride], ls[:nrhs * stride]
    start = ls.copy()
    pad = np.ones(nrhs * stride, dtype=bool)
    for k in active:
        start[k * stride:k * stride + n] = np.nan
        pad[k * stride:k * stride + n] = False
    d, dg, dx = desc(dims, Ls), D(g.astype(npt)), D(xs.astype(npt))
    if kernel == "I":
        launch = lambda got: qmg.dwf_inv5(dt, d, Ls, M, got, dx, pieces, ALPHA, W, nrhs, stride, mask)
    else:
        launch = lambda got: qmg.dwf_hops_inv5(dt, d, dg, Ls, M, got, dx, pieces, ALPHA, qmg.DWF_G5_IN, W, nrhs, stride, mask)
    h, again = twice(launch, start, npt)
    for k in active:
        want, S, cnt = tall_batch_reference(kernel, f32, k)
        held_to_the_twin(h[k * stride:k * stride + n], want, S, cnt, f32, second, (kernel, "system", k, "of", nrhs, f32))
    assert h[pad].tobytes() == ls.astype(npt)[pad].tobytes()        # the masked system and the padding: byte-identical
    assert again.tobytes() == h.tobytes()


# ---- refusals
def test_refusals_leave_lhs_untouched():
    dims, Ls = (16, 8), 8
    n = dims[0] * dims[1] * 2 * Ls
    g, x, t, l0 = D(gauge(*dims)), D(cvec(17 * n, 6)), D(cvec(17 * n, 8)), cvec(17 * n, 7)
    d = desc(dims, Ls)
    inf, nan = float("inf"), float("nan")

    def refused(status, entry="hops", pieces=None, desc_=d, Ls=Ls, nrhs=1, stride=0, mask=1, dtype=qmg.C64, inplace=False, alpha=ALPHA, flags=0, m=M, w=W, parity=0,
                alias=None):
        lhs = D(l0)
        target = x if inplace else lhs
        if entry == "inv5":
            rc = qmg.dwf_inv5_status(dtype, desc_, Ls, m, target, x, P.P_CLOVER if pieces is None else pieces, alpha, w, nrhs, stride, mask)
        elif entry == "hops":
            rc = qmg.dwf_hops_inv5_status(dtype, desc_, g, Ls, m, target, x, P.P_HOPPING | P.P_ZERO if pieces is None else pieces, alpha, flags, w, nrhs, stride, mask)
        else:
            tmp = {None: t, "tmp=rhs": x, "tmp=lhs": lhs}[alias]
            rc = qmg.dwf_schur_apply_status(dtype, desc_, g, Ls, m, target, x, tmp, parity, flags, w, nrhs, stride, mask)
        assert rc == status, (entry, rc, status)
        assert lhs.to_host().tobytes() == l0.tobytes()

    for entry in ("inv5", "hops", "schur"):
        # the coefficient refusals common to all entries
        refused(UNSUPPORTED, entry, desc_=desc(dims, Ls, dof_shift=0.023 + 0.01j))                      # dof_shift != 0
        refused(UNSUPPORTED, entry, desc_=desc(dims, Ls, shift=-2.2, eo_shift=0.0), w=1.0)              # |d| = 0.8 <= 1
        refused(UNSUPPORTED, entry, desc_=desc(dims, Ls, shift=-2.0, eo_shift=0.0), w=1.0)              # |d| = 1
        refused(INVALID, entry, desc_=desc(dims, 2, shift=-1.0, eo_shift=0.0), Ls=2, m=-4.0, w=1.0)     # d = 2: 1 + m d^-2 == 0
        refused(INVALID, entry, m=complex(nan, 0.0))
        refused(INVALID, entry, w=inf)
        refused(INVALID, entry, desc_=desc(dims, Ls, shift=complex(-1.0, inf)))
        # qmg_dwf_apply_direct's validity rules
        refused(INVALID, entry, desc_=qmg.make_desc(16, 8, 2 * Ls + 2, None, None, SHIFT, EO_SHIFT))    # nc != 2 Ls
        refused(INVALID, entry, desc_=qmg.make_desc(16, 8, 2, None, None, SHIFT, EO_SHIFT), Ls=1)
        refused(INVALID, entry, desc_=qmg.make_desc(16, 8, 66, None, None, SHIFT, EO_SHIFT), Ls=33)
        refused(INVALID, entry, nrhs=17, stride=n, mask=0x1FFFF)
        refused(INVALID, entry, nrhs=2, stride=n - 2, mask=3)                                           # systems that overlap
        refused(INVALID, entry, dtype=2)
    # |d| <= 1 on a parity that is neither processed nor inverted does not refuse kernels I and K ... (d_even = 2.5, d_odd = 0.5)
    lopsided = desc(dims, Ls, shift=-1.5, eo_shift=1.0)
    assert qmg.dwf_inv5_status(qmg.C64, lopsided, Ls, M, D(l0), x, P.P_CLOVER_E, ALPHA, 1.0) == 0
    assert qmg.dwf_hops_inv5_status(qmg.C64, lopsided, g, Ls, M, D(l0), x, P.P_EO, ALPHA, 0, 1.0) == 0
    refused(UNSUPPORTED, "inv5", pieces=P.P_CLOVER_O, desc_=lopsided, w=1.0)
    refused(UNSUPPORTED, "hops", pieces=P.P_OE, desc_=lopsided, w=1.0)
    refused(UNSUPPORTED, "schur", desc_=lopsided, w=1.0)                                                # ... the Schur complement uses both
    refused(UNSUPPORTED, "schur", desc_=lopsided, w=1.0, parity=1)
    # the piece sets
    refused(UNSUPPORTED, "inv5", pieces=P.P_CLOVER | P.P_SHIFT)
    refused(UNSUPPORTED, "inv5", pieces=P.P_EO)
    refused(UNSUPPORTED, "hops", pieces=P.P_EO | P.P_CLOVER_E | P.P_ZERO_E)                             # a clover bit
    refused(UNSUPPORTED, "hops", pieces=P.P_OE | P.P_SHIFT_O)                                           # a shift bit
    refused(UNSUPPORTED, "hops", pieces=P.P_EO_XP1 | P.P_ZERO_E)                                        # a partial hop set
    refused(UNSUPPORTED, "hops", pieces=P.P_HOPPING & ~(P.P_OE_XP1 << 3))
    refused(INVALID, "hops", inplace=True)                                                              # both parities in place
    refused(INVALID, "hops", flags=qmg.DWF_G5_OUT)                                                      # kernel K has no store flag
    refused(INVALID, "hops", alpha=complex(0.0, nan))
    refused(INVALID, "inv5", alpha=complex(inf, 0.0))
    refused(INVALID, "schur", inplace=True)
    refused(INVALID, "schur", alias="tmp=rhs")
    refused(INVALID, "schur", alias="tmp=lhs")
    refused(INVALID, "schur", parity=2)
    refused(INVALID, "schur", flags=4)
    # nothing active: success, nothing done
    lhs = D(l0)
    assert qmg.dwf_hops_inv5_status(qmg.C64, d, g, Ls, M, lhs, x, P.P_HOPPING | P.P_ZERO, ALPHA, 0, W, 3, n, 0) == 0
    assert qmg.dwf_inv5_status(qmg.C64, d, Ls, M, lhs, x, 0, ALPHA, W) == 0
    assert lhs.to_host().tobytes() == l0.tobytes()


# ---- the facade, through its driver
@pytest.mark.parametrize("L,Ls", [(16, 8), (8, 6), (8, 32)])
def test_dwf_eo_selftest_driver(L, Ls):
    exe = os.path.join(qmg.HERE, "drivers", "dwf_eo_selftest")
    assert os.path.exists(exe), "drivers/dwf_eo_selftest is not built"
    out = subprocess.run([exe, str(L), str(Ls), "0.05", "7"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    print(out.stdout)
    lines = {}
    for ln in out.stdout.splitlines():
        if ln.startswith("[QMG-DWF-EO] "):
            _, name, value, verdict = ln.split()
            lines[name] = (float(value), verdict)
    assert out.returncode == 0, out.stdout
    stored = Ls < 32                     # the parent's solver needs the stored nc = 2 Ls apply: not at Ls = 32
    expected = ["direct_route_on", "schur_vs_D_odd", "schur_vs_D", "schur_gamma5_hermiticity", "eo_iterations", "eo_true_residual"]
    if stored:
        expected += ["full_iterations", "full_true_residual", "eo_vs_full_solution"]
    assert sorted(lines) == sorted(expected)
    assert all(v == "PASS" for _, v in lines.values()), lines
    assert lines["schur_vs_D_odd"][0] < 1e-13 and lines["schur_vs_D"][0] < 1e-13
    assert lines["schur_gamma5_hermiticity"][0] < 1e-12
    assert lines["eo_true_residual"][0] <= 1e-8
    if stored:
        assert 0 < lines["eo_iterations"][0] < lines["full_iterations"][0]
        assert lines["eo_vs_full_solution"][0] <= 1e-7
