"""The Moebius domain-wall operator on the GPU (csrc/qmg_mobius.hip): the stored-stencil fill and the applies of D (op 0) and D^dagger (op 1)
straight from the gauge links, each against mobius_numpy's grid statements, which share no index arithmetic with the kernels
(tests/test_host_mobius.py validates them without a GPU).

Lattices: (2, 2) every neighbour is the same site through the wrap; (4, 6) small general case; (130, 2) Lx/2 = 65 lanes and +-y coincide;
(16, 8) regular.  Ls: 2, 3, 6, 8, 12 (3, 6, 12 do not divide the wavefront: sites straddle wavefronts and the last block is partial), and 32
for the links entry alone (nc = 64 is beyond the stored-stencil apply).

Bounds: stencil_numpy.elementwise_bound on the term-magnitude sum S and term count n that mobius_numpy returns -- fp64: (n + 1) 2^-50 S;
fp32 arithmetic: (n + 1) 2^-21 S + 2^-23 |want|, against the grid formula on the inputs as the kernel sees them (rounded to complex<float>)."""
import functools
import importlib
import math
import os
import subprocess

import numpy as np
import pytest

import dwf_numpy as dn
import mobius_numpy as mn
import stencil_numpy as sn
import stream_gate as sg

qmg = importlib.import_module("quantum-mg_amd")
pytestmark = pytest.mark.gpu
D = qmg.DeviceArray.from_host
P = qmg

LATTICES = [(2, 2), (4, 6), (130, 2), (16, 8)]
LS_STORED = [2, 3, 6, 8, 12]
M, M5 = 0.05 + 0.02j, -0.8
SHIFTS = (-0.2 + 0.03j, 0.011 - 0.02j, 0.023 + 0.01j)     # shift, eo_shift, dof_shift: all three nonzero
# (b5, c5, w): the Moebius pairs of the issue, both Wilson coefficients
PARAMS = [(1.5, 0.5, 1.0), (2.0, 1.0, 0.9), (1.0, 0.0, 0.9)]
OPS = [qmg.MOP_D, qmg.MOP_DAGGER]
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


def np_dtype(f32):
    return np.complex64 if f32 else np.complex128


@functools.lru_cache(maxsize=None)
def case(dims, Ls, f32):
    """the inputs of one (lattice, Ls, precision) as the kernel sees them, computed once"""
    Lx, Ly = dims
    n = Lx * Ly * 2 * Ls
    return rounded(gauge(Lx, Ly), f32), rounded(cvec(n, 1), f32), rounded(cvec(n, 2), f32)


@functools.lru_cache(maxsize=None)
def reference(dims, Ls, f32, b5, c5, w, op, pieces, shifts=SHIFTS, m=M):
    g, rhs, lhs0 = case(dims, Ls, f32)
    return mn.apply(dims[0], dims[1], Ls, g, m, w, M5, b5, c5, *shifts, pieces, rhs, lhs0, dagger=bool(op))


def bound_of(want, S, n, f32):
    return sn.elementwise_bound(S, n, want, fp32_arithmetic=True) if f32 else sn.elementwise_bound(S, n)


def within(got, want, S, n, f32):
    err = np.abs(got.astype(sn.CLD) - want)
    bound = bound_of(want, S, n, f32)
    worst = float(np.max(err / np.where(bound > 0, bound, 1)))
    return bool(np.all(err <= bound)), worst


def nan_prefill(lhs0, pieces):
    """what ZERO clears is never read: NaN there"""
    start = lhs0.copy()
    half = start.size // 2
    for p in (0, 1):
        if pieces & (P.P_ZERO_E << p):
            start[p * half:(p + 1) * half] = np.nan
    return start


# ---- the fill
@pytest.mark.parametrize("dims", LATTICES, ids=IDS)
@pytest.mark.parametrize("Ls", LS_STORED)
def test_fill_equals_the_numpy_fields(dims, Ls):
    """Both sides give every entry as its exact value rounded once (the kernel in double-double, the twin in long double and, for the wall
    entries of the hopping field, in rational arithmetic).  At w = 1, real m, M5 = -1 and (b5, c5) = (1.5, 0.5) the coefficients alpha = 2.5,
    kappa = -0.5, -m kappa and -m c5 are exact and an entry is one product of two doubles or an exact one: bit for bit.  (1.5 U itself is not
    exact in fp64 -- it is one correctly rounded product on both sides.)  Otherwise alpha, kappa and w/2 U are rounded on the way: 1 ulp."""
    Lx, Ly = dims
    nc2 = 4 * Ls * Ls
    g = gauge(Lx, Ly)
    dg = D(g)
    cl, hp = qmg.DeviceArray(Lx * Ly * nc2), qmg.DeviceArray(4 * Lx * Ly * nc2)
    qmg.mobius_fill(cl, hp, dg, Lx, Ly, Ls, 0.05, 1.0, -1.0, 1.5, 0.5)
    wc, wh = mn.fields(Lx, Ly, Ls, g, 0.05, 1.0, -1.0, 1.5, 0.5)
    assert np.array_equal(cl.to_host(), wc) and np.array_equal(hp.to_host(), wh)
    for b5, c5, w in PARAMS:
        qmg.mobius_fill(cl, hp, dg, Lx, Ly, Ls, M, w, M5, b5, c5)
        wc, wh = mn.fields(Lx, Ly, Ls, g, M, w, M5, b5, c5)
        for got, want in ((cl.to_host(), wc), (hp.to_host(), wh)):
            for part in (np.real, np.imag):
                assert np.all(np.abs(part(got) - part(want)) <= np.spacing(np.abs(part(want)))), (dims, Ls, b5, c5, w)
            assert np.array_equal(got == 0, want == 0)      # the zeros are zeros


# ---- the apply from the links, and the stored route beside it
PIECE_SETS = [P.P_ALL, P.P_ALL | P.P_ZERO]                                     # accumulating, and overwriting onto a NaN prefill
MORE_PIECES = [P.P_ALL | P.P_ZERO_E, P.P_CLOVER | P.P_HOPPING | P.P_SHIFT_O | P.P_ZERO]   # a mixed pair, at the first parameter set


@pytest.mark.parametrize("f32", [False, True], ids=["c64", "c32"])
@pytest.mark.parametrize("dims", LATTICES, ids=IDS)
@pytest.mark.parametrize("Ls", LS_STORED + [32])
def test_direct_apply_and_stored_route_against_the_grid_formula(dims, Ls, f32):
    Lx, Ly = dims
    nc = 2 * Ls
    dt, npt = (qmg.C32 if f32 else qmg.C64), np_dtype(f32)
    g, rhs, lhs0 = case(dims, Ls, f32)
    dg, dx = D(g.astype(npt)), D(rhs.astype(npt))
    d = qmg.make_desc(Lx, Ly, nc, None, None, *SHIFTS)
    for ip, (b5, c5, w) in enumerate(PARAMS):
        stored = None
        if Ls <= 12:     # the stored form of D and, built from it, of D^dagger (with the conjugated shifts)
            cm = Lx * Ly * nc * nc
            arrs = [qmg.DeviceArray(cm), qmg.DeviceArray(4 * cm), qmg.DeviceArray(cm), qmg.DeviceArray(4 * cm)]
            qmg.mobius_fill(arrs[0], arrs[1], D(gauge(Lx, Ly)), Lx, Ly, Ls, M, w, M5, b5, c5)
            qmg.build_dagger(arrs[2], arrs[3], arrs[0], arrs[1], Lx, Ly, nc)
            if f32:
                narrow = [qmg.DeviceArray(a.n, np.complex64) for a in arrs]
                for a32, a in zip(narrow, arrs):
                    qmg.convert(a32, qmg.C32, a, qmg.C64, a.n)
                arrs = narrow
            stored = (qmg.make_desc(Lx, Ly, nc, arrs[0], arrs[1], *SHIFTS), qmg.make_desc(Lx, Ly, nc, arrs[2], arrs[3], *[np.conj(s) for s in SHIFTS]))
        for op in OPS:
            for pieces in PIECE_SETS + (MORE_PIECES if ip == 0 else []):
                want, S, n = reference(dims, Ls, f32, b5, c5, w, op, pieces)
                start = nan_prefill(lhs0, pieces)
                got = D(start.astype(npt))
                qmg.mobius_apply_direct(dt, d, dg, Ls, M, got, dx, pieces, w, M5, b5, c5, op)
                h = got.to_host()
                tag = (b5, c5, w, op, hex(pieces))
                assert np.all(np.isfinite(h)), (tag, "NaN prefill survived")
                ok, worst = within(h, want, S, n, f32)
                print("mobius direct %s Ls=%d %s %s worst err/bound %.3f" % (dims, Ls, "c32" if f32 else "c64", tag, worst))
                assert ok, (tag, worst)
                if stored is not None:
                    gs = D(np.where(np.isfinite(start), start, 0).astype(npt))
                    qmg.stencil_apply_t(dt, stored[op], gs, dx, pieces)
                    ok, worst = within(gs.to_host(), want, S, n, f32)
                    assert ok, (tag, "stored route", worst)


BATCH_CASES = [((2, 2), 3), ((4, 6), 6), ((130, 2), 12), ((16, 8), 8), ((16, 8), 32)]


@pytest.mark.parametrize("f32", [False, True], ids=["c64", "c32"])
@pytest.mark.parametrize("dims,Ls", BATCH_CASES, ids=IDS)
def test_masked_batches_with_a_long_stride(dims, Ls, f32):
    """three systems, the middle one masked out, a stride longer than a vector: the masked system and the padding hold NaN and keep their bits"""
    Lx, Ly = dims
    nc = 2 * Ls
    n = Lx * Ly * nc
    stride = n + 4
    nrhs, mask = 3, 0b101
    b5, c5, w = PARAMS[1]
    dt, npt = (qmg.C32 if f32 else qmg.C64), np_dtype(f32)
    g = rounded(gauge(Lx, Ly), f32)
    xs, ls = rounded(cvec(nrhs * stride, 3), f32), rounded(cvec(nrhs * stride, 4), f32)
    active = np.zeros(nrhs * stride, dtype=bool)
    for k in range(nrhs):
        if (mask >> k) & 1:
            active[k * stride:k * stride + n] = True
    d = qmg.make_desc(Lx, Ly, nc, None, None, *SHIFTS)
    dg = D(g.astype(npt))
    for op in OPS:
        for pieces in PIECE_SETS:
            start = ls.copy()
            start[~active] = np.nan                                        # the masked system and the padding between the vectors
            xin = xs.copy()
            xin[~active] = np.nan                                          # ... of the source too: never read
            if pieces & P.P_ZERO:
                start[active] = np.nan
            got = D(start.astype(npt))
            qmg.mobius_apply_direct(dt, d, dg, Ls, M, got, D(xin.astype(npt)), pieces, w, M5, b5, c5, op, nrhs, stride, mask)
            h = got.to_host()
            for k in range(nrhs):
                sl = slice(k * stride, k * stride + n)
                if (mask >> k) & 1:
                    want, S, cnt = mn.apply(Lx, Ly, Ls, g, M, w, M5, b5, c5, *SHIFTS, pieces, xs[sl], ls[sl], dagger=bool(op))
                    ok, worst = within(h[sl], want, S, cnt, f32)
                    assert ok, (op, hex(pieces), k, worst)
            assert h[~active].tobytes() == start.astype(npt)[~active].tobytes(), (op, hex(pieces))     # untouched, bit for bit


@pytest.mark.parametrize("f32", [False, True], ids=["c64", "c32"])
@pytest.mark.parametrize("dims,Ls", BATCH_CASES, ids=IDS)
def test_shamir_limit_against_the_shamir_entry(dims, Ls, f32):
    """b5 = 1, c5 = 0 against qmg_dwf_apply_direct.  At w = 1 the Shamir shift is M5 itself; at w = 0.9 the Shamir diagonal is 3 w + shift where
    this operator has 2 w + M5 + 1, so the Shamir shift is M5 + 1 - w.  Both are within their own bound of the same exact result (each twin's S
    and n), so they differ by at most the two bounds added; bit for bit is not asked, the arithmetic order differs."""
    Lx, Ly = dims
    nc = 2 * Ls
    dt, npt = (qmg.C32 if f32 else qmg.C64), np_dtype(f32)
    g, rhs, lhs0 = case(dims, Ls, f32)
    dg, dx = D(g.astype(npt)), D(rhs.astype(npt))
    extra = (0.011 + 0.03j, 0.011 - 0.02j, 0.023 + 0.01j)
    for w in (1.0, 0.9):
        sh_shift = M5 + (1.0 - w) + extra[0]
        for pieces in PIECE_SETS:
            start = nan_prefill(lhs0, pieces)
            a, b = D(start.astype(npt)), D(start.astype(npt))
            qmg.mobius_apply_direct(dt, qmg.make_desc(Lx, Ly, nc, None, None, *extra), dg, Ls, M, a, dx, pieces, w, M5, 1.0, 0.0, 0)
            qmg.dwf_apply_direct(dt, qmg.make_desc(Lx, Ly, nc, None, None, sh_shift, extra[1], extra[2]), dg, Ls, M, b, dx, pieces, w)
            want, S, n = reference(dims, Ls, f32, 1.0, 0.0, w, 0, pieces, extra)
            want2, S2, n2 = dn.apply(Lx, Ly, Ls, g, M, w, sh_shift, extra[1], extra[2], pieces, rhs, lhs0)
            ha, hb = a.to_host(), b.to_host()
            assert within(ha, want, S, n, f32)[0] and within(hb, want2, S2, n2, f32)[0], (w, hex(pieces))
            diff = np.abs(ha.astype(sn.CLD) - hb.astype(sn.CLD))
            assert np.all(diff <= bound_of(want, S, n, f32) + bound_of(want2, S2, n2, f32)), (w, hex(pieces), float(np.max(diff)))


@pytest.mark.parametrize("f32", [False, True], ids=["c64", "c32"])
@pytest.mark.parametrize("dims,Ls", BATCH_CASES, ids=IDS)
def test_adjointness(dims, Ls, f32):
    """|<y, D x> - <D^dagger y, x>| <= sum over the sites of |y| bound(D x) + |x| bound(D^dagger y): the two exact values are equal"""
    Lx, Ly = dims
    nc = 2 * Ls
    n = Lx * Ly * nc
    dt, npt = (qmg.C32 if f32 else qmg.C64), np_dtype(f32)
    g = rounded(gauge(Lx, Ly), f32)
    x, y = rounded(cvec(n, 8), f32), rounded(cvec(n, 9), f32)
    zero = np.zeros(n, dtype=np.complex128)
    d = qmg.make_desc(Lx, Ly, nc, None, None, *SHIFTS)
    dg = D(g.astype(npt))
    for b5, c5, w in PARAMS:
        Dx, Ddy = D(np.full(n, np.nan).astype(npt)), D(np.full(n, np.nan).astype(npt))
        qmg.mobius_apply_direct(dt, d, dg, Ls, M, Dx, D(x.astype(npt)), P.P_ALL | P.P_ZERO, w, M5, b5, c5, 0)
        qmg.mobius_apply_direct(dt, d, dg, Ls, M, Ddy, D(y.astype(npt)), P.P_ALL | P.P_ZERO, w, M5, b5, c5, 1)
        w0, S0, n0 = mn.apply(Lx, Ly, Ls, g, M, w, M5, b5, c5, *SHIFTS, P.P_ALL | P.P_ZERO, x, zero)
        w1, S1, n1 = mn.apply(Lx, Ly, Ls, g, M, w, M5, b5, c5, *SHIFTS, P.P_ALL | P.P_ZERO, y, zero, dagger=True)
        lhs = np.sum(np.conj(y.astype(sn.CLD)) * Dx.to_host().astype(sn.CLD))
        rhs = np.sum(np.conj(Ddy.to_host().astype(sn.CLD)) * x.astype(sn.CLD))
        room = np.sum(np.abs(y) * bound_of(w0, S0, n0, f32)) + np.sum(np.abs(x) * bound_of(w1, S1, n1, f32))
        print("mobius adjointness %s Ls=%d %s (%g, %g, %g): %.3e of %.3e" % (dims, Ls, "c32" if f32 else "c64", b5, c5, w, abs(lhs - rhs), room))
        assert abs(lhs - rhs) <= room, (b5, c5, w)


# ---- past the cap of grid.y: 2 x 32770 at Ls = 2 is 65540 (parity, y) rows on 65535 blocks, so five blocks take a second row; for op 1 that
# trip uses the second LDS buffer and every lane of the block has to reach its barrier
TALL = (2, 32770)


@pytest.mark.parametrize("f32", [False, True], ids=["c64", "c32"])
@pytest.mark.parametrize("op", OPS)
def test_apply_walks_more_rows_than_the_grid_has_blocks(op, f32):
    Lx, Ly = TALL
    Ls, nc = 2, 4
    b5, c5, w = PARAMS[0]
    pieces = P.P_ALL | P.P_ZERO
    dt, npt = (qmg.C32 if f32 else qmg.C64), np_dtype(f32)
    fam, lps, block, gx, gy, flags, lds, nk = qmg.mobius_plan(dt, TALL, Ls, op, pieces)
    nrows = 2 * Ly
    assert gy == 65535 < nrows == 65540 and gx == 1
    second = np.zeros((2, Ly, (Lx // 2) * nc), dtype=bool)          # rows gy .. nrows - 1, row = 2 y + parity
    for row in range(gy, nrows):
        second[row & 1, row >> 1] = True
    second = second.ravel()
    assert np.count_nonzero(second) == 5 * (Lx // 2) * nc
    g, rhs, lhs0 = case(TALL, Ls, f32)
    want, S, cnt = reference(TALL, Ls, f32, b5, c5, w, op, pieces)
    d = qmg.make_desc(Lx, Ly, nc, None, None, *SHIFTS)
    dg, dx = D(g.astype(npt)), D(rhs.astype(npt))
    runs = []
    for _ in range(2):
        got = D(nan_prefill(lhs0, pieces).astype(npt))
        qmg.mobius_apply_direct(dt, d, dg, Ls, M, got, dx, pieces, w, M5, b5, c5, op)
        runs.append(got.to_host())
    h = runs[0]
    assert np.all(np.isfinite(h)), ("NaN prefill survived", int(np.count_nonzero(~np.isfinite(h[second]))), "of them on the second trip")
    for name, sel in (("whole", slice(None)), ("second trip", second)):
        ok, worst = within(h[sel], np.asarray(want)[sel], np.asarray(S)[sel], np.asarray(cnt)[sel], f32)
        print("mobius tall op %d %s %s: worst err/bound %.3f" % (op, "c32" if f32 else "c64", name, worst))
        assert ok, (name, worst)
    assert runs[1].tobytes() == h.tobytes()                # a second run on the same inputs: the same bytes


def test_refusals_leave_lhs_untouched():
    Lx, Ly, Ls = 16, 8, 8
    nc = 2 * Ls
    n = Lx * Ly * nc
    g, x, l0 = D(gauge(Lx, Ly)), D(cvec(17 * n, 6)), cvec(17 * n, 7)
    d = qmg.make_desc(Lx, Ly, nc, None, None, *SHIFTS)
    unsupported, invalid = 3, 1
    ok = dict(w=1.0, M5=M5, b5=1.5, c5=0.5)

    def refused(status, pieces=P.P_ALL | P.P_ZERO, desc=d, Ls=Ls, nrhs=1, stride=0, mask=1, dtype=qmg.C64, inplace=False, op=0, m=M, **kw):
        lhs = D(l0)
        p = dict(ok, **kw)
        for o in ((0, 1) if op == 0 else (op,)):
            rc = qmg.mobius_apply_direct_status(dtype, desc, g, Ls, m, x if inplace else lhs, x, pieces, p["w"], p["M5"], p["b5"], p["c5"], o, nrhs, stride, mask)
            assert rc == status, (rc, status, o)
        assert lhs.to_host().tobytes() == l0.tobytes()

    for pieces in (P.P_CLOVER_E | P.P_EO | P.P_SHIFT_E | P.P_ZERO_E, P.P_HOPPING | P.P_ZERO, P.P_EO | P.P_ZERO_E, P.P_EO_XP1 | P.P_ZERO_E,
                   P.P_ALL & ~(P.P_OE_XP1 << 3), P.P_CLOVER | P.P_ZERO, P.P_SHIFT | P.P_ZERO, P.P_ZERO):
        refused(unsupported, pieces)                                      # every other piece set: the stored stencil serves it
    refused(invalid, inplace=True)                                        # lhs == rhs
    refused(invalid, op=2)
    refused(invalid, op=-1)
    refused(invalid, desc=qmg.make_desc(Lx, Ly, nc + 2, None, None))      # nc != 2 Ls
    refused(invalid, desc=qmg.make_desc(Lx, Ly, 2, None, None), Ls=1)     # Ls = 1
    refused(invalid, desc=qmg.make_desc(Lx, Ly, 66, None, None), Ls=33)   # Ls = 33
    refused(invalid, nrhs=17, stride=n, mask=0x1FFFF)                     # nrhs = 17
    refused(invalid, nrhs=2, stride=n - 2, mask=3)                        # systems that overlap
    refused(invalid, dtype=2)
    for bad in (float("nan"), float("inf")):
        for name in ("b5", "c5", "M5", "w"):
            refused(invalid, **{name: bad})
        refused(invalid, m=complex(bad, 0.0))
    assert qmg.mobius_apply_direct_status(qmg.C64, d, g, Ls, M, D(l0), x, P.P_ALL | P.P_ZERO, 1.0, M5, 1.5, 0.5, 1, 3, n, 0) == 0   # nothing active: success, nothing done


# ---- the stream
@pytest.mark.parametrize("which", ["fill", "op0", "op1"])
def test_entry_runs_on_the_stream_it_is_given(which):
    """The inputs of the call reach the device behind a gate on a created stream (tests/stream_gate.py); the call is enqueued on that stream
    while the gate is shut and must give the bytes of a synchronised null-stream run.  A launch on another stream would read the poison."""
    Lx, Ly, Ls = 6, 4, 4
    nc = 2 * Ls
    n, cm = Lx * Ly * nc, Lx * Ly * nc * nc
    b5, c5, w = PARAMS[0]
    g, x, l0 = gauge(Lx, Ly), cvec(n, 12), cvec(n, 13)
    d = qmg.make_desc(Lx, Ly, nc, None, None, *SHIFTS)
    dg, dx = qmg.DeviceArray(g.size), qmg.DeviceArray(n)
    outs = [qmg.DeviceArray(cm), qmg.DeviceArray(4 * cm)] if which == "fill" else [qmg.DeviceArray(n)]

    def call(st):
        if which == "fill":
            qmg.mobius_fill(outs[0], outs[1], dg, Lx, Ly, Ls, M, w, M5, b5, c5, stream=st)
        else:
            qmg.mobius_apply_direct(qmg.C64, d, dg, Ls, M, outs[0], dx, P.P_ALL, w, M5, b5, c5, int(which[-1]), stream=st)

    def stage(values_g, values_x, st=None):
        qmg.memcpy_d2d(dg, values_g, dg.nbytes, stream=st)
        qmg.memcpy_d2d(dx, values_x, dx.nbytes, stream=st)
        if which != "fill":
            qmg.memcpy_d2d(outs[0], sl0, outs[0].nbytes, stream=st)

    sg_, sx, sl0 = D(g), D(x), D(l0)
    poison_g, poison_x = D(np.full(g.size, np.nan + 0j)), D(np.full(n, np.nan + 0j))
    stage(sg_, sx)
    call(None)
    qmg.sync()
    ref = [o.to_host().tobytes() for o in outs]
    st = qmg.stream_create()
    try:
        copies = max(4, int(math.ceil(10.0 / sg.copy_ms(st))))
        stage(poison_g, poison_x)                                          # what a call that escaped its stream would read
        for o in outs if which == "fill" else []:
            qmg.memcpy_d2d(o, D(np.full(o.n, np.nan + 0j)), o.nbytes)
        qmg.sync()
        gate = sg.Gate(st, copies)
        stage(sg_, sx, st)
        call(st)
        assert gate.closed(), "gate open: the case proves nothing"
        qmg.sync(st)
        qmg.sync()
        assert [o.to_host().tobytes() for o in outs] == ref
    finally:
        qmg.sync()
        qmg.stream_destroy(st)


# ---- the facade, through its driver
def run_driver(L, Ls, m, b5, c5, seed=7, solution=None):
    exe = os.path.join(qmg.HERE, "drivers", "mobius_selftest")
    assert os.path.exists(exe), "drivers/mobius_selftest is not built"
    cmd = [exe, str(L), str(Ls), str(m), str(b5), str(c5), str(seed)] + ([solution] if solution else [])
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    print(out.stdout)
    lines = {}
    for ln in out.stdout.splitlines():
        if ln.startswith("[QMG-MOBIUS] "):
            _, name, value, verdict = ln.split()
            lines[name] = (float(value), verdict)
    assert out.returncode == 0, out.stdout
    assert "[MOBIUS-SELFTEST] PASS" in out.stdout
    return lines


@pytest.mark.parametrize("L,Ls,b5,c5", [(16, 8, 1.5, 0.5), (8, 6, 1.5, 0.5), (8, 32, 1.5, 0.5)], ids=IDS)
def test_mobius_selftest_driver(L, Ls, b5, c5):
    lines = run_driver(L, Ls, 0.05, b5, c5)
    expected = ["links_route_on", "adjointness", "gamma5_violation", "shamir_limit", "cg_iterations", "cg_true_residual"]
    if Ls <= 12:
        expected += ["links_vs_stored", "dagger_links_vs_stored"]
    assert sorted(lines) == sorted(expected)
    assert all(v == "PASS" for _, v in lines.values()), lines
    if Ls <= 12:
        assert lines["links_vs_stored"][0] < 1e-13 and lines["dagger_links_vs_stored"][0] < 1e-13
    assert lines["adjointness"][0] < 1e-12 and lines["shamir_limit"][0] < 1e-13
    assert lines["gamma5_violation"][0] > 1e-3            # c5 = 0.5: Gamma5 D Gamma5 is not D^dagger
    assert lines["cg_true_residual"][0] <= 1e-8           # the driver's true residual at eps = 1e-10: the gate of dwf_eo_selftest
    assert 0 < lines["cg_iterations"][0] < 2000


def test_minv_mobius_cg_against_the_dense_solve(tmp_path):
    """the driver's solve at 4 x 4, Ls = 4, written out and held to numpy's dense solve of the same system.  The gate is ten times the distance
    the numpy CG of tests/test_host_mobius.py reaches at the same eps (1.509e-10 there: 1.6e-9); measured here on an MI355X: see the print."""
    s = mn.SOLVE
    L, Ls = s["dims"][0], s["Ls"]
    nc = 2 * Ls
    path = str(tmp_path / "solution.bin")
    lines = run_driver(L, Ls, s["m"], s["b5"], s["c5"], 7, path)
    raw = np.fromfile(path, dtype=np.complex128)
    ng, n = 2 * L * L, L * L * nc
    assert raw.size == ng + 2 * n
    g, b, x = raw[:ng], raw[ng:ng + n], raw[ng + n:]
    Dm, *_ = mn.dense(L, L, Ls, g, s["m"], s["w"], s["M5"], s["b5"], s["c5"])
    bg = np.asarray(sn.to_grid(b, L, L, nc)).astype(np.complex128).reshape(-1)
    xg = np.asarray(sn.to_grid(x, L, L, nc)).astype(np.complex128).reshape(-1)
    x_dense = np.linalg.solve(Dm, bg)
    dist = float(np.linalg.norm(xg - x_dense) / np.linalg.norm(x_dense))
    print("minv_mobius_cg: %d iterations, |x - x_dense| / |x_dense| = %.3e (gate %.1e)" % (lines["cg_iterations"][0], dist, 10 * mn.SOLVE_REACH))
    assert dist <= 10 * mn.SOLVE_REACH
