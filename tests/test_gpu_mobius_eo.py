"""The even-odd Moebius kernels on the GPU (csrc/qmg_mobius_eo.hip): qmg_mobius_inv5, qmg_mobius_hops_inv5 and qmg_mobius_schur_apply (M and
M^dagger, two launches each), each against mobius_eo_numpy's long-double statement, whose A^-1 is a Gauss-Jordan inverse and shares neither
the twisted-circulant tables nor the index arithmetic of the kernels (tests/test_host_mobius_eo.py validates it without a GPU).

Lattices: (2, 2) every neighbour pair coincides; (4, 6) small general case; (130, 2) Lx/2 = 65 sites per half row and +-y coincide;
(16, 8) regular.  Ls: 2, 3, 6, 8, 12, 32 -- 3, 6, 12 do not divide the wavefront (sites straddle wavefronts, the block is 255 / 252 / 252
lanes and the last one is partial); at (130, 2) with Ls = 8, 12, 32 a half row takes more than one block.

Parameters: b5 = 1.5, c5 = 0.5, w = 0.9, M5 = -0.8, m = 0.05 + 0.02i, shift = -0.2 + 0.03i, eo_shift = 0.011 - 0.02i (alpha_even != alpha_odd,
both complex, |kappa / alpha_p| ~ 0.22).

Bounds: stencil_numpy.elementwise_bound on the S and n mobius_eo_numpy returns -- fp64: (n + 1) 2^-50 S; fp32 arithmetic: (n + 1) 2^-21 S +
2^-23 |want| on inputs rounded to complex64.

Worst error as a fraction of the bound over every shape, measured on an MI355X: see DESIGN 26."""
import functools
import importlib
import itertools
import os
import subprocess

import numpy as np
import pytest

import dwf_eo_numpy as de
import mobius_eo_numpy as me
import mobius_numpy as mn
import stencil_numpy as sn

qmg = importlib.import_module("quantum-mg_amd")
pytestmark = pytest.mark.gpu
D = qmg.DeviceArray.from_host
P = qmg

LATTICES = [(2, 2), (4, 6), (130, 2), (16, 8)]
LS_ALL = [2, 3, 6, 8, 12, 32]
M, W, M5, B5, C5 = 0.05 + 0.02j, 0.9, -0.8, 1.5, 0.5
SHIFT, EO_SHIFT = 0.03j - 0.2, 0.011 - 0.02j
SCALE = 0.7 - 0.4j
MOB = dict(w=W, M5=M5, b5=B5, c5=C5)
TWIN = (M, W, M5, B5, C5, SHIFT, EO_SHIFT)
IDS = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)
PREC = pytest.mark.parametrize("f32", [False, True], ids=["c64", "c32"])
UNSUPPORTED, INVALID = 3, 1
TABLES = [(qmg.MOBIUS_S_ONE, "1"), (qmg.MOBIUS_S_AINV, "A^-1"), (qmg.MOBIUS_S_AINV_B, "A^-1 B")]
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _device():
    qmg.build()
    qmg.init(0)
    yield
    qmg.sync()
    for k in sorted(WORST):
        print("mobius eo worst err/bound over all shapes: %-12s %.3f" % (k, WORST[k]))


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


def within(got, want, S, n, f32, family=None):
    err = np.abs(got.astype(sn.CLD) - want)
    bound = sn.elementwise_bound(S, n, want, fp32_arithmetic=True) if f32 else sn.elementwise_bound(S, n)
    worst = float(np.max(err / np.where(bound > 0, bound, 1)))
    if family:
        key = "%s %s" % (family, "c32" if f32 else "c64")
        WORST[key] = max(WORST.get(key, 0.0), worst)
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


# ---- qmg_mobius_inv5
@PREC
@pytest.mark.parametrize("dims", LATTICES, ids=IDS)
@pytest.mark.parametrize("Ls", LS_ALL)
def test_inv5_against_the_gauss_jordan_inverse(dims, Ls, f32):
    Lx, Ly = dims
    dt, npt = types(f32)
    g, rhs, lhs0, _ = case(dims, Ls, f32)
    d, dx = desc(dims, Ls), D(rhs.astype(npt))
    for (table, name), (pieces, named) in itertools.product(TABLES[1:], ((P.P_CLOVER_E, [0]), (P.P_CLOVER_O, [1]), (P.P_CLOVER, [0, 1]))):
        want, S, n = me.inv5(Lx, Ly, Ls, *TWIN, pieces, table, SCALE, rhs, lhs0)
        got = D(prefill(lhs0, named).astype(npt))
        qmg.mobius_inv5(dt, d, Ls, M, got, dx, pieces, table, SCALE, **MOB)
        h = got.to_host()
        assert np.all(np.isfinite(h)), (name, hex(pieces), "NaN prefill survived")
        ok, worst = within(h, want, S, n, f32, "inv5")
        assert ok, (name, hex(pieces), worst)
        for p in (0, 1):
            if p not in named:
                assert h[halves(h.size)[p]].tobytes() == lhs0.astype(npt)[halves(h.size)[p]].tobytes(), (name, hex(pieces))
    v = D(rhs.astype(npt))                                       # in place
    qmg.mobius_inv5(dt, d, Ls, M, v, v, P.P_CLOVER, table, SCALE, **MOB)
    ok, worst = within(v.to_host(), want, S, n, f32, "inv5")
    assert ok, ("in place", worst)


# ---- qmg_mobius_hops_inv5
K_PIECES = [P.P_EO | P.P_ZERO_E, P.P_EO, P.P_OE | P.P_ZERO_O, P.P_OE, P.P_HOPPING | P.P_ZERO, P.P_HOPPING, P.P_HOPPING | P.P_ZERO_E]


@PREC
@pytest.mark.parametrize("dims", LATTICES, ids=IDS)
@pytest.mark.parametrize("Ls", LS_ALL)
def test_hops_inv5_every_table_and_source_against_the_grid_formula(dims, Ls, f32):
    """every S in {1, A^-1, A^-1 B} with every R in {1, B}, over the piece sets of kernel K; Gamma5 on the load on every other piece set, the
    other way round for the next (S, R), so that every piece set and every (S, R) meets both"""
    Lx, Ly = dims
    dt, npt = types(f32)
    g, rhs, lhs0, _ = case(dims, Ls, f32)
    d, dg, dx = desc(dims, Ls), D(g.astype(npt)), D(rhs.astype(npt))
    for c, ((table, name), source) in enumerate(itertools.product(TABLES, (qmg.MOBIUS_R_ONE, qmg.MOBIUS_R_B))):
        for i, pieces in enumerate(K_PIECES):
            flags = qmg.DWF_G5_IN if (i + c) & 1 else 0
            want, S, n = me.hops_inv5(Lx, Ly, Ls, g, *TWIN, pieces, table, source, SCALE, flags, rhs, lhs0)
            got = D(prefill(lhs0, [p for p in (0, 1) if pieces & (P.P_ZERO_E << p)]).astype(npt))
            qmg.mobius_hops_inv5(dt, d, dg, Ls, M, got, dx, pieces, table, source, SCALE, flags, **MOB)
            h = got.to_host()
            tag = (name, source, hex(pieces), flags)
            assert np.all(np.isfinite(h)), (tag, "NaN prefill survived")
            ok, worst = within(h, want, S, n, f32, "hops_inv5")
            assert ok, (tag, worst)
            untouched = np.asarray(n == 0)
            assert h[untouched].tobytes() == lhs0.astype(npt)[untouched].tobytes(), tag      # a parity no piece touches keeps its bits


@pytest.mark.parametrize("dims,Ls", [((2, 2), 3), ((4, 6), 6), ((130, 2), 12), ((16, 8), 8), ((16, 8), 32)], ids=IDS)
def test_hops_inv5_in_place(dims, Ls):
    """lhs == rhs: one parity written from the other (reconstruct's call)"""
    Lx, Ly = dims
    g, x, _, _ = case(dims, Ls, False)
    n = x.size
    for pieces, p in ((P.P_EO | P.P_ZERO_E, 0), (P.P_OE, 1)):
        v = D(x)
        qmg.mobius_hops_inv5(qmg.C64, desc(dims, Ls), D(g), Ls, M, v, v, pieces, qmg.MOBIUS_S_AINV, qmg.MOBIUS_R_B, SCALE, 0, **MOB)
        h = v.to_host()
        written, kept = halves(n)[p], halves(n)[1 - p]
        assert h[kept].tobytes() == x[kept].tobytes()
        want, S, cnt = me.hops_inv5(Lx, Ly, Ls, g, *TWIN, pieces, me.S_AINV, me.R_B, SCALE, 0, x, x)
        ok, worst = within(h[written], want[written], S[written], cnt[written], False, "hops_inv5")
        assert ok, (hex(pieces), worst)


# ---- the Schur complement and its dagger
@functools.lru_cache(maxsize=None)
def schur_reference(dims, Ls, f32, parity, op):
    g, rhs, lhs0, tmp0 = case(dims, Ls, f32)
    return me.schur(*dims, Ls, g, *TWIN, parity, op, rhs, lhs0, tmp0)


@PREC
@pytest.mark.parametrize("dims", LATTICES, ids=IDS)
@pytest.mark.parametrize("Ls", LS_ALL)
def test_schur_apply_both_ops_and_parities(dims, Ls, f32):
    dt, npt = types(f32)
    g, rhs, lhs0, tmp0 = case(dims, Ls, f32)
    n = rhs.size
    d, dg, dx = desc(dims, Ls), D(g.astype(npt)), D(rhs.astype(npt))
    for parity, op in itertools.product((0, 1), (0, 1)):
        want, S, cnt, wt, St, nt = schur_reference(dims, Ls, f32, parity, op)
        got, tmp = D(prefill(lhs0, [parity]).astype(npt)), D(prefill(tmp0, [1 - parity]).astype(npt))
        qmg.mobius_schur_apply(dt, d, dg, Ls, M, got, dx, tmp, parity, op, **MOB)
        h, t = got.to_host(), tmp.to_host()
        assert np.all(np.isfinite(h)) and np.all(np.isfinite(t)), (parity, op, "NaN prefill survived")
        ok, worst = within(h, want, S, cnt, f32, "schur op%d" % op)
        okt, worst_t = within(t, wt, St, nt, f32, "schur tmp")
        assert ok and okt, (parity, op, worst, worst_t)
        p_half, o_half = halves(n)[parity], halves(n)[1 - parity]
        assert h[o_half].tobytes() == lhs0.astype(npt)[o_half].tobytes()       # the 1-p half of lhs
        assert t[p_half].tobytes() == tmp0.astype(npt)[p_half].tobytes()       # the p half of tmp
        assert dx.to_host().tobytes() == rhs.astype(npt).tobytes()             # rhs, both halves


@PREC
@pytest.mark.parametrize("dims", LATTICES, ids=IDS)
@pytest.mark.parametrize("Ls", LS_ALL)
def test_schur_adjointness(dims, Ls, f32):
    """<y, M x> = <M^dagger y, x> on the device results, inside what the two elementwise bounds allow: sum |y| bound(M x) + sum |x| bound(M^dagger y)
    (the dot products themselves are formed in long double)"""
    dt, npt = types(f32)
    g, x, _, y = case(dims, Ls, f32)
    n = x.size
    zero = np.zeros(n, dtype=np.complex128)
    d, dg = desc(dims, Ls), D(g.astype(npt))
    for parity in (0, 1):
        sel = halves(n)[parity]
        _, S0, n0, *_ = schur_reference(dims, Ls, f32, parity, 0)                                # M x: rhs of the case is x (lhs0 lies outside sel)
        wd, S1, n1, *_ = me.schur(*dims, Ls, g, *TWIN, parity, 1, y, zero, zero)
        w0 = schur_reference(dims, Ls, f32, parity, 0)[0]
        Mx, Mdy, tmp = D(np.zeros(n, dtype=npt)), D(np.zeros(n, dtype=npt)), D(np.zeros(n, dtype=npt))
        qmg.mobius_schur_apply(dt, d, dg, Ls, M, Mx, D(x.astype(npt)), tmp, parity, 0, **MOB)
        qmg.mobius_schur_apply(dt, d, dg, Ls, M, Mdy, D(y.astype(npt)), tmp, parity, 1, **MOB)
        Mx, Mdy = Mx.to_host().astype(sn.CLD)[sel], Mdy.to_host().astype(sn.CLD)[sel]
        xs, ys = x.astype(sn.CLD)[sel], y.astype(sn.CLD)[sel]
        b0 = sn.elementwise_bound(S0, n0, w0, fp32_arithmetic=True) if f32 else sn.elementwise_bound(S0, n0)
        b1 = sn.elementwise_bound(S1, n1, wd, fp32_arithmetic=True) if f32 else sn.elementwise_bound(S1, n1)
        room = float(np.sum(np.abs(ys) * b0[sel]) + np.sum(np.abs(xs) * b1[sel]))
        gap = float(abs(np.vdot(ys, Mx) - np.vdot(Mdy, xs)))
        assert gap <= room, (parity, gap, room)
        WORST["adjointness " + ("c32" if f32 else "c64")] = max(WORST.get("adjointness " + ("c32" if f32 else "c64"), 0.0), gap / room)


# ---- batches
@PREC
@pytest.mark.parametrize("dims,Ls", [((2, 2), 3), ((4, 6), 6), ((130, 2), 12), ((16, 8), 8), ((16, 8), 32)], ids=IDS)
def test_batches_with_a_frozen_system_full_of_nan(dims, Ls, f32):
    Lx, Ly = dims
    n = Lx * Ly * 2 * Ls
    stride = n + 4 * n + 4                                 # systems apart by five vectors
    nrhs, mask = 3, 0b101
    dt, npt = types(f32)
    g = rounded(gauge(Lx, Ly), f32)
    xs, ls, ts = (rounded(cvec(nrhs * stride, s), f32) for s in (3, 4, 5))
    sl = lambda k: slice(k * stride, k * stride + n)
    for a in (xs, ls, ts):
        a[sl(1)] = np.nan                                  # the frozen system: nothing of it may be read into an active one, or written
    d, dg, dx = desc(dims, Ls), D(g.astype(npt)), D(xs.astype(npt))
    pad = np.ones(nrhs * stride, dtype=bool)
    for k in range(nrhs):
        pad[sl(k)] = False

    def check(h, start, ref, what):
        for k in range(nrhs):
            if not (mask >> k) & 1:
                assert h[sl(k)].tobytes() == start.astype(npt)[sl(k)].tobytes(), what       # the frozen system: byte-identical
                continue
            want, S, cnt = ref(k)
            assert np.all(np.isfinite(h[sl(k)])), (what, k)
            ok, worst = within(h[sl(k)], want, S, cnt, f32, "batch")
            assert ok, (what, k, worst)
        assert h[pad].tobytes() == start.astype(npt)[pad].tobytes(), what                   # nothing between the vectors is written

    got = D(ls.astype(npt))
    qmg.mobius_inv5(dt, d, Ls, M, got, dx, P.P_CLOVER, qmg.MOBIUS_S_AINV_B, SCALE, nrhs=nrhs, vec_stride=stride, mask=mask, **MOB)
    check(got.to_host(), ls, lambda k: me.inv5(Lx, Ly, Ls, *TWIN, P.P_CLOVER, me.S_AINV_B, SCALE, xs[sl(k)], ls[sl(k)]), "inv5")
    for pieces, table, source, flags in ((P.P_HOPPING, me.S_AINV, me.R_B, 0), (P.P_OE | P.P_ZERO_O, me.S_AINV_B, me.R_ONE, qmg.DWF_G5_IN)):
        got = D(ls.astype(npt))
        qmg.mobius_hops_inv5(dt, d, dg, Ls, M, got, dx, pieces, table, source, SCALE, flags, nrhs=nrhs, vec_stride=stride, mask=mask, **MOB)
        check(got.to_host(), ls, lambda k: me.hops_inv5(Lx, Ly, Ls, g, *TWIN, pieces, table, source, SCALE, flags, xs[sl(k)], ls[sl(k)]), hex(pieces))
    for op in (0, 1):
        got, tmp = D(ls.astype(npt)), D(ts.astype(npt))
        qmg.mobius_schur_apply(dt, d, dg, Ls, M, got, dx, tmp, 1, op, nrhs=nrhs, vec_stride=stride, mask=mask, **MOB)
        ref = functools.lru_cache(maxsize=None)(lambda k: me.schur(Lx, Ly, Ls, g, *TWIN, 1, op, xs[sl(k)], ls[sl(k)], ts[sl(k)]))
        check(got.to_host(), ls, lambda k: ref(k)[:3], "schur op%d lhs" % op)
        check(tmp.to_host(), ts, lambda k: ref(k)[3:], "schur op%d tmp" % op)


# ---- the Shamir limit
@PREC
@pytest.mark.parametrize("dims,Ls", [((2, 2), 2), ((4, 6), 3), ((130, 2), 8), ((16, 8), 12), ((16, 8), 32)], ids=IDS)
def test_shamir_limit_is_the_domain_wall_schur_complement(dims, Ls, f32):
    """b5 = 1, c5 = 0, w = 1: qmg_dwf_schur_apply with shift = M5 (op 1: its Gamma5 M Gamma5 with the conjugated mass and shifts), inside the sum
    of both twins' bounds"""
    dt, npt = types(f32)
    g, rhs, lhs0, tmp0 = case(dims, Ls, f32)
    d, dg, dx = desc(dims, Ls), D(g.astype(npt)), D(rhs.astype(npt))
    M5s = -1.3                                                       # alpha = 1.7 + shift: |d_p| ~ 1.5 > 1 in the Shamir form
    for parity, op in itertools.product((0, 1), (0, 1)):
        cj = np.conj if op else (lambda v: v)
        dwf_desc = desc(dims, Ls, cj(M5s + SHIFT), cj(EO_SHIFT))
        flags = qmg.DWF_G5_IN | qmg.DWF_G5_OUT if op else 0
        want, S, cnt, *_ = me.schur(*dims, Ls, g, M, 1.0, M5s, 1.0, 0.0, SHIFT, EO_SHIFT, parity, op, rhs, lhs0, tmp0)
        _, Sd, nd, *_ = de.schur(*dims, Ls, g, cj(M), 1.0, cj(M5s + SHIFT), cj(EO_SHIFT), parity, flags, rhs, lhs0, tmp0)
        a, b, ta, tb = (D(lhs0.astype(npt)) for _ in range(4))
        qmg.mobius_schur_apply(dt, d, dg, Ls, M, a, dx, ta, parity, op, 1.0, M5s, 1.0, 0.0)
        qmg.dwf_schur_apply(dt, dwf_desc, dg, Ls, cj(M), b, dx, tb, parity, flags, 1.0)
        ha, hb = a.to_host().astype(sn.CLD), b.to_host().astype(sn.CLD)
        if f32:
            bound = sn.elementwise_bound(S, cnt, want, fp32_arithmetic=True) + sn.elementwise_bound(Sd, nd, want, fp32_arithmetic=True)
        else:
            bound = sn.elementwise_bound(S, cnt) + sn.elementwise_bound(Sd, nd)
        err = np.abs(ha - hb)
        assert np.all(err <= bound), (parity, op, float(np.max(err / np.where(bound > 0, bound, 1))))
        assert np.any(ha != lhs0.astype(npt))


# ---- past the cap of grid.y: one parity of 2 x 65540 puts 65540 rows on 65535 blocks, so five blocks take a second row through the other LDS
# buffer, in every new kernel: the mixing kernel on the own chunk, with the hops mixed on the load and not, and both second stages
TALL, LS_TALL = (2, 65540), 2


def walked_second(plan, dims, Ls, parity):
    """asserts from the plan that grid.y is capped below the row count, and returns the mask over one vector of the rows of `parity` a block
    reaches on its second trip"""
    Lx, Ly = dims
    gy = plan[4]
    assert gy == 65535 < Ly == 65540, plan
    m = np.zeros((2, Ly, (Lx // 2) * 2 * Ls), dtype=bool)
    m[parity, gy:] = True
    return m.ravel()


def held_to_the_twin(h, want, S, cnt, f32, second, tag):
    assert np.all(np.isfinite(h)), (tag, "NaN prefill survived", int(np.count_nonzero(~np.isfinite(h[second]))), "of them on the second trip")
    for name, sel in (("whole", slice(None)), ("second trip", second)):
        ok, worst = within(h[sel], np.asarray(want)[sel], np.asarray(S)[sel], np.asarray(cnt)[sel], f32, "tall")
        assert ok, (tag, name, worst)


@PREC
@pytest.mark.parametrize("op", [0, 1])
def test_schur_apply_walks_more_rows_than_the_grid_has_blocks(op, f32):
    dims, Ls, parity = TALL, LS_TALL, 1
    dt, npt = types(f32)
    one = P.P_CLOVER_O | P.P_OE | P.P_SHIFT_O | P.P_ZERO_O
    plan1 = qmg.mobius_eo_plan(dt, dims, Ls, qmg.MEK_HOPS_INV5, P.P_EO | P.P_ZERO_E, 2 if op else 1, 0 if op else 1)
    plan2 = qmg.mobius_eo_plan(dt, dims, Ls, qmg.MEK_SCHUR2_DAGGER if op else qmg.MEK_SCHUR2, one)
    assert plan1[0] == qmg.MEF_HOPS_MIX and plan2[0] == (qmg.MEF_SCHUR2_DAGGER if op else qmg.MEF_SCHUR2), (plan1, plan2)
    assert bool(plan1[5] & qmg.MEPF_RMIX) == (op == 0)
    second_t, second = walked_second(plan1, dims, Ls, 1 - parity), walked_second(plan2, dims, Ls, parity)
    g, rhs, lhs0, tmp0 = case(dims, Ls, f32)
    n = rhs.size
    d, dg, dx = desc(dims, Ls), D(g.astype(npt)), D(rhs.astype(npt))
    want, S, cnt, wt, St, nt = me.schur(*dims, Ls, g, *TWIN, parity, op, rhs, lhs0, tmp0)
    got, tmp = D(prefill(lhs0, [parity]).astype(npt)), D(prefill(tmp0, [1 - parity]).astype(npt))
    qmg.mobius_schur_apply(dt, d, dg, Ls, M, got, dx, tmp, parity, op, **MOB)
    h, t = got.to_host(), tmp.to_host()
    held_to_the_twin(t, wt, St, nt, f32, second_t, ("schur tmp", op, f32))
    held_to_the_twin(h, want, S, cnt, f32, second, ("schur lhs", op, f32))
    p_half, o_half = halves(n)[parity], halves(n)[1 - parity]
    assert h[o_half].tobytes() == lhs0.astype(npt)[o_half].tobytes() and t[p_half].tobytes() == tmp0.astype(npt)[p_half].tobytes()


@PREC
def test_inv5_walks_more_rows_than_the_grid_has_blocks(f32):
    dims, Ls = TALL, LS_TALL
    dt, npt = types(f32)
    plan = qmg.mobius_eo_plan(dt, dims, Ls, qmg.MEK_INV5, P.P_CLOVER_O, qmg.MOBIUS_S_AINV_B)
    assert plan[0] == qmg.MEF_MIX and plan[2] == 256, plan
    second = walked_second(plan, dims, Ls, 1)
    g, rhs, lhs0, _ = case(dims, Ls, f32)
    want, S, n = me.inv5(*dims, Ls, *TWIN, P.P_CLOVER_O, me.S_AINV_B, SCALE, rhs, lhs0)
    got = D(prefill(lhs0, [1]).astype(npt))
    qmg.mobius_inv5(dt, desc(dims, Ls), Ls, M, got, D(rhs.astype(npt)), P.P_CLOVER_O, qmg.MOBIUS_S_AINV_B, SCALE, **MOB)
    h = got.to_host()
    held_to_the_twin(h, want, S, n, f32, second, ("inv5", f32))
    assert h[halves(h.size)[0]].tobytes() == lhs0.astype(npt)[halves(h.size)[0]].tobytes()


# ---- refusals
def test_refusals_leave_lhs_untouched():
    dims, Ls = (16, 8), 8
    n = dims[0] * dims[1] * 2 * Ls
    g, x, t, l0 = D(gauge(*dims)), D(cvec(17 * n, 6)), D(cvec(17 * n, 8)), cvec(17 * n, 7)
    d = desc(dims, Ls)
    inf, nan = float("inf"), float("nan")

    def refused(status, entry="hops", pieces=None, desc_=d, Ls=Ls, nrhs=1, stride=0, mask=1, dtype=qmg.C64, inplace=False, scale=SCALE, flags=0, m=M, parity=0,
                alias=None, table=qmg.MOBIUS_S_AINV, source=qmg.MOBIUS_R_B, op=0, **mob):
        lhs = D(l0)
        target = x if inplace else lhs
        kw = dict(MOB, **mob)
        if entry == "inv5":
            rc = qmg.mobius_inv5_status(dtype, desc_, Ls, m, target, x, P.P_CLOVER if pieces is None else pieces, table, scale, nrhs=nrhs, vec_stride=stride,
                                        mask=mask, **kw)
        elif entry == "hops":
            rc = qmg.mobius_hops_inv5_status(dtype, desc_, g, Ls, m, target, x, P.P_HOPPING | P.P_ZERO if pieces is None else pieces, table, source, scale, flags,
                                             nrhs=nrhs, vec_stride=stride, mask=mask, **kw)
        else:
            tmp = {None: t, "tmp=rhs": x, "tmp=lhs": lhs}[alias]
            rc = qmg.mobius_schur_apply_status(dtype, desc_, g, Ls, m, target, x, tmp, parity, op, nrhs=nrhs, vec_stride=stride, mask=mask, **kw)
        assert rc == status, (entry, rc, status)
        assert lhs.to_host().tobytes() == l0.tobytes()

    for entry in ("inv5", "hops", "schur"):
        for op in ((0, 1) if entry == "schur" else (0,)):
            # the coefficient refusals common to all entries.  w = 1, M5 = -1: d_w = 1, alpha = b5 + 1 + shift, kappa = c5 - 1
            refused(UNSUPPORTED, entry, op=op, desc_=desc(dims, Ls, dof_shift=0.023 + 0.01j))                         # dof_shift != 0
            refused(UNSUPPORTED, entry, op=op, desc_=desc(dims, Ls, 0.0, 0.0), w=1.0, M5=-1.0, b5=0.25, c5=3.0)       # |kappa| = 2 > |alpha| = 1.25
            refused(UNSUPPORTED, entry, op=op, desc_=desc(dims, Ls, 0.0, 0.0), w=1.0, M5=-1.0, b5=1.0, c5=3.0)        # |kappa| = |alpha| = 2
            refused(INVALID, entry, op=op, desc_=desc(dims, Ls, -2.5, 0.0), w=1.0, M5=-1.0, b5=1.5, c5=0.5)           # alpha_p == 0
            refused(INVALID, entry, op=op, desc_=desc(dims, 2, 0.0, 0.0), Ls=2, m=-4.0, w=1.0, M5=-1.0, b5=1.0, c5=0.0)   # r = 1/2: 1 + m r^2 == 0
            refused(INVALID, entry, op=op, m=complex(nan, 0.0))
            for name in ("w", "M5", "b5", "c5"):
                refused(INVALID, entry, op=op, **{name: inf})
            refused(INVALID, entry, op=op, desc_=desc(dims, Ls, shift=complex(-0.2, inf)))
            # qmg_mobius_apply_direct's validity rules
            refused(INVALID, entry, op=op, desc_=qmg.make_desc(16, 8, 2 * Ls + 2, None, None, SHIFT, EO_SHIFT))      # nc != 2 Ls
            refused(INVALID, entry, op=op, desc_=qmg.make_desc(16, 8, 2, None, None, SHIFT, EO_SHIFT), Ls=1)
            refused(INVALID, entry, op=op, desc_=qmg.make_desc(16, 8, 66, None, None, SHIFT, EO_SHIFT), Ls=33)
            refused(INVALID, entry, op=op, nrhs=17, stride=n, mask=0x1FFFF)
            refused(INVALID, entry, op=op, nrhs=2, stride=n - 2, mask=3)                                             # systems that overlap
            refused(INVALID, entry, op=op, dtype=2)
    # |kappa| >= |alpha_p| on a parity whose A is not inverted does not refuse (alpha_even = 3.5, alpha_odd = 0.5 - 1 + 1 = 0.5; kappa = -0.5 ...)
    lopsided = desc(dims, Ls, -0.5, 1.5)                               # alpha = 2.5: alpha_even = 3.5, alpha_odd = 0.5 = |kappa|
    flat = dict(w=1.0, M5=-1.0, b5=1.5, c5=0.5)
    assert qmg.mobius_inv5_status(qmg.C64, lopsided, Ls, M, D(l0), x, P.P_CLOVER_E, qmg.MOBIUS_S_AINV, SCALE, **flat) == 0
    assert qmg.mobius_hops_inv5_status(qmg.C64, lopsided, g, Ls, M, D(l0), x, P.P_EO, qmg.MOBIUS_S_AINV, qmg.MOBIUS_R_B, SCALE, 0, **flat) == 0
    assert qmg.mobius_hops_inv5_status(qmg.C64, lopsided, g, Ls, M, D(l0), x, P.P_OE, qmg.MOBIUS_S_ONE, qmg.MOBIUS_R_B, SCALE, 0, **flat) == 0   # S = 1 inverts nothing
    assert qmg.mobius_schur_apply_status(qmg.C64, lopsided, g, Ls, M, D(l0), x, t, 1, 0, **flat) == 0                  # parity 1 inverts A_even
    refused(UNSUPPORTED, "inv5", pieces=P.P_CLOVER_O, desc_=lopsided, **flat)
    refused(UNSUPPORTED, "hops", pieces=P.P_OE, desc_=lopsided, **flat)
    refused(UNSUPPORTED, "schur", desc_=lopsided, **flat)                                               # parity 0 inverts A_odd
    refused(UNSUPPORTED, "schur", desc_=lopsided, op=1, **flat)
    # the piece sets, tables and sources
    refused(UNSUPPORTED, "inv5", pieces=P.P_CLOVER | P.P_SHIFT)
    refused(UNSUPPORTED, "inv5", pieces=P.P_EO)
    refused(INVALID, "inv5", table=qmg.MOBIUS_S_ONE)
    refused(INVALID, "inv5", table=3)
    refused(UNSUPPORTED, "hops", pieces=P.P_EO | P.P_CLOVER_E | P.P_ZERO_E)                             # a clover bit
    refused(UNSUPPORTED, "hops", pieces=P.P_OE | P.P_SHIFT_O)                                           # a shift bit
    refused(UNSUPPORTED, "hops", pieces=P.P_EO_XP1 | P.P_ZERO_E)                                        # a partial hop set
    refused(UNSUPPORTED, "hops", pieces=P.P_HOPPING & ~(P.P_OE_XP1 << 3))
    refused(INVALID, "hops", table=-1)
    refused(INVALID, "hops", table=3)
    refused(INVALID, "hops", source=2)
    refused(INVALID, "hops", inplace=True)                                                              # both parities in place
    refused(INVALID, "hops", flags=qmg.DWF_G5_OUT)                                                      # no store flag
    refused(INVALID, "hops", scale=complex(0.0, nan))
    refused(INVALID, "inv5", scale=complex(inf, 0.0))
    refused(INVALID, "schur", inplace=True)
    refused(INVALID, "schur", alias="tmp=rhs")
    refused(INVALID, "schur", alias="tmp=lhs")
    refused(INVALID, "schur", parity=2)
    refused(INVALID, "schur", op=2)
    refused(INVALID, "schur", op=-1)
    # nothing active: success, nothing done
    lhs = D(l0)
    assert qmg.mobius_hops_inv5_status(qmg.C64, d, g, Ls, M, lhs, x, P.P_HOPPING | P.P_ZERO, nrhs=3, vec_stride=n, mask=0, **MOB) == 0
    assert qmg.mobius_inv5_status(qmg.C64, d, Ls, M, lhs, x, 0, **MOB) == 0
    assert qmg.mobius_schur_apply_status(qmg.C64, d, g, Ls, M, lhs, x, t, 0, 1, nrhs=3, vec_stride=n, mask=0, **MOB) == 0
    assert lhs.to_host().tobytes() == l0.tobytes()


# ---- the facade, through its driver
def run_driver(L, Ls, m, seed=7, solution=None):
    exe = os.path.join(qmg.HERE, "drivers", "mobius_eo_selftest")
    assert os.path.exists(exe), "drivers/mobius_eo_selftest is not built"
    cmd = [exe, str(L), str(Ls), str(m), str(seed)] + (["0", solution] if solution else [])
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    print(out.stdout)
    lines = {}
    for ln in out.stdout.splitlines():
        if ln.startswith("[QMG-MOBIUS-EO] "):
            _, name, value, verdict = ln.split()
            lines[name] = (float(value), verdict)
    assert out.returncode == 0, out.stdout
    return lines


@pytest.mark.parametrize("L,Ls", [(16, 8), (8, 6), (8, 32)])
def test_mobius_eo_selftest_driver(L, Ls):
    lines = run_driver(L, Ls, 0.05)
    expected = ["links_route_on", "schur_vs_D", "schur_adjointness", "eo_iterations", "eo_true_residual", "full_iterations", "full_true_residual", "eo_vs_full_solution"]
    assert sorted(lines) == sorted(expected)
    assert all(v == "PASS" for _, v in lines.values()), lines
    assert lines["schur_vs_D"][0] < 1e-13 and lines["schur_adjointness"][0] < 1e-12
    assert lines["eo_true_residual"][0] <= 1e-8
    assert 0 < lines["eo_iterations"][0] < lines["full_iterations"][0]
    assert lines["eo_vs_full_solution"][0] <= 1e-7


def test_minv_mobius_eo_cg_against_the_dense_solve(tmp_path):
    """the driver's even-odd solve at 4 x 4, Ls = 4, written out and held to numpy's dense solve of the same system.  The gate is ten times the
    distance the numpy CG on M^dagger M of tests/test_host_mobius_eo.py reaches at the same eps (5.658e-11 there: the gate is 6.0e-10)."""
    s = mn.SOLVE
    L, Ls = s["dims"][0], s["Ls"]
    nc = 2 * Ls
    path = str(tmp_path / "solution.bin")
    lines = run_driver(L, Ls, s["m"], 7, path)
    raw = np.fromfile(path, dtype=np.complex128)
    ng, n = 2 * L * L, L * L * nc
    assert raw.size == ng + 2 * n
    g, b, x = raw[:ng], raw[ng:ng + n], raw[ng + n:]
    Dm, *_ = mn.dense(L, L, Ls, g, s["m"], s["w"], s["M5"], s["b5"], s["c5"])
    bg = np.asarray(sn.to_grid(b, L, L, nc)).astype(np.complex128).reshape(-1)
    xg = np.asarray(sn.to_grid(x, L, L, nc)).astype(np.complex128).reshape(-1)
    x_dense = np.linalg.solve(Dm, bg)
    dist = float(np.linalg.norm(xg - x_dense) / np.linalg.norm(x_dense))
    print("minv_mobius_eo_cg: %d iterations, |x - x_dense| / |x_dense| = %.3e (gate %.1e)" % (lines["eo_iterations"][0], dist, 10 * me.SOLVE_REACH))
    assert dist <= 10 * me.SOLVE_REACH
