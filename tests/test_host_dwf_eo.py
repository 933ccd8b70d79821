"""CPU-side checks behind tests/test_gpu_dwf_eo.py (no GPU: qmg_dwf_eo_plan is host code and makes no HIP call).

1. dwf_eo_numpy, the reference of the GPU tests, against the dense operator of dwf_numpy.dense: A^-1 A = 1, M equals the dense Schur
   complement, Gamma5 M Gamma5 = M^dagger for real m, and prepare / solve / reconstruct reproduces D^-1 b.
2. The bound is reachable: A^-1 evaluated in complex128 by forward substitution with the wall correction and by the dense closed-form
   matrix -- the two algorithms a kernel could use -- stays inside stencil_numpy.elementwise_bound(S, n) against the long-double
   statement on every shape of the GPU tests, with n = n_hop + 2 Ls + 2.
3. qmg_dwf_eo_plan over dtype x Ls x lattice x kernel: the block is a multiple of Ls and at most 256, the grid covers the half row, the
   refusals, and plan_len handling.
"""
import importlib
import itertools

import numpy as np
import pytest

import dwf_eo_numpy as de
import dwf_numpy as dn
import stencil_numpy as sn

qmg = importlib.import_module("quantum-mg_amd")
P = qmg

LATTICES = [(2, 2), (4, 6), (130, 2), (16, 8)]
LS_ALL = [2, 3, 6, 8, 12, 32]
M, W, SHIFT, EO_SHIFT = 0.05 + 0.02j, 0.9, -1.0 + 0.03j, 0.011 - 0.02j
IDS = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.fixture(scope="module", autouse=True)
def _built():
    qmg.build()


def gauge(Lx, Ly, seed=11, width=0.4):
    return np.exp(1j * width * np.random.default_rng(seed).standard_normal(2 * Lx * Ly))


def cvec(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


# ---- 1. the reference against the dense operator
def grid_order(Lx, Ly, Ls):
    """perm with flat_eo[perm] = the grid ordering (x, y, s, sigma) of dwf_numpy.dense, and the parity of every grid element"""
    n = Lx * Ly * 2 * Ls
    perm = np.asarray(sn.to_grid(np.arange(n, dtype=np.float64), Lx, Ly, 2 * Ls)).real.astype(np.int64).reshape(-1)
    xs, ys = np.meshgrid(np.arange(Lx), np.arange(Ly), indexing="ij")
    par = np.repeat(((xs + ys) & 1).reshape(-1), 2 * Ls)
    return perm, par


@pytest.mark.parametrize("Ls", LS_ALL)
def test_gauss_jordan_inverse_and_the_closed_form(Ls):
    for p in (0, 1):
        A = de.a_blocks(Ls, de.diag(W, SHIFT, EO_SHIFT, p), M)
        B = de.inv_blocks(Ls, W, M, SHIFT, EO_SHIFT, p)
        C = de.closed_form_blocks(Ls, W, M, SHIFT, EO_SHIFT, p, np.clongdouble)
        for g in (0, 1):
            assert np.max(np.abs(B[g] @ A[g] - np.eye(Ls))) <= 1e-17
            assert np.max(np.abs(B[g] - C[g])) <= 1e-17
    # the clover block of the dense operator is A
    for M5 in (-1.0, -1.3):
        Dm, _ = dn.dense(2, 2, Ls, gauge(2, 2), 0.05, 1.0, M5)
        blk = Dm[:2 * Ls, :2 * Ls]
        A = de.a_blocks(Ls, de.diag(1.0, M5, 0.0, 0), 0.05, np.complex128)
        assert np.array_equal(blk[0::2, 0::2], A[0]) and np.array_equal(blk[1::2, 1::2], A[1]) and not np.any(blk[0::2, 1::2])


@pytest.mark.parametrize("dims,Ls", [((2, 2), 2), ((2, 2), 8), ((4, 6), 3), ((4, 6), 6), ((16, 8), 2)], ids=IDS)
def test_schur_complement_against_the_dense_operator(dims, Ls):
    Lx, Ly = dims
    n = Lx * Ly * 2 * Ls
    g = gauge(Lx, Ly, 5)
    m, w, M5 = 0.05, 1.0, -1.0
    Dm, G5 = dn.dense(Lx, Ly, Ls, g, m, w, M5)
    perm, par = grid_order(Lx, Ly, Ls)
    e, o = par == 0, par == 1
    Dee, Deo, Doe, Doo = Dm[np.ix_(e, e)], Dm[np.ix_(e, o)], Dm[np.ix_(o, e)], Dm[np.ix_(o, o)]
    Ms = Dee - Deo @ np.linalg.solve(Doo, Doe)
    x, y = cvec(n, 1), cvec(n, 2)
    zeros = np.zeros(n)
    to_grid = lambda v: np.asarray(v)[perm].astype(np.complex128)

    def schur(v, flags=0):
        out, S, cnt, t, _, _ = de.schur(Lx, Ly, Ls, g, m, w, M5, 0.0, 0, flags, v, zeros, zeros)
        return out, S, cnt

    out, S, cnt = schur(x)
    want = Ms @ x[perm][e]
    assert np.max(np.abs(to_grid(out)[e] - want)) <= 1e-13 * np.max(np.abs(want))
    assert not np.any(to_grid(out)[o])
    # Gamma5 M Gamma5 = M^dagger (real m and shifts): <y, G5 M G5 x> = <M y, x> on the even half
    g5, _, _ = schur(x, de.G5_IN | de.G5_OUT)
    My, _, _ = schur(y)
    lhs, rhs = np.vdot(to_grid(y)[e], to_grid(g5)[e]), np.vdot(to_grid(My)[e], to_grid(x)[e])
    assert abs(lhs - rhs) <= 1e-13 * abs(lhs)
    G5e = G5[np.ix_(e, e)]
    assert np.max(np.abs(G5e @ Ms @ G5e - Ms.conj().T)) <= 1e-14
    # prepare / solve / reconstruct reproduces D^-1 b
    b = cvec(n, 3)
    src, _, _ = de.inv5(Lx, Ly, Ls, m, w, M5, 0.0, P.P_CLOVER_O, 1.0, b, zeros)                       # A_oo^-1 b_o
    t, _, _ = dn.apply(Lx, Ly, Ls, g, m, w, M5, 0.0, 0.0, P.P_EO | P.P_ZERO_E, np.asarray(src), zeros)     # H_eo of that
    be = to_grid(b)[e] - to_grid(t)[e]
    be_dense = to_grid(b)[e] - Deo @ np.linalg.solve(Doo, to_grid(b)[o])
    ye = np.linalg.solve(Ms, be_dense)
    yfull = np.zeros(n, dtype=np.complex128)
    yfull_grid = np.zeros(n, dtype=np.complex128); yfull_grid[e] = ye
    yfull[perm] = yfull_grid
    # x_o = A^-1 (b_o - H_oe y_e) = A^-1 b_o - A^-1 H_oe y_e: kernel I and kernel K accumulating
    xo1, _, _ = de.inv5(Lx, Ly, Ls, m, w, M5, 0.0, P.P_CLOVER_O, 1.0, b, zeros)
    xo, _, _ = de.hops_inv5(Lx, Ly, Ls, g, m, w, M5, 0.0, P.P_OE, -1.0, 0, yfull, np.asarray(xo1))
    sol = to_grid(xo)
    sol[e] = ye
    assert np.max(np.abs(Dm @ sol - to_grid(b))) <= 1e-12 * np.max(np.abs(b))
    assert np.max(np.abs(be - be_dense)) <= 1e-13 * np.max(np.abs(be_dense))


# ---- 2. the bound is reachable by either algorithm in complex128
@pytest.mark.parametrize("dims", LATTICES, ids=IDS)
@pytest.mark.parametrize("Ls", LS_ALL)
def test_complex128_evaluations_stay_inside_the_bound(dims, Ls):
    Lx, Ly = dims
    n = Lx * Ly * 2 * Ls
    g, rhs, lhs0 = gauge(Lx, Ly), cvec(n, 1), cvec(n, 2)
    alpha = 0.7 - 0.4j
    par = de._parity(Lx, Ly)
    for pieces in (P.P_EO | P.P_ZERO_E, P.P_OE, P.P_HOPPING | P.P_ZERO_O):
        want, S, cnt = de.hops_inv5(Lx, Ly, Ls, g, M, W, SHIFT, EO_SHIFT, pieces, alpha, 0, rhs, lhs0)
        bound = sn.elementwise_bound(S, cnt)
        # the hop sum in complex128, as a kernel forms it
        Ux, Uy = dn.link_grids(g, Lx, Ly, np.complex128)
        x = de._grid(rhs, Lx, Ly, Ls, np.complex128)
        h, _, _ = dn._core(x, np.zeros_like(x), Ux, Uy, 0.0, W, 0.0, 0.0, 0.0, (pieces & P.P_HOPPING) | P.P_ZERO, np.complex128)
        l0 = de._grid(lhs0, Lx, Ly, Ls, np.complex128)
        for algorithm in ("forward", "dense"):
            got = l0.copy()
            for p in (0, 1):
                if not pieces & (P.P_EO, P.P_OE)[p]:
                    continue
                if algorithm == "forward":
                    y = de.forward_substitution(h, Ls, W, M, SHIFT, EO_SHIFT, p)
                else:
                    B = de.closed_form_blocks(Ls, W, M, SHIFT, EO_SHIFT, p)
                    y = np.stack([np.einsum("st,xyt->xys", B[s], h[:, :, :, s]) for s in (0, 1)], axis=-1)
                sel = par == p
                base = 0 if pieces & (P.P_ZERO_E << p) else got[sel]
                got[sel] = base + np.complex128(alpha) * y[sel]
            err = np.abs(de._flat(got, Lx, Ly, Ls).astype(sn.CLD) - want)
            worst = float(np.max(err / np.where(bound > 0, bound, 1)))
            assert np.all(err <= bound), (algorithm, hex(pieces), worst)


# ---- 3. qmg_dwf_eo_plan
EVEN2 = P.P_CLOVER_E | P.P_EO | P.P_SHIFT_E | P.P_ZERO_E
ODD2 = P.P_CLOVER_O | P.P_OE | P.P_SHIFT_O | P.P_ZERO_O
# kernel -> {pieces: (family, every processed parity overwritten, processed parities)}
SERVED = {
    qmg.DEK_INV5: {P.P_CLOVER_E: (qmg.DEF_INV5, True, 1), P.P_CLOVER_O: (qmg.DEF_INV5, True, 1), P.P_CLOVER: (qmg.DEF_INV5, True, 2)},
    qmg.DEK_HOPS_INV5: {P.P_EO | P.P_ZERO_E: (qmg.DEF_HOPS_INV5, True, 1), P.P_EO: (qmg.DEF_HOPS_INV5, False, 1), P.P_OE | P.P_ZERO_O: (qmg.DEF_HOPS_INV5, True, 1),
                        P.P_OE: (qmg.DEF_HOPS_INV5, False, 1), P.P_HOPPING | P.P_ZERO: (qmg.DEF_HOPS_INV5, True, 2), P.P_HOPPING: (qmg.DEF_HOPS_INV5, False, 2),
                        P.P_HOPPING | P.P_ZERO_E: (qmg.DEF_HOPS_INV5, False, 2)},
    qmg.DEK_SCHUR2: {EVEN2: (qmg.DEF_SCHUR2, True, 1), ODD2: (qmg.DEF_SCHUR2, True, 1)},
}
UNSUPPORTED = {
    qmg.DEK_INV5: [P.P_CLOVER_E | P.P_ZERO_E, P.P_CLOVER | P.P_SHIFT, P.P_EO, P.P_ALL],
    qmg.DEK_HOPS_INV5: [P.P_EO | P.P_CLOVER_E, P.P_OE | P.P_SHIFT_O, P.P_EO_XP1 | P.P_ZERO_E, P.P_HOPPING & ~(P.P_OE_XP1 << 3), P.P_ZERO_E, P.P_EO | P.P_ZERO_O, P.P_ALL],
    qmg.DEK_SCHUR2: [EVEN2 | ODD2, EVEN2 & ~P.P_ZERO_E, P.P_EO | P.P_ZERO_E, P.P_CLOVER_E],
}


def test_plan_grid_served_unsupported_invalid():
    for dtype, Ls, dims in itertools.product((qmg.C64, qmg.C32), LS_ALL + [4, 5, 7, 31], LATTICES):
        Lx, Ly = dims
        lanes = Ls * (Lx // 2)
        for kernel, table in SERVED.items():
            for pieces, (family, zero, npar) in table.items():
                for n_active, inplace in ((1, False), (3, False), (16, False), (1, True)):
                    fam, lps, block, gx, gy, flags, lds, nk = qmg.dwf_eo_plan(dtype, dims, Ls, kernel, pieces, n_active, inplace)
                    tag = (dtype, Ls, dims, kernel, hex(pieces), n_active, inplace)
                    if inplace and (kernel == qmg.DEK_SCHUR2 or (kernel == qmg.DEK_HOPS_INV5 and npar == 2)):
                        assert fam == qmg.DEF_INVALID, tag
                        continue
                    assert (fam, lps, nk) == (family, Ls, n_active), tag
                    # a site's Ls lanes never straddle a block; the blocks cover the half row with none of them idle
                    assert block % Ls == 0 and 256 - Ls < block <= 256, tag
                    assert gx * block >= lanes > (gx - 1) * block and gy == Ly * npar, tag
                    assert flags == (qmg.DPF_ZERO if zero else 0) | (qmg.DPF_BATCH if n_active > 1 else 0) | (qmg.DPF_F32 if dtype == qmg.C32 else 0), tag
                    # two buffers of one chunk per lane of the largest block; none for the second stage
                    assert lds == (0 if kernel == qmg.DEK_SCHUR2 else 2 * 256 * (16 if dtype == qmg.C32 else 32)), tag
            for pieces in UNSUPPORTED[kernel]:
                for inplace in (False, True):
                    assert qmg.dwf_eo_plan(dtype, dims, Ls, kernel, pieces, 1, inplace)[0] == qmg.DEF_UNSUPPORTED, (dtype, Ls, dims, kernel, hex(pieces), inplace)
            some = next(iter(table))
            assert qmg.dwf_eo_plan(dtype, dims, Ls, kernel, 0, 1)[0] == qmg.DEF_NOTHING
            assert qmg.dwf_eo_plan(dtype, dims, Ls, kernel, some, 0)[0] == qmg.DEF_NOTHING      # every system masked out
            assert qmg.dwf_eo_plan(dtype, dims, Ls, kernel, some, 17)[0] == qmg.DEF_INVALID
            assert qmg.dwf_eo_plan(dtype, dims, Ls, kernel, some, -1)[0] == qmg.DEF_INVALID


def test_plan_refuses_bad_arguments_before_the_piece_set_is_looked_at():
    for kernel, table in SERVED.items():
        for pieces in list(table) + UNSUPPORTED[kernel] + [0]:
            for Ls in (-1, 0, 1, 33, 64):
                assert qmg.dwf_eo_plan(qmg.C64, (16, 8), Ls, kernel, pieces)[0] == qmg.DEF_INVALID, (Ls, hex(pieces))
            for dims in [(3, 4), (4, 5), (0, 2), (2, 0)]:
                assert qmg.dwf_eo_plan(qmg.C64, dims, 8, kernel, pieces)[0] == qmg.DEF_INVALID, (dims, hex(pieces))
            for dtype in (-1, 2):
                assert qmg.dwf_eo_plan(dtype, (16, 8), 8, kernel, pieces)[0] == qmg.DEF_INVALID, (dtype, hex(pieces))
    for kernel in (-1, 3):
        assert qmg.dwf_eo_plan(qmg.C64, (16, 8), 8, kernel, P.P_EO)[0] == qmg.DEF_INVALID


def test_plan_output_buffer_contract_and_row_walk():
    import ctypes as C
    lib = qmg.lib()
    out = (C.c_int * 12)(*([7] * 12))
    assert lib.qmg_dwf_eo_plan(qmg.C64, 16, 8, 6, qmg.DEK_HOPS_INV5, C.c_uint(P.P_EO | P.P_ZERO_E), 1, 0, out, 12) == 0
    assert list(out[8:]) == [-1] * 4 and list(out[:5]) == [qmg.DEF_HOPS_INV5, 6, 252, 1, 8]
    assert lib.qmg_dwf_eo_plan(qmg.C64, 16, 8, 6, qmg.DEK_HOPS_INV5, C.c_uint(P.P_EO), 1, 0, out, 7) == 1
    assert lib.qmg_dwf_eo_plan(qmg.C64, 16, 8, 6, qmg.DEK_HOPS_INV5, C.c_uint(P.P_EO), 1, 0, None, 8) == 1
    # more rows than grid.y can hold: gy is capped and the blocks walk the rest
    fam, lps, block, gx, gy, *_ = qmg.dwf_eo_plan(qmg.C64, (4, 40000), 2, qmg.DEK_HOPS_INV5, P.P_HOPPING | P.P_ZERO)
    assert fam == qmg.DEF_HOPS_INV5 and gy == 65535
