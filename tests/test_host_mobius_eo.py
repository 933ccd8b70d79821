"""CPU-side checks behind tests/test_gpu_mobius_eo.py (no GPU: qmg_mobius_eo_plan is host code and makes no HIP call).

1. The reference of the GPU tests is validated before any GPU run: mobius_eo_numpy's M against the dense Schur complement of
   mobius_numpy.dense, its M^dagger against the conjugate transpose, the guard that Gamma5 M Gamma5 is NOT M^dagger once c5 != 0, and
   prepare / solve / reconstruct against D^-1 b.
2. The twisted-circulant tables the kernels take, evaluated in complex128, stay inside the bound the GPU tests use, on every shape they
   use; in long double they are the Gauss-Jordan inverse.
3. qmg_mobius_eo_plan walked over kernels, shapes and refusals.
4. A numpy CG on M^dagger M against the dense solve: the distance it reaches at eps fixes the gate of the GPU solve test.
"""
import importlib
import itertools

import numpy as np
import pytest

import dwf_eo_numpy as de
import mobius_eo_numpy as me
import mobius_numpy as mn
import stencil_numpy as sn

qmg = importlib.import_module("quantum-mg_amd")
P = qmg

LATTICES = [(2, 2), (4, 6), (130, 2), (16, 8)]      # the GPU tests' lattices ...
LS_ALL = [2, 3, 6, 8, 12, 32]                       # ... and their Ls values
M, W, M5 = 0.05 + 0.02j, 0.9, -0.8
SHIFT, EO_SHIFT = 0.03j - 0.2, 0.011 - 0.02j
IDS = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)
CLD = np.clongdouble


@pytest.fixture(scope="module", autouse=True)
def _built():
    qmg.build()


def gauge(Lx, Ly, seed, width=0.4):
    return np.exp(1j * width * np.random.default_rng(seed).standard_normal(2 * Lx * Ly))


def cvec(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


# ---- 1. the reference
def site_parity(Lx, Ly, nc):
    """the parity of every row of a dense matrix over the grid ordering (x, y, s, sigma)"""
    xs, ys = np.meshgrid(np.arange(Lx), np.arange(Ly), indexing="ij")
    return np.repeat(((xs + ys) & 1).reshape(-1), nc)


def dense_with_shifts(Lx, Ly, Ls, g, m, w, b5, c5, shift, eo_shift):
    Dm, A, B, H, G5 = mn.dense(Lx, Ly, Ls, g, m, w, M5, b5, c5)
    par = site_parity(Lx, Ly, 2 * Ls)
    return Dm + np.diag(shift + np.where(par == 0, 1.0, -1.0) * eo_shift), G5, par


def dense_schur(Dm, par, p):
    e, o = np.flatnonzero(par == p), np.flatnonzero(par != p)
    return Dm[np.ix_(e, e)] - Dm[np.ix_(e, o)] @ np.linalg.solve(Dm[np.ix_(o, o)], Dm[np.ix_(o, e)]), e


def twin_matrix(Lx, Ly, Ls, g, m, w, b5, c5, shift, eo_shift, p, op, rows):
    """the twin's M_p (op 0) or M_p^dagger (op 1) as a complex128 matrix over the sites `rows` of the grid ordering"""
    nc = 2 * Ls
    N = Lx * Ly * nc
    zero = np.zeros(N, dtype=CLD)
    cols = []
    for i in rows:
        e = np.zeros(N, dtype=CLD)
        e[i] = 1
        flat = np.asarray(sn.to_eo(e.reshape(Lx, Ly, nc), Lx, Ly, nc))
        out = me.schur(Lx, Ly, Ls, g, m, w, M5, b5, c5, shift, eo_shift, p, op, flat, zero, zero)[0]
        cols.append(np.asarray(sn.to_grid(out, Lx, Ly, nc)).reshape(-1)[rows])
    return np.array(cols).T.astype(np.complex128)


DENSE_SHAPES = [((2, 2), 2), ((2, 2), 3), ((4, 4), 4), ((4, 6), 3), ((6, 4), 2)]
BC = [(1.5, 0.5), (2.0, 1.0), (1.0, 0.0)]


@pytest.mark.parametrize("b5,c5", BC)
@pytest.mark.parametrize("dims,Ls", DENSE_SHAPES, ids=IDS)
def test_twin_schur_equals_the_dense_schur_complement_and_its_dagger(dims, Ls, b5, c5):
    Lx, Ly = dims
    g = gauge(Lx, Ly, 5)
    for p in (0, 1):
        Dm, G5, par = dense_with_shifts(Lx, Ly, Ls, g, M, W, b5, c5, SHIFT, EO_SHIFT)
        Md, rows = dense_schur(Dm, par, p)
        scale = np.max(np.abs(Md))
        got = twin_matrix(Lx, Ly, Ls, g, M, W, b5, c5, SHIFT, EO_SHIFT, p, 0, rows)
        assert np.max(np.abs(got - Md)) <= 1e-14 * scale, (p, float(np.max(np.abs(got - Md))))
        got_dag = twin_matrix(Lx, Ly, Ls, g, M, W, b5, c5, SHIFT, EO_SHIFT, p, 1, rows)
        assert np.max(np.abs(got_dag - Md.conj().T)) <= 1e-14 * scale, (p, float(np.max(np.abs(got_dag - Md.conj().T))))


@pytest.mark.parametrize("dims,Ls", DENSE_SHAPES, ids=IDS)
def test_gamma5_M_gamma5_is_not_M_dagger(dims, Ls):
    """the Shamir trick of the even-odd domain-wall kernels does not carry over: B stands on the other side of H"""
    Lx, Ly = dims
    g = gauge(Lx, Ly, 5)
    Dm, G5, par = dense_with_shifts(Lx, Ly, Ls, g, 0.05, 1.0, 1.5, 0.5, 0.0, 0.0)
    Md, rows = dense_schur(Dm, par, 0)
    G = G5[np.ix_(rows, rows)]
    gap = float(np.max(np.abs(G @ Md @ G - Md.conj().T)))
    print("|Gamma5 M Gamma5 - M^dagger| at b5 = 1.5, c5 = 0.5: %.3f" % gap)
    assert gap > 0.1
    Ds, G5, par = dense_with_shifts(Lx, Ly, Ls, g, 0.05, 1.0, 1.0, 0.0, 0.0, 0.0)
    Ms, rows = dense_schur(Ds, par, 0)
    assert np.max(np.abs(G @ Ms @ G - Ms.conj().T)) <= 1e-14        # the Shamir limit keeps Gamma5-hermiticity


@pytest.mark.parametrize("dims,Ls", [((2, 2), 3), ((4, 4), 4), ((4, 6), 2)], ids=IDS)
def test_prepare_solve_reconstruct_is_the_full_solve(dims, Ls):
    Lx, Ly = dims
    nc = 2 * Ls
    g = gauge(Lx, Ly, 7)
    b = cvec(Lx * Ly * nc, 3)
    Dm, G5, par = dense_with_shifts(Lx, Ly, Ls, g, M, W, 1.5, 0.5, SHIFT, EO_SHIFT)
    x_dense = np.linalg.solve(Dm, np.asarray(sn.to_grid(b, Lx, Ly, nc)).astype(np.complex128).reshape(-1))
    Mop, Mdag, prepare, reconstruct = me.full_ops(Lx, Ly, Ls, g, M, W, M5, 1.5, 0.5, SHIFT, EO_SHIFT)
    bp = np.asarray(prepare(b))
    Md, rows = dense_schur(Dm, par, 0)
    xe_grid = np.zeros(Lx * Ly * nc, dtype=np.complex128)
    xe_grid[rows] = np.linalg.solve(Md, np.asarray(sn.to_grid(bp, Lx, Ly, nc)).astype(np.complex128).reshape(-1)[rows])
    xe = np.asarray(sn.to_eo(xe_grid.reshape(Lx, Ly, nc), Lx, Ly, nc))
    x = np.asarray(sn.to_grid(reconstruct(xe, b), Lx, Ly, nc)).astype(np.complex128).reshape(-1)
    assert np.linalg.norm(x - x_dense) <= 1e-13 * np.linalg.norm(x_dense)


# ---- 2. the tables
GPU_SHAPES = [(dims, Ls) for dims in LATTICES for Ls in LS_ALL]
GPU_PARAMS = dict(m=M, w=W, M5=M5, b5=1.5, c5=0.5, shift=SHIFT, eo_shift=EO_SHIFT)      # tests/test_gpu_mobius_eo.py's


@pytest.mark.parametrize("Ls", [3, 6, 8, 32])
def test_closed_form_tables_are_the_gauss_jordan_inverse(Ls):
    q = GPU_PARAMS
    for p, table in itertools.product((0, 1), (me.S_AINV, me.S_AINV_B)):
        want = me.table_blocks(Ls, table, q["m"], q["w"], q["M5"], q["b5"], q["c5"], q["shift"], q["eo_shift"], p)
        f = me.closed_form_table(Ls, table, q["m"], q["w"], q["M5"], q["b5"], q["c5"], q["shift"], q["eo_shift"], p, ctype=CLD)
        got = me.circulant_blocks(f, q["m"])
        for g in (0, 1):
            assert np.max(np.abs(got[g] - want[g])) <= 1e-17 * Ls * np.max(np.abs(want[g])), (Ls, p, table, g)


@pytest.mark.parametrize("dims,Ls", GPU_SHAPES, ids=IDS)
def test_complex128_tables_stay_inside_the_bound(dims, Ls):
    Lx, Ly = dims
    q = GPU_PARAMS
    rhs, lhs0 = cvec(Lx * Ly * 2 * Ls, 1), cvec(Lx * Ly * 2 * Ls, 2)
    scale = 0.7 - 0.4j
    par = de._parity(Lx, Ly)
    h = de._grid(rhs, Lx, Ly, Ls).astype(np.complex128)
    for table in (me.S_AINV, me.S_AINV_B):
        want, S, n = me.inv5(Lx, Ly, Ls, q["m"], q["w"], q["M5"], q["b5"], q["c5"], q["shift"], q["eo_shift"], P.P_CLOVER, table, scale, rhs, lhs0)
        got = np.empty_like(h)
        for p in (0, 1):
            f = me.closed_form_table(Ls, table, q["m"], q["w"], q["M5"], q["b5"], q["c5"], q["shift"], q["eo_shift"], p)
            C = me.circulant_blocks(f, q["m"])
            for g in (0, 1):
                y = scale * np.einsum("st,xyt->xys", C[g], h[:, :, :, g])
                got[:, :, :, g] = np.where((par == p)[:, :, None], y, got[:, :, :, g])
        err, bound = np.abs(de._flat(got, Lx, Ly, Ls) - want), sn.elementwise_bound(S, n)
        assert np.all(err <= bound), (table, float(np.max(err / bound)))
        assert np.all(n == 2 * Ls + 2)


# ---- 3. qmg_mobius_eo_plan
E_FULL, O_FULL = P.P_CLOVER_E | P.P_EO | P.P_SHIFT_E | P.P_ZERO_E, P.P_CLOVER_O | P.P_OE | P.P_SHIFT_O | P.P_ZERO_O
HOP_SETS = {P.P_EO | P.P_ZERO_E: (1, True), P.P_EO: (1, False), P.P_OE | P.P_ZERO_O: (1, True), P.P_OE: (1, False), P.P_HOPPING | P.P_ZERO: (2, True),
            P.P_HOPPING: (2, False), P.P_HOPPING | P.P_ZERO_E: (2, False)}            # piece set -> (parities, every one overwritten)


def test_plan_kernels_shapes_and_refusals():
    for dtype, Ls, dims in itertools.product((qmg.C64, qmg.C32), LS_ALL, LATTICES):
        Lx, Ly = dims
        lanes = Ls * (Lx // 2)
        f32 = qmg.DPF_F32 if dtype == qmg.C32 else 0
        lds_bytes = 2 * 256 * (16 if dtype == qmg.C32 else 32)

        def held(plan, family, block, rows, flags, lds, n_active, tag):
            fam, lps, bl, gx, gy, fl, ld, nk = plan
            assert (fam, lps, bl, nk, ld) == (family, Ls, block, n_active, lds), (tag, plan)
            assert fl == flags | (qmg.DPF_BATCH if n_active > 1 else 0) | f32, (tag, plan)
            assert gx * bl >= lanes > (gx - 1) * bl and gy == rows and bl % Ls == (0 if lds else bl % Ls), (tag, plan)

        whole = Ls * (256 // Ls)
        for n_active in (1, 3, 16):
            for table in (qmg.MOBIUS_S_AINV, qmg.MOBIUS_S_AINV_B):
                for pieces, npar in ((P.P_CLOVER_E, 1), (P.P_CLOVER_O, 1), (P.P_CLOVER, 2)):
                    held(qmg.mobius_eo_plan(dtype, dims, Ls, qmg.MEK_INV5, pieces, table, 0, n_active), qmg.MEF_MIX, whole, npar * Ly, qmg.DPF_ZERO, lds_bytes,
                         n_active, ("inv5", hex(pieces)))
                    assert qmg.mobius_eo_plan(dtype, dims, Ls, qmg.MEK_INV5, pieces, table, 0, n_active, True)[0] == qmg.MEF_MIX      # in place
            for table, source in itertools.product(range(3), range(2)):
                for pieces, (npar, zero) in HOP_SETS.items():
                    held(qmg.mobius_eo_plan(dtype, dims, Ls, qmg.MEK_HOPS_INV5, pieces, table, source, n_active), qmg.MEF_HOPS_MIX, whole, npar * Ly,
                         (qmg.DPF_ZERO if zero else 0) | (qmg.MEPF_RMIX if source else 0), lds_bytes, n_active, ("hops", hex(pieces), table, source))
                    fam = qmg.mobius_eo_plan(dtype, dims, Ls, qmg.MEK_HOPS_INV5, pieces, table, source, n_active, True)[0]
                    assert fam == (qmg.MEF_HOPS_MIX if npar == 1 else qmg.MEF_INVALID)
            for pieces in (E_FULL, O_FULL):
                held(qmg.mobius_eo_plan(dtype, dims, Ls, qmg.MEK_SCHUR2, pieces, 0, 0, n_active), qmg.MEF_SCHUR2, 256, Ly, qmg.DPF_ZERO, 0, n_active, "schur2")
                held(qmg.mobius_eo_plan(dtype, dims, Ls, qmg.MEK_SCHUR2_DAGGER, pieces, 0, 0, n_active), qmg.MEF_SCHUR2_DAGGER, whole, Ly, qmg.DPF_ZERO, lds_bytes,
                     n_active, "schur2 dagger")
                for kernel in (qmg.MEK_SCHUR2, qmg.MEK_SCHUR2_DAGGER):
                    assert qmg.mobius_eo_plan(dtype, dims, Ls, kernel, pieces, 0, 0, n_active, True)[0] == qmg.MEF_INVALID
        # the piece sets
        for pieces in (P.P_CLOVER | P.P_SHIFT, P.P_EO, P.P_CLOVER_E | P.P_ZERO_E):
            assert qmg.mobius_eo_plan(dtype, dims, Ls, qmg.MEK_INV5, pieces)[0] == qmg.MEF_UNSUPPORTED, hex(pieces)
        for pieces in (P.P_EO | P.P_CLOVER_E | P.P_ZERO_E, P.P_OE | P.P_SHIFT_O, P.P_EO_XP1 | P.P_ZERO_E, P.P_HOPPING & ~(P.P_OE_XP1 << 3)):
            assert qmg.mobius_eo_plan(dtype, dims, Ls, qmg.MEK_HOPS_INV5, pieces)[0] == qmg.MEF_UNSUPPORTED, hex(pieces)
        for pieces in (E_FULL | O_FULL, E_FULL & ~P.P_ZERO_E, E_FULL & ~P.P_SHIFT_E, P.P_EO | P.P_ZERO_E, P.P_ALL | P.P_ZERO):
            for kernel in (qmg.MEK_SCHUR2, qmg.MEK_SCHUR2_DAGGER):
                assert qmg.mobius_eo_plan(dtype, dims, Ls, kernel, pieces)[0] == qmg.MEF_UNSUPPORTED, hex(pieces)
        for kernel in range(4):
            assert qmg.mobius_eo_plan(dtype, dims, Ls, kernel, 0)[0] == qmg.MEF_NOTHING
            assert qmg.mobius_eo_plan(dtype, dims, Ls, kernel, E_FULL, 1, 0, 0)[0] == qmg.MEF_NOTHING      # every system masked out
            assert qmg.mobius_eo_plan(dtype, dims, Ls, kernel, E_FULL, 1, 0, 17)[0] == qmg.MEF_INVALID
            assert qmg.mobius_eo_plan(dtype, dims, Ls, kernel, E_FULL, 1, 0, -1)[0] == qmg.MEF_INVALID


def test_plan_refuses_bad_arguments_before_the_piece_set_is_looked_at():
    for pieces in (P.P_CLOVER, P.P_HOPPING | P.P_ZERO, E_FULL, P.P_ALL, 0):
        for kernel in range(4):
            for Ls in (-1, 0, 1, 33, 64):
                assert qmg.mobius_eo_plan(qmg.C64, (16, 8), Ls, kernel, pieces)[0] == qmg.MEF_INVALID, (Ls, hex(pieces))
            for dims in [(3, 4), (4, 5), (0, 2), (2, 0)]:
                assert qmg.mobius_eo_plan(qmg.C64, dims, 8, kernel, pieces)[0] == qmg.MEF_INVALID, (dims, hex(pieces))
            for dtype in (-1, 2):
                assert qmg.mobius_eo_plan(dtype, (16, 8), 8, kernel, pieces)[0] == qmg.MEF_INVALID, (dtype, hex(pieces))
        for kernel in (-1, 4):
            assert qmg.mobius_eo_plan(qmg.C64, (16, 8), 8, kernel, pieces)[0] == qmg.MEF_INVALID
        for table in (-1, 0, 3):            # qmg_mobius_inv5 has no S = 1
            assert qmg.mobius_eo_plan(qmg.C64, (16, 8), 8, qmg.MEK_INV5, pieces, table)[0] == qmg.MEF_INVALID
        for table, source in ((-1, 0), (3, 0), (1, -1), (1, 2)):
            assert qmg.mobius_eo_plan(qmg.C64, (16, 8), 8, qmg.MEK_HOPS_INV5, pieces, table, source)[0] == qmg.MEF_INVALID


def test_plan_output_buffer_contract_and_the_cap_of_grid_y():
    import ctypes as C
    lib = qmg.lib()
    out = (C.c_int * 12)(*([7] * 12))
    assert lib.qmg_mobius_eo_plan(qmg.C64, 16, 8, 8, 1, C.c_uint(P.P_HOPPING | P.P_ZERO), 1, 1, 1, 0, out, 12) == 0
    assert list(out[8:]) == [-1] * 4 and out[0] == qmg.MEF_HOPS_MIX
    assert lib.qmg_mobius_eo_plan(qmg.C64, 16, 8, 8, 1, C.c_uint(P.P_HOPPING | P.P_ZERO), 1, 1, 1, 0, out, 7) == 1
    assert lib.qmg_mobius_eo_plan(qmg.C64, 16, 8, 8, 1, C.c_uint(P.P_HOPPING | P.P_ZERO), 1, 1, 1, 0, None, 8) == 1
    # 65540 rows: gy is capped and five blocks walk a second row, in every kernel
    for kernel, pieces, dims in ((qmg.MEK_INV5, P.P_CLOVER, (2, 32770)), (qmg.MEK_HOPS_INV5, P.P_HOPPING, (2, 32770)), (qmg.MEK_INV5, P.P_CLOVER_O, (2, 65540)),
                                 (qmg.MEK_HOPS_INV5, P.P_EO | P.P_ZERO_E, (2, 65540)), (qmg.MEK_SCHUR2, O_FULL, (2, 65540)), (qmg.MEK_SCHUR2_DAGGER, O_FULL, (2, 65540))):
        fam, lps, block, gx, gy, *_ = qmg.mobius_eo_plan(qmg.C64, dims, 2, kernel, pieces, 1, 1)
        assert fam not in (qmg.MEF_UNSUPPORTED, qmg.MEF_INVALID, qmg.MEF_NOTHING) and gy == 65535 and gx == 1, (kernel, fam, gy, gx)


# ---- 4. the solve
def test_numpy_cg_on_the_schur_complement_fixes_the_solve_gate():
    s = mn.SOLVE
    Lx, Ly = s["dims"]
    Ls, nc = s["Ls"], 2 * s["Ls"]
    g = gauge(Lx, Ly, s["gauge_seed"])
    b = cvec(Lx * Ly * nc, s["rhs_seed"])
    Dm, *_ = mn.dense(Lx, Ly, Ls, g, s["m"], s["w"], s["M5"], s["b5"], s["c5"])
    x_dense = np.asarray(sn.to_eo(np.linalg.solve(Dm, np.asarray(sn.to_grid(b, Lx, Ly, nc)).astype(np.complex128).reshape(-1)).reshape(Lx, Ly, nc), Lx, Ly, nc))
    Mop, Mdag, prepare, reconstruct = me.full_ops(Lx, Ly, Ls, g, s["m"], s["w"], s["M5"], s["b5"], s["c5"])
    c128 = lambda f: (lambda v: np.asarray(f(v)).astype(np.complex128))
    bp = c128(prepare)(b)
    bp[bp.size // 2:] = 0                                   # the system is the even half
    xe, it = mn.cg_normal(c128(Mop), c128(Mdag), bp, s["eps"], 2000)
    x = np.asarray(reconstruct(xe, b)).astype(np.complex128)
    reach = float(np.linalg.norm(x - x_dense) / np.linalg.norm(x_dense))
    print("numpy CG on M^dagger M: %d iterations (63 on D^dagger D), |x - x_dense| / |x_dense| = %.3e" % (it, reach))
    assert 0 < it < 63                                      # fewer than the full operator's (tests/mobius_numpy.py)
    assert reach <= me.SOLVE_REACH
