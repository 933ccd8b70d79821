"""CPU-side checks behind tests/test_gpu_mobius.py (no GPU: qmg_mobius_plan is host code and makes no HIP call).

1. The reference of the GPU tests is validated before any GPU run: mobius_numpy's grid statements of D and of D^dagger against a dense matrix
   built another way (Kronecker products), the Shamir limit against dwf_numpy, the operator identity the kernels use, and the guard that
   Gamma5 D Gamma5 is NOT D^dagger once c5 != 0.
2. A complex128 evaluation of the formulas stays inside the bound the GPU tests use, on every shape they use.
3. qmg_mobius_plan walked over ops, shapes and refusals.
4. A numpy CG on D^dagger D against the dense solve: the distance it reaches at eps fixes the gate of the GPU solve test.
"""
import importlib
import itertools

import numpy as np
import pytest

import dwf_numpy as dn
import mobius_numpy as mn
import stencil_numpy as sn

qmg = importlib.import_module("quantum-mg_amd")
P = qmg

LATTICES = [(2, 2), (4, 6), (130, 2), (16, 8)]      # the GPU tests' lattices
LS_STORED = [2, 3, 6, 8, 12]                        # ... and their Ls values; 32 for the links entry alone
LS_ALL = LS_STORED + [32]
BC = [(1.0, 0.0), (1.5, 0.5), (2.0, 1.0)]
M, M5 = 0.05 + 0.02j, -0.8
IDS = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)

SOLVE, SOLVE_REACH = mn.SOLVE, mn.SOLVE_REACH


@pytest.fixture(scope="module", autouse=True)
def _built():
    qmg.build()


def gauge(Lx, Ly, seed, width=0.4):
    return np.exp(1j * width * np.random.default_rng(seed).standard_normal(2 * Lx * Ly))


def cvec(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


# ---- 1. the reference
DENSE_SHAPES = [((2, 2), 2), ((2, 2), 3), ((2, 2), 8), ((4, 6), 2), ((4, 6), 3), ((16, 8), 2)]


@pytest.mark.parametrize("b5,c5", BC)
@pytest.mark.parametrize("dims,Ls", DENSE_SHAPES, ids=IDS)
def test_grid_forms_equal_the_dense_matrix(dims, Ls, b5, c5):
    Lx, Ly = dims
    g = gauge(Lx, Ly, 5)
    for w in (1.0, 0.9):
        Dm, A, B, H, G5 = mn.dense(Lx, Ly, Ls, g, M, w, M5, b5, c5)
        scale = np.max(np.abs(Dm))
        assert np.max(np.abs(mn.grid_operator(Lx, Ly, Ls, g, M, w, M5, b5, c5) - Dm)) <= 1e-14 * scale
        assert np.max(np.abs(mn.grid_operator(Lx, Ly, Ls, g, M, w, M5, b5, c5, dagger=True) - Dm.conj().T)) <= 1e-14 * scale
        assert np.max(np.abs(A @ B - B @ A)) <= 1e-14 * scale            # A and B commute


@pytest.mark.parametrize("dims,Ls", DENSE_SHAPES, ids=IDS)
def test_dagger_identity_and_the_gamma5_guard(dims, Ls):
    """D^dagger = Gamma5 (A' + B' H) Gamma5 with conj(m) in A', B' (for a real m: A, B themselves); Gamma5 D Gamma5 is D^dagger at c5 = 0
    and real m only -- a dagger built the Shamir way, from index flips, fails at c5 = 0.5"""
    Lx, Ly = dims
    g = gauge(Lx, Ly, 5)
    for m in (0.05, M):
        Dm, A, B, H, G5 = mn.dense(Lx, Ly, Ls, g, m, 1.0, M5, 1.5, 0.5)
        _, Ac, Bc, _, _ = mn.dense(Lx, Ly, Ls, g, np.conj(m), 1.0, M5, 1.5, 0.5)
        assert np.max(np.abs(G5 @ (Ac + Bc @ H) @ G5 - Dm.conj().T)) <= 1e-14 * np.max(np.abs(Dm))
        assert np.max(np.abs(G5 @ H @ G5 - H.conj().T)) <= 1e-15
    Dm, A, B, H, G5 = mn.dense(Lx, Ly, Ls, g, 0.05, 1.0, M5, 1.5, 0.5)
    assert np.max(np.abs(G5 @ Dm @ G5 - Dm.conj().T)) > 0.1            # B and H do not commute: of the order of c5 |H|
    Ds, *_ = mn.dense(Lx, Ly, Ls, g, 0.05, 1.0, M5, 1.0, 0.0)
    assert np.max(np.abs(G5 @ Ds @ G5 - Ds.conj().T)) <= 1e-15         # the Shamir limit keeps Gamma5-hermiticity


@pytest.mark.parametrize("dims,Ls", [((2, 2), 2), ((4, 6), 3), ((4, 6), 8), ((16, 8), 6), ((130, 2), 2)], ids=IDS)
def test_shamir_limit_is_dwf_numpy(dims, Ls):
    """b5 = 1, c5 = 0, w = 1: dwf_numpy's operator with shift = M5; at w != 1 the Shamir operator's diagonal is 3 w + M5 where this one has
    2 w + M5 + 1, so the descriptor's shift takes w - 1 on top"""
    Lx, Ly = dims
    nc = 2 * Ls
    g = gauge(Lx, Ly, 6)
    rhs, lhs0 = cvec(Lx * Ly * nc, 1), cvec(Lx * Ly * nc, 2)
    for w in (1.0, 0.9):
        for pieces in (P.P_ALL | P.P_ZERO, P.P_ALL):
            want, S, n = dn.apply(Lx, Ly, Ls, g, M, w, M5 + 0.011, 0.02j, 0.023, pieces, rhs, lhs0)
            got, S2, n2 = mn.apply(Lx, Ly, Ls, g, M, w, M5, 1.0, 0.0, 0.011 + (w - 1.0), 0.02j, 0.023, pieces, rhs, lhs0)
            assert np.all(np.abs(got - want) <= sn.elementwise_bound(S, n)), (w, hex(pieces))


GPU_SHAPES = [(dims, Ls) for dims in LATTICES for Ls in LS_ALL]


@pytest.mark.parametrize("dims,Ls", GPU_SHAPES, ids=IDS)
def test_complex128_evaluation_stays_inside_the_bound(dims, Ls):
    Lx, Ly = dims
    nc = 2 * Ls
    g = gauge(Lx, Ly, 11)
    rhs, lhs0 = cvec(Lx * Ly * nc, 1), cvec(Lx * Ly * nc, 2)
    shifts = (0.03j - 0.2, 0.011 - 0.02j, 0.023 + 0.01j)
    for (b5, c5), w, dagger in itertools.product(BC[1:], (1.0, 0.9), (False, True)):
        want, S, n = mn.apply(Lx, Ly, Ls, g, M, w, M5, b5, c5, *shifts, P.P_ALL, rhs, lhs0, dagger)
        got, _, _ = mn.apply(Lx, Ly, Ls, g, M, w, M5, b5, c5, *shifts, P.P_ALL, rhs, lhs0, dagger, ctype=np.complex128)
        err, bound = np.abs(got - want), sn.elementwise_bound(S, n)
        assert np.all(err <= bound), (b5, c5, w, dagger, float(np.max(err / bound)))
        assert np.all(n >= 40) and np.all(n <= 64)


@pytest.mark.parametrize("dims,Ls", [((2, 2), 2), ((4, 6), 3), ((16, 8), 6)], ids=IDS)
def test_stored_fields_reproduce_the_grid_formula(dims, Ls):
    """the twin of qmg_mobius_fill: its fields through the stored-stencil formula give D"""
    Lx, Ly = dims
    nc = 2 * Ls
    g = gauge(Lx, Ly, 6)
    shifts = (0.03j - 0.2, 0.011 - 0.02j, 0.023 + 0.01j)
    rhs, lhs0 = cvec(Lx * Ly * nc, 1), cvec(Lx * Ly * nc, 2)
    for (b5, c5), w in itertools.product(BC, (1.0, 0.9)):
        clover, hopping = mn.fields(Lx, Ly, Ls, g, M, w, M5, b5, c5)
        for pieces in (P.P_ALL | P.P_ZERO, P.P_ALL):
            want, S, n = mn.apply(Lx, Ly, Ls, g, M, w, M5, b5, c5, *shifts, pieces, rhs, lhs0)
            got, _, _ = sn.apply(Lx, Ly, nc, clover, hopping, *shifts, pieces, rhs, lhs0)
            assert np.all(np.abs(got - want) <= sn.elementwise_bound(S, n)), (b5, c5, w, hex(pieces))


# ---- 3. qmg_mobius_plan
SERVED = {P.P_ALL | P.P_ZERO: True, P.P_ALL: False, P.P_CLOVER | P.P_HOPPING | P.P_ZERO: True, P.P_CLOVER | P.P_HOPPING: False,
          P.P_ALL | P.P_ZERO_E: False, P.P_CLOVER | P.P_HOPPING | P.P_SHIFT_O | P.P_ZERO_O: False}       # piece set -> both parities overwritten
UNSUPPORTED = [
    P.P_CLOVER_E | P.P_EO | P.P_SHIFT_E | P.P_ZERO_E,     # one parity
    P.P_HOPPING | P.P_ZERO, P.P_EO | P.P_ZERO_E,           # hops alone
    P.P_EO_XP1 | P.P_ZERO_E,                               # a single direction
    P.P_ALL & ~(P.P_OE_XP1 << 3),                          # one hop missing
    P.P_CLOVER | P.P_ZERO, P.P_SHIFT | P.P_ZERO, P.P_ZERO, # clover, shift or clearing alone
]


def test_plan_ops_shapes_and_refusals():
    for dtype, Ls, dims, op in itertools.product((qmg.C64, qmg.C32), LS_ALL, LATTICES, (qmg.MOP_D, qmg.MOP_DAGGER)):
        Lx, Ly = dims
        lanes = Ls * (Lx // 2)
        for pieces, zero in SERVED.items():
            for n_active in (1, 3, 16):
                fam, lps, block, gx, gy, flags, lds, nk = qmg.mobius_plan(dtype, dims, Ls, op, pieces, n_active)
                tag = (dtype, Ls, dims, op, hex(pieces), n_active)
                assert fam == (qmg.MF_LOAD if op == qmg.MOP_D else qmg.MF_RESULT), tag
                assert (lps, nk) == (Ls, n_active), tag
                if op == qmg.MOP_D:
                    assert block == 256 and lds == 0, tag
                else:       # whole sites per block, two buffers of one chunk per lane of the largest block
                    assert block == Ls * (256 // Ls) and block % Ls == 0 and lds == 2 * 256 * (16 if dtype == qmg.C32 else 32) > 0, tag
                assert flags == (qmg.DPF_ZERO if zero else 0) | (qmg.DPF_BATCH if n_active > 1 else 0) | (qmg.DPF_F32 if dtype == qmg.C32 else 0), tag
                assert gx * block >= lanes > (gx - 1) * block and gy == 2 * Ly, tag
            assert qmg.mobius_plan(dtype, dims, Ls, op, pieces, 1, True)[0] == qmg.MF_INVALID      # lhs == rhs
        for pieces in UNSUPPORTED:
            for inplace in (False, True):
                assert qmg.mobius_plan(dtype, dims, Ls, op, pieces, 1, inplace)[0] == qmg.MF_UNSUPPORTED, (dtype, Ls, dims, op, hex(pieces), inplace)
        assert qmg.mobius_plan(dtype, dims, Ls, op, 0, 1)[0] == qmg.MF_NOTHING
        assert qmg.mobius_plan(dtype, dims, Ls, op, P.P_ALL | P.P_ZERO, 0)[0] == qmg.MF_NOTHING      # every system masked out
        assert qmg.mobius_plan(dtype, dims, Ls, op, P.P_ALL | P.P_ZERO, 17)[0] == qmg.MF_INVALID
        assert qmg.mobius_plan(dtype, dims, Ls, op, P.P_ALL | P.P_ZERO, -1)[0] == qmg.MF_INVALID


def test_plan_refuses_bad_arguments_before_the_piece_set_is_looked_at():
    for pieces in list(SERVED) + UNSUPPORTED + [0]:
        for Ls in (-1, 0, 1, 33, 64):
            assert qmg.mobius_plan(qmg.C64, (16, 8), Ls, 0, pieces)[0] == qmg.MF_INVALID, (Ls, hex(pieces))
        for dims in [(3, 4), (4, 5), (0, 2), (2, 0)]:
            assert qmg.mobius_plan(qmg.C64, dims, 8, 1, pieces)[0] == qmg.MF_INVALID, (dims, hex(pieces))
        for dtype in (-1, 2):
            assert qmg.mobius_plan(dtype, (16, 8), 8, 0, pieces)[0] == qmg.MF_INVALID, (dtype, hex(pieces))
        for op in (-1, 2):
            assert qmg.mobius_plan(qmg.C64, (16, 8), 8, op, pieces)[0] == qmg.MF_INVALID, (op, hex(pieces))


def test_plan_output_buffer_contract_and_the_cap_of_grid_y():
    import ctypes as C
    lib = qmg.lib()
    out = (C.c_int * 12)(*([7] * 12))
    assert lib.qmg_mobius_plan(qmg.C64, 16, 8, 8, 1, C.c_uint(P.P_ALL | P.P_ZERO), 1, 0, out, 12) == 0
    assert list(out[8:]) == [-1] * 4 and out[0] == qmg.MF_RESULT
    assert lib.qmg_mobius_plan(qmg.C64, 16, 8, 8, 1, C.c_uint(P.P_ALL | P.P_ZERO), 1, 0, out, 7) == 1
    assert lib.qmg_mobius_plan(qmg.C64, 16, 8, 8, 1, C.c_uint(P.P_ALL | P.P_ZERO), 1, 0, None, 8) == 1
    for op in (0, 1):       # 65540 rows: gy is capped and five blocks walk a second row
        fam, lps, block, gx, gy, *_ = qmg.mobius_plan(qmg.C64, (2, 32770), 2, op, P.P_ALL | P.P_ZERO)
        assert fam in (qmg.MF_LOAD, qmg.MF_RESULT) and gy == 65535 and gx == 1


# ---- 4. the solve
def solve_system():
    s = SOLVE
    Lx, Ly = s["dims"]
    g = gauge(Lx, Ly, s["gauge_seed"])
    b = cvec(Lx * Ly * 2 * s["Ls"], s["rhs_seed"])            # in the (eo, y, x, c) layout
    return g, b


def dense_solution(g, b):
    s = SOLVE
    Lx, Ly = s["dims"]
    nc = 2 * s["Ls"]
    Dm, *_ = mn.dense(Lx, Ly, s["Ls"], g, s["m"], s["w"], s["M5"], s["b5"], s["c5"])
    bg = np.asarray(sn.to_grid(b, Lx, Ly, nc)).astype(np.complex128).reshape(-1)
    return np.asarray(sn.to_eo(np.linalg.solve(Dm, bg).reshape(Lx, Ly, nc), Lx, Ly, nc)).astype(np.complex128), Dm


def test_numpy_cg_fixes_the_solve_gate():
    s = SOLVE
    Lx, Ly = s["dims"]
    g, b = solve_system()
    x_dense, Dm = dense_solution(g, b)
    print("condition number of D: %.1f" % np.linalg.cond(Dm))
    zero = np.zeros_like(b)
    ap = lambda dagger: (lambda v: np.asarray(mn.apply(Lx, Ly, s["Ls"], g, s["m"], s["w"], s["M5"], s["b5"], s["c5"], 0.0, 0.0, 0.0, P.P_ALL | P.P_ZERO, v, zero,
                                                       dagger, ctype=np.complex128)[0]))
    x, it = mn.cg_normal(ap(False), ap(True), b, s["eps"], 2000)
    reach = float(np.linalg.norm(x - x_dense) / np.linalg.norm(x_dense))
    print("numpy CG on D^dagger D: %d iterations, |x - x_dense| / |x_dense| = %.3e" % (it, reach))
    assert 0 < it < 2000
    assert reach <= SOLVE_REACH
