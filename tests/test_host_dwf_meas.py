"""CPU-side checks behind tests/test_gpu_dwf_meas.py (no GPU: qmg_dwf_meas_plan is host code and makes no HIP call).

1. dwf_meas_numpy's conventions against the dense operator of dwf_numpy.dense: the integrated axial Ward identity
   m |q|^2 + |q_mp|^2 = Re <eta, q> holds to rounding for Psi = D^-1 B on every gauge field; its residual-aware form
   lhs - rhs = -Re <Psi~, Gamma5 E r> (r = B - D Psi~, E = +1 for s < Ls/2, -1 otherwise) holds for a perturbed solution, so
   |defect| <= |Psi~| |r|; the other midpoint pairing and an odd Ls fail it by far more than rounding.
2. qmg_dwf_meas_plan over dtype x Ls x lattice x kernel: the block of the norms is a multiple of Ls, its partial blocks stride over the
   half row, the grids cover the lanes, the refusals, and plan_len handling.
3. The four symbols are declared, bound and exported.
"""
import importlib
import itertools

import numpy as np
import pytest

import dwf_meas_numpy as dm
import dwf_numpy as dn

qmg = importlib.import_module("quantum-mg_amd")

CASES = [((4, 6), 4), ((2, 2), 2), ((6, 4), 8), ((8, 8), 6)]
LATTICES = [(2, 2), (4, 6), (130, 2), (16, 8)]
LS_ALL = [2, 3, 6, 8, 12, 32]
M, W, M5 = 0.05, 1.0, -1.0
IDS = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.fixture(scope="module", autouse=True)
def _built():
    qmg.build()


def gauge(Lx, Ly, seed=11, width=0.4):
    return np.exp(1j * width * np.random.default_rng(seed).standard_normal(2 * Lx * Ly))


def cgrid(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def solved(dims, Ls, seed=3):
    """(D, Gamma5, eta[x, y, sigma], B, Psi = D^-1 B on the grid)"""
    Lx, Ly = dims
    Dm, G5 = dn.dense(Lx, Ly, Ls, gauge(Lx, Ly, 5), M, W, M5)
    eta = cgrid((Lx, Ly, 2), seed)
    B = dm.source_grid(eta, Ls)
    psi = np.linalg.solve(Dm, B.reshape(-1)).reshape(B.shape)
    return Dm, G5, eta, B, psi


# ---- 1. the conventions against the dense operator
@pytest.mark.parametrize("dims,Ls", CASES, ids=IDS)
def test_ward_identity_on_the_dense_operator(dims, Ls):
    Dm, G5, eta, B, psi = solved(dims, Ls)
    lhs, rhs = dm.ward_grid(eta, psi, M)
    print("ward %s Ls=%d lhs %.17g rhs %.17g rel %.2e" % (dims, Ls, lhs, rhs, abs(lhs - rhs) / abs(lhs)))
    assert abs(lhs - rhs) <= 1e-13 * abs(lhs)
    # the source sits on the walls opposite to the ones the projection reads (sigma 0: slice 0 against Ls-1): reflected in s it comes back
    assert np.array_equal(dm.project_grid(B[:, :, ::-1], "wall"), eta) and not np.any(dm.project_grid(B, "wall"))
    # the other pairing is not the midpoint
    wl, wr = dm.ward_grid(eta, psi, M, mid="wrong")
    print("wrong pairing rel defect %.3f" % (abs(wl - wr) / abs(wl)))
    # 1e-6: ten million times the level to which the right pairing holds; the defect is |q_wrong|^2 - |q_mp|^2, which shrinks with the
    # midpoint term itself as Ls grows (at Ls = 2 the other pairing is the walls themselves)
    assert abs(wl - wr) > 1e-6 * abs(wl), (wl, wr)


@pytest.mark.parametrize("dims,Ls", CASES, ids=IDS)
def test_residual_aware_form_on_a_perturbed_solution(dims, Ls):
    Lx, Ly = dims
    Dm, G5, eta, B, psi = solved(dims, Ls)
    pert = psi + 1e-3 * cgrid(psi.shape, 9)
    r = B.reshape(-1) - Dm @ pert.reshape(-1)
    E = np.where(np.arange(Ls) < Ls // 2, 1.0, -1.0)
    Er = (E[None, None, :, None] * r.reshape(psi.shape)).reshape(-1)
    lhs, rhs = dm.ward_grid(eta, pert, M)
    predicted = -np.vdot(pert.reshape(-1), G5 @ Er).real
    cap = np.linalg.norm(pert) * np.linalg.norm(r)
    print("residual form %s Ls=%d defect %.6e predicted %.6e |Psi||r| %.3e" % (dims, Ls, lhs - rhs, predicted, cap))
    assert abs((lhs - rhs) - predicted) <= 1e-13 * (abs(lhs) + cap)
    assert abs(lhs - rhs) <= cap
    assert abs(lhs - rhs) > 1e-8 * abs(lhs)     # the perturbation shows: the exact identity would not have passed by accident


@pytest.mark.parametrize("dims", [(4, 6), (2, 2)], ids=IDS)
def test_odd_ls_fails_the_identity(dims):
    Dm, G5, eta, B, psi = solved(dims, 3)
    lhs, rhs = dm.ward_grid(eta, psi, M)          # 'midpoint' (0, 0), (1, 1): there is none between the walls
    print("odd Ls %s rel defect %.3e" % (dims, abs(lhs - rhs) / abs(lhs)))
    assert abs(lhs - rhs) > 1e-6 * abs(lhs), (lhs, rhs)


def test_norms_and_correlators_are_consistent():
    Dm, G5, eta, B, psi = solved((4, 6), 4)
    N = dm.norms_grid(psi)
    assert N.shape == (6, 4, 2)
    assert abs(N.sum() - np.linalg.norm(psi) ** 2) <= 1e-13 * N.sum()
    cpi, cmp_, prof = dm.correlators(N)
    lhs, rhs = dm.ward_grid(eta, psi, M)
    assert abs(M * cpi.sum() + cmp_.sum() - lhs) <= 1e-14 * abs(lhs)
    assert abs(prof.sum() - 1) <= 1e-15


# ---- 2. qmg_dwf_meas_plan
KERNELS = (qmg.DMK_SOURCE, qmg.DMK_PROJECT_WALL, qmg.DMK_PROJECT_MID, qmg.DMK_NORMS)


def test_plan_grid_covers_the_lattice():
    for dtype, Ls, dims, nsys in itertools.product((qmg.C64, qmg.C32), LS_ALL + [4, 5, 7, 31], LATTICES + [(2048, 4)], (1, 3, 16)):
        Lx, Ly = dims
        for kernel in KERNELS:
            fam, lps, block, gx, gy, pbr, lds, nk = qmg.dwf_meas_plan(dtype, dims, Ls, kernel, nsys)
            tag = (dtype, Ls, dims, kernel, nsys)
            if kernel == qmg.DMK_PROJECT_MID and Ls % 2:
                assert fam == qmg.DMF_UNSUPPORTED, tag
                continue
            assert gy == 2 * Ly and nk == nsys, tag
            if kernel == qmg.DMK_NORMS:
                lanes = Ls * (Lx // 2)
                cover = -(-lanes // block)
                assert (fam, lps) == (qmg.DMF_NORMS, Ls), tag
                # a lane that strides by whole blocks keeps its s; no block is idle; the partial blocks reach every lane of the half row
                assert block % Ls == 0 and 256 - Ls < block <= 256, tag
                assert gx == pbr == min(cover, 4) and (pbr - 1) * block < lanes, tag
                assert (gx * block) % Ls == 0 and lds == 256 * 16, tag
            else:
                want_lps = Ls if kernel == qmg.DMK_SOURCE else 2
                lanes = want_lps * (Lx // 2)
                assert (fam, lps, block, pbr, lds) == (qmg.DMF_SOURCE if kernel == qmg.DMK_SOURCE else qmg.DMF_PROJECT, want_lps, 256, 0, 0), tag
                assert gx * block >= lanes > (gx - 1) * block, tag
    # the shapes the GPU tests lean on: more than one partial block per half row at (130, 2) from Ls = 8 on, strides at Ls = 32
    assert qmg.dwf_meas_plan(qmg.C64, (130, 2), 8, qmg.DMK_NORMS)[3] == 3
    assert qmg.dwf_meas_plan(qmg.C64, (130, 2), 12, qmg.DMK_NORMS)[2:4] == (252, 4)
    assert qmg.dwf_meas_plan(qmg.C64, (130, 2), 32, qmg.DMK_NORMS)[3] == 4 and 4 * 256 < 65 * 32
    assert qmg.dwf_meas_plan(qmg.C64, (16, 8), 3, qmg.DMK_NORMS)[2:4] == (255, 1)


def test_plan_refusals():
    for kernel in KERNELS:
        for Ls in (-1, 0, 1, 33, 64):
            assert qmg.dwf_meas_plan(qmg.C64, (16, 8), Ls, kernel)[0] == qmg.DMF_INVALID, (kernel, Ls)
        for dims in [(3, 4), (4, 5), (0, 2), (2, 0)]:
            assert qmg.dwf_meas_plan(qmg.C64, dims, 8, kernel)[0] == qmg.DMF_INVALID, (kernel, dims)
        for dtype in (-1, 2):
            assert qmg.dwf_meas_plan(dtype, (16, 8), 8, kernel)[0] == qmg.DMF_INVALID, (kernel, dtype)
        for nsys in (-1, 0, 17):
            assert qmg.dwf_meas_plan(qmg.C64, (16, 8), 8, kernel, nsys)[0] == qmg.DMF_INVALID, (kernel, nsys)
        # a half row beyond 32-bit byte offsets
        assert qmg.dwf_meas_plan(qmg.C64, (1 << 23, 2), 32, kernel)[0] == qmg.DMF_INVALID
    for kernel in (-1, 4):
        assert qmg.dwf_meas_plan(qmg.C64, (16, 8), 8, kernel)[0] == qmg.DMF_INVALID
    for Ls in (3, 5, 31):
        assert qmg.dwf_meas_plan(qmg.C64, (16, 8), Ls, qmg.DMK_PROJECT_MID)[0] == qmg.DMF_UNSUPPORTED
        assert qmg.dwf_meas_plan(qmg.C64, (16, 8), Ls, qmg.DMK_PROJECT_WALL)[0] == qmg.DMF_PROJECT


def test_plan_output_buffer_contract_and_row_walk():
    import ctypes as C
    lib = qmg.lib()
    out = (C.c_int * 12)(*([7] * 12))
    assert lib.qmg_dwf_meas_plan(qmg.C64, 16, 8, 6, qmg.DMK_NORMS, 3, out, 12) == 0
    assert list(out[8:]) == [-1] * 4 and list(out[:8]) == [qmg.DMF_NORMS, 6, 252, 1, 16, 1, 4096, 3]
    assert lib.qmg_dwf_meas_plan(qmg.C64, 16, 8, 6, qmg.DMK_NORMS, 1, out, 7) == 1
    assert lib.qmg_dwf_meas_plan(qmg.C64, 16, 8, 6, qmg.DMK_NORMS, 1, None, 8) == 1
    # more rows than grid.y can hold: gy is capped and the blocks walk the rest
    assert qmg.dwf_meas_plan(qmg.C64, (4, 40000), 2, qmg.DMK_NORMS)[4] == 65535


# ---- 3. the symbols
def test_symbols_are_declared_bound_and_exported():
    names = ["qmg_dwf_wall_source", "qmg_dwf_wall_project", "qmg_dwf_slice_norms", "qmg_dwf_meas_plan"]
    import os
    header = open(os.path.join(qmg.ROOT, "include", "qmg_hip.h")).read()
    for name in names:
        assert name in qmg.ABI_SYMBOLS and ("int %s(" % name) in header
        assert hasattr(qmg.lib(), name)
