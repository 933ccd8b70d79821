"""Every stencil-apply kernel (csrc/qmg_stencil*.hip, csrc/qmg_site.hip) against an independent reference, one row per route.

ROUTES is the table: entry point, storage, (Lx, Ly, nc), nrhs, mask, pieces, flags, tuning knobs where they are not the defaults, and the
plan of every pass the row is meant to hit, in qmg_stencil_plan's terms.  A row first asserts that the library routes the request as the row
says, so a retune that moves a kernel out from under its row fails here, and tests/test_host_stencil_plan.py fails when a plan exists that no
row expects.  Then the entry point runs on padded strides, masks with holes, a non-zero initial lhs and all three shifts set (the dof shift at
even nc), and EVERY active system is compared with stencil_numpy's long-double reference (inputs rounded to complex<float> / complex<half>
first where the storage is narrow, so that only arithmetic error is measured):
  whole vector   relative L2 < 1e-13 (fp64 results), TOL32_ROUND = 3e-7 (fp64 arithmetic, complex<float> results; 2e-6 with complex<half>
                 matrices, test_gpu_f32.py), TOL32 = 5e-6 (fp32 arithmetic: kernel A in float, kernel S storages 0 and 1); kernel C with narrow matrices AND vectors also
                 computes in fp32 (the f32 matrix pipe) and keeps the TOL32_ROUND / 2e-6 its earlier tests hold it to
  elementwise    |got - want| <= (n + 1) 2^-50 S, or (n + 1) 2^-21 S for fp32 arithmetic (those three), plus 2^-23 |want| for complex<float> results
                 (stencil_numpy.elementwise_bound)
Frozen systems, all padding and a parity no piece touches must come back bit-identical, and a second run of the same call must give the same
bytes, norms and dots included (every kernel here has one writer per output and a fixed summation order).  Fused-norm rows hold the norms, epilogue rows `out` and the
three dots, to long-double sums at the reductions' 1e-12.

Every kernel that caps grid.y has a `tall` row: 65 540 rows (kernel A2: row pairs) on 65 535 blocks, so that five blocks take a second row.
Such a row asserts the cap from the plan, starts what the call overwrites as NaN and compares the rows walked second on their own as well.
Kernels B32 and C are there at nc = 6 and nc = 8 on 2 x 32770 and 4 x 32770: stencil_numpy keeps the grids of the fields it applied last, so
the five systems kernel C needs take 4 s on the narrow lattice and 9 s on the wide one, the two slowest rows of the table (260 MB on the device each).
The `dotscap` row does the same for the epilogue's dots, whose partial sums cap grid.y at 2048 / gx.
"""
import functools
import importlib

import numpy as np
import pytest

import coordspace as cs
import stencil_numpy as sn

qmg = importlib.import_module("quantum-mg_amd")

pytestmark = pytest.mark.gpu

TOL64 = 1e-13
TOL32 = 5e-6          # fp32 arithmetic (test_gpu_f32.py)
TOL32_ROUND = 3e-7    # fp64 arithmetic, one fp32 rounding of the result (test_gpu_f32.py)
TOL32_M16 = 2e-6      # ... with complex<half> matrices (test_gpu_f32.py::test_coarse_apply_with_16_bit_stored_matrices)
TOL_REDUCE = 1e-12    # norms and dots
PAD = 6               # padding elements behind every vector (even: a complex<float> system stays 16-byte aligned)
SHIFTS = (0.3 - 0.1j, -0.2 + 0.05j, 0.15 - 0.25j)    # shift, eo_shift, dof_shift
DEFAULT_KNOBS = {"stencil_site": 3, "stencil_pair": 2, "stencil_mfma": 1, "pair_prefetch": 1}

P = qmg
PIECES = {
    "M0": P.P_ALL | P.P_ZERO, "M+": P.P_ALL,
    "EO0": P.P_EO | P.P_ZERO_E, "OE+": P.P_OE, "OE0": P.P_OE | P.P_ZERO_O,
    "HOP0": P.P_HOPPING | P.P_ZERO, "HOP+": P.P_HOPPING,
    "DIAG0": P.P_CLOVER | P.P_SHIFT | P.P_ZERO,
    "XPYM+": P.P_EO_XP1 | (P.P_OE_XP1 << 3),                      # even sites from +x, odd sites from -y
    "YPXM0": (P.P_EO_XP1 << 1) | (P.P_OE_XP1 << 2) | P.P_ZERO,    # even sites from +y, odd sites from -x
    "XM+": P.P_EO_XP1 << 2, "YM+": P.P_EO_XP1 << 3, "OXP+": P.P_OE_XP1, "OYP+": P.P_OE_XP1 << 1,
    "MIX0": P.P_CLOVER_E | P.P_EO | P.P_OE | P.P_ZERO,            # the two parities ask for different sets
    "EVEN0": P.P_CLOVER_E | P.P_EO | P.P_SHIFT_E | P.P_ZERO_E,
    "ODD+": P.P_CLOVER_O | P.P_OE | P.P_SHIFT_O,
    "SHIFT+": P.P_SHIFT, "ZERO": P.P_ZERO,
    "NONE": 0,
}
#            matrices      vectors        mat  vec32
STORAGE = {"c64": (np.complex128, np.complex128, 0, 0), "c32": (np.complex64, np.complex64, 1, 1), "m32": (np.complex64, np.complex128, 1, 0),
           "m16": (np.float16, np.complex128, 2, 0), "m16v32": (np.float16, np.complex64, 2, 1), "h16": (np.float16, np.complex64, 2, 1)}
ENTRY = {"apply": qmg.SE_APPLY, "masked": qmg.SE_MASKED, "h16": qmg.SE_H16, "norm2": qmg.SE_NORM2, "epi": qmg.SE_EPI,
         "slab0": qmg.SE_SLAB, "slab1": qmg.SE_SLAB, "slab2": qmg.SE_SLAB}
GEN_FAMILIES = (qmg.SF_GEN, qmg.SF_GEN32, qmg.SF_MFMA)
M32, V32, M16 = qmg.SST_M32, qmg.SST_V32, qmg.SST_M16
C32BITS, H16BITS = M32 | V32, M32 | V32 | M16


# ---- plans, as (family, storage, NC, P, K, flags, S, H) of qmg_stencil_plan's twelve ints (K: KR of kernels B / B32, the systems of a pass
#      of kernel C, 0 elsewhere)
def A(NC, st=0):
    return (qmg.SF_ELEM, st, NC, 0, 0, 0, 0, 0)


def A2(NC, norm=False, pf=False):
    return (qmg.SF_PAIR, 0, NC, 2, 0, (qmg.SPF_NORM if norm else 0) | (qmg.SPF_PF if pf else 0), 0, 0)


def S(st, shape, zero=False, batch=False):
    return (qmg.SF_SITE, st, 2, shape, 0, (qmg.SPF_ZERO if zero else 0) | (qmg.SPF_BATCH if batch else 0), 0, 0)


def B(st, PT, KR, S_, H, epi=0):
    return (qmg.SF_GEN, st, 0, PT, KR, (0, qmg.SPF_EPI, qmg.SPF_EPI | qmg.SPF_DOTS)[epi], S_, H)


def B32(st, PP, KR, S_, H, epi=0):
    return (qmg.SF_GEN32, st, 0, PP, KR, (0, qmg.SPF_EPI, qmg.SPF_EPI | qmg.SPF_DOTS)[epi], S_, H)


def C(st, nc, mode, nk, vl=True, pair=False):
    return (qmg.SF_MFMA, st, 16 if pair else nc, mode, nk, (qmg.SPF_VL if vl else 0) | (qmg.SPF_PAIR if pair else 0), 0, 0)


def V1(st, zero, shift):
    return (qmg.SF_VOLUME1, st, 0, 0, 0, (qmg.SPF_ZERO if zero else 0) | (qmg.SPF_SHIFT if shift else 0), 0, 0)


NOTHING = (qmg.SF_NOTHING, 0, 0, 0, 0, 0, 0, 0)
UNSUPPORTED = (qmg.SF_UNSUPPORTED, 0, 0, 0, 0, 0, 0, 0)
INVALID = (qmg.SF_INVALID, 0, 0, 0, 0, 0, 0, 0)


def instantiation(p):
    """the part of a pass of qmg_stencil_plan that a row states"""
    return (p[0], p[1], p[2], p[3], p[4] if p[0] in GEN_FAMILIES else 0, p[5], p[6], p[7])


def kernel_of(inst):
    """the instantiation alone (no tile, no pass length): what the coverage test wants a row for"""
    return (inst[0], inst[1], inst[2], inst[3], inst[4] if inst[0] in (qmg.SF_GEN, qmg.SF_GEN32) else 0, inst[5])


# ---- table begin
# (entry, storage, (Lx, Ly, nc), nrhs, mask, pieces, flags, knobs, plans of the passes)
ROUTES = [
    # ======== one row per instantiation the plan can produce over the domain of tests/test_host_stencil_plan.py, on the smallest shape that
    #          gives it, with a ragged last tile and a mask with holes where the route admits them
    # ---- kernel A (k_stencil_elem)
    ('masked', 'c64', (520, 4, 1), 1, 0b1, 'EO0', '', {}, [A(1)]),
    ('masked', 'c64', (6, 4, 2), 3, 0b101, 'EO0', '', {}, [A(2)]),
    ('masked', 'c64', (6, 4, 4), 1, 0b1, 'EO0', '', {}, [A(4)]),
    ('masked', 'c32', (520, 4, 1), 1, 0b1, 'HOP0', '', {}, [A(1, C32BITS)]),
    ('masked', 'c32', (6, 4, 2), 1, 0b1, 'M0', '', {'stencil_site': 0}, [A(2, C32BITS)]),
    ('masked', 'c32', (6, 4, 4), 1, 0b1, 'M0', 'nohopping', {}, [A(4, C32BITS)]),
    # ---- kernel A2 (k_stencil_pair)
    ('masked', 'c64', (520, 4, 1), 1, 0b1, 'DIAG0', '', {}, [A2(1)]),
    ('norm2', 'c64', (520, 4, 1), 1, 0b1, 'M0', '', {}, [A2(1, norm=True)]),
    ('masked', 'c64', (520, 4, 1), 3, 0b101, 'MIX0', '', {}, [A2(1, pf=True)]),
    ('norm2', 'c64', (520, 4, 1), 2, 0b11, 'M0', '', {}, [A2(1, norm=True, pf=True)]),
    ('masked', 'c64', (6, 4, 2), 1, 0b1, 'M0', '', {}, [A2(2)]),
    ('norm2', 'c64', (6, 4, 2), 1, 0b1, 'M+', '', {}, [A2(2, norm=True)]),
    ('masked', 'c64', (6, 4, 4), 1, 0b1, 'HOP0', '', {}, [A2(4)]),
    # ---- kernel S (k_stencil_site)
    ('masked', 'c64', (6, 4, 2), 1, 0b1, 'M+', '', {'stencil_site': 7}, [S(0, 1)]),
    ('masked', 'c64', (6, 4, 2), 1, 0b1, 'M0', '', {'stencil_site': 7}, [S(0, 1, zero=True)]),
    ('masked', 'c64', (6, 4, 2), 3, 0b101, 'M+', '', {'stencil_site': 7}, [S(0, 1, batch=True)]),
    ('masked', 'c64', (6, 4, 2), 3, 0b101, 'M0', '', {'stencil_site': 7}, [S(0, 1, zero=True, batch=True)]),
    ('masked', 'c64', (6, 4, 2), 1, 0b1, 'OE+', 'inplace', {}, [S(0, 2)]),
    ('masked', 'c64', (6, 4, 2), 1, 0b1, 'EO0', '', {}, [S(0, 2, zero=True)]),
    ('masked', 'c64', (6, 4, 2), 3, 0b101, 'EO0', '', {'stencil_site': 7}, [S(0, 2, zero=True, batch=True)]),
    ('masked', 'c32', (6, 4, 2), 1, 0b1, 'M0', 'nohopping', {}, [S(C32BITS, 0)]),
    ('masked', 'c32', (6, 4, 2), 3, 0b101, 'M0', 'nohopping', {}, [S(C32BITS, 0, batch=True)]),
    ('masked', 'c32', (6, 4, 2), 1, 0b1, 'M+', '', {}, [S(C32BITS, 1)]),
    ('masked', 'c32', (6, 4, 2), 1, 0b1, 'M0', '', {}, [S(C32BITS, 1, zero=True)]),
    ('masked', 'c32', (6, 4, 2), 3, 0b101, 'M+', '', {}, [S(C32BITS, 1, batch=True)]),
    ('masked', 'c32', (6, 4, 2), 3, 0b101, 'M0', '', {}, [S(C32BITS, 1, zero=True, batch=True)]),
    ('masked', 'c32', (6, 4, 2), 1, 0b1, 'OE+', 'inplace', {}, [S(C32BITS, 2)]),
    ('masked', 'c32', (6, 4, 2), 1, 0b1, 'EO0', '', {}, [S(C32BITS, 2, zero=True)]),
    ('masked', 'c32', (6, 4, 2), 3, 0b101, 'OE+', 'inplace', {}, [S(C32BITS, 2, batch=True)]),
    ('masked', 'c32', (6, 4, 2), 3, 0b101, 'EO0', '', {}, [S(C32BITS, 2, zero=True, batch=True)]),
    ('h16', 'h16', (6, 4, 2), 1, 0b1, 'M0', 'nohopping', {}, [S(H16BITS, 0)]),
    ('h16', 'h16', (6, 4, 2), 3, 0b101, 'M0', 'nohopping', {}, [S(H16BITS, 0, batch=True)]),
    ('h16', 'h16', (6, 4, 2), 1, 0b1, 'M+', '', {}, [S(H16BITS, 1)]),
    ('h16', 'h16', (6, 4, 2), 1, 0b1, 'M0', '', {}, [S(H16BITS, 1, zero=True)]),
    ('h16', 'h16', (6, 4, 2), 3, 0b101, 'M+', '', {}, [S(H16BITS, 1, batch=True)]),
    ('h16', 'h16', (6, 4, 2), 3, 0b101, 'M0', '', {}, [S(H16BITS, 1, zero=True, batch=True)]),
    ('h16', 'h16', (6, 4, 2), 1, 0b1, 'EO0', '', {}, [S(H16BITS, 2, zero=True)]),
    ('h16', 'h16', (6, 4, 2), 3, 0b101, 'EO0', '', {}, [S(H16BITS, 2, zero=True, batch=True)]),
    # ---- kernel B (k_stencil_gen)
    ('masked', 'c64', (6, 4, 3), 1, 0b1, 'MIX0', '', {}, [B(0, 1, 1, 3, 3)]),
    ('epi', 'c64', (6, 4, 3), 2, 0b1, 'M0', 'other', {}, [B(0, 1, 1, 3, 3, epi=1)]),
    ('epi', 'c64', (6, 4, 3), 2, 0b1, 'M0', 'dots', {}, [B(0, 1, 1, 3, 3, epi=2)]),
    ('masked', 'c64', (6, 4, 3), 3, 0b101, 'M+', '', {}, [B(0, 1, 4, 3, 3)]),
    ('masked', 'c64', (6, 4, 3), 6, 0b111101, 'EO0', '', {}, [B(0, 1, 8, 3, 3)]),
    ('masked', 'c64', (16, 4, 6), 1, 0b1, 'HOP0', '', {}, [B(0, 2, 1, 8, 5)]),
    ('epi', 'c64', (16, 4, 6), 2, 0b1, 'M0', '', {}, [B(0, 2, 1, 8, 5, epi=1)]),
    ('epi', 'c64', (16, 4, 6), 2, 0b1, 'M0', 'dots other', {}, [B(0, 2, 1, 8, 5, epi=2)]),
    ('masked', 'c64', (16, 4, 6), 3, 0b101, 'DIAG0', '', {}, [B(0, 2, 4, 8, 5)]),
    ('masked', 'c64', (16, 4, 6), 6, 0b111101, 'XPYM+', '', {}, [B(0, 2, 8, 8, 5)]),
    ('masked', 'c64', (520, 4, 3), 1, 0b1, 'MIX0', '', {}, [B(0, 3, 1, 85, 1)]),
    ('epi', 'c64', (520, 4, 3), 2, 0b1, 'M0', 'other', {}, [B(0, 3, 1, 85, 1, epi=1)]),
    ('epi', 'c64', (520, 4, 3), 2, 0b1, 'M0', 'dots', {}, [B(0, 3, 1, 85, 1, epi=2)]),
    ('masked', 'c64', (520, 4, 3), 3, 0b101, 'M+', '', {}, [B(0, 3, 4, 85, 1)]),
    ('masked', 'c64', (520, 4, 3), 6, 0b111101, 'EO0', '', {}, [B(0, 3, 8, 85, 1)]),
    ('masked', 'c64', (34, 4, 7), 1, 0b1, 'HOP0', '', {}, [B(0, 4, 1, 17, 2)]),
    ('epi', 'c64', (34, 4, 7), 2, 0b1, 'M0', '', {}, [B(0, 4, 1, 17, 2, epi=1)]),
    ('epi', 'c64', (34, 4, 7), 2, 0b1, 'M0', 'dots other', {}, [B(0, 4, 1, 17, 2, epi=2)]),
    ('masked', 'c64', (34, 4, 7), 3, 0b101, 'DIAG0', '', {}, [B(0, 4, 4, 17, 2)]),
    ('masked', 'c64', (520, 4, 8), 6, 0b111101, 'M0', '', {'stencil_mfma': 0}, [B(0, 4, 8, 16, 2)]),
    ('masked', 'c64', (34, 4, 8), 1, 0b1, 'MIX0', '', {}, [B(0, 5, 1, 17, 1)]),
    ('epi', 'c64', (34, 4, 8), 2, 0b1, 'M0', 'other', {}, [B(0, 5, 1, 17, 1, epi=1)]),
    ('epi', 'c64', (34, 4, 8), 2, 0b1, 'M0', 'dots', {}, [B(0, 5, 1, 17, 1, epi=2)]),
    ('masked', 'c64', (34, 4, 8), 3, 0b101, 'M+', '', {}, [B(0, 5, 4, 17, 1)]),
    ('masked', 'c64', (34, 4, 8), 6, 0b111101, 'EO0', '', {'stencil_mfma': 0}, [B(0, 5, 8, 17, 1)]),
    ('masked', 'c64', (520, 4, 6), 1, 0b1, 'HOP0', '', {}, [B(0, 6, 1, 42, 1)]),
    ('epi', 'c64', (520, 4, 6), 2, 0b1, 'M0', '', {}, [B(0, 6, 1, 42, 1, epi=1)]),
    ('epi', 'c64', (520, 4, 6), 2, 0b1, 'M0', 'dots other', {}, [B(0, 6, 1, 42, 1, epi=2)]),
    ('masked', 'c64', (34, 4, 16), 3, 0b101, 'DIAG0', '', {}, [B(0, 6, 4, 6, 2)]),
    ('masked', 'c64', (34, 4, 12), 6, 0b111101, 'M0', '', {'stencil_mfma': 0}, [B(0, 6, 8, 9, 2)]),
    ('masked', 'c64', (520, 4, 7), 1, 0b1, 'MIX0', '', {}, [B(0, 7, 1, 36, 1)]),
    ('epi', 'c64', (520, 4, 7), 2, 0b1, 'M0', 'other', {}, [B(0, 7, 1, 36, 1, epi=1)]),
    ('epi', 'c64', (520, 4, 7), 2, 0b1, 'M0', 'dots', {}, [B(0, 7, 1, 36, 1, epi=2)]),
    ('masked', 'c64', (520, 4, 7), 3, 0b101, 'M+', '', {}, [B(0, 7, 4, 36, 1)]),
    ('masked', 'c64', (10, 4, 24), 6, 0b111101, 'EO0', '', {'stencil_mfma': 0}, [B(0, 7, 8, 3, 3)]),
    ('masked', 'c64', (520, 4, 8), 1, 0b1, 'HOP0', '', {}, [B(0, 8, 1, 32, 1)]),
    ('epi', 'c64', (520, 4, 8), 2, 0b1, 'M0', '', {}, [B(0, 8, 1, 32, 1, epi=1)]),
    ('epi', 'c64', (520, 4, 8), 2, 0b1, 'M0', 'dots other', {}, [B(0, 8, 1, 32, 1, epi=2)]),
    ('masked', 'c64', (520, 4, 8), 3, 0b101, 'DIAG0', '', {}, [B(0, 8, 4, 32, 1)]),
    ('masked', 'c64', (6, 4, 32), 6, 0b111101, 'M0', '', {'stencil_mfma': 0}, [B(0, 8, 8, 2, 4)]),
    ('masked', 'c64', (6, 4, 48), 1, 0b1, 'MIX0', '', {}, [B(0, 9, 1, 1, 5)]),
    ('epi', 'c64', (6, 4, 48), 2, 0b1, 'M0', 'other', {}, [B(0, 9, 1, 1, 5, epi=1)]),
    ('epi', 'c64', (6, 4, 48), 2, 0b1, 'M0', 'dots', {}, [B(0, 9, 1, 1, 5, epi=2)]),
    ('masked', 'c64', (6, 4, 48), 3, 0b101, 'M+', '', {}, [B(0, 9, 4, 1, 5)]),
    ('masked', 'c64', (6, 4, 48), 6, 0b111101, 'EO0', '', {}, [B(0, 9, 8, 1, 5)]),
    ('masked', 'c64', (34, 4, 12), 1, 0b1, 'HOP0', '', {}, [B(0, 10, 1, 17, 1)]),
    ('epi', 'c64', (34, 4, 12), 2, 0b1, 'M0', '', {}, [B(0, 10, 1, 17, 1, epi=1)]),
    ('epi', 'c64', (34, 4, 12), 2, 0b1, 'M0', 'dots other', {}, [B(0, 10, 1, 17, 1, epi=2)]),
    ('masked', 'c64', (34, 4, 12), 3, 0b101, 'DIAG0', '', {}, [B(0, 10, 4, 17, 1)]),
    ('masked', 'c64', (12, 4, 24), 1, 0b1, 'XPYM+', '', {}, [B(0, 12, 1, 5, 2)]),
    ('epi', 'c64', (12, 4, 24), 2, 0b1, 'M0', '', {}, [B(0, 12, 1, 5, 2, epi=1)]),
    ('epi', 'c64', (12, 4, 24), 2, 0b1, 'M0', 'dots other', {}, [B(0, 12, 1, 5, 2, epi=2)]),
    ('masked', 'c64', (12, 4, 24), 3, 0b101, 'M0', '', {}, [B(0, 12, 4, 5, 2)]),
    ('masked', 'm32', (6, 4, 3), 1, 0b1, 'M+', '', {}, [B(M32, 1, 1, 3, 3)]),
    ('epi', 'm32', (6, 4, 3), 2, 0b1, 'EO0', '', {}, [B(M32, 1, 1, 3, 3, epi=1)]),
    ('epi', 'm32', (6, 4, 3), 2, 0b1, 'M0', 'dots other', {}, [B(M32, 1, 1, 3, 3, epi=2)]),
    ('masked', 'm32', (6, 4, 3), 3, 0b101, 'M0', 'noclover', {}, [B(M32, 1, 4, 3, 3)]),
    ('masked', 'm32', (6, 4, 3), 6, 0b111101, 'M0', 'nohopping', {}, [B(M32, 1, 8, 3, 3)]),
    ('masked', 'm32', (12, 4, 7), 1, 0b1, 'DIAG0', '', {}, [B(M32, 2, 1, 6, 6)]),
    ('epi', 'm32', (12, 4, 7), 2, 0b1, 'M0', 'other', {}, [B(M32, 2, 1, 6, 6, epi=1)]),
    ('epi', 'm32', (12, 4, 7), 2, 0b1, 'M0', 'dots', {}, [B(M32, 2, 1, 6, 6, epi=2)]),
    ('masked', 'm32', (12, 4, 7), 3, 0b101, 'M0', '', {}, [B(M32, 2, 4, 6, 6)]),
    ('masked', 'm32', (12, 4, 7), 6, 0b111101, 'M0', '', {}, [B(M32, 2, 8, 6, 6)]),
    ('masked', 'm32', (520, 4, 3), 1, 0b1, 'M+', '', {}, [B(M32, 3, 1, 85, 1)]),
    ('epi', 'm32', (520, 4, 3), 2, 0b1, 'EO0', '', {}, [B(M32, 3, 1, 85, 1, epi=1)]),
    ('epi', 'm32', (520, 4, 3), 2, 0b1, 'M0', 'dots other', {}, [B(M32, 3, 1, 85, 1, epi=2)]),
    ('masked', 'm32', (520, 4, 3), 3, 0b101, 'M0', 'noclover', {}, [B(M32, 3, 4, 85, 1)]),
    ('masked', 'm32', (520, 4, 3), 6, 0b111101, 'M0', 'nohopping', {}, [B(M32, 3, 8, 85, 1)]),
    ('masked', 'm32', (34, 4, 7), 1, 0b1, 'DIAG0', '', {}, [B(M32, 4, 1, 17, 2)]),
    ('epi', 'm32', (34, 4, 7), 2, 0b1, 'M0', 'other', {}, [B(M32, 4, 1, 17, 2, epi=1)]),
    ('epi', 'm32', (34, 4, 7), 2, 0b1, 'M0', 'dots', {}, [B(M32, 4, 1, 17, 2, epi=2)]),
    ('masked', 'm32', (34, 4, 7), 3, 0b101, 'M0', '', {}, [B(M32, 4, 4, 17, 2)]),
    ('masked', 'm32', (34, 4, 7), 6, 0b111101, 'M0', '', {}, [B(M32, 4, 8, 17, 2)]),
    ('masked', 'm32', (520, 4, 7), 1, 0b1, 'M+', '', {}, [B(M32, 7, 1, 36, 1)]),
    ('epi', 'm32', (520, 4, 7), 2, 0b1, 'EO0', '', {}, [B(M32, 7, 1, 36, 1, epi=1)]),
    ('epi', 'm32', (520, 4, 7), 2, 0b1, 'M0', 'dots other', {}, [B(M32, 7, 1, 36, 1, epi=2)]),
    ('masked', 'm32', (520, 4, 7), 3, 0b101, 'M0', 'noclover', {}, [B(M32, 7, 4, 36, 1)]),
    ('masked', 'm32', (520, 4, 7), 6, 0b111101, 'M0', 'nohopping', {}, [B(M32, 7, 8, 36, 1)]),
    ('masked', 'c32', (6, 4, 3), 1, 0b1, 'DIAG0', '', {}, [B(C32BITS, 1, 1, 3, 3)]),
    ('epi', 'c32', (6, 4, 3), 2, 0b1, 'M0', 'other', {}, [B(C32BITS, 1, 1, 3, 3, epi=1)]),
    ('epi', 'c32', (6, 4, 3), 2, 0b1, 'M0', 'dots', {}, [B(C32BITS, 1, 1, 3, 3, epi=2)]),
    ('masked', 'c32', (6, 4, 3), 3, 0b101, 'M0', '', {}, [B(C32BITS, 1, 4, 3, 3)]),
    ('masked', 'c32', (6, 4, 3), 6, 0b111101, 'M0', '', {}, [B(C32BITS, 1, 8, 3, 3)]),
    ('masked', 'c32', (12, 4, 7), 1, 0b1, 'M+', '', {}, [B(C32BITS, 2, 1, 6, 6)]),
    ('epi', 'c32', (12, 4, 7), 2, 0b1, 'EO0', '', {}, [B(C32BITS, 2, 1, 6, 6, epi=1)]),
    ('epi', 'c32', (12, 4, 7), 2, 0b1, 'M0', 'dots other', {}, [B(C32BITS, 2, 1, 6, 6, epi=2)]),
    ('masked', 'c32', (12, 4, 7), 3, 0b101, 'M0', 'noclover', {}, [B(C32BITS, 2, 4, 6, 6)]),
    ('masked', 'c32', (12, 4, 7), 6, 0b111101, 'M0', 'nohopping', {}, [B(C32BITS, 2, 8, 6, 6)]),
    ('masked', 'c32', (520, 4, 3), 1, 0b1, 'DIAG0', '', {}, [B(C32BITS, 3, 1, 85, 1)]),
    ('epi', 'c32', (520, 4, 3), 2, 0b1, 'M0', 'other', {}, [B(C32BITS, 3, 1, 85, 1, epi=1)]),
    ('epi', 'c32', (520, 4, 3), 2, 0b1, 'M0', 'dots', {}, [B(C32BITS, 3, 1, 85, 1, epi=2)]),
    ('masked', 'c32', (520, 4, 3), 3, 0b101, 'M0', '', {}, [B(C32BITS, 3, 4, 85, 1)]),
    ('masked', 'c32', (520, 4, 3), 6, 0b111101, 'M0', '', {}, [B(C32BITS, 3, 8, 85, 1)]),
    ('masked', 'c32', (34, 4, 7), 1, 0b1, 'M+', '', {}, [B(C32BITS, 4, 1, 17, 2)]),
    ('epi', 'c32', (34, 4, 7), 2, 0b1, 'EO0', '', {}, [B(C32BITS, 4, 1, 17, 2, epi=1)]),
    ('epi', 'c32', (34, 4, 7), 2, 0b1, 'M0', 'dots other', {}, [B(C32BITS, 4, 1, 17, 2, epi=2)]),
    ('masked', 'c32', (34, 4, 7), 3, 0b101, 'M0', 'noclover', {}, [B(C32BITS, 4, 4, 17, 2)]),
    ('masked', 'c32', (34, 4, 7), 6, 0b111101, 'M0', 'nohopping', {}, [B(C32BITS, 4, 8, 17, 2)]),
    ('masked', 'c32', (520, 4, 7), 1, 0b1, 'DIAG0', '', {}, [B(C32BITS, 7, 1, 36, 1)]),
    ('epi', 'c32', (520, 4, 7), 2, 0b1, 'M0', 'other', {}, [B(C32BITS, 7, 1, 36, 1, epi=1)]),
    ('epi', 'c32', (520, 4, 7), 2, 0b1, 'M0', 'dots', {}, [B(C32BITS, 7, 1, 36, 1, epi=2)]),
    ('masked', 'c32', (520, 4, 7), 3, 0b101, 'M0', '', {}, [B(C32BITS, 7, 4, 36, 1)]),
    ('masked', 'c32', (520, 4, 7), 6, 0b111101, 'M0', '', {}, [B(C32BITS, 7, 8, 36, 1)]),
    # ---- kernel B32 (k_stencil_gen32)
    ('masked', 'm32', (6, 4, 6), 1, 0b1, 'M+', '', {}, [B32(M32, 1, 1, 3, 6)]),
    ('epi', 'm32', (6, 4, 6), 2, 0b1, 'EO0', '', {}, [B32(M32, 1, 1, 3, 6, epi=1)]),
    ('epi', 'm32', (6, 4, 6), 2, 0b1, 'M0', 'dots other', {}, [B32(M32, 1, 1, 3, 6, epi=2)]),
    ('masked', 'm32', (6, 4, 6), 3, 0b101, 'M0', 'noclover', {}, [B32(M32, 1, 4, 3, 6)]),
    ('masked', 'm32', (6, 4, 6), 6, 0b111101, 'M0', 'nohopping', {}, [B32(M32, 1, 8, 3, 6)]),
    ('masked', 'm32', (34, 4, 6), 1, 0b1, 'DIAG0', '', {}, [B32(M32, 2, 1, 17, 2)]),
    ('epi', 'm32', (34, 4, 6), 2, 0b1, 'M0', 'other', {}, [B32(M32, 2, 1, 17, 2, epi=1)]),
    ('epi', 'm32', (34, 4, 6), 2, 0b1, 'M0', 'dots', {}, [B32(M32, 2, 1, 17, 2, epi=2)]),
    ('masked', 'm32', (34, 4, 6), 3, 0b101, 'M0', '', {}, [B32(M32, 2, 4, 17, 2)]),
    ('masked', 'm32', (34, 4, 6), 6, 0b111101, 'M0', '', {}, [B32(M32, 2, 8, 17, 2)]),
    ('masked', 'm32', (520, 4, 6), 1, 0b1, 'M+', '', {}, [B32(M32, 3, 1, 42, 1)]),
    ('epi', 'm32', (520, 4, 6), 2, 0b1, 'EO0', '', {}, [B32(M32, 3, 1, 42, 1, epi=1)]),
    ('epi', 'm32', (520, 4, 6), 2, 0b1, 'M0', 'dots other', {}, [B32(M32, 3, 1, 42, 1, epi=2)]),
    ('masked', 'm32', (520, 4, 6), 3, 0b101, 'M0', 'noclover', {}, [B32(M32, 3, 4, 42, 1)]),
    ('masked', 'm32', (34, 4, 8), 6, 0b111101, 'M0', '', {'stencil_mfma': 0}, [B32(M32, 3, 8, 17, 1)]),
    ('masked', 'm32', (520, 4, 8), 1, 0b1, 'DIAG0', '', {}, [B32(M32, 4, 1, 32, 1)]),
    ('epi', 'm32', (520, 4, 8), 2, 0b1, 'M0', 'other', {}, [B32(M32, 4, 1, 32, 1, epi=1)]),
    ('epi', 'm32', (520, 4, 8), 2, 0b1, 'M0', 'dots', {}, [B32(M32, 4, 1, 32, 1, epi=2)]),
    ('masked', 'm32', (520, 4, 8), 3, 0b101, 'M0', '', {}, [B32(M32, 4, 4, 32, 1)]),
    ('masked', 'm32', (6, 4, 24), 6, 0b111101, 'M0', '', {'stencil_mfma': 0}, [B32(M32, 4, 8, 3, 3)]),
    ('masked', 'm32', (34, 4, 12), 1, 0b1, 'M+', '', {}, [B32(M32, 5, 1, 17, 1)]),
    ('epi', 'm32', (34, 4, 12), 2, 0b1, 'EO0', '', {}, [B32(M32, 5, 1, 17, 1, epi=1)]),
    ('epi', 'm32', (34, 4, 12), 2, 0b1, 'M0', 'dots other', {}, [B32(M32, 5, 1, 17, 1, epi=2)]),
    ('masked', 'm32', (34, 4, 12), 3, 0b101, 'M0', 'noclover', {}, [B32(M32, 5, 4, 17, 1)]),
    ('masked', 'm32', (6, 4, 48), 6, 0b111101, 'M0', 'nohopping', {}, [B32(M32, 5, 8, 1, 5)]),
    ('masked', 'm32', (12, 4, 24), 1, 0b1, 'DIAG0', '', {}, [B32(M32, 6, 1, 5, 2)]),
    ('epi', 'm32', (12, 4, 24), 2, 0b1, 'M0', 'other', {}, [B32(M32, 6, 1, 5, 2, epi=1)]),
    ('epi', 'm32', (12, 4, 24), 2, 0b1, 'M0', 'dots', {}, [B32(M32, 6, 1, 5, 2, epi=2)]),
    ('masked', 'm32', (12, 4, 24), 3, 0b101, 'M0', '', {}, [B32(M32, 6, 4, 5, 2)]),
    ('masked', 'm32', (12, 4, 24), 6, 0b111101, 'M0', '', {'stencil_mfma': 0}, [B32(M32, 6, 8, 5, 2)]),
    ('masked', 'c32', (6, 4, 6), 1, 0b1, 'M+', '', {}, [B32(C32BITS, 1, 1, 3, 6)]),
    ('epi', 'c32', (6, 4, 6), 2, 0b1, 'EO0', '', {}, [B32(C32BITS, 1, 1, 3, 6, epi=1)]),
    ('epi', 'c32', (6, 4, 6), 2, 0b1, 'M0', 'dots other', {}, [B32(C32BITS, 1, 1, 3, 6, epi=2)]),
    ('masked', 'c32', (6, 4, 6), 3, 0b101, 'M0', 'noclover', {}, [B32(C32BITS, 1, 4, 3, 6)]),
    ('masked', 'c32', (6, 4, 6), 6, 0b111101, 'M0', 'nohopping', {}, [B32(C32BITS, 1, 8, 3, 6)]),
    ('masked', 'c32', (34, 4, 6), 1, 0b1, 'DIAG0', '', {}, [B32(C32BITS, 2, 1, 17, 2)]),
    ('epi', 'c32', (34, 4, 6), 2, 0b1, 'M0', 'other', {}, [B32(C32BITS, 2, 1, 17, 2, epi=1)]),
    ('epi', 'c32', (34, 4, 6), 2, 0b1, 'M0', 'dots', {}, [B32(C32BITS, 2, 1, 17, 2, epi=2)]),
    ('masked', 'c32', (34, 4, 6), 3, 0b101, 'M0', '', {}, [B32(C32BITS, 2, 4, 17, 2)]),
    ('masked', 'c32', (34, 4, 6), 6, 0b111101, 'M0', '', {}, [B32(C32BITS, 2, 8, 17, 2)]),
    ('masked', 'c32', (520, 4, 6), 1, 0b1, 'M+', '', {}, [B32(C32BITS, 3, 1, 42, 1)]),
    ('epi', 'c32', (520, 4, 6), 2, 0b1, 'EO0', '', {}, [B32(C32BITS, 3, 1, 42, 1, epi=1)]),
    ('epi', 'c32', (520, 4, 6), 2, 0b1, 'M0', 'dots other', {}, [B32(C32BITS, 3, 1, 42, 1, epi=2)]),
    ('masked', 'c32', (520, 4, 6), 3, 0b101, 'M0', 'noclover', {}, [B32(C32BITS, 3, 4, 42, 1)]),
    ('masked', 'c32', (34, 4, 8), 6, 0b111101, 'M0', '', {'stencil_mfma': 0}, [B32(C32BITS, 3, 8, 17, 1)]),
    ('masked', 'c32', (520, 4, 8), 1, 0b1, 'DIAG0', '', {}, [B32(C32BITS, 4, 1, 32, 1)]),
    ('epi', 'c32', (520, 4, 8), 2, 0b1, 'M0', 'other', {}, [B32(C32BITS, 4, 1, 32, 1, epi=1)]),
    ('epi', 'c32', (520, 4, 8), 2, 0b1, 'M0', 'dots', {}, [B32(C32BITS, 4, 1, 32, 1, epi=2)]),
    ('masked', 'c32', (520, 4, 8), 3, 0b101, 'M0', '', {}, [B32(C32BITS, 4, 4, 32, 1)]),
    ('masked', 'c32', (6, 4, 24), 6, 0b111101, 'M0', '', {'stencil_mfma': 0}, [B32(C32BITS, 4, 8, 3, 3)]),
    ('masked', 'c32', (34, 4, 12), 1, 0b1, 'M+', '', {}, [B32(C32BITS, 5, 1, 17, 1)]),
    ('epi', 'c32', (34, 4, 12), 2, 0b1, 'EO0', '', {}, [B32(C32BITS, 5, 1, 17, 1, epi=1)]),
    ('epi', 'c32', (34, 4, 12), 2, 0b1, 'M0', 'dots other', {}, [B32(C32BITS, 5, 1, 17, 1, epi=2)]),
    ('masked', 'c32', (34, 4, 12), 3, 0b101, 'M0', 'noclover', {}, [B32(C32BITS, 5, 4, 17, 1)]),
    ('masked', 'c32', (6, 4, 48), 6, 0b111101, 'M0', 'nohopping', {}, [B32(C32BITS, 5, 8, 1, 5)]),
    ('masked', 'c32', (12, 4, 24), 1, 0b1, 'DIAG0', '', {}, [B32(C32BITS, 6, 1, 5, 2)]),
    ('epi', 'c32', (12, 4, 24), 2, 0b1, 'M0', 'other', {}, [B32(C32BITS, 6, 1, 5, 2, epi=1)]),
    ('epi', 'c32', (12, 4, 24), 2, 0b1, 'M0', 'dots', {}, [B32(C32BITS, 6, 1, 5, 2, epi=2)]),
    ('masked', 'c32', (12, 4, 24), 3, 0b101, 'M0', '', {}, [B32(C32BITS, 6, 4, 5, 2)]),
    ('masked', 'c32', (12, 4, 24), 6, 0b111101, 'M0', '', {'stencil_mfma': 0}, [B32(C32BITS, 6, 8, 5, 2)]),
    ('masked', 'm16', (6, 4, 8), 1, 0b1, 'M+', '', {}, [B32(M32 | M16, 1, 1, 3, 8)]),
    ('epi', 'm16', (6, 4, 8), 2, 0b1, 'EO0', '', {}, [B32(M32 | M16, 1, 1, 3, 8, epi=1)]),
    ('epi', 'm16', (6, 4, 8), 2, 0b1, 'M0', 'dots other', {}, [B32(M32 | M16, 1, 1, 3, 8, epi=2)]),
    ('masked', 'm16', (6, 4, 8), 3, 0b101, 'M0', 'noclover', {}, [B32(M32 | M16, 1, 4, 3, 8)]),
    ('masked', 'm16', (6, 4, 8), 6, 0b111101, 'M0', '', {'stencil_mfma': 0}, [B32(M32 | M16, 1, 8, 3, 8)]),
    ('masked', 'm16', (520, 4, 8), 1, 0b1, 'DIAG0', '', {}, [B32(M32 | M16, 2, 1, 32, 1)]),
    ('epi', 'm16', (520, 4, 8), 2, 0b1, 'M0', 'other', {}, [B32(M32 | M16, 2, 1, 32, 1, epi=1)]),
    ('epi', 'm16', (520, 4, 8), 2, 0b1, 'M0', 'dots', {}, [B32(M32 | M16, 2, 1, 32, 1, epi=2)]),
    ('masked', 'm16', (520, 4, 8), 3, 0b101, 'M0', '', {}, [B32(M32 | M16, 2, 4, 32, 1)]),
    ('masked', 'm16', (34, 4, 8), 6, 0b111101, 'M0', '', {'stencil_mfma': 0}, [B32(M32 | M16, 2, 8, 17, 1)]),
    ('masked', 'm16', (12, 4, 24), 1, 0b1, 'M+', '', {}, [B32(M32 | M16, 3, 1, 5, 2)]),
    ('epi', 'm16', (12, 4, 24), 2, 0b1, 'EO0', '', {}, [B32(M32 | M16, 3, 1, 5, 2, epi=1)]),
    ('epi', 'm16', (12, 4, 24), 2, 0b1, 'M0', 'dots other', {}, [B32(M32 | M16, 3, 1, 5, 2, epi=2)]),
    ('masked', 'm16', (12, 4, 24), 3, 0b101, 'M0', 'noclover', {}, [B32(M32 | M16, 3, 4, 5, 2)]),
    ('masked', 'm16', (12, 4, 24), 6, 0b111101, 'M0', '', {'stencil_mfma': 0}, [B32(M32 | M16, 3, 8, 5, 2)]),
    ('masked', 'm16v32', (6, 4, 8), 1, 0b1, 'DIAG0', '', {}, [B32(H16BITS, 1, 1, 3, 8)]),
    ('epi', 'm16v32', (6, 4, 8), 2, 0b1, 'M0', 'other', {}, [B32(H16BITS, 1, 1, 3, 8, epi=1)]),
    ('epi', 'm16v32', (6, 4, 8), 2, 0b1, 'M0', 'dots', {}, [B32(H16BITS, 1, 1, 3, 8, epi=2)]),
    ('masked', 'm16v32', (6, 4, 8), 3, 0b101, 'M0', '', {}, [B32(H16BITS, 1, 4, 3, 8)]),
    ('masked', 'm16v32', (6, 4, 8), 6, 0b111101, 'M0', '', {'stencil_mfma': 0}, [B32(H16BITS, 1, 8, 3, 8)]),
    ('masked', 'm16v32', (520, 4, 8), 1, 0b1, 'M+', '', {}, [B32(H16BITS, 2, 1, 32, 1)]),
    ('epi', 'm16v32', (520, 4, 8), 2, 0b1, 'EO0', '', {}, [B32(H16BITS, 2, 1, 32, 1, epi=1)]),
    ('epi', 'm16v32', (520, 4, 8), 2, 0b1, 'M0', 'dots other', {}, [B32(H16BITS, 2, 1, 32, 1, epi=2)]),
    ('masked', 'm16v32', (520, 4, 8), 3, 0b101, 'M0', 'noclover', {}, [B32(H16BITS, 2, 4, 32, 1)]),
    ('masked', 'm16v32', (34, 4, 8), 6, 0b111101, 'M0', '', {'stencil_mfma': 0}, [B32(H16BITS, 2, 8, 17, 1)]),
    ('masked', 'm16v32', (12, 4, 24), 1, 0b1, 'DIAG0', '', {}, [B32(H16BITS, 3, 1, 5, 2)]),
    ('epi', 'm16v32', (12, 4, 24), 2, 0b1, 'M0', 'other', {}, [B32(H16BITS, 3, 1, 5, 2, epi=1)]),
    ('epi', 'm16v32', (12, 4, 24), 2, 0b1, 'M0', 'dots', {}, [B32(H16BITS, 3, 1, 5, 2, epi=2)]),
    ('masked', 'm16v32', (12, 4, 24), 3, 0b101, 'M0', '', {}, [B32(H16BITS, 3, 4, 5, 2)]),
    ('masked', 'm16v32', (12, 4, 24), 6, 0b111101, 'M0', '', {'stencil_mfma': 0}, [B32(H16BITS, 3, 8, 5, 2)]),
    # ---- kernel C (k_stencil_mfma)
    ('masked', 'c64', (6, 4, 8), 6, 0b111101, 'M+', '', {'stencil_mfma': 2}, [C(0, 8, 0, 5)]),
    ('masked', 'c64', (6, 4, 8), 6, 0b111101, 'EO0', '', {}, [C(0, 8, 1, 5)]),
    ('masked', 'c64', (6, 4, 8), 10, 0x3fd, 'HOP0', '', {}, [C(0, 8, 2, 9)]),
    ('masked', 'c64', (6, 4, 12), 10, 0x3fd, 'M0', 'noclover', {}, [C(0, 12, 0, 9)]),
    ('masked', 'c64', (6, 4, 12), 6, 0b111101, 'M0', 'nohopping', {}, [C(0, 12, 1, 5)]),
    ('masked', 'c64', (6, 4, 16), 10, 0x3fd, 'DIAG0', '', {}, [C(0, 16, 0, 9)]),
    ('masked', 'c64', (6, 4, 16), 6, 0b111101, 'XPYM+', '', {}, [C(0, 16, 1, 5)]),
    ('masked', 'c64', (12, 4, 8), 6, 0b111101, 'MIX0', '', {}, [C(0, 8, 1, 5, pair=True)]),
    ('masked', 'c64', (6, 4, 24), 5, 0b11101, 'M0', '', {'stencil_mfma': 2}, [C(0, 24, 0, 4)]),
    ('masked', 'c64', (6, 4, 24), 5, 0b11101, 'M0', '', {}, [C(0, 24, 1, 4)]),
    ('masked', 'c64', (6, 4, 24), 10, 0x3fd, 'M+', '', {}, [C(0, 24, 2, 9)]),
    ('masked', 'c64', (6, 4, 32), 10, 0x3fd, 'EO0', '', {}, [C(0, 32, 0, 9)]),
    ('masked', 'c64', (6, 4, 32), 5, 0b11101, 'HOP0', '', {}, [C(0, 32, 1, 4)]),
    ('masked', 'm32', (6, 4, 8), 10, 0x3fd, 'M0', 'noclover', {}, [C(M32, 8, 0, 9, vl=False)]),
    ('masked', 'm32', (6, 4, 8), 6, 0b111101, 'M0', 'nohopping', {}, [C(M32, 8, 1, 5)]),
    ('masked', 'm32', (6, 4, 12), 10, 0x3fd, 'DIAG0', '', {}, [C(M32, 12, 0, 9, vl=False)]),
    ('masked', 'm32', (6, 4, 12), 6, 0b111101, 'XPYM+', '', {}, [C(M32, 12, 1, 5)]),
    ('masked', 'm32', (6, 4, 16), 10, 0x3fd, 'MIX0', '', {}, [C(M32, 16, 0, 9, vl=False)]),
    ('masked', 'm32', (6, 4, 16), 6, 0b111101, 'M0', '', {}, [C(M32, 16, 1, 5)]),
    ('masked', 'm32', (12, 4, 8), 6, 0b111101, 'M0', '', {}, [C(M32, 8, 1, 5, pair=True)]),
    ('masked', 'm32', (6, 4, 24), 10, 0x3fd, 'M+', '', {}, [C(M32, 24, 0, 9, vl=False)]),
    ('masked', 'm32', (6, 4, 24), 5, 0b11101, 'EO0', '', {}, [C(M32, 24, 1, 4)]),
    ('masked', 'm32', (6, 4, 32), 10, 0x3fd, 'HOP0', '', {}, [C(M32, 32, 0, 9, vl=False)]),
    ('masked', 'm32', (6, 4, 32), 5, 0b11101, 'M0', 'noclover', {}, [C(M32, 32, 1, 4)]),
    ('masked', 'c32', (6, 4, 8), 10, 0x3fd, 'M0', 'nohopping', {}, [C(C32BITS, 8, 0, 9, vl=False)]),
    ('masked', 'c32', (6, 4, 8), 6, 0b111101, 'DIAG0', '', {}, [C(C32BITS, 8, 1, 5)]),
    ('masked', 'c32', (6, 4, 12), 10, 0x3fd, 'XPYM+', '', {}, [C(C32BITS, 12, 0, 9, vl=False)]),
    ('masked', 'c32', (6, 4, 12), 6, 0b111101, 'MIX0', '', {}, [C(C32BITS, 12, 1, 5)]),
    ('masked', 'c32', (6, 4, 16), 10, 0x3fd, 'M0', '', {}, [C(C32BITS, 16, 0, 9, vl=False)]),
    ('masked', 'c32', (6, 4, 16), 6, 0b111101, 'M0', '', {}, [C(C32BITS, 16, 1, 5)]),
    ('masked', 'c32', (12, 4, 8), 6, 0b111101, 'M+', '', {}, [C(C32BITS, 8, 1, 5, pair=True)]),
    ('masked', 'c32', (6, 4, 24), 10, 0x3fd, 'EO0', '', {}, [C(C32BITS, 24, 0, 9, vl=False)]),
    ('masked', 'c32', (6, 4, 24), 5, 0b11101, 'HOP0', '', {}, [C(C32BITS, 24, 1, 4)]),
    ('masked', 'c32', (6, 4, 32), 10, 0x3fd, 'M0', 'noclover', {}, [C(C32BITS, 32, 0, 9, vl=False)]),
    ('masked', 'c32', (6, 4, 32), 5, 0b11101, 'M0', 'nohopping', {}, [C(C32BITS, 32, 1, 4)]),
    ('masked', 'm16', (6, 4, 8), 10, 0x3fd, 'DIAG0', '', {}, [C(M32 | M16, 8, 0, 9, vl=False)]),
    ('masked', 'm16', (6, 4, 8), 6, 0b111101, 'XPYM+', '', {}, [C(M32 | M16, 8, 1, 5)]),
    ('masked', 'm16', (6, 4, 12), 10, 0x3fd, 'MIX0', '', {}, [C(M32 | M16, 12, 0, 9, vl=False)]),
    ('masked', 'm16', (6, 4, 12), 6, 0b111101, 'M0', '', {}, [C(M32 | M16, 12, 1, 5)]),
    ('masked', 'm16', (6, 4, 16), 10, 0x3fd, 'M0', '', {}, [C(M32 | M16, 16, 0, 9, vl=False)]),
    ('masked', 'm16', (6, 4, 16), 6, 0b111101, 'M+', '', {}, [C(M32 | M16, 16, 1, 5)]),
    ('masked', 'm16', (12, 4, 8), 6, 0b111101, 'EO0', '', {}, [C(M32 | M16, 8, 1, 5, pair=True)]),
    ('masked', 'm16', (6, 4, 24), 10, 0x3fd, 'HOP0', '', {}, [C(M32 | M16, 24, 0, 9, vl=False)]),
    ('masked', 'm16', (6, 4, 24), 5, 0b11101, 'M0', 'noclover', {}, [C(M32 | M16, 24, 1, 4)]),
    ('masked', 'm16', (6, 4, 32), 10, 0x3fd, 'M0', 'nohopping', {}, [C(M32 | M16, 32, 0, 9, vl=False)]),
    ('masked', 'm16', (6, 4, 32), 5, 0b11101, 'DIAG0', '', {}, [C(M32 | M16, 32, 1, 4)]),
    ('masked', 'm16v32', (6, 4, 8), 10, 0x3fd, 'XPYM+', '', {}, [C(H16BITS, 8, 0, 9, vl=False)]),
    ('masked', 'm16v32', (6, 4, 8), 6, 0b111101, 'MIX0', '', {}, [C(H16BITS, 8, 1, 5)]),
    ('masked', 'm16v32', (6, 4, 12), 10, 0x3fd, 'M0', '', {}, [C(H16BITS, 12, 0, 9, vl=False)]),
    ('masked', 'm16v32', (6, 4, 12), 6, 0b111101, 'M0', '', {}, [C(H16BITS, 12, 1, 5)]),
    ('masked', 'm16v32', (6, 4, 16), 10, 0x3fd, 'M+', '', {}, [C(H16BITS, 16, 0, 9, vl=False)]),
    ('masked', 'm16v32', (6, 4, 16), 6, 0b111101, 'EO0', '', {}, [C(H16BITS, 16, 1, 5)]),
    ('masked', 'm16v32', (12, 4, 8), 6, 0b111101, 'HOP0', '', {}, [C(H16BITS, 8, 1, 5, pair=True)]),
    ('masked', 'm16v32', (6, 4, 24), 10, 0x3fd, 'M0', 'noclover', {}, [C(H16BITS, 24, 0, 9, vl=False)]),
    ('masked', 'm16v32', (6, 4, 24), 5, 0b11101, 'M0', 'nohopping', {}, [C(H16BITS, 24, 1, 4)]),
    ('masked', 'm16v32', (6, 4, 32), 10, 0x3fd, 'DIAG0', '', {}, [C(H16BITS, 32, 0, 9, vl=False)]),
    ('masked', 'm16v32', (6, 4, 32), 5, 0b11101, 'XPYM+', '', {}, [C(H16BITS, 32, 1, 4)]),
    # ---- the 1 x 1 lattice
    ('masked', 'c64', (1, 1, 1), 1, 0b1, 'HOP0', '', {}, [V1(0, True, False)]),
    ('masked', 'c64', (1, 1, 1), 1, 0b1, 'M+', '', {}, [V1(0, False, True)]),
    ('masked', 'c64', (1, 1, 1), 1, 0b1, 'M0', '', {}, [V1(0, True, True)]),
    ('masked', 'c32', (1, 1, 1), 1, 0b1, 'HOP0', '', {}, [V1(C32BITS, True, False)]),
    ('masked', 'c32', (1, 1, 1), 1, 0b1, 'M+', '', {}, [V1(C32BITS, False, True)]),
    ('masked', 'c32', (1, 1, 1), 1, 0b1, 'M0', '', {}, [V1(C32BITS, True, True)]),
    # ---- nothing to launch
    ('masked', 'c64', (6, 4, 1), 1, 0b1, 'NONE', '', {}, [NOTHING]),
    # ======== edges and hand-overs
    # ---- Lx = 2: Lx / 2 = 1, +x and -x are the same site
    ('apply', 'c64', (2, 4, 1), 1, 0b1, 'M+', '', {}, [A2(1)]),
    ('apply', 'c64', (2, 4, 2), 1, 0b1, 'M+', '', {}, [A2(2)]),
    ('apply', 'c64', (2, 4, 4), 1, 0b1, 'M0', '', {}, [A2(4)]),
    ('masked', 'c32', (2, 4, 1), 3, 0b101, 'M+', '', {}, [A(1, C32BITS)]),
    ('masked', 'c32', (2, 4, 2), 3, 0b101, 'M+', '', {}, [S(C32BITS, 1, batch=True)]),
    ('masked', 'c32', (2, 4, 4), 3, 0b101, 'M0', '', {}, [A(4, C32BITS)]),
    ('masked', 'c32', (2, 4, 2), 3, 0b101, 'M+', '', {'stencil_site': 0}, [A(2, C32BITS)]),
    ('apply', 'c64', (2, 4, 2), 1, 0b1, 'HOP+', '', {}, [S(0, 2)]),
    ('apply', 'c64', (2, 4, 2), 1, 0b1, 'M+', '', {'stencil_site': 7}, [S(0, 1)]),
    ('h16', 'h16', (2, 4, 2), 3, 0b110, 'M+', '', {}, [S(H16BITS, 1, batch=True)]),
    ('apply', 'c64', (2, 4, 3), 1, 0b1, 'M+', '', {}, [B(0, 1, 1, 1, 3)]),
    ('masked', 'c64', (2, 4, 3), 4, 0b1101, 'M+', '', {}, [B(0, 1, 4, 1, 3)]),
    ('masked', 'm32', (2, 4, 6), 4, 0b1101, 'M+', '', {}, [B32(M32, 1, 4, 1, 6)]),
    ('masked', 'c32', (2, 4, 6), 1, 0b1, 'M+', '', {}, [B32(C32BITS, 1, 1, 1, 6)]),
    ('masked', 'c64', (2, 4, 8), 6, 0b101111, 'M+', '', {}, [C(0, 8, 1, 5)]),
    ('masked', 'c64', (2, 4, 24), 6, 0b101111, 'M+', '', {}, [C(0, 24, 1, 5)]),
    ('masked', 'm16', (2, 4, 12), 6, 0b101111, 'M+', '', {}, [C(M32 | M16, 12, 1, 5)]),
    ('masked', 'c64', (2, 4, 16), 14, 0x3ffd, 'M+', '', {}, [C(0, 16, 0, 13)]),
    # ---- Ly = 2: +y and -y are the same row
    ('apply', 'c64', (6, 2, 1), 1, 0b1, 'M+', '', {}, [A2(1)]),
    ('apply', 'c64', (6, 2, 2), 1, 0b1, 'M+', '', {}, [A2(2)]),
    ('apply', 'c64', (6, 2, 4), 2, 0b11, 'M+', '', {}, [A2(4)]),
    ('masked', 'c32', (6, 2, 1), 3, 0b101, 'M+', '', {}, [A(1, C32BITS)]),
    ('masked', 'c32', (6, 2, 2), 3, 0b101, 'M+', '', {}, [S(C32BITS, 1, batch=True)]),
    ('masked', 'c32', (6, 2, 4), 1, 0b1, 'M+', '', {}, [A(4, C32BITS)]),
    ('apply', 'c64', (6, 2, 2), 1, 0b1, 'HOP0', '', {}, [S(0, 2, zero=True)]),
    ('apply', 'c64', (6, 2, 2), 3, 0b111, 'M+', '', {'stencil_site': 7}, [S(0, 1, batch=True)]),
    ('h16', 'h16', (6, 2, 2), 1, 0b1, 'M+', '', {}, [S(H16BITS, 1)]),
    ('apply', 'c64', (6, 2, 3), 1, 0b1, 'M+', '', {}, [B(0, 1, 1, 3, 3)]),
    ('masked', 'm32', (6, 2, 6), 4, 0b1101, 'M+', '', {}, [B32(M32, 1, 4, 3, 6)]),
    ('masked', 'm16v32', (6, 2, 8), 3, 0b101, 'M+', '', {}, [B32(H16BITS, 1, 4, 3, 8)]),
    ('masked', 'c64', (10, 2, 8), 6, 0b101111, 'M+', '', {}, [C(0, 8, 1, 5)]),
    ('masked', 'c64', (12, 2, 8), 6, 0b101111, 'M+', '', {}, [C(0, 8, 1, 5, pair=True)]),
    ('masked', 'c32', (10, 2, 24), 5, 0b11111, 'M+', '', {}, [C(C32BITS, 24, 1, 5)]),
    ('masked', 'c64', (10, 2, 12), 10, 0x3ff, 'M+', '', {}, [C(0, 12, 0, 10)]),
    # ---- ragged tiles: Lx / 2 = S + 1 in kernels B / B32 (nc = 24: the production tile PT = 12, S = 5), Lx / 2 in {1, 5, 6} in kernel C, Lx / 2 > 256 at nc = 1
    ('apply', 'c64', (12, 4, 24), 1, 0b1, 'M+', '', {}, [B(0, 12, 1, 5, 2)]),
    ('masked', 'c64', (12, 4, 24), 3, 0b101, 'M0', '', {}, [B(0, 12, 4, 5, 2)]),
    ('masked', 'c64', (12, 4, 24), 6, 0b101111, 'M+', '', {'stencil_mfma': 0}, [B(0, 7, 8, 3, 3)]),
    ('masked', 'm32', (12, 4, 24), 1, 0b1, 'M+', '', {}, [B32(M32, 6, 1, 5, 2)]),
    ('masked', 'c32', (12, 4, 24), 3, 0b101, 'M0', '', {}, [B32(C32BITS, 6, 4, 5, 2)]),
    ('masked', 'm16', (12, 4, 24), 3, 0b110, 'M+', '', {}, [B32(M32 | M16, 3, 4, 5, 2)]),
    ('masked', 'c64', (10, 4, 8), 6, 0b101111, 'M+', '', {}, [C(0, 8, 1, 5)]),
    ('masked', 'c64', (12, 4, 8), 6, 0b101111, 'M0', '', {}, [C(0, 8, 1, 5, pair=True)]),
    ('masked', 'c64', (10, 4, 24), 5, 0b11111, 'M+', '', {}, [C(0, 24, 1, 5)]),
    ('masked', 'c64', (12, 4, 24), 5, 0b11111, 'EO0', '', {}, [C(0, 24, 1, 5)]),
    ('masked', 'c32', (12, 4, 8), 6, 0b101111, 'M+', '', {}, [C(C32BITS, 8, 1, 5, pair=True)]),
    ('masked', 'm16v32', (10, 4, 16), 6, 0b101111, 'M+', '', {}, [C(H16BITS, 16, 1, 5)]),
    ('masked', 'm32', (12, 4, 32), 12, 0xfff, 'M+', '', {}, [C(M32, 32, 0, 12, vl=False)]),
    ('apply', 'c64', (2060, 2, 1), 1, 0b1, 'M+', '', {}, [A2(1)]),
    ('apply', 'c64', (2060, 2, 1), 3, 0b111, 'M0', '', {}, [A2(1, pf=True)]),
    ('masked', 'c32', (2060, 2, 1), 3, 0b101, 'M+', '', {}, [A(1, C32BITS)]),
    ('apply', 'c64', (2060, 2, 1), 1, 0b1, 'EO0', 'inplace', {}, [A(1)]),
    # ---- kernel C: 16 + 3 systems (two passes), and the hand-over from kernel B at exactly 4 and 5 systems (nc <= 16) / 3 and 4 (nc >= 24)
    ('apply', 'c64', (10, 4, 8), 19, 0x7ffff, 'M+', '', {}, [C(0, 8, 2, 16), C(0, 8, 1, 3)]),
    ('apply', 'c64', (12, 4, 24), 19, 0x7ffff, 'M0', '', {}, [C(0, 24, 2, 16), C(0, 24, 1, 3)]),
    ('apply', 'c64', (10, 4, 12), 19, 0x7ffff, 'M+', '', {}, [C(0, 12, 0, 16), C(0, 12, 1, 3)]),
    ('apply', 'c64', (10, 4, 24), 19, 0x7ffff, 'M+', '', {'stencil_mfma': 2}, [C(0, 24, 0, 16), C(0, 24, 0, 3)]),
    ('apply', 'c64', (12, 4, 32), 17, 0x1ffff, 'M+', '', {}, [C(0, 32, 0, 16), C(0, 32, 1, 1)]),
    ('masked', 'c64', (10, 4, 16), 5, 0b10111, 'M+', '', {}, [B(0, 5, 4, 5, 3)]),
    ('masked', 'c64', (10, 4, 16), 6, 0b101111, 'M+', '', {}, [C(0, 16, 1, 5)]),
    ('masked', 'c64', (10, 4, 24), 4, 0b1111, 'M+', '', {}, [C(0, 24, 1, 4)]),
    ('masked', 'c64', (10, 4, 24), 5, 0b11011, 'M+', '', {}, [C(0, 24, 1, 4)]),
    ('masked', 'c64', (10, 4, 24), 4, 0b1101, 'M+', '', {}, [B(0, 12, 4, 5, 2)]),
    ('masked', 'c64', (10, 4, 8), 5, 0b10111, 'M+', '', {}, [B(0, 2, 4, 5, 6)]),
    ('masked', 'c64', (10, 4, 32), 4, 0b1111, 'M+', '', {}, [C(0, 32, 1, 4)]),
    ('masked', 'c64', (10, 4, 32), 3, 0b111, 'M+', '', {}, [B(0, 12, 4, 3, 2)]),
    # ---- kernel B: the LDS-driven tile halving (nc = 16) and the KR fallback (nc = 32, 48) with the matrix cores off
    ('masked', 'c64', (34, 4, 16), 6, 0b101111, 'M+', '', {'stencil_mfma': 0}, [B(0, 6, 8, 6, 2)]),
    ('masked', 'c64', (34, 4, 16), 3, 0b101, 'M+', '', {}, [B(0, 6, 4, 6, 2)]),
    ('masked', 'c64', (12, 4, 32), 6, 0b101111, 'M+', '', {'stencil_mfma': 0}, [B(0, 8, 8, 2, 4)]),
    ('masked', 'c64', (12, 4, 32), 3, 0b101, 'M+', '', {'stencil_mfma': 0}, [B(0, 12, 4, 3, 2)]),
    ('masked', 'c64', (6, 4, 48), 6, 0b101111, 'M+', '', {}, [B(0, 9, 8, 1, 5)]),
    ('masked', 'c64', (6, 4, 48), 3, 0b101, 'M0', '', {}, [B(0, 9, 4, 1, 5)]),
    ('masked', 'c32', (6, 4, 48), 6, 0b101111, 'M+', '', {}, [B32(C32BITS, 5, 8, 1, 5)]),
    ('masked', 'm32', (34, 4, 16), 6, 0b101111, 'M+', '', {'stencil_mfma': 0}, [B32(M32, 6, 4, 12, 1)]),
    # ---- kernel S: the full route at stencil_site = 7 (the twin of the slab and direct-Wilson tests) and the decline at the default knob
    ('apply', 'c64', (10, 4, 2), 1, 0b1, 'M0', '', {'stencil_site': 7}, [S(0, 1, zero=True)]),
    ('apply', 'c64', (10, 4, 2), 1, 0b1, 'M+', '', {'stencil_site': 7}, [S(0, 1)]),
    ('masked', 'c64', (10, 4, 2), 4, 0b1101, 'M0', '', {'stencil_site': 7}, [S(0, 1, zero=True, batch=True)]),
    ('masked', 'c64', (10, 4, 2), 4, 0b1101, 'HOP+', '', {'stencil_site': 7}, [S(0, 2, batch=True)]),
    ('apply', 'c64', (10, 4, 2), 1, 0b1, 'XPYM+', '', {'stencil_site': 7}, [S(0, 0)]),
    ('apply', 'c64', (10, 4, 2), 1, 0b1, 'EVEN0', '', {'stencil_site': 7}, [S(0, 1, zero=True)]),
    ('apply', 'c64', (10, 4, 2), 1, 0b1, 'M0', '', {}, [A2(2)]),
    ('apply', 'c64', (10, 4, 2), 1, 0b1, 'HOP0', '', {}, [S(0, 2, zero=True)]),
    ('masked', 'c64', (10, 4, 2), 4, 0b1101, 'HOP0', '', {}, [A2(2)]),
    ('apply', 'c64', (10, 4, 2), 1, 0b1, 'M0', 'noclover', {}, [S(0, 2, zero=True)]),
    ('masked', 'c32', (10, 4, 2), 4, 0b1101, 'MIX0', '', {}, [S(C32BITS, 0, batch=True)]),
    ('masked', 'c32', (10, 4, 2), 1, 0b1, 'ODD+', '', {}, [S(C32BITS, 1)]),
    ('h16', 'h16', (10, 4, 2), 4, 0b1101, 'YPXM0', '', {}, [S(H16BITS, 0, batch=True)]),
    ('h16', 'h16', (1030, 2, 2), 1, 0b1, 'M0', '', {}, [S(H16BITS, 1, zero=True)]),
    ('masked', 'c32', (10, 4, 2), 4, 0b1101, 'M0', 'nohopping', {}, [S(C32BITS, 0, batch=True)]),
    ('masked', 'c32', (10, 4, 2), 4, 0b1101, 'M0', 'noclover', {}, [S(C32BITS, 2, zero=True, batch=True)]),
    ('masked', 'c64', (10, 4, 2), 4, 0b1101, 'XPYM+', '', {'stencil_site': 7}, [S(0, 0, batch=True)]),          # fp64, no complete set of hops, batch
    ('h16', 'h16', (10, 4, 2), 1, 0b1, 'HOP+', '', {}, [S(H16BITS, 2)]),                                         # 16-bit, four hops accumulated
    ('h16', 'h16', (10, 4, 2), 4, 0b1101, 'HOP+', '', {}, [S(H16BITS, 2, batch=True)]),
    # ---- kernels A2 against A: both parities or one, lhs == rhs, fp32, stencil_pair = 0, the prefetch on and off
    ('apply', 'c64', (10, 4, 1), 3, 0b111, 'M0', '', {}, [A2(1, pf=True)]),
    ('apply', 'c64', (10, 4, 1), 3, 0b111, 'M0', '', {'pair_prefetch': 0}, [A2(1)]),
    ('masked', 'c64', (10, 4, 1), 4, 0b1101, 'M+', '', {}, [A2(1, pf=True)]),
    ('apply', 'c64', (10, 4, 1), 3, 0b111, 'M0', '', {'stencil_pair': 0}, [A(1)]),
    ('apply', 'c64', (10, 4, 1), 1, 0b1, 'EO0', 'inplace', {}, [A(1)]),
    ('apply', 'c64', (10, 4, 1), 1, 0b1, 'OE0', 'inplace', {}, [A(1)]),
    ('apply', 'c64', (10, 4, 4), 1, 0b1, 'EO0', 'inplace', {}, [A(4)]),
    ('apply', 'c64', (10, 4, 1), 1, 0b1, 'ODD+', '', {}, [A(1)]),
    ('masked', 'c64', (10, 4, 4), 4, 0b1101, 'XPYM+', '', {}, [A2(4)]),
    ('masked', 'c64', (10, 4, 4), 4, 0b1101, 'EVEN0', '', {}, [A(4)]),
    ('masked', 'c32', (10, 4, 4), 4, 0b1101, 'YPXM0', '', {}, [A(4, C32BITS)]),
    ('masked', 'c32', (10, 4, 1), 4, 0b1101, 'EVEN0', '', {}, [A(1, C32BITS)]),
    ('norm2', 'c64', (10, 4, 1), 3, 0b111, 'M0', '', {}, [A2(1, norm=True, pf=True)]),
    ('norm2', 'c64', (10, 4, 1), 3, 0b111, 'M+', '', {'pair_prefetch': 0}, [A2(1, norm=True)]),
    ('norm2', 'c64', (10, 4, 2), 3, 0b111, 'M0', '', {}, [A2(2, norm=True)]),
    ('norm2', 'c64', (2060, 2, 1), 1, 0b1, 'HOP0', '', {}, [A2(1, norm=True)]),
    # ---- single directions, one parity, a missing field in kernels B / B32 / C
    ('apply', 'c64', (10, 4, 3), 1, 0b1, 'XPYM+', '', {}, [B(0, 1, 1, 5, 3)]),
    ('masked', 'c64', (10, 4, 3), 4, 0b1101, 'YPXM0', '', {}, [B(0, 1, 4, 5, 3)]),
    ('apply', 'c64', (10, 4, 3), 1, 0b1, 'XM+', '', {}, [B(0, 1, 1, 5, 3)]),
    ('apply', 'c64', (10, 4, 3), 1, 0b1, 'YM+', '', {}, [B(0, 1, 1, 5, 3)]),
    ('apply', 'c64', (10, 4, 3), 1, 0b1, 'OXP+', '', {}, [B(0, 1, 1, 5, 3)]),
    ('apply', 'c64', (10, 4, 3), 1, 0b1, 'OYP+', '', {}, [B(0, 1, 1, 5, 3)]),
    ('apply', 'c64', (10, 4, 3), 1, 0b1, 'ODD+', '', {}, [B(0, 1, 1, 5, 3)]),
    ('apply', 'c64', (10, 4, 3), 1, 0b1, 'SHIFT+', '', {}, [B(0, 1, 1, 5, 3)]),
    ('apply', 'c64', (10, 4, 3), 1, 0b1, 'M0', 'noclover', {}, [B(0, 1, 1, 5, 3)]),
    ('apply', 'c64', (10, 4, 3), 1, 0b1, 'M0', 'nohopping', {}, [B(0, 1, 1, 5, 3)]),
    ('apply', 'c64', (10, 4, 3), 1, 0b1, 'EO0', 'inplace', {}, [B(0, 1, 1, 5, 3)]),
    ('masked', 'm32', (10, 4, 6), 4, 0b1101, 'XPYM+', '', {}, [B32(M32, 1, 4, 5, 6)]),
    ('masked', 'c32', (10, 4, 6), 4, 0b1101, 'YPXM0', '', {}, [B32(C32BITS, 1, 4, 5, 6)]),
    ('masked', 'm16', (10, 4, 8), 4, 0b1101, 'ODD+', '', {}, [B32(M32 | M16, 1, 4, 5, 6)]),
    ('masked', 'm32', (10, 4, 6), 4, 0b1101, 'M0', 'noclover', {}, [B32(M32, 1, 4, 5, 6)]),
    ('masked', 'c64', (10, 4, 12), 6, 0b101111, 'XPYM+', '', {}, [C(0, 12, 1, 5)]),
    ('masked', 'c64', (10, 4, 12), 6, 0b101111, 'YPXM0', '', {}, [C(0, 12, 1, 5)]),
    ('masked', 'c64', (10, 4, 12), 6, 0b101111, 'ODD+', '', {}, [C(0, 12, 1, 5)]),
    ('masked', 'c64', (10, 4, 12), 6, 0b101111, 'M0', 'noclover', {}, [C(0, 12, 1, 5)]),
    ('masked', 'c64', (10, 4, 12), 6, 0b101111, 'M0', 'nohopping', {}, [C(0, 12, 1, 5)]),
    ('masked', 'c32', (12, 4, 8), 6, 0b101111, 'XPYM+', '', {}, [C(C32BITS, 8, 1, 5, pair=True)]),
    ('masked', 'm16', (10, 4, 16), 12, 0xffd, 'YPXM0', '', {}, [C(M32 | M16, 16, 0, 11, vl=False)]),
    ('masked', 'c64', (10, 4, 8), 6, 0b101111, 'EO0', 'inplace', {}, [C(0, 8, 1, 5)]),
    # ---- the epilogue: out = other_scale other + acc_scale acc, with and without the dots, on system 0 and another
    ('epi', 'c64', (12, 4, 24), 2, 0b10, 'M0', 'other dots', {}, [B(0, 12, 1, 5, 2, epi=2)]),
    ('epi', 'c64', (10, 4, 3), 2, 0b1, 'EO0', 'other', {}, [B(0, 1, 1, 5, 3, epi=1)]),
    ('epi', 'c64', (10, 4, 3), 2, 0b10, 'OE0', 'dots', {}, [B(0, 1, 1, 5, 3, epi=2)]),
    ('epi', 'm32', (12, 4, 24), 2, 0b10, 'M0', 'other dots', {}, [B32(M32, 6, 1, 5, 2, epi=2)]),
    ('epi', 'c32', (10, 4, 8), 2, 0b1, 'M0', 'other dots', {}, [B32(C32BITS, 1, 1, 5, 6, epi=2)]),
    ('epi', 'm16', (10, 4, 12), 2, 0b10, 'EO0', 'other dots', {}, [B32(M32 | M16, 1, 1, 5, 4, epi=2)]),
    ('epi', 'm32', (10, 4, 7), 2, 0b10, 'M0', 'other dots', {}, [B(M32, 1, 1, 5, 7, epi=2)]),
    # ---- the 1 x 1 lattice: the shift term alone on the one (even) site
    ('masked', 'c64', (1, 1, 4), 3, 0b101, 'M+', '', {}, [V1(0, False, True)]),
    ('masked', 'c64', (1, 1, 3), 3, 0b101, 'M0', '', {}, [V1(0, True, True)]),
    ('masked', 'c64', (1, 1, 2), 1, 0b1, 'HOP0', '', {}, [V1(0, True, False)]),
    ('masked', 'c64', (1, 1, 2), 2, 0b11, 'HOP+', '', {}, [NOTHING]),
    ('masked', 'c32', (1, 1, 4), 3, 0b101, 'M+', '', {}, [V1(C32BITS, False, True)]),
    ('masked', 'c32', (1, 1, 3), 3, 0b110, 'M0', '', {}, [V1(C32BITS, True, True)]),
    ('masked', 'c32', (1, 1, 1), 1, 0b1, 'ZERO', '', {}, [V1(C32BITS, True, False)]),
    ('apply', 'c64', (1, 1, 70), 2, 0b11, 'M0', '', {}, [V1(0, True, True)]),
    # ---- rows beyond grid.y = 65535: 65540 rows (kernel A2: 65540 row pairs) that blocks walk
    ('apply', 'c64', (2, 131080, 1), 1, 0b1, 'M0', 'tall', {}, [A2(1)]),
    ('apply', 'c64', (2, 131080, 2), 1, 0b1, 'M+', 'tall', {}, [A2(2)]),
    ('apply', 'c64', (2, 32770, 1), 1, 0b1, 'M0', 'tall', {'stencil_pair': 0}, [A(1)]),
    ('apply', 'c64', (2, 32770, 2), 2, 0b11, 'M0', 'tall', {'stencil_pair': 0}, [A(2)]),
    ('masked', 'c32', (2, 32770, 1), 2, 0b10, 'M+', 'tall', {}, [A(1, C32BITS)]),
    ('masked', 'c32', (2, 32770, 2), 2, 0b10, 'M0', 'tall', {}, [S(C32BITS, 1, zero=True)]),
    ('apply', 'c64', (2, 32770, 2), 1, 0b1, 'M0', 'tall', {'stencil_site': 7}, [S(0, 1, zero=True)]),
    ('h16', 'h16', (2, 32770, 2), 1, 0b1, 'M+', 'tall', {}, [S(H16BITS, 1)]),
    ('apply', 'c64', (2, 32770, 3), 1, 0b1, 'M0', 'tall', {}, [B(0, 1, 1, 1, 3)]),
    # ---- ... kernel A2 with the fused norm: the LDS accumulator of a block lives across the row pairs it walks; two systems
    ('norm2', 'c64', (2, 131080, 1), 2, 0b11, 'M0', 'tall', {}, [A2(1, norm=True, pf=True)]),
    ('norm2', 'c64', (2, 131080, 2), 2, 0b11, 'M+', 'tall', {}, [A2(2, norm=True)]),
    # ---- ... kernel B32 at nc = 6, the smallest even nc the plan sends there with complex<float> matrices
    ('masked', 'm32', (2, 32770, 6), 1, 0b1, 'M0', 'tall', {}, [B32(M32, 1, 1, 1, 6)]),
    # ---- ... kernel C (nc = 8, five systems), which restages its matrix tiles per row: the plain form where hr = 1 is odd with complex<float>
    #      matrices (168 MB of them), the PAIR form at hr = 2 with complex<half> matrices and complex<float> vectors (168 MB + 84 MB)
    ('masked', 'm32', (2, 32770, 8), 5, 0b11111, 'M0', 'tall', {}, [C(M32, 8, 1, 5)]),
    ('masked', 'm16v32', (4, 32770, 8), 5, 0b11111, 'M0', 'tall', {}, [C(H16BITS, 8, 1, 5, pair=True)]),
    # ---- the dots cap of kernel B's epilogue: gx = 1, so grid.y = 2048 blocks walk the 2060 (parity, y) rows
    ('epi', 'c64', (2, 1030, 3), 2, 0b10, 'M0', 'other dots dotscap', {}, [B(0, 1, 1, 1, 3, epi=2)]),
]
# ---- table end


def route_id(row):
    entry, storage, dims, nrhs, mask, pieces, flags, knobs = row[:8]
    return "%s-%s-%dx%dx%d-n%d-%x-%s%s%s" % ((entry, storage) + dims + (nrhs, mask, pieces, "-" + flags.replace(" ", "-") if flags else "",
                                                                       "".join("-%s%d" % kv for kv in sorted(knobs.items()))))


def active(mask, nrhs):
    return [k for k in range(nrhs) if (mask >> k) & 1]


def expected_family(row):
    return row[8][0][0]


def set_knobs(knobs):
    for key, value in {**DEFAULT_KNOBS, **knobs}.items():
        qmg.set_tuning(key, value)


def plan_of(entry, storage, dims, n_active, holes, pieces, flags):
    """what qmg_stencil_plan answers at the current knobs"""
    mat, vec32 = STORAGE[storage][2:]
    return qmg.stencil_plan(ENTRY[entry], mat, vec32, dims, PIECES[pieces], n_active, holes, "inplace" in flags, "noclover" not in flags, "nohopping" not in flags,
                            (2 if "dots" in flags else 1) if entry == "epi" else 0, int(entry[4]) if entry.startswith("slab") else 0)


def planned(row):
    entry, storage, dims, nrhs, mask, pieces, flags = row[:7]
    act = active(mask, nrhs)
    return plan_of(entry, storage, dims, len(act), (act[0] != 0) if entry == "epi" else len(act) < nrhs, pieces, flags)


@pytest.fixture(scope="module", autouse=True)
def _device():
    qmg.build()
    qmg.init(0)
    yield
    set_knobs({})
    qmg.sync()


def r32(a):
    return np.ascontiguousarray(a, dtype=np.complex64).astype(np.complex128)


def r16(a):
    return a.real.astype(np.float16).astype(np.float64) + 1j * a.imag.astype(np.float16).astype(np.float64)


def to_device(a, dtype):
    """a complex host array in its device storage; complex<half> as interleaved float16 pairs"""
    if dtype == np.float16:
        h = np.empty(2 * a.size, dtype=np.float16)
        h[0::2], h[1::2] = a.real, a.imag
        return qmg.DeviceArray.from_host(h)
    return qmg.DeviceArray.from_host(np.ascontiguousarray(a, dtype=dtype))


@functools.lru_cache(maxsize=4)
def operator(dims, mdtype):
    """(clover, hopping) of a lattice as the storage holds them, computed once per shape and storage"""
    vol = dims[0] * dims[1] * dims[2] * dims[2]
    rnd = {np.complex128: lambda a: a, np.complex64: r32, np.float16: r16}[mdtype]
    return rnd(cs.gaussian_cvec(vol, 1)), rnd(cs.gaussian_cvec(4 * vol, 2))


def status_call(status, what):
    if status:
        raise qmg.QmgError("%s: status %d" % (what, status))


def call(row, desc, dl, dr, stride, extra):
    entry, storage, dims, nrhs, mask, pieces = row[:6]
    pc = PIECES[pieces]
    if entry == "apply":
        qmg.stencil_apply(desc, dl, dr, pc, nrhs, stride)
    elif entry == "h16":
        qmg.stencil_apply_h16(desc, dl, dr, pc, nrhs, stride, mask)
    elif entry == "norm2":
        extra["norms"] = qmg.stencil_apply_norm2(desc, dl, dr, pc, nrhs, stride)
    elif entry == "epi":
        system = active(mask, nrhs)[0]
        epi = qmg.make_epilogue(extra.get("other"), extra["other_scale"], extra["acc_scale"], extra.get("dotv"))
        status_call(qmg.stencil_apply_epi(qmg.C32 if STORAGE[storage][3] else qmg.C64, STORAGE[storage][2], desc, dl, dr, pc, epi, stride, system), "qmg_stencil_apply_epi_t")
        if "dotv" in extra:
            extra["dots"] = qmg.batch_mr_read_dots(nrhs)[system]
    elif storage == "c64":
        qmg.stencil_apply_batch(desc, dl, dr, pc, nrhs, stride, mask)
    elif storage == "c32":
        qmg.stencil_apply_t(qmg.C32, desc, dl, dr, pc, nrhs, stride, mask)
    elif storage == "m32":
        qmg.stencil_apply_mat32(desc, dl, dr, pc, nrhs, stride, mask)
    else:
        status_call(qmg.stencil_apply_mat16(qmg.C32 if storage == "m16v32" else qmg.C64, desc, dl, dr, pc, nrhs, stride, mask), "qmg_stencil_apply_mat16_t")


@pytest.mark.parametrize("row", ROUTES, ids=route_id)
def test_route_against_numpy_reference(row):
    try:
        set_knobs(row[7])
        check_route(row)
    finally:
        set_knobs({})


def walked_second(plan, dims, flags):
    """asserts from the plan that grid.y is capped below the rows the blocks walk (at 65535, or at 2048 / gx by the dots), and returns the mask
    over one vector of the rows reached on a second trip: rows gy .. of the kernel's own numbering -- kernel A2: the pair (2 row, 2 row + 1)
    of both parities; every other kernel: row = 2 y + parity"""
    Lx, Ly, nc = dims
    family, gx, gy = plan[0], plan[9], plan[10]
    walked = Ly // 2 if family == qmg.SF_PAIR else 2 * Ly
    assert gy < walked and (gx * gy == 2048 if "dotscap" in flags else gy == 65535 and walked == 65540), plan
    m = np.zeros((2, Ly, Lx // 2 * nc), dtype=bool)
    for r in range(gy, walked):
        if family == qmg.SF_PAIR:
            m[:, 2 * r:2 * r + 2] = True
        else:
            m[r & 1, r >> 1] = True
    return m.reshape(-1)


def check_route(row):
    entry, storage, dims, nrhs, mask, pieces, flags, knobs, plans = row
    got_plans = planned(row)
    assert [instantiation(p) for p in got_plans] == plans
    Lx, Ly, nc = dims
    size, pc = Lx * Ly * nc, PIECES[pieces]
    act = active(mask, nrhs)
    assert sum(p[11] for p in got_plans) == len(act) or plans[0][0] in (qmg.SF_UNSUPPORTED, qmg.SF_INVALID)
    second = walked_second(got_plans[0], dims, flags) if "tall" in flags or "dotscap" in flags else None
    mdtype, vdtype, _, vec32 = STORAGE[storage]
    stride = size + PAD
    clover, hopping = operator(dims, mdtype)
    if "noclover" in flags:
        clover = None
    if "nohopping" in flags:
        hopping = None
    shifts = SHIFTS if nc % 2 == 0 else SHIFTS[:2] + (0.0,)
    rhs0, lhs0 = cs.gaussian_cvec(nrhs * stride, 3), cs.gaussian_cvec(nrhs * stride, 4)
    other0, dotv0 = cs.gaussian_cvec(nrhs * stride, 5), cs.gaussian_cvec(nrhs * stride, 6)
    if vec32:
        rhs0, lhs0, other0, dotv0 = r32(rhs0), r32(lhs0), r32(other0), r32(dotv0)
    inplace = "inplace" in flags
    if inplace:
        lhs0 = rhs0
    if second is not None and pc & P.P_ZERO == P.P_ZERO:      # what the call overwrites and never reads starts as NaN
        assert not inplace
        for k in act:
            lhs0[k * stride:k * stride + size] = np.nan
    dcl = None if clover is None else to_device(clover, mdtype)
    dhop = None if hopping is None else to_device(hopping, mdtype)
    desc = qmg.make_desc(Lx, Ly, nc, dcl, dhop, *shifts)
    extra = {}
    if entry == "epi":
        extra.update(other_scale=0.75, acc_scale=-1.25)
        if "other" in flags:
            extra["other"] = to_device(other0, vdtype)
        if "dots" in flags:
            extra["dotv"] = to_device(dotv0, vdtype)

    def run():
        dl = to_device(lhs0, vdtype)
        dr = dl if inplace else to_device(rhs0, vdtype)
        call(row, desc, dl, dr, stride, extra)
        return dl.to_host()

    def reductions():     # what the last run left beside lhs: the fused norms, the epilogue's dots
        return tuple(np.array(extra[key]).tobytes() for key in ("norms", "dots") if key in extra)

    if plans[0][0] in (qmg.SF_UNSUPPORTED, qmg.SF_INVALID):
        with pytest.raises(qmg.QmgError):
            run()
        return
    raw = run()
    first_reductions = reductions()
    got = raw.astype(np.complex128)
    family = plans[0][0]
    # Arithmetic in fp32: kernel A in float, kernel S storages 0 and 1 -- and kernel C whenever matrices AND vectors are narrow (c32, m16v32):
    # its products then run on the f32 matrix pipe (v_mfma_f32_16x16x4_f32) with fp32 accumulators (qmg_stencil_mfma.hip: F32M = M32 && V32), so
    # its error scales with 2^-24 S, not 2^-53 S: an element whose terms cancel is off by far more than one rounding of the result.  Found by the
    # c32 / m16v32 rows of kernel C, which miss the fp64 bound by factors up to 148 while their relative L2 stays below TOL32_ROUND; the fp32
    # class bound (n + 1) 2^-21 S is the one that states this arithmetic.  Kernels B / B32 accumulate in fp64 in every storage.
    fp32_arithmetic = bool(plans[0][1] & V32) and family in (qmg.SF_ELEM, qmg.SF_SITE, qmg.SF_MFMA)
    l2_limit = TOL64 if not vec32 else TOL32 if fp32_arithmetic and family != qmg.SF_MFMA else TOL32_M16 if storage == "m16v32" else TOL32_ROUND
    untouched = np.ones(nrhs * stride, dtype=bool)
    half = size // 2
    for i, k in enumerate(act):
        seg = slice(k * stride, k * stride + size)
        want, S_, n = sn.apply(Lx, Ly, nc, clover, hopping, *shifts, pc, rhs0[seg], lhs0[seg])
        if entry == "epi":     # out = other_scale other + acc_scale acc on the processed parities (their lhs is overwritten: ZERO)
            o = other0[seg].astype(sn.CLD) if "other" in flags else np.zeros(size, dtype=sn.CLD)
            done = np.asarray(n > 0)
            want = np.where(done, extra["other_scale"] * o + extra["acc_scale"] * want, want)
            S_ = np.where(done, abs(extra["other_scale"]) * np.abs(o) + abs(extra["acc_scale"]) * S_, S_)
            n = n + 2 * done
        if Lx == 1:            # a parity with work is compared; one without must keep its bytes (the 1 x 1 lattice: its one site)
            if pc & (P.P_ZERO | P.P_SHIFT_E):
                untouched[seg] = False
        else:
            for p in (0, 1):
                if pc & ((P.P_CLOVER_E | P.P_SHIFT_E | P.P_ZERO_E) << p | (P.P_EO << (4 * p))):
                    untouched[k * stride + p * half:k * stride + (p + 1) * half] = False
        err = np.abs(got[seg].astype(sn.CLD) - want)
        bound = sn.elementwise_bound(S_, n, want if vec32 else None, fp32_arithmetic)
        ratio = float(np.max(np.where(err > 0, err / np.where(bound > 0, bound, np.longdouble(1e-300)), 0)))
        l2 = float(np.linalg.norm(err) / max(float(np.linalg.norm(want)), 1e-300))
        # (the figures DESIGN 10.6 quotes per family and storage: run with -s)
        print("route %s system %d plan %s: max err/bound %.3f, rel L2 %.3e" % (route_id(row), k, plans[min(i // 16, len(plans) - 1)], ratio, l2))
        assert l2 < l2_limit, (k, l2)
        assert np.all(err <= bound), (k, int(np.argmax(err - bound)), ratio)
        if second is not None:     # the rows walked second, on their own
            assert np.all(np.isfinite(raw[seg])), (k, "NaN prefill survived", int(np.count_nonzero(~np.isfinite(raw[seg][second]))), "of them on the second trip")
            l2 = float(np.linalg.norm(err[second]) / float(np.linalg.norm(want[second])))
            assert np.any(second) and l2 < l2_limit and np.all(err[second] <= bound[second]), (k, "second trip", l2)
        if entry == "norm2":
            ref = float(np.sum(np.abs(want) ** 2))
            assert abs(extra["norms"][k] - ref) <= TOL_REDUCE * ref, (k, extra["norms"][k], ref)
        if "dots" in flags:    # (Re <p, r>, Im <p, r>, <p, p>), p = out as stored, r = dotv, over the processed parities
            p_, r_ = got[seg].astype(sn.CLD)[np.asarray(n > 0)], dotv0[seg].astype(sn.CLD)[np.asarray(n > 0)]
            pr, pp = np.vdot(p_, r_), np.vdot(p_, p_).real
            scale = np.sqrt(pp * np.vdot(r_, r_).real)
            d = extra["dots"]
            assert abs(complex(d[0], d[1]) - pr) <= TOL_REDUCE * scale and abs(d[2] - pp) <= TOL_REDUCE * pp, (d, pr, pp)
    # frozen systems, every padding element, a parity no piece touches: the initial bytes
    init = np.ascontiguousarray(lhs0, dtype=vdtype)
    assert np.array_equal(raw[untouched].view(np.uint8), init[untouched].view(np.uint8))
    assert run().tobytes() == raw.tobytes()
    assert reductions() == first_reductions          # the reductions sum in a fixed order: the same bits
