"""Every kernel of the Wilson apply from the gauge links (csrc/qmg_wilson.hip: kernels W, W2, W2 on two rows) against an independent
reference, one row per instantiation qmg_wilson_plan can name, after tests/test_gpu_stencil_routes.py.

ROUTES is the table: entry point, storage, the vectors' lattice, nrhs, mask, pieces, flags, the "wilson_pair" knob and the plan the row is
meant to hit as (family, shape, ZERO, BATCH, emode).  A row first asserts that the library plans the request as the row says
(tests/test_host_wilson_plan.py fails when the plan can name an instantiation that no row expects).  Then the entry point runs on padded
strides, a mask with a hole for batch rows, a non-zero initial lhs and all three shifts set, and EVERY active system is compared with
stencil_numpy's long-double apply on oracle_lib.wilson_fill's fields (the hops entries: the hopping field times hop_scale; complex<float>
rows: links and vectors rounded to complex<float> first, so that only arithmetic error is measured):
  complex<double>   relative L2 < 1e-13 and |got - want| <= stencil_numpy.elementwise_bound
  complex<float>    relative L2 < 5e-6 (fp32 arithmetic: test_gpu_f32.py's TOL32)
  epilogue rows     `out` to the same bars, the three dots to long-double sums at the reductions' 1e-12
Frozen systems, all padding, a parity no piece touches and the rows a slab call leaves out must come back bit-identical, and a second run of
the same call must give the same bytes, dots included.  Refused rows assert that the entry point returns exactly the plan's status and
writes nothing.

Shapes: 130 x 6 (padding lanes in the last wavefront, a row count that is no power of two) unless a row is about an edge -- 2 x 2 (hr = 1:
every x-neighbour is the site's own column, +y and -y are the same row), 516 x 2 (more than one block along x in both precisions, the last
one partial), 2 x 4100 with the mode-1 epilogue (the dots cap makes each of the three forms walk several rows per block), 2 x 32770, 2 x 65540 and 2 x 131080 (65 540
(parity, y) rows, rows and row pairs: five more than the grid.y of kernel W, W2 and W2 on two rows can hold; such a `tall` row asserts the cap from the plan,
starts what it overwrites as NaN and compares the rows walked second on their own as well), the upper of two slabs of a 16 x 8 lattice with rows 0, 1, 2.
"""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import coordspace as cs
import oracle_lib as ol
import stencil_numpy as sn
from test_gpu_stencil_routes import PIECES

qmg = importlib.import_module("quantum-mg_amd")

pytestmark = pytest.mark.gpu

TOL64 = 1e-13
TOL32 = 5e-6          # fp32 arithmetic (test_gpu_f32.py)
TOL_REDUCE = 1e-12    # the dots
PAD = 6               # padding elements behind every vector and halo row pair (even: a complex<float> system stays 16-byte aligned)
SHIFTS = (0.3 - 0.1j, -0.2 + 0.05j, 0.15 - 0.25j)    # shift, eo_shift, dof_shift
W_COEFF, HOP_SCALE = 0.9, 0.53
OTHER_SCALE, ACC_SCALE = 0.75, -1.25
P = qmg


# ---- plans, as (family, shape, ZERO, BATCH, emode) of qmg_wilson_plan's sixteen ints
def W(shape, zero=False, batch=False, e=0):
    return (qmg.WF_DIRECT, shape, zero, batch, e)


def W2(zero=False, batch=False, e=0):
    return (qmg.WF_PAIR, 1, zero, batch, e)


def W22(zero=False, e=0):
    return (qmg.WF_PAIR2, 1, zero, False, e)


NOTHING = (qmg.WF_NOTHING, 0, False, False, 0)
UNSUPPORTED = (qmg.WF_UNSUPPORTED, 0, False, False, 0)
INVALID = (qmg.WF_INVALID, 0, False, False, 0)
SERVED = (qmg.WF_DIRECT, qmg.WF_PAIR, qmg.WF_PAIR2)
STATUS = {qmg.WF_NOTHING: 0, qmg.WF_INVALID: 1, qmg.WF_UNSUPPORTED: 3}

# ---- table begin
# (entry, storage, (Lx, Ly), nrhs, mask, pieces, flags, wilson_pair, plan)
#   entry  apply / hops: qmg_wilson_apply_direct / qmg_wilson_hops_direct; apply_epi / hops_epi: their _epi forms
#   flags  inplace | other (epi->other) | dots (epi->dotv, a vector of its own) | dotsrhs (epi->dotv = rhs) | dotsother (epi->dotv = epi->other) |
#          aliaslhs (epi->other = lhs) | slab0 / slab1 / slab2 (the upper half of a lattice of 2 Ly rows, rows = 0 / 1 / 2) | nohalos | tall
ROUTES = [
    # ======== one row per instantiation the plan can name, complex<double>
    # ---- kernel W (k_wilson_direct)
    ('apply', 'c64', (130, 6), 1, 0b1, 'ODD+', '', 2, W(1)),
    ('apply', 'c64', (130, 6), 1, 0b1, 'EVEN0', '', 2, W(1, zero=True)),
    ('apply', 'c64', (130, 6), 3, 0b101, 'M+', '', 0, W(1, batch=True)),
    ('apply', 'c64', (130, 6), 3, 0b101, 'M0', '', 0, W(1, zero=True, batch=True)),
    ('apply', 'c64', (130, 6), 1, 0b1, 'OE+', 'inplace', 2, W(2)),
    ('apply', 'c64', (130, 6), 1, 0b1, 'EO0', '', 2, W(2, zero=True)),
    ('apply', 'c64', (130, 6), 3, 0b101, 'HOP+', '', 2, W(2, batch=True)),
    ('apply', 'c64', (130, 6), 3, 0b101, 'HOP0', '', 2, W(2, zero=True, batch=True)),
    ('hops', 'c64', (130, 6), 1, 0b1, 'OE+', 'inplace', 2, W(3)),
    ('hops', 'c64', (130, 6), 1, 0b1, 'EO0', '', 2, W(3, zero=True)),
    ('hops', 'c64', (130, 6), 3, 0b101, 'HOP+', '', 2, W(3, batch=True)),
    ('hops', 'c64', (130, 6), 3, 0b101, 'HOP0', '', 2, W(3, zero=True, batch=True)),
    ('apply_epi', 'c64', (130, 6), 2, 0b10, 'EVEN0', 'dotsrhs', 2, W(1, zero=True, e=1)),
    ('apply_epi', 'c64', (130, 6), 2, 0b10, 'EVEN0', 'other', 2, W(1, zero=True, e=2)),
    ('apply_epi', 'c64', (130, 6), 2, 0b10, 'EVEN0', 'other dotsother', 2, W(1, zero=True, e=3)),
    ('apply_epi', 'c64', (130, 6), 2, 0b10, 'EVEN0', 'dots', 2, W(1, zero=True, e=4)),
    ('apply_epi', 'c64', (130, 6), 2, 0b10, 'HOP0', 'other', 2, W(2, zero=True, e=2)),
    ('apply_epi', 'c64', (130, 6), 2, 0b10, 'EO0', 'other dotsother', 2, W(2, zero=True, e=3)),
    ('apply_epi', 'c64', (130, 6), 2, 0b10, 'OE0', 'dots', 2, W(2, zero=True, e=4)),
    ('hops_epi', 'c64', (130, 6), 2, 0b10, 'EO0', 'other', 2, W(3, zero=True, e=2)),
    ('hops_epi', 'c64', (130, 6), 2, 0b10, 'OE0', 'other dotsother', 2, W(3, zero=True, e=3)),
    ('hops_epi', 'c64', (130, 6), 2, 0b10, 'HOP0', 'dots', 2, W(3, zero=True, e=4)),
    # ---- kernel W2 (k_wilson_pair)
    ('apply', 'c64', (130, 6), 1, 0b1, 'M+', '', 1, W2()),
    ('apply', 'c64', (130, 6), 1, 0b1, 'M0', '', 1, W2(zero=True)),
    ('apply', 'c64', (130, 6), 3, 0b101, 'M+', '', 2, W2(batch=True)),
    ('apply', 'c64', (130, 6), 3, 0b101, 'M0', '', 2, W2(zero=True, batch=True)),
    ('apply_epi', 'c64', (130, 6), 2, 0b10, 'M0', 'dotsrhs', 1, W2(zero=True, e=1)),
    ('apply_epi', 'c64', (130, 6), 2, 0b10, 'M0', 'other', 2, W2(zero=True, e=2)),
    ('apply_epi', 'c64', (130, 6), 2, 0b10, 'M0', 'other dotsother', 2, W2(zero=True, e=3)),
    ('apply_epi', 'c64', (130, 6), 2, 0b10, 'M0', 'dots', 2, W2(zero=True, e=4)),
    # ---- kernel W2 on two rows (k_wilson_pair2)
    ('apply', 'c64', (130, 6), 1, 0b1, 'M+', '', 2, W22()),
    ('apply', 'c64', (130, 6), 1, 0b1, 'M0', '', 2, W22(zero=True)),
    ('apply_epi', 'c64', (130, 6), 2, 0b10, 'M0', 'dotsrhs', 2, W22(zero=True, e=1)),
    # ======== the same, complex<float>; 516 x 2 and 2 x 2 take turns with 130 x 6
    ('apply', 'c32', (130, 6), 1, 0b1, 'ODD+', '', 2, W(1)),
    ('apply', 'c32', (516, 2), 1, 0b1, 'EVEN0', '', 2, W(1, zero=True)),
    ('apply', 'c32', (130, 6), 3, 0b101, 'M+', '', 0, W(1, batch=True)),
    ('apply', 'c32', (2, 2), 3, 0b101, 'M0', '', 0, W(1, zero=True, batch=True)),
    ('apply', 'c32', (130, 6), 1, 0b1, 'OE+', 'inplace', 2, W(2)),
    ('apply', 'c32', (516, 2), 1, 0b1, 'EO0', '', 2, W(2, zero=True)),
    ('apply', 'c32', (130, 6), 3, 0b101, 'HOP+', '', 2, W(2, batch=True)),
    ('apply', 'c32', (2, 2), 3, 0b101, 'HOP0', '', 2, W(2, zero=True, batch=True)),
    ('hops', 'c32', (130, 6), 1, 0b1, 'OE+', 'inplace', 2, W(3)),
    ('hops', 'c32', (516, 2), 1, 0b1, 'EO0', '', 2, W(3, zero=True)),
    ('hops', 'c32', (130, 6), 3, 0b101, 'HOP+', '', 2, W(3, batch=True)),
    ('hops', 'c32', (2, 2), 3, 0b101, 'HOP0', '', 2, W(3, zero=True, batch=True)),
    ('apply_epi', 'c32', (130, 6), 2, 0b10, 'EVEN0', 'dotsrhs', 2, W(1, zero=True, e=1)),
    ('apply_epi', 'c32', (130, 6), 2, 0b10, 'EVEN0', 'other', 2, W(1, zero=True, e=2)),
    ('apply_epi', 'c32', (516, 2), 2, 0b10, 'EVEN0', 'other dotsother', 2, W(1, zero=True, e=3)),
    ('apply_epi', 'c32', (130, 6), 2, 0b10, 'EVEN0', 'dots', 2, W(1, zero=True, e=4)),
    ('apply_epi', 'c32', (130, 6), 2, 0b10, 'HOP0', 'other', 2, W(2, zero=True, e=2)),
    ('apply_epi', 'c32', (130, 6), 2, 0b10, 'EO0', 'other dotsother', 2, W(2, zero=True, e=3)),
    ('apply_epi', 'c32', (516, 2), 2, 0b10, 'OE0', 'dots', 2, W(2, zero=True, e=4)),
    ('hops_epi', 'c32', (130, 6), 2, 0b10, 'EO0', 'other', 2, W(3, zero=True, e=2)),
    ('hops_epi', 'c32', (130, 6), 2, 0b10, 'OE0', 'other dotsother', 2, W(3, zero=True, e=3)),
    ('hops_epi', 'c32', (516, 2), 2, 0b10, 'HOP0', 'dots', 2, W(3, zero=True, e=4)),
    ('apply', 'c32', (130, 6), 1, 0b1, 'M+', '', 1, W2()),
    ('apply', 'c32', (516, 2), 1, 0b1, 'M0', '', 1, W2(zero=True)),
    ('apply', 'c32', (130, 6), 3, 0b101, 'M+', '', 2, W2(batch=True)),
    ('apply', 'c32', (516, 2), 3, 0b101, 'M0', '', 2, W2(zero=True, batch=True)),
    ('apply_epi', 'c32', (130, 6), 2, 0b10, 'M0', 'dotsrhs', 1, W2(zero=True, e=1)),
    ('apply_epi', 'c32', (130, 6), 2, 0b10, 'M0', 'other', 2, W2(zero=True, e=2)),
    ('apply_epi', 'c32', (516, 2), 2, 0b10, 'M0', 'other dotsother', 2, W2(zero=True, e=3)),
    ('apply_epi', 'c32', (130, 6), 2, 0b10, 'M0', 'dots', 2, W2(zero=True, e=4)),
    ('apply', 'c32', (130, 6), 1, 0b1, 'M+', '', 2, W22()),
    ('apply', 'c32', (516, 2), 1, 0b1, 'M0', '', 2, W22(zero=True)),
    ('apply_epi', 'c32', (130, 6), 2, 0b10, 'M0', 'dotsrhs', 2, W22(zero=True, e=1)),
    # ======== edges
    # ---- 2 x 2: hr = 1, +x and -x are the site's own column, +y and -y the same row
    ('apply', 'c64', (2, 2), 1, 0b1, 'M0', '', 2, W22(zero=True)),
    ('apply', 'c64', (2, 2), 1, 0b1, 'M+', '', 1, W2()),
    ('apply', 'c64', (2, 2), 3, 0b110, 'M0', '', 0, W(1, zero=True, batch=True)),
    ('apply', 'c64', (2, 2), 1, 0b1, 'EO0', 'inplace', 2, W(2, zero=True)),
    ('hops', 'c64', (2, 2), 1, 0b1, 'HOP+', '', 2, W(3)),
    ('apply_epi', 'c64', (2, 2), 1, 0b1, 'M0', 'dotsrhs', 2, W22(zero=True, e=1)),
    ('apply_epi', 'c64', (2, 2), 2, 0b10, 'M0', 'other dotsother', 2, W2(zero=True, e=3)),
    ('apply', 'c32', (2, 2), 1, 0b1, 'M0', '', 2, W22(zero=True)),
    ('apply', 'c32', (2, 2), 1, 0b1, 'M+', '', 1, W2()),
    # ---- 516 x 2: three blocks along x in fp64 (the last one 4 lanes), two in fp32 (the last one 2 lanes)
    ('apply', 'c64', (516, 2), 1, 0b1, 'M0', '', 2, W22(zero=True)),
    ('apply', 'c64', (516, 2), 1, 0b1, 'M+', '', 1, W2()),
    ('apply', 'c64', (516, 2), 1, 0b1, 'M0', '', 0, W(1, zero=True)),
    ('apply', 'c64', (516, 2), 3, 0b101, 'HOP+', '', 2, W(2, batch=True)),
    ('apply_epi', 'c64', (516, 2), 2, 0b10, 'M0', 'dotsrhs', 2, W22(zero=True, e=1)),
    ('apply_epi', 'c64', (516, 2), 2, 0b10, 'M0', 'other dotsother', 2, W2(zero=True, e=3)),
    ('hops_epi', 'c64', (516, 2), 2, 0b10, 'HOP0', 'dots', 2, W(3, zero=True, e=4)),
    ('apply_epi', 'c32', (516, 2), 2, 0b10, 'M0', 'dotsrhs', 2, W22(zero=True, e=1)),
    # ---- the dots cap: gx = 1, so at most 2048 blocks walk the 2050 row pairs / 4100 rows / 8200 (parity, y) rows
    ('apply_epi', 'c64', (2, 4100), 1, 0b1, 'M0', 'dotsrhs', 2, W22(zero=True, e=1)),
    ('apply_epi', 'c64', (2, 4100), 1, 0b1, 'M0', 'dotsrhs', 1, W2(zero=True, e=1)),
    ('apply_epi', 'c64', (2, 4100), 1, 0b1, 'M0', 'dotsrhs', 0, W(1, zero=True, e=1)),
    ('apply_epi', 'c32', (2, 4100), 1, 0b1, 'M0', 'dotsrhs', 2, W22(zero=True, e=1)),
    # ---- rows beyond grid.y = 65535: 65 540 (parity, y) rows that the blocks of kernel W walk
    ('apply', 'c64', (2, 32770), 1, 0b1, 'M0', 'tall', 0, W(1, zero=True)),
    # ---- ... 65 540 rows y that the blocks of kernel W2 walk (both parities of a row per block), alone and as a batch with a masked system
    ('apply', 'c64', (2, 65540), 1, 0b1, 'M0', 'tall', 1, W2(zero=True)),
    ('apply', 'c64', (2, 65540), 3, 0b101, 'M+', 'tall', 2, W2(batch=True)),
    # ---- ... 65 540 row pairs (2 yi, 2 yi + 1) that the blocks of the two-row form walk
    ('apply', 'c64', (2, 131080), 1, 0b1, 'M0', 'tall', 2, W22(zero=True)),
    ('apply', 'c32', (2, 131080), 1, 0b1, 'M0', 'tall', 2, W22(zero=True)),
    # ---- y-slabs: rows 4 .. 7 of a 16 x 8 lattice, the links indexed on the whole lattice, rows -1 and Ly of the right-hand side from halos
    ('apply', 'c64', (16, 4), 1, 0b1, 'M0', 'slab0', 2, W22(zero=True)),
    ('apply', 'c64', (16, 4), 1, 0b1, 'M0', 'slab1', 2, W22(zero=True)),        # the interior: a row pair that starts at the odd row 1
    ('apply', 'c64', (16, 4), 1, 0b1, 'M0', 'slab2', 2, W2(zero=True)),         # the two boundary rows
    ('apply', 'c64', (16, 4), 3, 0b101, 'M+', 'slab0', 2, W2(batch=True)),
    ('apply', 'c64', (16, 4), 3, 0b101, 'M0', 'slab2', 2, W2(zero=True, batch=True)),
    ('apply', 'c64', (16, 4), 1, 0b1, 'EVEN0', 'slab1', 2, W(1, zero=True)),
    ('hops', 'c64', (16, 4), 3, 0b101, 'HOP0', 'slab0', 2, W(3, zero=True, batch=True)),
    ('hops', 'c64', (16, 4), 1, 0b1, 'OE+', 'slab2 inplace', 2, W(3)),
    ('apply', 'c32', (16, 4), 1, 0b1, 'M0', 'slab0', 2, W22(zero=True)),
    ('apply', 'c32', (16, 4), 3, 0b101, 'M0', 'slab1', 2, W2(zero=True, batch=True)),
    # ---- nothing to launch
    ('apply', 'c64', (130, 6), 1, 0b1, 'NONE', '', 2, NOTHING),
    ('apply', 'c64', (130, 6), 2, 0b00, 'M0', '', 2, NOTHING),                  # every system masked out
    ('apply', 'c64', (16, 2), 1, 0b1, 'M0', 'slab1', 2, NOTHING),               # the interior of a slab of two rows
    # ---- refused: the entry point returns the plan's status and writes nothing
    ('apply', 'c64', (130, 6), 1, 0b1, 'DIAG0', '', 2, UNSUPPORTED),            # no hops
    ('apply', 'c64', (130, 6), 1, 0b1, 'XPYM+', '', 2, UNSUPPORTED),            # single directions
    ('apply', 'c64', (130, 6), 1, 0b1, 'MIX0', '', 2, UNSUPPORTED),             # the parities ask for different sets
    ('apply', 'c64', (130, 6), 1, 0b1, 'ZERO', '', 2, UNSUPPORTED),
    ('apply', 'c32', (130, 6), 1, 0b1, 'SHIFT+', '', 2, UNSUPPORTED),
    ('hops', 'c64', (130, 6), 1, 0b1, 'M0', '', 2, UNSUPPORTED),                # the hops entries take no clover or shift piece
    ('hops', 'c64', (130, 6), 1, 0b1, 'XM+', '', 2, UNSUPPORTED),
    ('apply', 'c64', (130, 6), 1, 0b1, 'M0', 'inplace', 2, INVALID),
    ('apply', 'c64', (130, 6), 1, 0b1, 'EVEN0', 'inplace', 2, INVALID),
    ('hops', 'c32', (130, 6), 1, 0b1, 'HOP0', 'inplace', 2, INVALID),           # in place on both parities
    ('apply', 'c64', (16, 4), 1, 0b1, 'M0', 'slab0 nohalos', 2, INVALID),       # a slab needs its halos
    ('apply_epi', 'c64', (130, 6), 3, 0b101, 'M0', 'other', 2, UNSUPPORTED),    # an epilogue serves one system per launch
    ('apply_epi', 'c64', (130, 6), 2, 0b10, 'M0', 'other dots', 2, UNSUPPORTED),   # two different epilogue vectors
    ('apply_epi', 'c64', (130, 6), 2, 0b10, 'M+', 'other', 2, INVALID),         # an epilogue needs overwrite
    ('apply_epi', 'c64', (130, 6), 2, 0b10, 'M0', 'aliaslhs', 2, INVALID),
    ('hops_epi', 'c64', (130, 6), 1, 0b1, 'OE0', 'inplace dots', 2, INVALID),   # ... and an output of its own
]
# ---- table end


def route_id(row):
    entry, storage, dims, nrhs, mask, pieces, flags, pair = row[:8]
    return "%s-%s-%dx%d-n%d-%x-%s%s-pair%d" % ((entry, storage) + dims + (nrhs, mask, pieces, "-" + flags.replace(" ", "-") if flags else "", pair))


def active(mask, nrhs):
    return [k for k in range(nrhs) if (mask >> k) & 1]


def kernel_of(row):
    """(family, F32, shape, ZERO, BATCH, emode): the instantiation a row expects"""
    fam, shape, zero, batch, e = row[8]
    return (fam, row[1] == "c32", shape, zero, batch, e)


def slab_of(flags):
    """rows of a slab row's call, or None"""
    for f in flags.split():
        if f.startswith("slab"):
            return int(f[4])
    return None


def epi_bits(entry, flags):
    fl = flags.split()
    if not entry.endswith("_epi"):
        return 0
    return (qmg.WPE_ON | (qmg.WPE_OTHER if "other" in fl or "aliaslhs" in fl else 0) | (qmg.WPE_DOTV if {"dots", "dotsrhs", "dotsother"} & set(fl) else 0) |
            (qmg.WPE_DOTV_IS_OTHER if "dotsother" in fl else 0) | (qmg.WPE_DOTV_IS_RHS if "dotsrhs" in fl else 0) | (qmg.WPE_ALIASES_LHS if "aliaslhs" in fl else 0))


def planned(row):
    """what qmg_wilson_plan answers for a row's request at the current "wilson_pair" """
    entry, storage, dims, nrhs, mask, pieces, flags = row[:7]
    rows = slab_of(flags)
    return qmg.wilson_plan(qmg.C32 if storage == "c32" else qmg.C64, dims, PIECES[pieces], len(active(mask, nrhs)), "inplace" in flags, entry.startswith("hops"),
                           epi_bits(entry, flags), gauge_Ly=dims[1] if rows is None else 2 * dims[1], y0=0 if rows is None else dims[1],
                           halos=rows is not None and "nohalos" not in flags, rows=rows or 0)


def instantiation(plan):
    """the part of qmg_wilson_plan's answer that a row states"""
    family, lps, block, gx, gy, flags, shape, emode = plan[:8]
    return (family, shape, bool(flags & qmg.WPF_ZERO), bool(flags & qmg.WPF_BATCH), emode)


@pytest.fixture(scope="module", autouse=True)
def _device():
    qmg.build()
    qmg.init(0)
    yield
    qmg.set_tuning("wilson_pair", 2)
    qmg.sync()


def r32(a):
    return np.ascontiguousarray(a, dtype=np.complex64).astype(np.complex128)


@functools.lru_cache(maxsize=16)
def operator(Lx, gLy, f32):
    """(links, clover, hopping) of a lattice, computed once per shape and precision; the links as the storage holds them"""
    rng = np.random.default_rng(Lx * 1000003 + gLy)
    gauge = np.exp(1j * rng.uniform(-np.pi, np.pi, size=2 * Lx * gLy))
    if f32:
        gauge = r32(gauge)
    clover, hopping = ol.wilson_fill(gauge, Lx, gLy, W_COEFF)
    return gauge, clover, hopping


def slab_rows(a, Lx, gLy, y0, Ly):
    """rows y0 .. y0 + Ly - 1 of a vector of the Lx x gLy lattice: (parity, y, x / 2, c) with nc = 2"""
    return a.reshape(2, gLy, Lx)[:, y0:y0 + Ly].reshape(-1)


def vp(a):
    return C.c_void_p(None if a is None else a.ptr)


def call(row, dtype, desc, gauge, gLy, y0, dl, dr, lo, hi, stride, hstride, epi):
    """the entry point's status"""
    entry, storage, dims, nrhs, mask, pieces, flags = row[:7]
    lib, rows = qmg.lib(), slab_of(flags) or 0
    head = (dtype, C.byref(desc), vp(gauge), gLy, y0, C.c_double(W_COEFF)) + ((C.c_double(HOP_SCALE),) if entry.startswith("hops") else ())
    tail = (vp(dl), vp(dr), vp(lo), vp(hi), C.c_uint(PIECES[pieces]), nrhs, C.c_size_t(stride), C.c_size_t(hstride), C.c_uint(mask))
    if entry.endswith("_epi"):
        return getattr(lib, "qmg_wilson_%s_direct_epi" % entry[:-4])(*(head + tail + (C.byref(epi), None)))
    return getattr(lib, "qmg_wilson_%s_direct" % entry)(*(head + tail + (rows, None)))


@pytest.mark.parametrize("row", ROUTES, ids=route_id)
def test_route_against_numpy_reference(row):
    try:
        qmg.set_tuning("wilson_pair", row[7])
        check_route(row)
    finally:
        qmg.set_tuning("wilson_pair", 2)


def walked_second(plan, Lx, Ly):
    """asserts from the plan that grid.y is capped below the rows the blocks walk, and returns the mask over one vector of the rows reached on
    a second trip: rows gy .. of the kernel's own numbering -- kernel W: row = 2 y + parity on both parities; W2: y; W2 on two rows: the pair
    (2 row, 2 row + 1)"""
    family, gy, par_first, par_count = plan[0], plan[4], plan[14], plan[15]
    walked = {qmg.WF_DIRECT: Ly * par_count, qmg.WF_PAIR: Ly, qmg.WF_PAIR2: Ly // 2}[family]
    assert gy == 65535 < walked == 65540, plan
    m = np.zeros((2, Ly, Lx), dtype=bool)
    for r in range(gy, walked):
        if family == qmg.WF_PAIR2:
            m[:, 2 * r:2 * r + 2] = True
        elif family == qmg.WF_PAIR:
            m[:, r] = True
        elif par_count == 2:
            m[r & 1, r >> 1] = True
        else:
            m[par_first, r] = True
    return m.reshape(-1)


def check_route(row):
    entry, storage, dims, nrhs, mask, pieces, flags, pair, plan = row
    got_plan = planned(row)
    assert instantiation(got_plan) == plan
    fl = flags.split()
    f32 = storage == "c32"
    dtype, vdtype = (qmg.C32, np.complex64) if f32 else (qmg.C64, np.complex128)
    Lx, Ly = dims
    rows = slab_of(flags)
    gLy, y0 = (Ly, 0) if rows is None else (2 * Ly, Ly)
    size, gsize, pc = 2 * Lx * Ly, 2 * Lx * gLy, PIECES[pieces]
    act = active(mask, nrhs)
    served = plan[0] in SERVED
    if served:
        assert got_plan[8] == len(act) and got_plan[13] == 0
    second = None
    if "tall" in fl:                        # blocks walk the rows beyond grid.y
        second = walked_second(got_plan, Lx, Ly)
    if served and got_plan[5] & qmg.WPF_DOTS and Ly > 4096:
        assert got_plan[3] * got_plan[4] == 2048     # the dots cap: fewer blocks than rows
    rnd = r32 if f32 else (lambda a: a)
    gauge, clover, hopping = operator(Lx, gLy, f32)
    scaled = entry.startswith("hops")
    if scaled:
        clover, hopping = None, hopping * HOP_SCALE
    stride, hstride = size + PAD, 2 * Lx + PAD
    inplace = "inplace" in fl

    def local(seed):
        """the same random vector per system on the whole lattice and, with padding behind every system, as the call sees it"""
        g = rnd(cs.gaussian_cvec(nrhs * gsize, seed)).reshape(nrhs, gsize)
        loc = rnd(cs.gaussian_cvec(nrhs * stride, seed + 100))
        for k in range(nrhs):
            loc[k * stride:k * stride + size] = slab_rows(g[k], Lx, gLy, y0, Ly)
        return g, loc

    rhs_g, rhs0 = local(3)
    lhs_g, lhs0 = (rhs_g, rhs0) if inplace else local(4)
    other_g, other0 = local(5)
    dotv_g, dotv0 = local(6)
    dg = qmg.DeviceArray.from_host(np.ascontiguousarray(gauge, dtype=vdtype))
    desc = qmg.make_desc(Lx, Ly, 2, None, None, *SHIFTS)
    lo = hi = None
    if rows is not None and "nohalos" not in fl:
        halo = lambda y: np.concatenate([np.concatenate([rhs_g[k].reshape(2, gLy, Lx)[:, y % gLy].reshape(-1), np.zeros(PAD)]) for k in range(nrhs)])
        lo, hi = (qmg.DeviceArray.from_host(np.ascontiguousarray(halo(y), dtype=vdtype)) for y in (y0 - 1, y0 + Ly))
    dev = lambda a: qmg.DeviceArray.from_host(np.ascontiguousarray(a, dtype=vdtype))
    dots = {}
    start = lhs0
    if second is not None and plan[2]:      # ZERO: every processed parity is overwritten and never read, so it starts as NaN
        start = lhs0.copy()
        for k in act:
            for p in range(got_plan[14], got_plan[14] + got_plan[15]):
                start[k * stride + p * (size // 2):k * stride + (p + 1) * (size // 2)] = np.nan

    def run():
        dl = dev(start)
        dr = dl if inplace else dev(rhs0)
        epi = None
        if entry.endswith("_epi"):
            d_other = dl if "aliaslhs" in fl else dev(other0) if "other" in fl else None
            d_dotv = dr if "dotsrhs" in fl else d_other if "dotsother" in fl else dev(dotv0) if "dots" in fl else None
            epi = qmg.make_epilogue(d_other, OTHER_SCALE, ACC_SCALE, d_dotv)
        status = call(row, dtype, desc, dg, gLy, y0, dl, dr, lo, hi, stride, hstride, epi)
        if status == 0 and served and got_plan[5] & qmg.WPF_DOTS:
            dots["last"] = qmg.batch_mr_read_dots(nrhs)[act[0]]
        return status, dl.to_host()

    status, raw = run()
    init = np.ascontiguousarray(start, dtype=vdtype)
    if not served:
        assert status == STATUS[plan[0]] == got_plan[13]
        assert raw.tobytes() == init.tobytes()
        return
    assert status == 0
    first_dots = None if "last" not in dots else dots["last"].tobytes()
    got = raw.astype(np.complex128)
    row_on = np.zeros((2, Ly, Lx), dtype=bool)         # the rows of this call
    row_on[:, {None: slice(None), 0: slice(None), 1: slice(1, Ly - 1), 2: [0, Ly - 1]}[rows]] = True
    row_on = row_on.reshape(-1)
    dot_vec = rhs0 if "dotsrhs" in fl else other0 if "dotsother" in fl else dotv0
    untouched = np.ones(nrhs * stride, dtype=bool)
    for k in act:
        seg = slice(k * stride, k * stride + size)
        want, S_, n = (slab_rows(a, Lx, gLy, y0, Ly) for a in sn.apply(Lx, gLy, 2, clover, hopping, *SHIFTS, pc, rhs_g[k], lhs_g[k]))
        done = np.asarray(n > 0) & row_on              # every served piece set has the hops on each parity it processes
        if entry.endswith("_epi"):     # out = other_scale other + acc_scale acc (the processed parities are overwritten: ZERO)
            o = other0[seg].astype(sn.CLD) if "other" in fl else np.zeros(size, dtype=sn.CLD)
            want = OTHER_SCALE * o + ACC_SCALE * want
            S_ = abs(OTHER_SCALE) * np.abs(o) + abs(ACC_SCALE) * S_
            n = n + 2
        untouched[seg] = ~done
        err = np.abs(got[seg].astype(sn.CLD) - want)[done]
        l2 = float(np.linalg.norm(err) / max(float(np.linalg.norm(want[done])), 1e-300))
        print("route %s system %d plan %s: rel L2 %.3e" % (route_id(row), k, got_plan, l2))
        assert l2 < (TOL32 if f32 else TOL64), (k, l2)
        if not f32:
            bound = sn.elementwise_bound(S_, n)[done]
            assert np.all(err <= bound), (k, float(np.max(err / bound)))
        if second is not None:      # the rows walked second, on their own
            assert np.all(np.isfinite(raw[seg])), (k, "NaN prefill survived", int(np.count_nonzero(~np.isfinite(raw[seg][second]))), "of them on the second trip")
            err2 = np.abs(got[seg].astype(sn.CLD) - want)[done & second]
            l2 = float(np.linalg.norm(err2) / float(np.linalg.norm(want[done & second])))
            assert np.count_nonzero(done & second) > 0 and l2 < (TOL32 if f32 else TOL64), (k, "second trip", l2)
            assert f32 or np.all(err2 <= sn.elementwise_bound(S_, n)[done & second]), (k, "second trip")
        if "last" in dots:     # (Re <p, r>, Im <p, r>, <p, p>), p = out as stored, r = dotv, over the processed parities
            p_, r_ = got[seg].astype(sn.CLD)[done], dot_vec[seg].astype(sn.CLD)[done]
            pr, pp = np.vdot(p_, r_), np.vdot(p_, p_).real
            d = dots["last"]
            assert abs(complex(d[0], d[1]) - pr) <= TOL_REDUCE * np.sqrt(pp * np.vdot(r_, r_).real) and abs(d[2] - pp) <= TOL_REDUCE * pp, (d, pr, pp)
    # frozen systems, every padding element, a parity no piece touches, the rows a slab call leaves out: the initial bytes
    assert np.array_equal(raw[untouched].view(np.uint8), init[untouched].view(np.uint8))
    status2, raw2 = run()
    assert status2 == 0 and raw2.tobytes() == raw.tobytes()
    assert first_dots is None or dots["last"].tobytes() == first_dots          # the dots sum in a fixed order: the same bits
