"""Every batch vector kernel of csrc/qmg_batch.hip against an independent reference, one row per route.

ROUTES is the table.  A row names the entry point, the storage, n / stride padding / nrhs / mask, nj or ns (with the shift masks), the flags of
the call and the plan of every pass, in qmg_batch_plan's terms (family, W, nt, J, variant).  A row first asserts that the library routes the
request as the row says, so a retune that moves a kernel out from under its row fails here, and tests/test_host_batch_plan.py fails when a
pass exists that no row expects.  Then the entry point runs on padded strides, masks with holes and non-zero initial contents -- the output
systems that are not active hold NaN -- and EVERY element of EVERY active system is compared with batch_numpy's long-double reference
(inputs rounded to complex<float> first where the storage is narrow):
  elementwise    |got - want| <= (terms + 1) 2^-50 S, plus 2^-23 |want| for complex<float> results (batch_numpy.elementwise_bound); a
                 complex<float> sum of more than 8 vector sets is stored between its passes of 8: the reference rounds there too, and the
                 bound adds 2^-23 of those stored partial results (as r of a complex<float> GCR update adds 2^-23 |a| |w|)
  whole vector   relative L2 < 1e-13 (fp64 results) or TOL32_ROUND = 3e-7 (complex<float> results)
  reductions     |got - want| <= 1e-12 sqrt(|x|^2 |y|^2) per system and dot
Frozen systems, frozen (system, shift) pairs, all padding and every read-only operand must come back byte-identical, and a second run of the
same call on the same inputs must give the same bytes (one writer per output, fixed summation order).

Multi-axpy and GCR rows set the coefficient of vector set j for system k to zero where (j + k) % 3 == 1 and fill those slots with NaN and
Inf: a zero coefficient means "not read" (DESIGN 10.6), so every result must be finite and within the bound.

The MR update is held to the mathematics on the slot it reads: the dots the device left are compared with the reference's under the reduction
tolerance, and the update is then compared elementwise with x + alpha r, r - alpha p at alpha = omega <p,r> / <p,p> formed in long double from
those very slot values (the kernel's two fp64 roundings of alpha are inside the elementwise bound; the 1e-12 of a reduction would not be).
"""
import importlib

import numpy as np
import pytest

import batch_numpy as bn

qmg = importlib.import_module("quantum-mg_amd")

pytestmark = pytest.mark.gpu

TOL64 = 1e-13
TOL32_ROUND = 3e-7    # fp64 arithmetic, one fp32 rounding of the result (test_gpu_f32.py)
NT_DEFAULT = 256      # blas_nt_mb

C64, C32 = "c64", "c32"
DTYPE = {C64: qmg.C64, C32: qmg.C32}
NP = {C64: np.complex128, C32: np.complex64}
# the smallest long vector of each storage: BATCH_LONG_BYTES (csrc/qmg_batch_plan.h) per system
LONG_N = {C64: qmg.BATCH_LONG_BYTES // 16, C32: qmg.BATCH_LONG_BYTES // 8}
assert LONG_N == {C64: 1 << 20, C32: 1 << 21}


# ---- passes, as qmg_batch_plan writes them: (family, W, nt, J, variant)
def BLAS(W, nt, op):
    return (qmg.BF_BLAS, W, nt, 0, op)


def SMALL(W, nt, J):
    return (qmg.BF_MAXPY_SMALL, W, nt, J, 0)


def LONG(W, nt, J):
    return (qmg.BF_MAXPY_LONG, W, nt, J, 0)


def SINGLE(nt):
    return (qmg.BF_MAXPY_SINGLE, 1, nt, 0, 0)


def GCR(W, nt, J, zn):
    return (qmg.BF_GCR, W, nt, J, zn)


def CGM(W, nt, J, most):
    return (qmg.BF_CGM, W, nt, J, most)


def RED(W, nt, op):
    return (qmg.BF_REDUCE, W, nt, 0, op)


def MDOT(W, nt, KT):
    return (qmg.BF_MULTIDOT, W, nt, KT, 0)


def MRD(W, nt):
    return (qmg.BF_MR_DOTS, W, nt, 2, 0)


def MRU(W, nt, xset, rout):
    return (qmg.BF_MR_UPDATE, W, nt, 0, (qmg.BPV_XSET if xset else 0) | (qmg.BPV_ROUT if rout else 0))


NOTHING = (qmg.BF_NOTHING, 0, 0, 0, 0)

# ---- shapes: (storage, n, stride pad, nrhs, mask, W[, "misaligned"]).  W = 2 needs complex<float>, 16-byte aligned bases, even n and (nrhs > 1) an even stride.
HOLE9 = 0b101101101
SHAPES = [
    (C64, 1, 0, 1, 0b1, 1), (C64, 2, 2, 3, 0b010, 1), (C64, 255, 1, 16, 0xFFFF, 1), (C64, 256, 0, 16, 0x8421, 1), (C64, 257, 3, 9, HOLE9, 1),
    (C64, 777, 1, 3, 0b010, 1), (C64, 4098, 1, 3, 0b101, 1), (C64, 4096, 6, 1, 0b1, 1),
    (C32, 2, 0, 1, 0b1, 2), (C32, 2, 2, 3, 0b010, 2), (C32, 256, 0, 16, 0xFFFF, 2), (C32, 256, 2, 16, 0x8421, 2), (C32, 4098, 1, 1, 0b1, 2),   # (odd stride, one system: W = 2)
    (C32, 4096, 6, 9, HOLE9, 2),
    (C32, 1, 0, 1, 0b1, 1), (C32, 255, 1, 16, 0xFFFF, 1), (C32, 257, 3, 9, HOLE9, 1), (C32, 777, 1, 3, 0b010, 1),
    (C32, 4098, 1, 3, 0b101, 1),                      # even n, odd stride, three systems: W = 1
    (C32, 4096, 6, 3, 0b110, 1, "misaligned"),        # every base 8 bytes past a 16-byte boundary
]
CLASSES = [(C64, 1), (C32, 2), (C32, 1)]
# a batch that passes blas_nt_mb = 1: 8 active systems of 1 MiB / 8 each, one per (storage, W); W = 1 in complex<float> from an odd n
NT_SHAPE = {(C64, 1): (C64, 8192, 0, 8, 0xFF, 1), (C32, 2): (C32, 16384, 2, 8, 0xFF, 2), (C32, 1): (C32, 16385, 1, 8, 0xFF, 1)}
# five systems of which system 0 is idle in the non-temporal multi-shift rows below: the four others pass blas_nt_mb = 1
NT_SHAPE5 = {(C64, 1): (C64, 16384, 0, 5, 0x1F, 1), (C32, 2): (C32, 32768, 2, 5, 0x1F, 2), (C32, 1): (C32, 32769, 1, 5, 0x1F, 1)}


def shapes_of(cls):
    return [s for s in SHAPES if (s[0], s[5]) == cls]


def row(entry, shape, plans, **kw):
    r = dict(entry=entry, st=shape[0], n=shape[1], pad=shape[2], nrhs=shape[3], mask=shape[4], mis=len(shape) > 6, plans=plans, op=0, nj=0, shift_masks=None, znext=False,
             xset=False, rout="distinct", alias=False, nt_mb=None)
    r.update(kw)
    return r


def chunks8(make, nj):
    """the passes of nj vector sets, 8 at a time"""
    return [make(min(8, nj - j0)) for j0 in range(0, nj, 8)]


def gcr_small(W, nt, nj, zn):
    """all but the last chunk of 8 through the multi-axpy, the rest with the update"""
    lead = ((nj - 1) // 8) * 8 if nj > 8 else 0
    return [SMALL(W, nt, 8)] * (lead // 8) + [GCR(W, nt, nj - lead, zn)]


def stair(ns, nrhs, cap):
    """shift masks in which system k iterates (k % (cap + 1), at most the launch's shifts) of every launch of 8 shifts, at rotating slots"""
    masks = [0] * ns
    for s0 in range(0, ns, 8):
        J = min(8, ns - s0)
        for k in range(nrhs):
            for j in range(J):
                if (j + k) % J < min(k % (cap + 1), J):
                    masks[s0 + j] |= 1 << k
    return masks


def flat(ns, nrhs, most):
    """shift masks in which every system but system 0 iterates `most` of the ns <= 8 shifts, at rotating slots"""
    return [sum(1 << k for k in range(1, nrhs) if (j + k) % ns < most) for j in range(ns)]


ROUTES = []

# ======== qmg_batch_blas_t: the ten ops on every shape, and past blas_nt_mb (CAXPBYZ there with y aliasing z -- then y is the in/out operand -- and distinct)
for op in range(10):
    for sh in SHAPES:
        ROUTES.append(row("blas", sh, [BLAS(sh[5], 0, op)], op=op))
    for cls in CLASSES:
        ROUTES.append(row("blas", NT_SHAPE[cls], [BLAS(cls[1], 1, op)], op=op, nt_mb=1))
for cls in CLASSES:
    ROUTES.append(row("blas", NT_SHAPE[cls], [BLAS(cls[1], 1, bn.CAXPBYZ)], op=bn.CAXPBYZ, nt_mb=1, alias=True))
    ROUTES.append(row("blas", shapes_of(cls)[2], [BLAS(cls[1], 0, bn.CAXPBYZ)], op=bn.CAXPBYZ, alias=True))

# ======== qmg_batch_multi_caxpy_t, short vectors: every chunk width 1..8 and nj across one, two and four launches, on rotating shapes
for cls in CLASSES:
    W = cls[1]
    sel = shapes_of(cls)
    for i, nj in enumerate((0, 1, 7, 8, 9, 16, 17, 32, 2, 3, 4, 5, 6)):
        sh = sel[i % len(sel)]
        ROUTES.append(row("maxpy", sh, chunks8(lambda J: SMALL(W, 0, J), nj) or [NOTHING], nj=nj))
    for nj in range(1, 9):
        ROUTES.append(row("maxpy", NT_SHAPE[cls], [SMALL(W, 1, nj)], nj=nj, nt_mb=1))
# ======== ... long vectors: k_bmulti_caxpy with each of its eight instantiations, plain and non-temporal
for nj in range(1, 9):
    ROUTES.append(row("maxpy", (C64, LONG_N[C64], 2, 2, 0b11, 1), [LONG(1, 0, nj)], nj=nj))
    ROUTES.append(row("maxpy", (C64, LONG_N[C64], 2, 2, 0b10, 1), [LONG(1, 1, nj)], nj=nj, nt_mb=1))
    ROUTES.append(row("maxpy", (C32, LONG_N[C32], 2, 1, 0b1, 2), [LONG(2, 0, nj)], nj=nj))
    ROUTES.append(row("maxpy", (C32, LONG_N[C32], 2, 1, 0b1, 2), [LONG(2, 1, nj)], nj=nj, nt_mb=1))
    ROUTES.append(row("maxpy", (C32, LONG_N[C32], 2, 1, 0b1, 1, "misaligned"), [LONG(1, 0, nj)], nj=nj))
    ROUTES.append(row("maxpy", (C32, LONG_N[C32], 2, 1, 0b1, 1, "misaligned"), [LONG(1, 1, nj)], nj=nj, nt_mb=1))
ROUTES.append(row("maxpy", (C64, LONG_N[C64], 2, 2, 0b10, 1), [LONG(1, 0, 8), LONG(1, 0, 3)], nj=11))
# ======== ... ONE complex<double> system on long vectors: the single-vector kernel
for nj in (1, 5, 9):
    ROUTES.append(row("maxpy", (C64, LONG_N[C64], 0, 1, 0b1, 1), [SINGLE(0)], nj=nj))
ROUTES.append(row("maxpy", (C64, LONG_N[C64], 0, 1, 0b1, 1), [SINGLE(1)], nj=5, nt_mb=1))
# (one element short of a long vector: the short form, for one system and for two)
ROUTES.append(row("maxpy", (C64, LONG_N[C64] - 1, 1, 1, 0b1, 1), [SMALL(1, 0, 2)], nj=2))

# ======== qmg_batch_gcr_update_t, short vectors: nj across the `lead` split (9, 16, 17), every tail width 0..8, with and without z_next
for cls in CLASSES:
    W = cls[1]
    sel = shapes_of(cls)
    for i, nj in enumerate((0, 1, 7, 8, 9, 16, 17, 32, 2, 3, 4, 5, 6)):
        for zn in (0, 1):
            ROUTES.append(row("gcr", sel[(i + zn) % len(sel)], gcr_small(W, 0, nj, zn), nj=nj, znext=bool(zn)))
    for nj in range(0, 9):
        for zn in (0, 1):
            ROUTES.append(row("gcr", NT_SHAPE[cls], [GCR(W, 1, nj, zn)], nj=nj, znext=bool(zn), nt_mb=1))
# ======== ... long vectors: every chunk through the multi-axpy (lead = nj), the update itself with no vector set
for zn, nj in ((1, 0), (0, 3), (1, 9)):
    ROUTES.append(row("gcr", (C64, LONG_N[C64], 0, 1, 0b1, 1), ([SINGLE(0)] if nj else []) + [GCR(1, 0, 0, zn)], nj=nj, znext=bool(zn)))
    ROUTES.append(row("gcr", (C64, LONG_N[C64], 2, 2, 0b11, 1), chunks8(lambda J: LONG(1, 0, J), nj) + [GCR(1, 0, 0, zn)], nj=nj, znext=bool(zn)))
ROUTES.append(row("gcr", (C32, LONG_N[C32], 2, 1, 0b1, 2), [LONG(2, 0, 3), GCR(2, 0, 0, 1)], nj=3, znext=True))

# ======== qmg_batch_cgm_update_t: every (shifts of the launch, largest per-system count) pair, per-system counts 0 .. that (system 0 of the nine
# iterates nothing: all its shifts are frozen), plain and non-temporal
for cls in CLASSES:
    W = cls[1]
    small9 = {(C64, 1): (C64, 257, 3, 9, 0x1FF, 1), (C32, 2): (C32, 256, 2, 9, 0x1FF, 2), (C32, 1): (C32, 777, 1, 9, 0x1FF, 1)}[cls]
    for J in range(1, 9):
        for most in range(1, J + 1):
            ROUTES.append(row("cgm", small9, [CGM(W, 0, J, most)], nj=J, shift_masks=stair(J, 9, most)))
            ROUTES.append(row("cgm", NT_SHAPE5[cls], [CGM(W, 1, J, most)], nj=J, shift_masks=flat(J, 5, most), nt_mb=1))
# ... sixteen systems whose counts take every value 0..8 in one launch; ns across the launch split (8 + 1, 8 + 8); holes in the mask; one system
ROUTES += [
    row("cgm", (C64, 255, 1, 16, 0xFFFF, 1), [CGM(1, 0, 8, 8)], nj=8, shift_masks=stair(8, 16, 8)),
    row("cgm", (C32, 256, 0, 16, 0xFFFF, 2), [CGM(2, 0, 8, 8), CGM(2, 0, 8, 8)], nj=16, shift_masks=stair(16, 16, 8)),
    row("cgm", (C64, 256, 0, 16, 0x8421, 1), [CGM(1, 0, 8, 6), CGM(1, 0, 1, 1)], nj=9, shift_masks=stair(9, 16, 8)),   # (of systems 0, 5, 10, 15: counts 0, 5, 1, 6)
    row("cgm", (C64, 4098, 1, 3, 0b101, 1), [CGM(1, 0, 3, 2)], nj=3, shift_masks=stair(3, 3, 3)),
    row("cgm", (C32, 4098, 1, 3, 0b101, 1), [CGM(1, 0, 4, 2)], nj=4, shift_masks=stair(4, 3, 4)),
    row("cgm", (C32, 4096, 6, 3, 0b110, 1, "misaligned"), [CGM(1, 0, 5, 2)], nj=5, shift_masks=stair(5, 3, 5)),
    row("cgm", (C64, 1, 0, 1, 0b1, 1), [CGM(1, 0, 1, 1)], nj=1, shift_masks=[1]),
    row("cgm", (C32, 2, 0, 1, 0b1, 2), [CGM(2, 0, 3, 3)], nj=3, shift_masks=[1, 1, 1]),
    row("cgm", (C64, 4096, 6, 1, 0b1, 1), [CGM(1, 0, 8, 8), CGM(1, 0, 8, 8)], nj=16, shift_masks=[1] * 16),
    # a launch with no active system: the first eight shifts are frozen everywhere / the last eight are
    row("cgm", (C64, 777, 1, 3, 0b111, 1), [NOTHING, CGM(1, 0, 1, 1)], nj=9, shift_masks=[0] * 8 + [0b010]),
    row("cgm", (C32, 256, 2, 16, 0x8421, 2), [CGM(2, 0, 8, 8), NOTHING], nj=16, shift_masks=[0x8421] * 8 + [0x7BDE] * 8),
    row("cgm", (C64, 2, 2, 3, 0b010, 1), [NOTHING], nj=3, shift_masks=[0b101] * 3),
]

# ======== qmg_batch_reduce_t: the three ops on every shape, past BRED_BLOCKS * 256 elements (the grid-stride loop runs), past blas_nt_mb
for op in range(3):
    for sh in SHAPES:
        ROUTES.append(row("reduce", sh, [RED(sh[5], 0, op)], op=op))
    for cls in CLASSES:
        ROUTES.append(row("reduce", NT_SHAPE[cls], [RED(cls[1], 1, op)], op=op, nt_mb=1))
    ROUTES.append(row("reduce", (C64, 300001, 1, 2, 0b10, 1), [RED(1, 0, op)], op=op))
    ROUTES.append(row("reduce", (C32, 600002, 2, 2, 0b11, 2), [RED(2, 0, op)], op=op))

# ======== qmg_batch_multidot_t: 15 walks 8 + 4 + 2 + 1
for cls in CLASSES:
    W = cls[1]
    sel = shapes_of(cls)
    for i, nj in enumerate((1, 2, 3, 4, 8, 15, 32)):
        plans = {1: [1], 2: [2], 3: [2, 1], 4: [4], 8: [8], 15: [8, 4, 2, 1], 32: [8, 8, 8, 8]}[nj]
        ROUTES.append(row("multidot", sel[i % len(sel)], [MDOT(W, 0, kt) for kt in plans], nj=nj))
    ROUTES.append(row("multidot", NT_SHAPE[cls], [MDOT(W, 1, kt) for kt in (8, 4, 2, 1)], nj=15, nt_mb=1))
ROUTES.append(row("multidot", (C64, 300001, 1, 2, 0b11, 1), [MDOT(1, 0, 2), MDOT(1, 0, 1)], nj=3))

# ======== qmg_batch_mr_dots_t then qmg_batch_mr_update_t: both XSET values, r_out NULL / aliasing r_in / distinct; where the shape has more than
# one active system the first of them has p = 0 (<p,p> = 0: alpha = 0, the system comes back as it was)
for cls in CLASSES:
    W = cls[1]
    sel = shapes_of(cls)
    i = 0
    for xset in (False, True):
        for rout in ("null", "alias", "distinct"):
            sh = sel[i % len(sel)]
            i += 1
            ROUTES.append(row("mr", sh, [MRD(W, 0), MRU(W, 0, xset, rout != "null")], xset=xset, rout=rout))
            ROUTES.append(row("mr", NT_SHAPE[cls], [MRD(W, 1), MRU(W, 1, xset, rout != "null")], xset=xset, rout=rout, nt_mb=1))
    ROUTES.append(row("mr", sel[-1], [MRD(W, 0), MRU(W, 0, False, True)]))
ROUTES.append(row("mr", (C64, 300001, 1, 2, 0b11, 1), [MRD(1, 0), MRU(1, 0, False, True)]))


def route_id(r):
    extra = "".join([
        "-op%d" % r["op"] if r["entry"] in ("blas", "reduce") else "",
        "-nj%d" % r["nj"] if r["entry"] in ("maxpy", "gcr", "multidot", "cgm") else "",
        "-sm" + ".".join("%x" % m for m in r["shift_masks"]) if r["shift_masks"] is not None else "",
        "-zn" if r["znext"] else "", "-xset" if r["xset"] else "", "-rout_" + r["rout"] if r["entry"] == "mr" else "", "-alias" if r["alias"] else "",
        "-mis" if r["mis"] else "", "-nt%d" % r["nt_mb"] if r["nt_mb"] is not None else ""])
    return "%s-%s-n%d+%d-k%d-%x%s" % (r["entry"], r["st"], r["n"], r["pad"], r["nrhs"], r["mask"], extra)


assert len({route_id(r) for r in ROUTES}) == len(ROUTES)


def active(mask, nrhs):
    return [k for k in range(nrhs) if (mask >> k) & 1]


def planned(r):
    """what qmg_batch_plan answers for the row's request at the row's blas_nt_mb (the caller sets it)"""
    dt, n, stride, nrhs, mask, al = DTYPE[r["st"]], r["n"], r["n"] + r["pad"], r["nrhs"], r["mask"], not r["mis"]
    ask = lambda entry, **kw: qmg.batch_plan(entry, dt, n, stride, nrhs, mask, aligned16=al, **kw)
    e = r["entry"]
    if e == "blas":
        return ask(qmg.BE_BLAS, op=r["op"])
    if e == "maxpy":
        return ask(qmg.BE_MULTI_CAXPY, nj=r["nj"])
    if e == "gcr":
        return ask(qmg.BE_GCR_UPDATE, nj=r["nj"], flags=qmg.BPV_ZNEXT if r["znext"] else 0)
    if e == "cgm":
        return ask(qmg.BE_CGM_UPDATE, nj=r["nj"], shift_masks=r["shift_masks"])
    if e == "reduce":
        return ask(qmg.BE_REDUCE, op=r["op"])
    if e == "multidot":
        return ask(qmg.BE_MULTIDOT, nj=r["nj"])
    assert e == "mr"
    return ask(qmg.BE_MR_DOTS) + ask(qmg.BE_MR_UPDATE, flags=(qmg.BPV_XSET if r["xset"] else 0) | (qmg.BPV_ROUT if r["rout"] != "null" else 0))


class tuned:
    """the row's blas_nt_mb for the length of a `with`, then the default again"""

    def __init__(self, r):
        self.mb = r["nt_mb"]

    def __enter__(self):
        if self.mb is not None:
            qmg.set_tuning("blas_nt_mb", self.mb)

    def __exit__(self, *exc):
        if self.mb is not None:
            qmg.set_tuning("blas_nt_mb", NT_DEFAULT)


@pytest.fixture(scope="module", autouse=True)
def _device():
    qmg.build()
    qmg.init(0)
    yield
    qmg.sync()


class Dev:
    """A host array on the device in the row's storage, behind one leading element when the row asks for pointers that are not 16-byte
    aligned (complex<float>: 8 bytes past a 16-byte boundary)."""

    def __init__(self, a, st, mis):
        self.shift = 1 if mis else 0
        self.arr = qmg.DeviceArray.from_host(np.concatenate([np.zeros(self.shift, dtype=NP[st]), np.asarray(a).astype(NP[st])]))
        self.ptr = self.arr.offset(self.shift)
        assert (self.ptr % 16 == 8) if mis else (self.ptr % 16 == 0)

    def host(self):
        return self.arr.to_host()[self.shift:]


class Case:
    """The operands of one row: `ro` read-only, `io` in/out (name -> complex128 host array holding what the device will hold)."""

    def __init__(self, r):
        self.r = r
        self.st, self.n, self.nrhs, self.mask = r["st"], r["n"], r["nrhs"], r["mask"]
        self.stride = r["n"] + r["pad"]
        self.act = active(r["mask"], r["nrhs"])
        self.rng = np.random.default_rng(20241)
        self.ro, self.io = {}, {}

    def vec(self):
        m = self.nrhs * self.stride
        v = self.rng.standard_normal(m) + 1j * self.rng.standard_normal(m)
        return bn.r32(v) if self.st == C32 else v

    def out_vec(self):
        """non-zero everywhere, NaN in the systems that are not active"""
        v = self.vec()
        for k in range(self.nrhs):
            if k not in self.act:
                self.seg(v, k)[:] = complex(np.nan, np.nan)
        return v

    def seg(self, v, k):
        return v[k * self.stride:k * self.stride + self.n]

    def storage(self, v):
        return np.asarray(v).astype(NP[self.st])

    def run(self, call):
        """the call twice on fresh copies of the in/out operands: the results of the first, after the two have been compared byte for byte"""
        dro = {k: Dev(v, self.st, self.r["mis"]) for k, v in self.ro.items()}

        def once():
            dio = {k: Dev(v, self.st, self.r["mis"]) for k, v in self.io.items()}
            d = dict(dro)
            d.update(dio)
            res = call(d)
            return {k: v.host() for k, v in dio.items()}, res

        with tuned(self.r):
            got, res = once()
            got2, res2 = once()
        for k in got:
            assert got[k].tobytes() == got2[k].tobytes(), "two runs differ in " + k
        if res is not None:
            assert np.asarray(res).tobytes() == np.asarray(res2).tobytes(), "two runs differ in the returned values"
        for k, d in dro.items():
            assert d.host().tobytes() == self.storage(self.ro[k]).tobytes(), "read-only operand %s was written" % k
        return got, res

    def check(self, name, raw, wants):
        """raw: what came back for in/out operand `name`; wants: {system: (want, bound)}.  Everything outside those systems' n elements: the initial bytes."""
        got = raw.astype(np.complex128)
        untouched = np.ones(self.nrhs * self.stride, dtype=bool)
        for k, (want, bound) in wants.items():
            s = slice(k * self.stride, k * self.stride + self.n)
            untouched[s] = False
            assert np.all(np.isfinite(got[s])), (name, k)
            err = np.abs(got[s].astype(bn.CLD) - want)
            nw = float(np.linalg.norm(want))
            l2 = float(np.linalg.norm(err)) / nw if nw > 0 else float(np.max(err, initial=0.0))
            ratio = err / np.where(bound > 0, bound, 1)
            worst = float(np.max(np.where(bound > 0, ratio, np.where(err > 0, np.inf, 0)), initial=0.0))
            # (the figures DESIGN 10.6 quotes: run with -s)
            print("route %s %s system %d: max err/bound %.3f, rel L2 %.3e" % (route_id(self.r), name, k, worst, l2))
            assert l2 < (TOL32_ROUND if self.st == C32 else TOL64), (name, k, l2)
            assert np.all(err <= bound), (name, k, int(np.argmax(ratio)), worst)
        assert raw[untouched].tobytes() == self.storage(self.io[name])[untouched].tobytes(), "frozen system or padding of %s was written" % name

    def bound(self, terms, S, want, slack=None):
        return bn.elementwise_bound(terms, S, want if self.st == C32 else None, slack if self.st == C32 else None)


def coefficients(c, nj):
    """coeffs[j][k], zero where (j + k) % 3 == 1"""
    cf = np.array([[(0.3 + 0.1 * j - 0.05 * k) + 1j * (0.2 - 0.07 * j + 0.03 * k) for k in range(c.nrhs)] for j in range(nj)], dtype=np.complex128).reshape(nj, c.nrhs)
    for j in range(nj):
        for k in range(c.nrhs):
            if (j + k) % 3 == 1:
                cf[j, k] = 0
    return cf


def vector_sets(c, cf, nj):
    """nj read-only vector sets; the slots whose coefficient is zero hold NaN and Inf"""
    for j in range(nj):
        v = c.vec()
        for k in range(c.nrhs):
            if cf[j, k] == 0:
                s = c.seg(v, k)
                s[0::2] = complex(np.nan, np.inf)
                s[1::2] = complex(-np.inf, np.nan)
        c.ro["x%d" % j] = v


def run_blas(c):
    r = c.r
    a = np.array([0.3 - 0.2j + 0.1 * k for k in range(c.nrhs)])
    b = np.array([-0.7 + 0.05j * k for k in range(c.nrhs)])
    c.ro["x"], c.io["z"] = c.vec(), c.out_vec()
    if not r["alias"]:
        c.ro["y"] = c.vec()
    got, _ = c.run(lambda d: qmg.batch_blas_t(DTYPE[c.st], r["op"], d["z"].ptr, c.n, c.nrhs, c.stride, c.mask, a=a, b=b, x=d["x"].ptr,
                                              y=d["z"].ptr if r["alias"] else d["y"].ptr))
    wants = {}
    for k in c.act:
        z = c.seg(c.io["z"], k)
        want, S, terms = bn.blas(r["op"], a[k], b[k], c.seg(c.ro["x"], k), z if r["alias"] else c.seg(c.ro["y"], k), z)
        wants[k] = (want, c.bound(terms, S, want))
    c.check("z", got["z"], wants)


def run_maxpy(c):
    nj = c.r["nj"]
    cf = coefficients(c, nj)
    vector_sets(c, cf, nj)
    c.io["y"] = c.out_vec()
    got, _ = c.run(lambda d: qmg.batch_multi_caxpy_t(DTYPE[c.st], cf, [d["x%d" % j] for j in range(nj)], d["y"].ptr, c.n, c.nrhs, c.stride, c.mask))
    wants = {}
    for k in c.act:
        want, S, terms, P = bn.multi_axpy(cf[:, k], [c.seg(c.ro["x%d" % j], k) for j in range(nj)], c.seg(c.io["y"], k), c.st == C32)
        wants[k] = (want, c.bound(terms, S, want, P))
    c.check("y", got["y"], wants)


def run_gcr(c):
    nj, zn = c.r["nj"], c.r["znext"]
    cf = coefficients(c, nj)
    vector_sets(c, cf, nj)
    a = np.array([-0.6 + 0.25j - 0.04 * k for k in range(c.nrhs)])
    c.io["w"], c.io["r"] = c.out_vec(), c.out_vec()
    if zn:
        c.io["zn"] = c.out_vec()
    got, _ = c.run(lambda d: qmg.batch_gcr_update_t(DTYPE[c.st], cf, [d["x%d" % j] for j in range(nj)], d["w"].ptr, a, d["r"].ptr, d["zn"].ptr if zn else None,
                                                    c.n, c.nrhs, c.stride, c.mask))
    ww, wr = {}, {}
    for k in c.act:
        wn, Sw, tw, Pw, rn, Sr, tr, slack = bn.gcr_update(cf[:, k], [c.seg(c.ro["x%d" % j], k) for j in range(nj)], c.seg(c.io["w"], k), a[k], c.seg(c.io["r"], k), c.st == C32)
        ww[k] = (wn, c.bound(tw, Sw, wn, Pw))
        wr[k] = (rn, c.bound(tr, Sr, rn, slack))
    c.check("w", got["w"], ww)
    c.check("r", got["r"], wr)
    if zn:
        c.check("zn", got["zn"], wr)
        for k in c.act:   # z_next = r: the same bytes
            assert c.seg(got["zn"], k).tobytes() == c.seg(got["r"], k).tobytes()


def run_cgm(c):
    ns, sm = c.r["nj"], c.r["shift_masks"]
    a, z, cc = (np.array([[sgn * (0.2 + 0.11 * s + 0.013 * k) for k in range(c.nrhs)] for s in range(ns)]) for sgn in (1.0, -0.7, 0.45))
    c.ro["r"] = c.vec()
    on = lambda s, k: bool((c.mask & sm[s]) >> k & 1)
    for s in range(ns):
        for name in ("x%d" % s, "p%d" % s):
            v = c.vec()
            for k in range(c.nrhs):
                if not on(s, k):   # a frozen (system, shift) pair
                    c.seg(v, k)[:] = complex(np.nan, np.nan)
            c.io[name] = v
    got, _ = c.run(lambda d: qmg.batch_cgm_update_t(DTYPE[c.st], [d["x%d" % s].ptr for s in range(ns)], [d["p%d" % s].ptr for s in range(ns)], a, z, cc, sm, d["r"].ptr,
                                                    c.n, c.nrhs, c.stride, c.mask))
    for s in range(ns):
        wx, wp = {}, {}
        for k in range(c.nrhs):
            if on(s, k):
                xn, Sx, tx, pn, Sp, tp = bn.cgm_update(a[s, k], z[s, k], cc[s, k], c.seg(c.io["x%d" % s], k), c.seg(c.io["p%d" % s], k), c.seg(c.ro["r"], k))
                wx[k], wp[k] = (xn, c.bound(tx, Sx, xn)), (pn, c.bound(tp, Sp, pn))
        c.check("x%d" % s, got["x%d" % s], wx)
        c.check("p%d" % s, got["p%d" % s], wp)


def run_reduce(c):
    op = c.r["op"]
    c.ro["x"], c.ro["y"] = c.vec(), c.vec()
    _, res = c.run(lambda d: qmg.batch_reduce_t(DTYPE[c.st], op, d["x"].ptr, None if op == bn.NORM2 else d["y"].ptr, c.n, c.nrhs, c.stride, c.mask))
    for k in range(c.nrhs):
        if k in c.act:
            want, scale = bn.reduce(op, c.seg(c.ro["x"], k), c.seg(c.ro["y"], k))
            err = abs(bn.CLD(res[k]) - want)
            print("route %s system %d: err/scale %.3e" % (route_id(c.r), k, float(err / scale)))
            assert err <= bn.RTOL_RED * scale, (k, float(err / scale))
            if op != bn.DOT:
                assert res[k].imag == 0
        else:
            assert np.isnan(res[k].real) and np.isnan(res[k].imag)   # (inactive entries of out_host are left as the caller had them)


def run_multidot(c):
    nj = c.r["nj"]
    c.ro["y"] = c.vec()
    for j in range(nj):
        c.ro["x%d" % j] = c.vec()
    _, res = c.run(lambda d: qmg.batch_multidot_t(DTYPE[c.st], [d["x%d" % j] for j in range(nj)], d["y"].ptr, c.n, c.nrhs, c.stride, c.mask))
    for k in range(c.nrhs):
        if k in c.act:
            wants, scales = bn.multidot([c.seg(c.ro["x%d" % j], k) for j in range(nj)], c.seg(c.ro["y"], k))
            for j in range(nj):
                err = abs(bn.CLD(res[k][j]) - wants[j])
                assert err <= bn.RTOL_RED * scales[j], (k, j, float(err / scales[j]))
        else:
            assert np.all(np.isnan(res[k].real)) and np.all(np.isnan(res[k].imag))


def run_mr(c):
    r = c.r
    xset, rout, omega = r["xset"], r["rout"], 0.85
    # r = (0.7 - 0.2i) p + noise: <p,r> is no cancelling sum, alpha is of order one
    p = c.vec()
    noise = c.vec()
    rin = bn.r32((0.7 - 0.2j) * p + 0.3 * noise) if c.st == C32 else (0.7 - 0.2j) * p + 0.3 * noise
    dead = c.act[0] if len(c.act) > 1 else None   # <p,p> = 0 there
    if dead is not None:
        c.seg(p, dead)[:] = 0
    c.ro["p"] = p
    c.io["x"] = c.out_vec()
    if rout == "alias":
        c.io["r"] = rin
    else:
        c.ro["r"] = rin
        if rout == "distinct":
            c.io["ro"] = c.out_vec()
    dt = DTYPE[c.st]

    def call(d):
        qmg.batch_mr_dots(dt, d["r"].ptr, d["p"].ptr, c.n, c.nrhs, c.stride, c.mask)
        dots = qmg.batch_mr_read_dots(c.nrhs).copy()
        qmg.batch_mr_update(dt, omega, d["x"].ptr, d["r"].ptr, {"null": None, "alias": d["r"].ptr, "distinct": d.get("ro") and d["ro"].ptr}[rout], d["p"].ptr, xset,
                            c.n, c.nrhs, c.stride, c.mask)
        return dots

    got, dots = c.run(call)
    wx, wr = {}, {}
    for k in c.act:
        pk, rk, xk = c.seg(p, k), c.seg(rin, k), c.seg(c.io["x"], k)
        pr, pp, s_pr, s_pp = bn.mr_dots(rk, pk)
        assert abs(bn.CLD(complex(dots[k][0], dots[k][1])) - pr) <= bn.RTOL_RED * s_pr, k
        assert abs(bn.LD(dots[k][2]) - pp) <= bn.RTOL_RED * s_pp, k
        assert (dots[k][2] == 0) == (k == dead)
        alpha = bn.mr_alpha(omega, bn.CLD(complex(dots[k][0], dots[k][1])), bn.LD(dots[k][2]))   # from the slot the update read
        xn, Sx, tx, rn, Sr, tr = bn.mr_update(alpha, xk, rk, pk, xset)
        wx[k], wr[k] = (xn, c.bound(tx, Sx, xn)), (rn, c.bound(tr, Sr, rn))
        if k == dead and not xset:   # alpha = 0: the system as it was, byte for byte
            assert c.seg(got["x"], k).tobytes() == c.seg(c.storage(c.io["x"]), k).tobytes()
            for name in ("r",) if rout == "alias" else ():
                assert c.seg(got[name], k).tobytes() == c.seg(c.storage(c.io[name]), k).tobytes()
    c.check("x", got["x"], wx)
    if rout == "alias":
        c.check("r", got["r"], wr)
    elif rout == "distinct":
        c.check("ro", got["ro"], wr)


RUN = {"blas": run_blas, "maxpy": run_maxpy, "gcr": run_gcr, "cgm": run_cgm, "reduce": run_reduce, "multidot": run_multidot, "mr": run_mr}


@pytest.mark.parametrize("r", ROUTES, ids=route_id)
def test_route_against_numpy_reference(r):
    with tuned(r):
        assert planned(r) == r["plans"]
    RUN[r["entry"]](Case(r))
