"""Every stream-taking entry point of include/qmg_hip.h held to the stream it is given.

qmg_stream_create makes non-blocking streams, so work that a call leaves on the null stream is not ordered against the caller's stream.
CASES is the table, keyed by header symbol: a case names its device inputs as host arrays (`ins`), the outputs (`outs`), the in/out
arguments (`inout`) and a closure call(bufs, stream).  tests/test_host_stream_binding.py holds the table to the header: every stream-taking
symbol has a case or is in EXEMPT (the machinery itself and the two documented no-ops), and nothing else may be exempt.

An ASYNCHRONOUS case runs three times.  (1) Reference: inputs uploaded on the null stream, outputs preset to 0xFF bytes, call(None), device
synchronised, outputs downloaded; this run also grows every library scratch buffer, so that the gated run neither frees nor allocates (either
would wait for the device and open the gate).  The yardstick is the same entry point on the synchronised null stream -- other tests pin that
to independent references -- and what is held here is ORDERING, which is why the comparison is bit for bit.  (2) Decoy: the same call on
different inputs of the same shapes, so that library scratch holds the decoy's intermediates and a later kernel of a multi-kernel call that
ran too early reads wrong intermediates, not stale correct ones.  (3) Gated: inputs, in/out arguments and outputs hold 0xFF bytes (NaN in
every dtype used), the true inputs sit in staging buffers; on the created stream `st`, in order: the Gate (tests/stream_gate.py), the
qmg_memcpy_d2d of staging into the inputs, a qmg_memcpy_d2d of 0xFF bytes over every output (so that an escaped writer that has no device
input at all -- a random fill -- is caught too: what it wrote too early is overwritten), call(st).  On return the gate must still be closed ("gate open: case proves nothing" otherwise: no
pass, no skip, no retry); then a qmg_memcpy_d2d of every output into a second buffer goes on `st`, `st` is synchronised, and the outputs and
their copies must equal the reference and the pure inputs the staged values, byte for byte.  A launch, memset or copy of the call that went
to the null stream ran before the canary read that found the gate closed, that is before its input existed, and read NaN.

A HOST-RETURNING case (the reductions' host forms, the U(1) observables, qmg_batch_mr_read_dots, qmg_memcpy_h2d / _d2h) must synchronise
inside, so nothing can be asked after it returns: the gate is asserted closed immediately BEFORE the call and the returned values must equal
the reference's.  This is weaker: an escaped kernel is caught because it runs milliseconds before its input exists, by timing, not by
ordering.  Where such an entry point has a device-resident output the asynchronous case for that form is in the table as well.

For the entry points a plan dispatches there is one case per kernel family the plan can name (each family has its own launch site), on
shapes taken from the route tests, and the case first asserts through the plan query that it reaches the family it claims.

test_escaped_call_is_caught is the negative control: for a BLAS-1 call, a plan-dispatched apply and a multi-kernel setup call the gated
protocol runs with call(None) while the inputs are still behind the gate on `st`; the result must DIFFER from the reference (it reads the
NaN poison).  A harness that cannot fail proves nothing.

test_first_use_on_a_created_stream starts tests/stream_first_use_worker.py once per per-thread workspace of the library.

Measured on an MI355X: the slowest asynchronous case takes 0.17 ms of host time from the first staging copy to the return of call(st) (median
0.02 ms), one gate copy of 256 MiB takes 0.10 ms, and a gate of 102 copies measures 10.0 - 10.1 ms by its event pair -- sixty times the slowest
enqueue, where ten times was asked for: the canary decides, the margin only keeps a stalled Python thread from opening the gate.  The 215
table cases and controls run in 4 s, the ten first-use children in 4 s.
"""
import ctypes as C
import importlib
import math
import os
import subprocess
import sys
import time
import types

import numpy as np
import pytest

import stream_gate as sg

qmg = importlib.import_module("quantum-mg_amd")

pytestmark = pytest.mark.gpu

# Measured on an MI355X: the slowest asynchronous case of the table takes SLOWEST_ENQUEUE_MS of host time from the first staging copy to the
# return of call(st); the gate is ten times that by its event pair (a loaded host can stall a Python thread for several enqueue times).
SLOWEST_ENQUEUE_MS = 0.17
GATE_MS = 10.0     # at least 10 * SLOWEST_ENQUEUE_MS

EXEMPT = {
    "qmg_stream_sync": "the machinery itself: every case ends on it",
    "qmg_stream_destroy": "the machinery itself",
    "qmg_event_record": "the machinery itself: the gate's event pair",
    "qmg_allreduce_sum_f64": "with one rank a documented no-op with no device work",
    "qmg_poison_scratch": "does nothing, no launch, with the default tuning key",
}

C64, C32 = qmg.C64, qmg.C32
c128, c64, f64 = np.complex128, np.complex64, np.float64
NPT = {C64: c128, C32: c64}
TAG = {C64: "c64", C32: "c32"}
P = qmg
M0, MP = P.P_ALL | P.P_ZERO, P.P_ALL
EO0, HOP0 = P.P_EO | P.P_ZERO_E, P.P_HOPPING | P.P_ZERO
DEFAULT_KNOBS = {"stencil_pair": 2, "pair_prefetch": 1, "stencil_site": 3, "stencil_mfma": 1, "blas_nt_mb": 256, "wilson_pair": 2, "setup_fused": 1}


class Bufs(dict):
    __getattr__ = dict.__getitem__


class Case:
    """host: the call returns its results to the host; blocking: it leaves them on the device but synchronises the stream inside.  Both take
    the host-returning protocol."""

    def __init__(self, call, ins=None, outs=None, inout=None, host=False, blocking=False, reach=None, knobs=None, decoy=None):
        self.call, self.ins, self.outs, self.inout = call, dict(ins or {}), dict(outs or {}), dict(inout or {})
        self.host, self.blocking, self.reach, self.knobs, self.decoy = host, blocking, reach, dict(knobs or {}), dict(decoy or {})


CASES = {}    # header symbol -> [(label, maker)]


def case(*symbols, label=""):
    def deco(maker):
        for s in symbols:
            CASES.setdefault(s, []).append((label, maker))
        return maker
    return deco


# ---------------------------------------------------------------- host data
def cv(n, seed, dt=c128):
    r = np.random.default_rng(seed)
    return (r.standard_normal(n) + 1j * r.standard_normal(n)).astype(dt)


def rv(n, seed):
    return np.random.default_rng(seed).standard_normal(n)


def links(Lx, Ly, seed, dt=c128):
    return np.exp(1j * np.random.default_rng(seed).uniform(-3, 3, 2 * Lx * Ly)).astype(dt)


def to_half(a):
    """complex<half> storage of a complex array, as float16 (re, im) pairs"""
    return np.stack([a.real, a.imag], axis=-1).astype(np.float16).reshape(-1)


def vp(x):
    return qmg._vp(x)


def dbl(x):
    return C.cast(C.c_void_p(x.ptr), C.POINTER(C.c_double))


def dev_form(sym, args, out, s):
    """a reduction with its results left in device memory: (..., out_dev, out_host = NULL, stream)"""
    qmg.check(getattr(qmg.lib(), sym)(*args, dbl(out), None, C.c_void_p(s)), sym)


def checked(rc, what):
    qmg.check(rc, what)


# ---------------------------------------------------------------- runtime
@case("qmg_memcpy_d2d")
def _():
    return Case(lambda b, s: qmg.memcpy_d2d(b.dst, b.src, 1031 * 16, stream=s), ins={"src": cv(1031, 1)}, outs={"dst": (c128, 1031)})


@case("qmg_memset_zero")
def _():
    return Case(lambda b, s: qmg.memset_zero(b.x, 1031 * 16, stream=s), outs={"x": (c128, 1031)})


@case("qmg_memcpy_d2h")
def _():
    def call(b, s):
        out = np.zeros(1031, dtype=c128)
        qmg.memcpy_d2h(out, b.src, stream=s)
        qmg.sync(s)
        return out
    return Case(call, ins={"src": cv(1031, 2)}, host=True)


@case("qmg_memcpy_h2d")
def _():
    src = cv(1031, 3)

    def call(b, s):
        # dst = src + gated input: the upload alone would not depend on the gate
        out = np.zeros(1031, dtype=c128)
        qmg.memcpy_h2d(b.dst, src, stream=s)
        qmg.caxpy(1.0, b.x, b.dst, 1031, stream=s)
        qmg.memcpy_d2h(out, b.dst, stream=s)
        qmg.sync(s)
        return out
    return Case(call, ins={"x": cv(1031, 4)}, outs={"dst": (c128, 1031)}, host=True)


# ---------------------------------------------------------------- BLAS-1 and reductions on one vector
N1 = 1031
A1, B1 = 0.7 - 0.3j, -0.2 + 1.1j


def _blas1(sym, ins, inout, outs, f):
    @case(sym)
    def _():
        return Case(f, ins={k: cv(N1, 10 + i) for i, k in enumerate(ins)}, inout={k: cv(N1, 20 + i) for i, k in enumerate(inout)},
                    outs={k: (c128, N1) for k in outs})


_blas1("qmg_zero_vector", "", "", "x", lambda b, s: qmg.zero_vector(b.x, N1, stream=s))
_blas1("qmg_copy_vector", "x", "", "y", lambda b, s: qmg.copy_vector(b.y, b.x, N1, stream=s))
_blas1("qmg_cax", "", "x", "", lambda b, s: qmg.cax(A1, b.x, N1, stream=s))
_blas1("qmg_caxy", "x", "", "y", lambda b, s: qmg.caxy(A1, b.x, b.y, N1, stream=s))
_blas1("qmg_caxpy", "x", "y", "", lambda b, s: qmg.caxpy(A1, b.x, b.y, N1, stream=s))
_blas1("qmg_cxpy", "x", "y", "", lambda b, s: qmg.cxpy(b.x, b.y, N1, stream=s))
_blas1("qmg_cxpay", "x", "y", "", lambda b, s: qmg.cxpay(b.x, A1, b.y, N1, stream=s))
_blas1("qmg_caxpby", "x", "y", "", lambda b, s: qmg.caxpby(A1, b.x, B1, b.y, N1, stream=s))
_blas1("qmg_cxpyz", "xy", "", "z", lambda b, s: qmg.cxpyz(b.x, b.y, b.z, N1, stream=s))
_blas1("qmg_caxpbyz", "xy", "", "z", lambda b, s: qmg.caxpbyz(A1, b.x, B1, b.y, b.z, N1, stream=s))
_blas1("qmg_multi_caxpy", "xyz", "w", "", lambda b, s: qmg.multi_caxpy([A1, B1, 0.5], [b.x, b.y, b.z], b.w, N1, stream=s))
_blas1("qmg_gaussian", "", "", "x", lambda b, s: qmg.gaussian(b.x, N1, 77, stream=s))
_blas1("qmg_convert", "x", "", "y", lambda b, s: (qmg.convert(b.y, C32, b.x, C64, N1 // 2, stream=s), qmg.convert(b.y.offset(N1 // 2), C64, b.y, C32, N1 // 4, stream=s)))
_blas1("qmg_c64_to_c32", "x", "", "y", lambda b, s: qmg.c64_to_c32(b.y, b.x, N1, stream=s))
_blas1("qmg_convert_to_c16", "x", "", "y", lambda b, s: qmg.convert_to_c16(b.y, b.x, C64, N1, stream=s))
_blas1("qmg_convert_from_c16", "x", "", "yz", lambda b, s: (qmg.convert_to_c16(b.y, b.x, C64, N1, stream=s), qmg.convert_from_c16(b.z, C64, b.y, N1, stream=s)))


@case("qmg_caxy_pattern")
def _():
    nsite, nc = 259, 4
    return Case(lambda b, s: qmg.caxy_pattern([1.0, -1.0, 2.0, 0.5], [1, 0, 3, 2], b.x, b.y, nsite, stream=s),
                ins={"x": cv(nsite * nc, 5)}, outs={"y": (c128, nsite * nc)})


def _reduce1(sym, wrapper, nvec):
    names = "xy"[:nvec]

    @case(sym, label="host")
    def _():
        return Case(lambda b, s: np.asarray(wrapper(*[b[k] for k in names], N1, stream=s)), ins={k: cv(N1, 30 + i) for i, k in enumerate(names)}, host=True)

    @case(sym, label="out_dev")
    def _():
        return Case(lambda b, s: dev_form(sym, [vp(b[k]) for k in names] + [C.c_size_t(N1)], b.o, s), ins={k: cv(N1, 30 + i) for i, k in enumerate(names)},
                    outs={"o": (f64, 2)})


_reduce1("qmg_norm2sq", qmg.norm2sq, 1)
_reduce1("qmg_dot", qmg.dot, 2)
_reduce1("qmg_diffnorm2sq", qmg.diffnorm2sq, 2)
_reduce1("qmg_norminf", qmg.norminf, 1)


def _ptrs(xs):
    return (C.c_void_p * len(xs))(*[x.ptr for x in xs])


@case("qmg_multidot", label="host")
def _():
    return Case(lambda b, s: qmg.multidot([b.x, b.y, b.z], b.w, N1, stream=s), ins={k: cv(N1, 40 + i) for i, k in enumerate("xyzw")}, host=True)


@case("qmg_multidot", label="out_dev-two-passes")
def _():
    # 33 vectors: a pass of 32 and a second launch for the rest
    names = ["x%d" % i for i in range(33)]
    return Case(lambda b, s: dev_form("qmg_multidot", [_ptrs([b[k] for k in names]), 33, vp(b.w), C.c_size_t(N1)], b.o, s),
                ins=dict({k: cv(N1, 50 + i) for i, k in enumerate(names)}, w=cv(N1, 49)), outs={"o": (f64, 66)})


TS = (6, 10, 3)   # Lx, Ly, nc of the per-timeslice sums


def _timeslice(sym, wrapper, nvec, width):
    Lx, Ly, nc = TS
    names = "ab"[:nvec]

    @case(sym, label="host")
    def _():
        return Case(lambda b, s: wrapper(*[b[k] for k in names], Lx, Ly, nc, stream=s), ins={k: cv(Lx * Ly * nc, 60 + i) for i, k in enumerate(names)}, host=True)

    @case(sym, label="out_dev")
    def _():
        return Case(lambda b, s: dev_form(sym, [vp(b[k]) for k in names] + [Lx, Ly, nc], b.o, s), ins={k: cv(Lx * Ly * nc, 60 + i) for i, k in enumerate(names)},
                    outs={"o": (f64, width * Ly)})


_timeslice("qmg_norm2sq_cv_timeslice", qmg.norm2sq_cv_timeslice, 1, 1)
_timeslice("qmg_dot_cv_timeslice", qmg.dot_cv_timeslice, 2, 2)
_timeslice("qmg_redot_cv_timeslice", qmg.redot_cv_timeslice, 2, 1)


@case("qmg_gaussian_wall_source")
def _():
    Lx, Ly, nc = TS
    return Case(lambda b, s: checked(qmg.gaussian_wall_source(b.x, Lx, Ly, nc, 3, 1, 5, 0.5, 0.25, stream=s), "qmg_gaussian_wall_source"), outs={"x": (c128, Lx * Ly * nc)})


@case("qmg_gaussian_slab")
def _():
    return Case(lambda b, s: qmg.gaussian_slab(b.x, 6, 12, 4, 4, 2, 9, stream=s), outs={"x": (c128, 6 * 4 * 2)})


# ---------------------------------------------------------------- lock-step batch vectors (qmg_batch_plan)
BN, BSTRIDE, BNRHS, BMASK = 515, 520, 3, 0b101


def bvec(seed, dt=c128, nrhs=BNRHS, stride=BSTRIDE):
    return cv(stride * nrhs, seed, dt)


def batch_reach(entry, dtype, families, n=BN, stride=BSTRIDE, nrhs=BNRHS, mask=BMASK, **kw):
    def reach():
        plan = qmg.batch_plan(entry, dtype, n, stride, nrhs, mask, **kw)
        assert [p[0] for p in plan] == list(families), plan
    return reach


COEF3 = np.array([0.5 - 1j, 2.0, -0.25 + 0.5j])


def _batch_typed(dtype, typed):
    dt, tag = NPT[dtype], TAG[dtype] if typed else ""
    sfx = "_t" if typed else ""
    T = (lambda f: (lambda *a, **k: f(dtype, *a, **k))) if typed else (lambda f: f)
    blas, maxpy, red, mdot = (T(getattr(qmg, n + sfx)) for n in ("batch_blas", "batch_multi_caxpy", "batch_reduce", "batch_multidot"))

    @case("qmg_batch_blas" + sfx, label=tag)
    def _():
        return Case(lambda b, s: blas(qmg.BOP_CAXPBYZ, b.z, BN, BNRHS, BSTRIDE, BMASK, a=COEF3, b=COEF3[::-1], x=b.x, y=b.y, stream=s),
                    ins={"x": bvec(1, dt), "y": bvec(2, dt)}, outs={"z": (dt, BSTRIDE * BNRHS)},
                    reach=batch_reach(qmg.BE_BLAS, dtype, [qmg.BF_BLAS], op=qmg.BOP_CAXPBYZ))

    @case("qmg_batch_multi_caxpy" + sfx, label=tag + "small-two-passes")
    def _():
        nj = 9     # 8 vector sets and a second launch for the ninth
        names = ["x%d" % j for j in range(nj)]
        coeffs = cv(nj * BNRHS, 5).reshape(nj, BNRHS)
        return Case(lambda b, s: maxpy(coeffs, [b[k] for k in names], b.y, BN, BNRHS, BSTRIDE, BMASK, stream=s),
                    ins={k: bvec(10 + j, dt) for j, k in enumerate(names)}, inout={"y": bvec(3, dt)},
                    reach=batch_reach(qmg.BE_MULTI_CAXPY, dtype, [qmg.BF_MAXPY_SMALL] * 2, nj=nj))

    @case("qmg_batch_reduce" + sfx, label=tag)
    def _():
        return Case(lambda b, s: red(qmg.BRED_DOT, b.x, b.y, BN, BNRHS, BSTRIDE, BMASK, stream=s)[[0, 2]], ins={"x": bvec(1, dt), "y": bvec(2, dt)}, host=True,
                    reach=batch_reach(qmg.BE_REDUCE, dtype, [qmg.BF_REDUCE], op=qmg.BRED_DOT))

    @case("qmg_batch_multidot" + sfx, label=tag + "two-passes")
    def _():
        nj = 9
        names = ["x%d" % j for j in range(nj)]

        def reach():
            plan = qmg.batch_plan(qmg.BE_MULTIDOT, dtype, BN, BSTRIDE, BNRHS, BMASK, nj=nj)
            assert len(plan) >= 2 and all(p[0] == qmg.BF_MULTIDOT for p in plan), plan
        return Case(lambda b, s: mdot([b[k] for k in names], b.y, BN, BNRHS, BSTRIDE, BMASK, stream=s)[[0, 2]],
                    ins=dict({k: bvec(10 + j, dt) for j, k in enumerate(names)}, y=bvec(3, dt)), host=True, reach=reach)


_batch_typed(C64, False)
_batch_typed(C64, True)
_batch_typed(C32, True)

LONG_N = {C64: 1 << 20, C32: 1 << 21}    # the smallest long vector of each storage: 16 MiB per system


def _batch_t_only(dtype):
    dt, tag = NPT[dtype], TAG[dtype]

    @case("qmg_batch_multi_caxpy_t", label=tag + "-long")
    def _():
        n = LONG_N[dtype]
        return Case(lambda b, s: qmg.batch_multi_caxpy_t(dtype, COEF3[:2].reshape(1, 2), [b.x], b.y, n, 2, n, 0b11, stream=s),
                    ins={"x": cv(2 * n, 1, dt)}, inout={"y": cv(2 * n, 2, dt)},
                    reach=batch_reach(qmg.BE_MULTI_CAXPY, dtype, [qmg.BF_MAXPY_LONG], n=n, stride=n, nrhs=2, mask=0b11, nj=1))

    @case("qmg_batch_gcr_update_t", label=tag)
    def _():
        coeffs = cv(2 * BNRHS, 6).reshape(2, BNRHS)
        return Case(lambda b, s: qmg.batch_gcr_update_t(dtype, coeffs, [b.w0, b.w1], b.w, COEF3, b.r, b.z, BN, BNRHS, BSTRIDE, BMASK, stream=s),
                    ins={"w0": bvec(1, dt), "w1": bvec(2, dt)}, inout={"w": bvec(3, dt), "r": bvec(4, dt)}, outs={"z": (dt, BSTRIDE * BNRHS)},
                    reach=batch_reach(qmg.BE_GCR_UPDATE, dtype, [qmg.BF_GCR], nj=2, flags=qmg.BPV_ZNEXT))

    @case("qmg_batch_cgm_update_t", label=tag)
    def _():
        ns, sm = 2, [0b101, 0b100]
        a, z, c = (rv(ns * BNRHS, 7 + i).reshape(ns, BNRHS) for i in range(3))
        return Case(lambda b, s: qmg.batch_cgm_update_t(dtype, [b.x0, b.x1], [b.p0, b.p1], a, z, c, sm, b.r, BN, BNRHS, BSTRIDE, BMASK, stream=s),
                    ins={"r": bvec(1, dt)}, inout={"x0": bvec(2, dt), "x1": bvec(3, dt), "p0": bvec(4, dt), "p1": bvec(5, dt)},
                    reach=batch_reach(qmg.BE_CGM_UPDATE, dtype, [qmg.BF_CGM], nj=ns, shift_masks=sm))

    @case("qmg_batch_mr_dots_t", "qmg_batch_mr_update_t", label=tag)
    def _():
        # the dots go to the calling thread's device slot; the update forms alpha from that slot on the device
        def call(b, s):
            qmg.batch_mr_dots(dtype, b.r, b.p, BN, BNRHS, BSTRIDE, BMASK, stream=s)
            qmg.batch_mr_update(dtype, 0.85, b.x, b.r, b.r2, b.p, False, BN, BNRHS, BSTRIDE, BMASK, stream=s)

        def reach():
            batch_reach(qmg.BE_MR_DOTS, dtype, [qmg.BF_MR_DOTS])()
            batch_reach(qmg.BE_MR_UPDATE, dtype, [qmg.BF_MR_UPDATE], flags=qmg.BPV_ROUT)()
        return Case(call, ins={"r": bvec(1, dt), "p": bvec(2, dt)}, inout={"x": bvec(3, dt)}, outs={"r2": (dt, BSTRIDE * BNRHS)}, reach=reach)

    @case("qmg_batch_mr_read_dots", label=tag)
    def _():
        def call(b, s):
            qmg.batch_mr_dots(dtype, b.r, b.p, BN, BNRHS, BSTRIDE, BMASK, stream=s)
            return qmg.batch_mr_read_dots(BNRHS, stream=s)[[0, 2], :3]
        return Case(call, ins={"r": bvec(1, dt), "p": bvec(2, dt)}, host=True)

    # ---- one basis shared by the batch (csrc/qmg_deflate.hip)
    nv, ldv = 5, BN + 5

    @case("qmg_basis_dot_t", label=tag + "-host")
    def _():
        return Case(lambda b, s: qmg.basis_dot_t(dtype, b.V, nv, ldv, b.B, BN, BNRHS, BSTRIDE, BMASK, stream=s)[[0, 2]],
                    ins={"V": cv(nv * ldv, 1, dt), "B": bvec(2, dt)}, host=True)

    @case("qmg_basis_dot_t", label=tag + "-out_dev")
    def _():
        return Case(lambda b, s: qmg.basis_dot_t(dtype, b.V, nv, ldv, b.B, BN, BNRHS, BSTRIDE, BMASK, out_dev=b.o, stream=s),
                    ins={"V": cv(nv * ldv, 1, dt), "B": bvec(2, dt)}, outs={"o": (c128, BNRHS * nv)})

    @case("qmg_basis_update_t", label=tag + "-host-coeffs")
    def _():
        coeffs = cv(BNRHS * nv, 8).reshape(BNRHS, nv)
        return Case(lambda b, s: qmg.basis_update_t(dtype, coeffs, b.V, nv, ldv, b.B, BN, BNRHS, BSTRIDE, BMASK, stream=s),
                    ins={"V": cv(nv * ldv, 1, dt)}, inout={"B": bvec(2, dt)})

    @case("qmg_basis_update_t", label=tag + "-device-coeffs")
    def _():
        return Case(lambda b, s: qmg.basis_update_t(dtype, b.c, b.V, nv, ldv, b.B, BN, BNRHS, BSTRIDE, BMASK, stream=s),
                    ins={"V": cv(nv * ldv, 1, dt), "c": cv(BNRHS * nv, 8)}, inout={"B": bvec(2, dt)})

    @case("qmg_batch_deflate_t", label=tag)
    def _():
        return Case(lambda b, s: qmg.batch_deflate_t(dtype, b.V, nv, ldv, b.il, b.B, b.E, BN, BNRHS, BSTRIDE, BMASK, stream=s),
                    ins={"V": cv(nv * ldv, 1, dt), "il": 1.0 + np.abs(rv(nv, 9)), "B": bvec(2, dt)}, outs={"E": (dt, BSTRIDE * BNRHS)})


_batch_t_only(C64)
_batch_t_only(C32)


@case("qmg_batch_multi_caxpy_t", label="c64-single-long")
def _():
    n = LONG_N[C64]
    return Case(lambda b, s: qmg.batch_multi_caxpy_t(C64, COEF3[:2].reshape(2, 1), [b.x0, b.x1], b.y, n, 1, n, 0b1, stream=s),
                ins={"x0": cv(n, 1), "x1": cv(n, 2)}, inout={"y": cv(n, 3)},
                reach=batch_reach(qmg.BE_MULTI_CAXPY, C64, [qmg.BF_MAXPY_SINGLE], n=n, stride=n, nrhs=1, mask=0b1, nj=2))


# ---------------------------------------------------------------- stencil applies (qmg_stencil_plan)
SHIFTS = (0.3 - 0.1j, -0.2 + 0.05j, 0.15 - 0.25j)
PAD = 6


def stencil_case(fn, entry, family, dims, nrhs, mask, pieces, vdt=c128, mat=0, knobs=None, epilogue=0, extra_ins=None, extra_outs=None, slab_rows=0, inplace=False):
    Lx, Ly, nc = dims
    vol, n = Lx * Ly, Lx * Ly * nc
    stride = n + PAD
    cl, ho = cv(vol * nc * nc, 1), cv(4 * vol * nc * nc, 2)
    if mat == 1:
        cl, ho = cl.astype(c64), ho.astype(c64)
    elif mat == 2:
        cl, ho = to_half(cl), to_half(ho)
    shifts = SHIFTS if nc % 2 == 0 else SHIFTS[:2]
    n_active = bin(mask).count("1")
    holes = mask != (1 << n_active) - 1

    def call(b, s):
        return fn(qmg.make_desc(Lx, Ly, nc, b.cl, b.ho, *shifts), b, pieces, nrhs, stride, mask, s)

    def reach():
        plan = qmg.stencil_plan(entry, mat, vdt == c64, dims, pieces, n_active, holes=holes, inplace=inplace, epilogue=epilogue, slab_rows=slab_rows)
        assert plan and all(p[0] == family if family is not None else p[0] not in (qmg.SF_UNSUPPORTED, qmg.SF_NOTHING, qmg.SF_INVALID) for p in plan), plan
    ins = dict({"cl": cl, "ho": ho, "rhs": cv(stride * nrhs, 3, vdt)}, **(extra_ins or {}))
    return Case(call, ins=ins, inout={"lhs": cv(stride * nrhs, 4, vdt)}, outs=extra_outs, reach=reach, knobs=knobs)


def f_apply(d, b, pieces, nrhs, stride, mask, s):
    qmg.stencil_apply(d, b.lhs, b.rhs, pieces, nrhs, stride, stream=s)


def f_batch(d, b, pieces, nrhs, stride, mask, s):
    qmg.stencil_apply_batch(d, b.lhs, b.rhs, pieces, nrhs, stride, mask, stream=s)


def f_t(dtype):
    return lambda d, b, pieces, nrhs, stride, mask, s: qmg.stencil_apply_t(dtype, d, b.lhs, b.rhs, pieces, nrhs, stride, mask, stream=s)


def f_mat32(d, b, pieces, nrhs, stride, mask, s):
    qmg.stencil_apply_mat32(d, b.lhs, b.rhs, pieces, nrhs, stride, mask, stream=s)


def f_mat16(dtype):
    return lambda d, b, pieces, nrhs, stride, mask, s: checked(qmg.stencil_apply_mat16(dtype, d, b.lhs, b.rhs, pieces, nrhs, stride, mask, stream=s), "qmg_stencil_apply_mat16_t")


def f_h16(d, b, pieces, nrhs, stride, mask, s):
    qmg.stencil_apply_h16(d, b.lhs, b.rhs, pieces, nrhs, stride, mask, stream=s)


SE = qmg.SE_MASKED
STENCIL_ROWS = [
    # symbol, label, fn, entry, family, dims, nrhs, mask, pieces, vdt, mat, knobs
    ("qmg_stencil_apply", "pair", f_apply, qmg.SE_APPLY, qmg.SF_PAIR, (6, 4, 2), 1, 0b1, M0, c128, 0, None),
    ("qmg_stencil_apply", "gen", f_apply, qmg.SE_APPLY, qmg.SF_GEN, (6, 4, 3), 2, 0b11, MP, c128, 0, None),
    ("qmg_stencil_apply_batch", "elem", f_batch, SE, qmg.SF_ELEM, (6, 4, 2), 3, 0b101, EO0, c128, 0, None),
    ("qmg_stencil_apply_batch", "pair", f_batch, SE, qmg.SF_PAIR, (520, 4, 1), 3, 0b101, M0, c128, 0, None),
    ("qmg_stencil_apply_batch", "site", f_batch, SE, qmg.SF_SITE, (6, 4, 2), 3, 0b101, MP, c128, 0, {"stencil_site": 7}),
    ("qmg_stencil_apply_batch", "gen", f_batch, SE, qmg.SF_GEN, (6, 4, 6), 3, 0b101, M0, c128, 0, None),
    ("qmg_stencil_apply_batch", "mfma", f_batch, SE, qmg.SF_MFMA, (6, 4, 8), 6, 0b110111, M0, c128, 0, None),
    ("qmg_stencil_apply_batch", "volume1", f_batch, SE, qmg.SF_VOLUME1, (1, 1, 1), 1, 0b1, M0, c128, 0, None),
    ("qmg_stencil_apply_t", "c64-elem", f_t(C64), SE, qmg.SF_ELEM, (6, 4, 4), 1, 0b1, EO0, c128, 0, None),
    ("qmg_stencil_apply_t", "c32-elem", f_t(C32), SE, qmg.SF_ELEM, (520, 4, 1), 1, 0b1, HOP0, c64, 1, None),
    ("qmg_stencil_apply_t", "c32-site", f_t(C32), SE, qmg.SF_SITE, (6, 4, 2), 3, 0b101, M0, c64, 1, None),
    ("qmg_stencil_apply_t", "c32-gen32", f_t(C32), SE, qmg.SF_GEN32, (6, 4, 6), 3, 0b101, M0, c64, 1, None),
    ("qmg_stencil_apply_t", "c32-mfma", f_t(C32), SE, qmg.SF_MFMA, (6, 4, 8), 6, 0b110111, M0, c64, 1, None),
    ("qmg_stencil_apply_mat32", "gen32", f_mat32, SE, qmg.SF_GEN32, (6, 4, 6), 3, 0b101, M0, c128, 1, None),
    ("qmg_stencil_apply_mat32", "mfma", f_mat32, SE, qmg.SF_MFMA, (6, 4, 8), 6, 0b110111, M0, c128, 1, None),
    ("qmg_stencil_apply_mat16_t", "c64-gen32", f_mat16(C64), SE, qmg.SF_GEN32, (6, 4, 8), 3, 0b101, M0, c128, 2, None),
    ("qmg_stencil_apply_mat16_t", "c32-gen32", f_mat16(C32), SE, qmg.SF_GEN32, (6, 4, 8), 3, 0b101, M0, c64, 2, None),
    ("qmg_stencil_apply_mat16_t", "c64-mfma", f_mat16(C64), SE, qmg.SF_MFMA, (6, 4, 8), 6, 0b110111, M0, c128, 2, None),
    ("qmg_stencil_apply_h16", "site", f_h16, qmg.SE_H16, qmg.SF_SITE, (6, 4, 2), 3, 0b101, M0, c64, 2, None),
]
for _row in STENCIL_ROWS:
    case(_row[0], label=_row[1])(lambda r=_row: stencil_case(r[2], r[3], r[4], r[5], r[6], r[7], r[8], vdt=r[9], mat=r[10], knobs=r[11]))


@case("qmg_stencil_apply_norm2", label="host")
def _():
    c = stencil_case(lambda d, b, pieces, nrhs, stride, mask, s: qmg.stencil_apply_norm2(d, b.lhs, b.rhs, pieces, nrhs, stride, stream=s),
                     qmg.SE_NORM2, qmg.SF_PAIR, (6, 4, 2), 2, 0b11, M0)
    c.host = True
    return c


@case("qmg_stencil_apply_norm2", label="norms_dev")
def _():
    return stencil_case(lambda d, b, pieces, nrhs, stride, mask, s: qmg.stencil_apply_norm2(d, b.lhs, b.rhs, pieces, nrhs, stride, norms_dev=b.o.ptr, stream=s),
                        qmg.SE_NORM2, qmg.SF_PAIR, (520, 4, 1), 2, 0b11, M0, extra_outs={"o": (f64, 2)})


def _epi_case(dtype, mat):
    # out = other_scale other + acc_scale acc of system 1, and the dots against `other` into the MR slot, which the update behind it consumes
    dims, vdt = (6, 4, 3), NPT[dtype]
    n = dims[0] * dims[1] * dims[2]
    stride = n + PAD

    def fn(d, b, pieces, nrhs, stride_, mask, s):
        epi = qmg.make_epilogue(other=b.other, other_scale=1.0, acc_scale=-1.0, dotv=b.other)
        checked(qmg.stencil_apply_epi(dtype, 1 if dtype == C32 else mat, d, b.lhs, b.rhs, pieces, epi, vec_stride=stride, system=1, stream=s), "qmg_stencil_apply_epi_t")
        qmg.batch_mr_update(dtype, 0.85, b.x, b.other, None, b.lhs, True, n, 2, stride, 0b10, stream=s)
    return stencil_case(fn, qmg.SE_EPI, qmg.SF_GEN, dims, 2, 0b10, M0, vdt=vdt, mat=1 if (mat or dtype == C32) else 0, epilogue=2,
                        extra_ins={"other": cv(stride * 2, 7, vdt)}, extra_outs={"x": (vdt, stride * 2)})


case("qmg_stencil_apply_epi_t", label="c64-gen")(lambda: _epi_case(C64, 0))
case("qmg_stencil_apply_epi_t", label="c32-gen")(lambda: _epi_case(C32, 0))
case("qmg_stencil_apply_epi_t", label="c64-m32-gen")(lambda: _epi_case(C64, 1))


# ---------------------------------------------------------------- y-slabs on one rank: the halo exchange is the on-device copy path
def _halo_case(dtype, parity):
    Lx, Ly, nc, nrhs = 6, 4, 2, 2
    vdt, n = NPT[dtype], 6 * 4 * 2
    stride, hstride = n + PAD, Lx * nc + PAD

    def call(b, s):
        if parity:
            qmg.halo_exchange_parity(dtype, b.v, Lx, Ly, nc, b.lo, b.hi, parity, nrhs, stride, hstride, stream=s)
        else:
            qmg.halo_exchange(dtype, b.v, Lx, Ly, nc, b.lo, b.hi, nrhs, stride, hstride, stream=s)
    return Case(call, ins={"v": cv(stride * nrhs, 1, vdt)}, outs={"lo": (vdt, hstride * nrhs), "hi": (vdt, hstride * nrhs)})


for _dt in (C64, C32):
    case("qmg_halo_exchange", label=TAG[_dt])(lambda d=_dt: _halo_case(d, 0))
    case("qmg_halo_exchange_parity", label=TAG[_dt] + "-odd")(lambda d=_dt: _halo_case(d, 2))


def _slab_case(rows, storage=C64, nc=2, family=None, mat=0):
    Lx, Ly = 6, 4
    vdt = NPT[storage & 1]
    hstride = Lx * nc + PAD

    def fn(d, b, pieces, nrhs, stride, mask, s):
        qmg.halo_exchange(storage & 1, b.rhs, Lx, Ly, nc, b.lo, b.hi, nrhs, stride, hstride, stream=s)
        qmg.stencil_apply_slab(storage, d, b.lhs, b.rhs, b.lo, b.hi, pieces, nrhs, stride, hstride, mask, rows, stream=s)
    c = stencil_case(fn, qmg.SE_SLAB, family, (Lx, Ly, nc), 2, 0b11, M0, vdt=vdt, mat=mat, slab_rows=rows,
                     extra_outs={"lo": (vdt, hstride * 2), "hi": (vdt, hstride * 2)})
    return c


for _rows in (0, 1, 2):
    case("qmg_stencil_apply_slab", label="rows%d" % _rows)(lambda r=_rows: _slab_case(r))
case("qmg_stencil_apply_slab", label="c32")(lambda: _slab_case(0, C32, mat=1))
case("qmg_stencil_apply_slab", label="m32-nc6")(lambda: _slab_case(0, C64 | qmg.SLAB_M32, nc=6, mat=1))


# ---------------------------------------------------------------- operator construction
FL = (6, 4)


def _fill(sym, f, outs, slab=False):
    @case(sym)
    def _():
        Lx, Ly = FL
        gLy = 3 * Ly if slab else Ly
        return Case(f, ins={"g": links(Lx, gLy, 1)}, outs={k: (c128, n * Lx * Ly) for k, n in outs.items()})


_fill("qmg_wilson_fill", lambda b, s: qmg.wilson_fill(b.cl, b.ho, b.g, *FL, 0.9, stream=s), {"cl": 4, "ho": 16})
_fill("qmg_staggered_fill", lambda b, s: qmg.staggered_fill(b.ho, b.g, *FL, stream=s), {"ho": 4})
_fill("qmg_laplace_fill", lambda b, s: qmg.laplace_fill(b.cl, b.ho, b.g, *FL, stream=s), {"cl": 1, "ho": 4})
_fill("qmg_wilson_fill_slab", lambda b, s: qmg.wilson_fill_slab(b.cl, b.ho, b.g, FL[0], 3 * FL[1], FL[1], FL[1], 0.9, stream=s), {"cl": 4, "ho": 16}, slab=True)
_fill("qmg_staggered_fill_slab", lambda b, s: qmg.staggered_fill_slab(b.ho, b.g, FL[0], 3 * FL[1], FL[1], FL[1], stream=s), {"ho": 4}, slab=True)
_fill("qmg_laplace_fill_slab", lambda b, s: qmg.laplace_fill_slab(b.cl, b.ho, b.g, FL[0], 3 * FL[1], FL[1], FL[1], stream=s), {"cl": 1, "ho": 4}, slab=True)


def _well(vol, nc, seed):
    """a clover field whose blocks invert well"""
    return (cv(vol * nc * nc, seed).reshape(vol, nc, nc) + 4 * nc * np.eye(nc)).reshape(-1)


@case("qmg_cshift")
def _():
    Lx, Ly, dof = 6, 4, 3
    n = Lx * Ly * dof

    def call(b, s):
        qmg.cshift(b.y, b.x, qmg.CSHIFT_XP1, qmg.EO_FROM_EVENODD, dof, Lx, Ly, stream=s)
        qmg.cshift(b.z, b.x, qmg.CSHIFT_FROM_0, qmg.EO_FROM_EVENODD, dof, Lx, Ly, stream=s)      # the copy path
    return Case(call, ins={"x": cv(n, 1)}, outs={"y": (c128, n), "z": (c128, n)})


@case("qmg_build_dagger")
def _():
    Lx, Ly, nc = 6, 4, 3
    cm = Lx * Ly * nc * nc
    return Case(lambda b, s: qmg.build_dagger(b.dc, b.dh, b.cl, b.ho, Lx, Ly, nc, stream=s), ins={"cl": cv(cm, 1), "ho": cv(4 * cm, 2)},
                outs={"dc": (c128, cm), "dh": (c128, 4 * cm)})


@case("qmg_build_dagger_slab")
def _():
    Lx, Ly, nc = 6, 4, 3
    cm, hn = Lx * Ly * nc * nc, Lx * nc * nc

    def call(b, s):
        # the -y field's `hi` buffer and the +y field's `lo` buffer, exchanged as fields of nc^2 components per site
        qmg.halo_exchange(C64, b.ho.offset(3 * cm), Lx, Ly, nc * nc, b.t0, b.ymhi, stream=s)
        qmg.halo_exchange(C64, b.ho.offset(cm), Lx, Ly, nc * nc, b.yplo, b.t1, stream=s)
        qmg.build_dagger_slab(b.dc, b.dh, b.cl, b.ho, Lx, Ly, nc, b.ymhi, b.yplo, stream=s)
    return Case(call, ins={"cl": cv(cm, 1), "ho": cv(4 * cm, 2)},
                outs={"dc": (c128, cm), "dh": (c128, 4 * cm), "t0": (c128, hn), "t1": (c128, hn), "ymhi": (c128, hn), "yplo": (c128, hn)})


@case("qmg_build_rbjacobi")
def _():
    Lx, Ly, nc = 6, 4, 3
    cm = Lx * Ly * nc * nc

    def reach():
        assert qmg.setup_plan(qmg.SETUP_OP_CINV, (Lx, Ly, nc), a=1, b=1)[0] == qmg.SUF_CINV
    return Case(lambda b, s: qmg.build_rbjacobi(b.ci, b.rc, b.rh, qmg.make_desc(Lx, Ly, nc, b.cl, b.ho, 0.1), stream=s), ins={"cl": _well(Lx * Ly, nc, 1), "ho": cv(4 * cm, 2)},
                outs={"ci": (c128, cm), "rc": (c128, cm), "rh": (c128, 4 * cm)}, reach=reach)


@case("qmg_rb_hopping_slab")
def _():
    Lx, Ly, nc = 6, 4, 3
    cm, hn = Lx * Ly * nc * nc, Lx * nc * nc

    def call(b, s):
        d = qmg.make_desc(Lx, Ly, nc, b.cl, b.ho, 0.1)
        qmg.build_rbjacobi(b.ci, b.rc, None, d, stream=s)
        qmg.halo_exchange(C64, b.ci, Lx, Ly, nc * nc, b.lo, b.hi, stream=s)
        qmg.rb_hopping_slab(b.rh, d, b.ci, b.lo, b.hi, stream=s)
    return Case(call, ins={"cl": _well(Lx * Ly, nc, 1), "ho": cv(4 * cm, 2)},
                outs={"ci": (c128, cm), "rc": (c128, cm), "rh": (c128, 4 * cm), "lo": (c128, hn), "hi": (c128, hn)})


@case("qmg_cmat_conjtrans")
def _():
    return Case(lambda b, s: qmg.cmat_conjtrans(b.y, b.x, 37, 3, stream=s), ins={"x": cv(37 * 9, 1)}, outs={"y": (c128, 37 * 9)})


# ---------------------------------------------------------------- transfer (qmg_transfer_plan) and setup (qmg_setup_plan)
XR, XP = qmg.XFER_RESTRICT, qmg.XFER_PROLONG


def xfer_case(sym, label, op, dtype, fdims, cdims, nrhs, mask, families, single=False, null32=False):
    vdt = NPT[dtype]
    nvec = cdims[2]
    fs, cs_ = fdims[0] * fdims[1] * fdims[2], cdims[0] * cdims[1] * cdims[2]
    fstride, cstride = (fs, cs_) if single else (fs + PAD, cs_ + PAD)
    n_active = bin(mask).count("1")
    src, dst, sn_, dn = ("f", "c", fstride, cstride) if op == XR else ("c", "f", cstride, fstride)

    def call(b, s):
        T = (dtype,) if sym.endswith("_t") else ()
        if single:
            getattr(qmg, sym[4:])(b.nv, nvec, b[src], b[dst], fdims, cdims, stream=s)
        elif op == XR:
            getattr(qmg, sym[4:])(*T, b.nv, nvec, b.f, b.c, fdims, cdims, nrhs, fstride, cstride, mask, stream=s)
        else:
            getattr(qmg, sym[4:])(*T, b.nv, nvec, b.c, b.f, fdims, cdims, nrhs, cstride, fstride, mask, stream=s)

    def reach():
        plan = qmg.transfer_plan(op, dtype, null32, nvec, fdims, cdims, n_active)
        assert [p[0] for p in plan] == list(families), plan
    return Case(call, ins={"nv": cv(nvec * fs, 1, c64 if null32 else vdt), src: cv(sn_ * nrhs, 2, vdt)}, inout={dst: cv(dn * nrhs, 3, vdt)}, reach=reach)


XFER_ROWS = [
    ("qmg_restrict", "", XR, C64, (8, 8, 2), (2, 2, 6), 1, 1, [qmg.XF_RESTRICT], True),
    ("qmg_restrict", "generic", XR, C64, (6, 6, 3), (2, 2, 5), 1, 1, [qmg.XF_RESTRICT_GENERIC], True),
    ("qmg_prolong", "", XP, C64, (8, 8, 2), (2, 2, 6), 1, 1, [qmg.XF_PROLONG], True),
    ("qmg_restrict_batch", "small", XR, C64, (8, 8, 2), (2, 2, 13), 3, 0b101, [qmg.XF_BRESTRICT_SMALL], False),
    ("qmg_restrict_batch", "tile", XR, C64, (8, 8, 3), (2, 2, 6), 4, 0b1111, [qmg.XF_BRESTRICT_TILE], False),
    ("qmg_prolong_batch", "tile", XP, C64, (8, 8, 2), (2, 2, 6), 3, 0b101, [qmg.XF_BPROLONG_TILE], False),
    ("qmg_restrict_batch_t", "c64-small", XR, C64, (8, 4, 2), (4, 2, 6), 2, 0b11, [qmg.XF_BRESTRICT_SMALL], False),
    ("qmg_restrict_batch_t", "c32-small", XR, C32, (8, 8, 2), (2, 2, 6), 2, 0b11, [qmg.XF_BRESTRICT_SMALL], False),
    ("qmg_restrict_batch_t", "c32-tile", XR, C32, (8, 8, 3), (2, 2, 6), 2, 0b11, [qmg.XF_BRESTRICT_TILE], False),
    ("qmg_restrict_batch_t", "c32-mfma", XR, C32, (8, 8, 2), (2, 2, 16), 5, 0b11111, [qmg.XF_BRESTRICT_MFMA], False),
    ("qmg_restrict_batch_t", "c32-mfma-two-passes", XR, C32, (8, 8, 2), (2, 2, 16), 13, 0x1FFF, [qmg.XF_BRESTRICT_MFMA] * 2, False),
    ("qmg_restrict_batch_t", "c64-one", XR, C64, (8, 8, 2), (2, 2, 6), 1, 1, [qmg.XF_RESTRICT], False),
    ("qmg_prolong_batch_t", "c64-tile", XP, C64, (8, 8, 2), (2, 2, 6), 3, 0b101, [qmg.XF_BPROLONG_TILE], False),
    ("qmg_prolong_batch_t", "c32-tile", XP, C32, (8, 8, 2), (2, 2, 16), 5, 0b11111, [qmg.XF_BPROLONG_TILE], False),
    ("qmg_prolong_batch_t", "c64-one", XP, C64, (8, 8, 2), (2, 2, 6), 1, 1, [qmg.XF_PROLONG], False),
    ("qmg_restrict_batch_nv32", "", XR, C64, (8, 8, 2), (2, 2, 6), 2, 0b10, [qmg.XF_RESTRICT_NV32], False),
    ("qmg_prolong_batch_nv32", "", XP, C64, (8, 8, 2), (2, 2, 6), 2, 0b10, [qmg.XF_PROLONG_NV32], False),
]
for _row in XFER_ROWS:
    case(_row[0], label=_row[1])(lambda r=_row: xfer_case(*r, null32=r[0].endswith("nv32")))


def ortho_case(sym, fdims, cdims, family, knobs=None, passes=2):
    nvec = cdims[2]
    fs, blocks = fdims[0] * fdims[1] * fdims[2], cdims[0] * cdims[1]

    def call(b, s):
        if sym == "qmg_block_orthonormalize":
            qmg.block_orthonormalize(b.nv, nvec, fdims, cdims[0], cdims[1], cholesky=b.ch, stream=s)
        elif sym == "qmg_block_orthonormalize_n":
            qmg.block_orthonormalize_n(b.nv, nvec, fdims, cdims[0], cdims[1], cholesky=b.ch, passes=passes, stream=s)
        else:
            qmg.block_bi_orthonormalize(b.nv, b.rv, nvec, fdims, cdims[0], cdims[1], block_L=b.ch, block_U=b.bu, stream=s)

    def reach():
        assert family is None or qmg.setup_plan(qmg.SETUP_OP_ORTHO, fdims, cdims[:2], nvec, a=passes)[0] == family
    inout = {"nv": cv(nvec * fs, 1)}
    outs = {"ch": (c128, blocks * nvec * nvec)}
    if sym == "qmg_block_bi_orthonormalize":
        inout["rv"] = cv(nvec * fs, 2)
        outs["bu"] = (c128, blocks * nvec * nvec)
    # the pass-by-pass formulations (csrc/qmg_transfer.hip) allocate their temporaries and synchronise the stream before they free them
    return Case(call, inout=inout, outs=outs, reach=reach, knobs=knobs, blocking=family != qmg.SUF_ORTHO_LDS and sym != "qmg_block_orthonormalize")


case("qmg_block_orthonormalize")(lambda: ortho_case("qmg_block_orthonormalize", (8, 8, 2), (2, 2, 4), None))
case("qmg_block_orthonormalize_n", label="lds")(lambda: ortho_case("qmg_block_orthonormalize_n", (8, 8, 2), (2, 2, 4), qmg.SUF_ORTHO_LDS))
case("qmg_block_orthonormalize_n", label="passes")(lambda: ortho_case("qmg_block_orthonormalize_n", (8, 8, 2), (2, 2, 4), qmg.SUF_ORTHO_PASSES, knobs={"setup_fused": 0}))
case("qmg_block_bi_orthonormalize")(lambda: ortho_case("qmg_block_bi_orthonormalize", (8, 8, 2), (2, 2, 4), None))


def galerkin_case(slab, family, knobs=None, sep_r=False):
    fdims, cdims = (8, 8, 2), (2, 2, 4)
    Lx, Ly, nc = fdims
    nvec = cdims[2]
    fs, cm, ccm = Lx * Ly * nc, Lx * Ly * nc * nc, cdims[0] * cdims[1] * nvec * nvec
    hstride = Lx * nc

    def call(b, s):
        d = qmg.make_desc(Lx, Ly, nc, b.cl, b.ho)
        if slab:
            qmg.halo_exchange(C64, b.nv, Lx, Ly, nc, b.lo, b.hi, nvec, fs, hstride, stream=s)
            qmg.coarse_build_slab(b.cc, b.ch, d, b.nv, cdims, b.lo, b.hi, hstride, stream=s)
        else:
            qmg.coarse_build(b.cc, b.ch, d, b.nv, cdims, restrict_vecs=b.rv if sep_r else None, stream=s)

    def reach():
        assert qmg.setup_plan(qmg.SETUP_OP_GALERKIN, fdims, cdims[:2], nvec, a=slab)[0] == family
    ins = {"cl": cv(cm, 1), "ho": cv(4 * cm, 2), "nv": cv(nvec * fs, 3)}
    if sep_r:
        ins["rv"] = cv(nvec * fs, 4)
    outs = {"cc": (c128, ccm), "ch": (c128, 4 * ccm)}
    if slab:
        outs.update(lo=(c128, nvec * hstride), hi=(c128, nvec * hstride))
    return Case(call, ins=ins, outs=outs, reach=reach, knobs=knobs, blocking=family == qmg.SUF_GALERKIN_PROBES)


case("qmg_coarse_build", label="galerkin")(lambda: galerkin_case(False, qmg.SUF_GALERKIN, sep_r=True))
case("qmg_coarse_build", label="probes")(lambda: galerkin_case(False, qmg.SUF_GALERKIN_PROBES, knobs={"setup_fused": 0}))
case("qmg_coarse_build_slab")(lambda: galerkin_case(True, qmg.SUF_GALERKIN))


# ---------------------------------------------------------------- the Wilson operator from the links (qmg_wilson_plan)
def wilson_case(sym, dtype, family, dims, nrhs, mask, pieces, knobs=None, epi=False, slab=False):
    Lx, Ly = dims
    vdt, n = NPT[dtype], Lx * Ly * 2
    stride, hstride = n + PAD, 2 * Lx + PAD
    gLy, y0 = (3 * Ly, Ly) if slab else (Ly, 0)
    hops = "hops" in sym
    n_active = bin(mask).count("1")

    def call(b, s):
        d = qmg.make_desc(Lx, Ly, 2, None, None, 0.2)
        lo, hi = (b.lo, b.hi) if slab else (None, None)
        if slab:
            qmg.halo_exchange(dtype, b.rhs, Lx, Ly, 2, b.lo, b.hi, nrhs, stride, hstride, stream=s)
        if epi:
            e = qmg.make_epilogue(other=b.other, other_scale=1.0, acc_scale=-1.0)
            f = qmg.lib().qmg_wilson_hops_direct_epi if hops else qmg.lib().qmg_wilson_apply_direct_epi
            sc = (C.c_double(0.9), C.c_double(0.37)) if hops else (C.c_double(0.9),)
            checked(f(dtype, C.byref(d), vp(b.g), gLy, y0, *sc, vp(b.lhs), vp(b.rhs), vp(lo), vp(hi), C.c_uint(pieces), nrhs, C.c_size_t(stride), C.c_size_t(hstride),
                      C.c_uint(mask), C.byref(e), C.c_void_p(s)), sym)
        elif hops:
            qmg.wilson_hops_direct(dtype, d, b.g, b.lhs, b.rhs, pieces, 0.9, 0.37, nrhs, stride, mask, gLy, y0, lo, hi, hstride, 0, stream=s)
        else:
            qmg.wilson_apply_direct(dtype, d, b.g, b.lhs, b.rhs, pieces, 0.9, nrhs, stride, mask, gLy, y0, lo, hi, hstride, 0, stream=s)

    def reach():
        plan = qmg.wilson_plan(dtype, dims, pieces, n_active, scaled=hops, epi=(qmg.WPE_ON | qmg.WPE_OTHER) if epi else 0, gauge_Ly=gLy, y0=y0, halos=slab)
        assert plan[0] == family and plan[13] == 0, plan
    ins = {"g": links(Lx, gLy, 1, vdt), "rhs": cv(stride * nrhs, 2, vdt)}
    outs = {"lo": (vdt, hstride * nrhs), "hi": (vdt, hstride * nrhs)} if slab else {}
    if epi:
        ins["other"] = cv(stride * nrhs, 4, vdt)
    return Case(call, ins=ins, inout={"lhs": cv(stride * nrhs, 3, vdt)}, outs=outs, reach=reach, knobs=knobs)


WA, WH = "qmg_wilson_apply_direct", "qmg_wilson_hops_direct"
WILSON_ROWS = [
    (WA, "c64-pair2", C64, qmg.WF_PAIR2, (6, 4), 1, 0b1, M0, None),
    (WA, "c64-pair", C64, qmg.WF_PAIR, (6, 4), 3, 0b101, M0, None),
    (WA, "c64-direct", C64, qmg.WF_DIRECT, (6, 4), 3, 0b101, EO0, None),
    (WA, "c32-pair", C32, qmg.WF_PAIR, (6, 4), 3, 0b101, M0, None),
    (WA, "c32-direct", C32, qmg.WF_DIRECT, (6, 4), 1, 0b1, M0, {"wilson_pair": 0}),
    (WH, "c64", C64, qmg.WF_DIRECT, (6, 4), 3, 0b101, HOP0, None),
    (WH, "c32", C32, qmg.WF_DIRECT, (6, 4), 1, 0b1, EO0, None),
]
for _row in WILSON_ROWS:
    case(_row[0], label=_row[1])(lambda r=_row: wilson_case(r[0], r[2], r[3], r[4], r[5], r[6], r[7], knobs=r[8]))
case(WA, label="c64-slab")(lambda: wilson_case(WA, C64, qmg.WF_PAIR, (6, 4), 2, 0b11, M0, slab=True))
case(WH, label="c64-slab")(lambda: wilson_case(WH, C64, qmg.WF_DIRECT, (6, 4), 2, 0b11, HOP0, slab=True))
for _dt in (C64, C32):
    case(WA + "_epi", label=TAG[_dt])(lambda d=_dt: wilson_case(WA + "_epi", d, qmg.WF_PAIR, (6, 4), 2, 0b10, M0, epi=True))
    case(WH + "_epi", label=TAG[_dt])(lambda d=_dt: wilson_case(WH + "_epi", d, qmg.WF_DIRECT, (6, 4), 2, 0b10, HOP0, epi=True))


# ---------------------------------------------------------------- domain-wall (qmg_dwf_plan, qmg_dwf_eo_plan, qmg_dwf_meas_plan, qmg_hmc_dwf_plan)
DW = (6, 4)
DLS = 4
DMASS = 0.05


def dwf_desc():
    return qmg.make_desc(DW[0], DW[1], 2 * DLS, None, None, -1.0)    # M5 = -1 in the identity shift: d_p = 3 w - 1 = 2


def dwf_vec(seed, dt, nrhs):
    return cv((DW[0] * DW[1] * 2 * DLS + PAD) * nrhs, seed, dt)


DSTRIDE = DW[0] * DW[1] * 2 * DLS + PAD


@case("qmg_dwf_fill")
def _():
    cm = DW[0] * DW[1] * (2 * DLS) ** 2
    return Case(lambda b, s: qmg.dwf_fill(b.cl, b.ho, b.g, DW[0], DW[1], DLS, DMASS, 1.0, stream=s), ins={"g": links(*DW, 1)}, outs={"cl": (c128, cm), "ho": (c128, 4 * cm)})


def dwf_apply_case(dtype, family, nrhs, mask, pieces):
    vdt = NPT[dtype]

    def reach():
        assert qmg.dwf_plan(dtype, DW, DLS, pieces, bin(mask).count("1"))[0] == family
    return Case(lambda b, s: qmg.dwf_apply_direct(dtype, dwf_desc(), b.g, DLS, DMASS, b.lhs, b.rhs, pieces, 1.0, nrhs, DSTRIDE, mask, stream=s),
                ins={"g": links(*DW, 1, vdt), "rhs": dwf_vec(2, vdt, nrhs)}, inout={"lhs": dwf_vec(3, vdt, nrhs)}, reach=reach)


for _dt in (C64, C32):
    case("qmg_dwf_apply_direct", label=TAG[_dt] + "-pair")(lambda d=_dt: dwf_apply_case(d, qmg.DF_PAIR, 3, 0b101, M0))
    case("qmg_dwf_apply_direct", label=TAG[_dt] + "-direct")(lambda d=_dt: dwf_apply_case(d, qmg.DF_DIRECT, 3, 0b101, EO0))


def dwf_eo_case(sym, dtype):
    vdt, nrhs, mask = NPT[dtype], 3, 0b101
    inv_p, hop_p = P.P_CLOVER_E | P.P_CLOVER_O, P.P_OE | P.P_ZERO_O

    def call(b, s):
        if sym == "qmg_dwf_inv5":
            qmg.dwf_inv5(dtype, dwf_desc(), DLS, DMASS, b.lhs, b.rhs, inv_p, 0.7 - 0.2j, 1.0, nrhs, DSTRIDE, mask, stream=s)
        elif sym == "qmg_dwf_hops_inv5":
            qmg.dwf_hops_inv5(dtype, dwf_desc(), b.g, DLS, DMASS, b.lhs, b.rhs, hop_p, 0.7 - 0.2j, qmg.DWF_G5_IN, 1.0, nrhs, DSTRIDE, mask, stream=s)
        else:
            qmg.dwf_schur_apply(dtype, dwf_desc(), b.g, DLS, DMASS, b.lhs, b.rhs, b.tmp, 0, qmg.DWF_G5_OUT, 1.0, nrhs, DSTRIDE, mask, stream=s)

    def reach():
        n_active = 2
        if sym == "qmg_dwf_inv5":
            assert qmg.dwf_eo_plan(dtype, DW, DLS, qmg.DEK_INV5, inv_p, n_active)[0] == qmg.DEF_INV5
        elif sym == "qmg_dwf_hops_inv5":
            assert qmg.dwf_eo_plan(dtype, DW, DLS, qmg.DEK_HOPS_INV5, hop_p, n_active)[0] == qmg.DEF_HOPS_INV5
        else:
            assert qmg.dwf_eo_plan(dtype, DW, DLS, qmg.DEK_HOPS_INV5, P.P_OE | P.P_ZERO_O, n_active)[0] == qmg.DEF_HOPS_INV5
            assert qmg.dwf_eo_plan(dtype, DW, DLS, qmg.DEK_SCHUR2, P.P_CLOVER_E | P.P_EO | P.P_SHIFT_E | P.P_ZERO_E, n_active)[0] == qmg.DEF_SCHUR2
    ins = {"rhs": dwf_vec(2, vdt, nrhs)}
    if sym != "qmg_dwf_inv5":
        ins["g"] = links(*DW, 1, vdt)
    return Case(call, ins=ins, inout={"lhs": dwf_vec(3, vdt, nrhs)}, outs={"tmp": (vdt, DSTRIDE * nrhs)} if sym == "qmg_dwf_schur_apply" else {}, reach=reach)


for _sym in ("qmg_dwf_inv5", "qmg_dwf_hops_inv5", "qmg_dwf_schur_apply"):
    for _dt in (C64, C32):
        case(_sym, label=TAG[_dt])(lambda y=_sym, d=_dt: dwf_eo_case(y, d))


def dwf_meas_case(sym, dtype, which=0, host=False):
    vdt, nsys = NPT[dtype], 2
    n4 = DW[0] * DW[1] * 2
    s4, s5 = n4 + PAD, DSTRIDE
    kernel = {"qmg_dwf_wall_source": qmg.DMK_SOURCE, "qmg_dwf_wall_project": qmg.DMK_PROJECT_MID if which else qmg.DMK_PROJECT_WALL, "qmg_dwf_slice_norms": qmg.DMK_NORMS}[sym]
    family = {"qmg_dwf_wall_source": qmg.DMF_SOURCE, "qmg_dwf_wall_project": qmg.DMF_PROJECT, "qmg_dwf_slice_norms": qmg.DMF_NORMS}[sym]

    def reach():
        assert qmg.dwf_meas_plan(dtype, DW, DLS, kernel, nsys)[0] == family
    if sym == "qmg_dwf_wall_source":
        return Case(lambda b, s: qmg.dwf_wall_source(dtype, DW, DLS, b.psi, b.eta, nsys, s5, s4, stream=s), ins={"eta": cv(s4 * nsys, 1, vdt)}, outs={"psi": (vdt, s5 * nsys)}, reach=reach)
    if sym == "qmg_dwf_wall_project":
        return Case(lambda b, s: qmg.dwf_wall_project(dtype, DW, DLS, b.q, b.psi, which, nsys, s4, s5, stream=s), ins={"psi": dwf_vec(1, vdt, nsys)}, outs={"q": (vdt, s4 * nsys)}, reach=reach)
    if host:
        return Case(lambda b, s: qmg.dwf_slice_norms(dtype, DW, DLS, b.psi, nsys, s5, stream=s), ins={"psi": dwf_vec(1, vdt, nsys)}, host=True, reach=reach)
    return Case(lambda b, s: checked(qmg.dwf_slice_norms_status(dtype, DW, DLS, b.psi, nsys, s5, out_dev=b.o, stream=s), sym), ins={"psi": dwf_vec(1, vdt, nsys)},
                outs={"o": (f64, nsys * DW[1] * 2 * DLS)}, reach=reach)


for _dt in (C64, C32):
    case("qmg_dwf_wall_source", label=TAG[_dt])(lambda d=_dt: dwf_meas_case("qmg_dwf_wall_source", d))
    case("qmg_dwf_wall_project", label=TAG[_dt] + "-wall")(lambda d=_dt: dwf_meas_case("qmg_dwf_wall_project", d, 0))
    case("qmg_dwf_wall_project", label=TAG[_dt] + "-midpoint")(lambda d=_dt: dwf_meas_case("qmg_dwf_wall_project", d, 1))
    case("qmg_dwf_slice_norms", label=TAG[_dt] + "-host")(lambda d=_dt: dwf_meas_case("qmg_dwf_slice_norms", d, host=True))
    case("qmg_dwf_slice_norms", label=TAG[_dt] + "-out_dev")(lambda d=_dt: dwf_meas_case("qmg_dwf_slice_norms", d))


# ---------------------------------------------------------------- flavour-singlet loops (qmg_singlet_plan)
SG = (6, 8, 2)
DIL = (2, 1, 1)


@case("qmg_noise_z4")
def _():
    return Case(lambda b, s: qmg.noise_z4(b.eta, 1031, 5, stream=s), outs={"eta": (c128, 1031)})


def singlet_reach():
    assert qmg.singlet_plan(SG[:2], SG[2], DIL, 1, 3, 0b101)[0] == qmg.SGF_ROWS


for _dt in (C64, C32):
    @case("qmg_noise_dilute_batch", label=TAG[_dt])
    def _(dtype=_dt):
        stride = SG[0] * SG[1] * SG[2] + PAD
        return Case(lambda b, s: qmg.noise_dilute_batch(dtype, b.o, SG[:2], SG[2], DIL, 1, 5, 3, stride, 0b101, stream=s), outs={"o": (NPT[dtype], stride * 3)}, reach=singlet_reach)

    @case("qmg_loops_timeslice_batch", label=TAG[_dt] + "-host")
    def _(dtype=_dt):
        stride = SG[0] * SG[1] * SG[2] + PAD
        return Case(lambda b, s: qmg.loops_timeslice_batch(dtype, b.psi, SG[:2], SG[2], DIL, 1, 5, 0, 3, stride, 0b101, stream=s), ins={"psi": cv(stride * 3, 1, NPT[dtype])},
                    host=True, reach=singlet_reach)

    @case("qmg_loops_timeslice_batch", label=TAG[_dt] + "-out_dev")
    def _(dtype=_dt):
        stride = SG[0] * SG[1] * SG[2] + PAD
        return Case(lambda b, s: checked(qmg.loops_timeslice_batch_status(dtype, b.psi, SG[:2], SG[2], DIL, 1, 5, 0, 3, stride, 0b101, out_dev=b.o, stream=s), "qmg_loops_timeslice_batch"),
                    ins={"psi": cv(stride * 3, 1, NPT[dtype])}, outs={"o": (f64, 3 * SG[1] * 5)}, reach=singlet_reach)


# ---------------------------------------------------------------- U(1) fields, flow, HMC
U = (6, 8)
UV = U[0] * U[1]
NL = 2 * UV


def _u1(sym, f, ins="", inout="", outs="", host=False, kinds=None):
    """ins / inout / outs: letters g (links), t (a second link field), p (phases / momenta, real), q (a second real field), x y (spinors), w (nc = 1 vector)"""
    def make(name, seed):
        return {"g": lambda: links(*U, seed), "t": lambda: links(*U, seed), "p": lambda: rv(NL, seed), "q": lambda: rv(NL, seed), "r": lambda: rv(NL, seed),
                "x": lambda: cv(2 * UV, seed), "y": lambda: cv(2 * UV, seed), "w": lambda: cv(UV, seed)}[name]()
    shape = {"g": (c128, NL), "t": (c128, NL), "p": (f64, NL), "q": (f64, NL), "r": (f64, NL), "x": (c128, 2 * UV), "y": (c128, 2 * UV), "w": (c128, UV)}

    @case(sym)
    def _():
        return Case(f, ins={k: make(k, 70 + i) for i, k in enumerate(ins)}, inout={k: make(k, 80 + i) for i, k in enumerate(inout)}, outs={k: shape[k] for k in outs}, host=host)


_u1("qmg_u1_heatbath_noncompact", lambda b, s: qmg.u1_heatbath_noncompact(b.p, *U, 6.0, 2, 11, 3, stream=s), inout="p")
_u1("qmg_u1_phase_to_gauge", lambda b, s: qmg.u1_phase_to_gauge(b.g, b.p, NL, stream=s), ins="p", outs="g")
_u1("qmg_u1_gauge_to_phase", lambda b, s: qmg.u1_gauge_to_phase(b.p, b.g, NL, stream=s), ins="g", outs="p")
_u1("qmg_u1_plaquette", lambda b, s: np.asarray(qmg.u1_plaquette(b.g, *U, stream=s), dtype=c128), ins="g", host=True)
_u1("qmg_u1_noncompact_action", lambda b, s: np.asarray(qmg.u1_noncompact_action(b.p, *U, 6.0, stream=s)), ins="p", host=True)
_u1("qmg_u1_hot_gauge", lambda b, s: qmg.u1_hot_gauge(b.g, *U, 5, stream=s), outs="g")
_u1("qmg_u1_gauss_gauge", lambda b, s: qmg.u1_gauss_gauge(b.g, *U, 6.0, 5, stream=s), outs="g")
_u1("qmg_u1_random_trans", lambda b, s: qmg.u1_random_trans(b.w, *U, 5, stream=s), outs="w")
_u1("qmg_u1_gauge_transform", lambda b, s: qmg.u1_gauge_transform(b.g, b.w, *U, stream=s), ins="w", inout="g")
_u1("qmg_u1_ape_smear", lambda b, s: qmg.u1_ape_smear(b.t, b.g, *U, 0.5, 3, stream=s), ins="g", outs="t")
_u1("qmg_u1_instanton", lambda b, s: qmg.u1_instanton(b.g, *U, 1.0, 2, 3, stream=s), inout="g")
_u1("qmg_u1_noncompact_instanton", lambda b, s: qmg.u1_noncompact_instanton(b.p, *U, 1.0, stream=s), inout="p")
_u1("qmg_hmc_momentum_update", lambda b, s: qmg.hmc_momentum_update(b.p, b.g, b.x, b.y, *U, 6.0, 0.1, stream=s), ins="gxy", inout="p")
_u1("qmg_hmc_link_update", lambda b, s: qmg.hmc_link_update(b.q, b.g, b.p, NL, 0.1, stream=s), ins="p", inout="q", outs="g")
_u1("qmg_hmc_gauge_step", lambda b, s: qmg.hmc_gauge_step(b.q, b.t, b.g, b.p, *U, 6.0, 0.1, 0.2, stream=s), ins="g", inout="qp", outs="t")
_u1("qmg_hmc_momentum_refresh", lambda b, s: qmg.hmc_momentum_refresh(b.p, NL, 5, 7, stream=s), outs="p")
_u1("qmg_u1_stout_force_level", lambda b, s: qmg.u1_stout_force_level(b.q, b.p, b.g, *U, 0.1, stream=s), ins="pg", outs="q")
_u1("qmg_hmc_momentum_update_stout", lambda b, s: qmg.hmc_momentum_update_stout(b.p, b.g, b.q, *U, 6.0, 0.1, 0.1, stream=s), ins="gq", inout="p")
_u1("qmg_u1_wilson_loops", lambda b, s: qmg.u1_wilson_loops(b.g, *U, 2, 3, stream=s), ins="g", host=True)
_u1("qmg_u1_polyakov", lambda b, s: np.asarray(qmg.u1_polyakov(b.g, *U, stream=s)), ins="g", host=True)


def _poles(sym, npole, f, extra_out=None, w=False):
    @case(sym, label="%d-poles" % npole)
    def _():
        ins = {"g": links(*U, 1)}
        for j in range(npole):
            if w:
                ins["w%d" % j] = cv(UV, 10 + j)
            else:
                ins["x%d" % j], ins["y%d" % j] = cv(2 * UV, 10 + j), cv(2 * UV, 40 + j)
        weights = list(0.5 + np.abs(rv(npole, 3)))
        return Case(lambda b, s: f(b, [b["%s%d" % ("w" if w else "x", j)] for j in range(npole)], None if w else [b["y%d" % j] for j in range(npole)], weights, s),
                    ins=ins, inout={} if extra_out else {"p": rv(NL, 2)}, outs=extra_out or {})


# 17 poles: 16 in the first launch, the last in a second one
_poles("qmg_hmc_momentum_update_poles", 17, lambda b, X, Y, wts, s: qmg.hmc_momentum_update_poles(b.p, b.g, X, Y, wts, *U, 6.0, 0.1, stream=s))
_poles("qmg_hmc_momentum_update_staggered", 17, lambda b, X, Y, wts, s: qmg.hmc_momentum_update_staggered(b.p, b.g, X, wts, *U, 6.0, 0.1, stream=s), w=True)
_poles("qmg_hmc_fermion_force", 17, lambda b, X, Y, wts, s: qmg.hmc_fermion_force(b.F, b.g, X, Y, wts, *U, stream=s), extra_out={"F": (f64, NL)})


@case("qmg_u1_stout_smear")
def _():
    return Case(lambda b, s: qmg.u1_stout_smear(b.lv, b.g, *U, 0.1, 3, stream=s), ins={"g": links(*U, 1)}, outs={"lv": (c128, 3 * NL)})


@case("qmg_u1_flow_stage")
def _():
    def call(b, s):
        qmg.u1_flow_stage(b.th, b.acc, b.t, b.g, *U, 0.02, 1, stream=s)
        qmg.u1_flow_stage(b.th, b.acc, b.g2, b.t, *U, 0.02, 2, stream=s)
        qmg.u1_flow_stage(b.th, b.acc, b.t, b.g2, *U, 0.02, 3, stream=s)
    return Case(call, ins={"g": links(*U, 1)}, inout={"th": rv(NL, 2), "acc": rv(NL, 3)}, outs={"t": (c128, NL), "g2": (c128, NL)})


@case("qmg_u1_flow")
def _():
    th = np.random.default_rng(4).uniform(-3, 3, NL)
    return Case(lambda b, s: qmg.u1_flow(b.th, b.g, *U, 0.02, 2, stream=s), inout={"th": th, "g": np.exp(1j * th)})


def hmc_dwf_case(n_pairs, family, flags=0):
    n5 = DW[0] * DW[1] * 2 * DLS

    def reach():
        plan = qmg.hmc_dwf_plan(DW, DLS, n_pairs, flags)
        assert plan[0] == family and (n_pairs <= 4 or plan[6] >= 2), plan
    ins = {"g": links(*DW, 1)}
    for j in range(n_pairs):
        ins["x%d" % j], ins["y%d" % j] = cv(n5, 10 + j), cv(n5, 40 + j)
    weights = list(0.5 + np.abs(rv(max(n_pairs, 1), 3)))[:n_pairs]
    return Case(lambda b, s: qmg.hmc_momentum_update_dwf(b.p, b.g, [b["x%d" % j] for j in range(n_pairs)], [b["y%d" % j] for j in range(n_pairs)], weights, DLS, *DW, 6.0, 0.1,
                                                          flags, stream=s), ins=ins, inout={"p": rv(2 * DW[0] * DW[1], 2)}, reach=reach)


case("qmg_hmc_momentum_update_dwf", label="fused-two-launches")(lambda: hmc_dwf_case(5, qmg.HDF_FUSED, qmg.HMC_DWF_G5_Y))
case("qmg_hmc_momentum_update_dwf", label="gauge-only")(lambda: hmc_dwf_case(0, qmg.HDF_GAUGE))


# ---------------------------------------------------------------- the protocol
ALL = [(sym, label, maker) for sym in sorted(CASES) for label, maker in CASES[sym]]
IDS = [sym[4:] + ("-" + label if label else "") for sym, label, _ in ALL]
assert len(set(IDS)) == len(IDS), [i for i in IDS if IDS.count(i) > 1]


@pytest.fixture(scope="module")
def gate_stream():
    """the one created stream of the module, and the gate copies that make GATE_MS"""
    qmg.init(0)
    st = qmg.stream_create()
    per_copy = sg.copy_ms(st)
    copies = max(4, int(math.ceil(GATE_MS / per_copy)))
    print("\n[streams] one gate copy of %d MiB: %.3f ms; %d copies per gate" % (sg.GATE_BYTES >> 20, per_copy, copies))
    yield types.SimpleNamespace(st=st, copies=copies)
    qmg.sync()
    qmg.stream_destroy(st)


class knobs:
    def __init__(self, kv):
        self.kv = kv

    def __enter__(self):
        for k, v in self.kv.items():
            qmg.set_tuning(k, v)

    def __exit__(self, *exc):
        for k in self.kv:
            qmg.set_tuning(k, DEFAULT_KNOBS[k])


def raw(d):
    return d.to_host().view(np.uint8).copy()


def poison(d):
    qmg.memcpy_h2d(d, np.full(d.nbytes, 0xFF, dtype=np.uint8))


def decoy_of(name, a, case_):
    if name in case_.decoy:
        return case_.decoy[name]
    return np.ascontiguousarray(np.roll(a, 1 + a.size // 3))


def as_bytes(r):
    return np.ascontiguousarray(np.asarray(r)).view(np.uint8).copy()


def run_case(c, gs, escape=False):
    """(what the gated run left, the reference), each a dict of bytes per output (or {'ret': ...} for a host-returning case)"""
    given = dict(c.ins, **c.inout)
    written = list(c.outs) + list(c.inout)
    bufs = Bufs()
    for k, a in given.items():
        bufs[k] = qmg.DeviceArray(a.size, a.dtype)
    for k, (dt, n) in c.outs.items():
        bufs[k] = qmg.DeviceArray(n, dt)
    with knobs(c.knobs):
        if c.reach:
            c.reach()

        def null_run(values):
            for k, a in given.items():
                bufs[k].upload(values(k, a))
            for k in c.outs:
                poison(bufs[k])
            r = c.call(bufs, None)
            qmg.sync()
            return r
        # 1. the reference, on the synchronised null stream (also grows every library scratch buffer)
        r = null_run(lambda k, a: a)
        ref_written = {k: raw(bufs[k]) for k in written}
        ref = {"ret": as_bytes(r)} if c.host else dict(ref_written)
        # 2. the decoy: library scratch now holds another call's intermediates
        null_run(lambda k, a: decoy_of(k, a, c))
        # 3. the gated run
        staging = {k: qmg.DeviceArray.from_host(a) for k, a in given.items()}
        copies = {k: qmg.DeviceArray(bufs[k].n, bufs[k].dtype) for k in written}
        for d in list(bufs.values()) + list(copies.values()):
            poison(d)
        qmg.sync()
        st = gs.st
        gate = sg.Gate(st, gs.copies)
        t0 = time.perf_counter()
        for k in given:
            qmg.memcpy_d2d(bufs[k], staging[k], bufs[k].nbytes, stream=st)
        for k in c.outs:      # and the outputs are poisoned once more behind the gate: what a writer without device inputs left too early is lost
            qmg.memcpy_d2d(bufs[k], copies[k], bufs[k].nbytes, stream=st)
        if c.host or c.blocking:
            assert gate.closed(), "gate open: case proves nothing"
            r = c.call(bufs, None if escape else st)
            qmg.sync(st)
            qmg.sync()
            got = {"ret": as_bytes(r)} if c.host else {}
            if c.host and written:
                ref.update({k: ref_written[k] for k in written})
            got.update({k: raw(bufs[k]) for k in written})
        else:
            c.call(bufs, None if escape else st)
            enqueue_ms = 1e3 * (time.perf_counter() - t0)
            assert gate.closed(), "gate open: case proves nothing"
            for k in written:
                qmg.memcpy_d2d(copies[k], bufs[k], bufs[k].nbytes, stream=st)
            qmg.sync(st)
            qmg.sync()
            print("[streams] enqueue %.3f ms, gate %.1f ms" % (enqueue_ms, gate.length_ms()))
            got = {k: raw(bufs[k]) for k in written}
            got.update({"copy of " + k: raw(copies[k]) for k in written})
            ref.update({"copy of " + k: ref[k] for k in written})
        for k, a in c.ins.items():
            got["input " + k], ref["input " + k] = raw(bufs[k]), as_bytes(a)
    return got, ref


@pytest.mark.parametrize("sym,label,maker", ALL, ids=IDS)
def test_call_stays_on_its_stream(sym, label, maker, gate_stream):
    got, ref = run_case(maker(), gate_stream)
    assert sorted(got) == sorted(ref)
    for k in ref:
        assert np.array_equal(got[k], ref[k]), "%s %s: `%s` differs from the synchronised null-stream run in %d of %d bytes" % (
            sym, label, k, int(np.count_nonzero(got[k] != ref[k])), ref[k].size)


CONTROLS = [("qmg_caxpy", ""), ("qmg_stencil_apply_batch", "pair"), ("qmg_block_orthonormalize_n", "lds")]


@pytest.mark.parametrize("sym,label", CONTROLS, ids=[s[4:] for s, _ in CONTROLS])
def test_escaped_call_is_caught(sym, label, gate_stream):
    """The negative control: the call goes to the null stream while its inputs are still behind the gate; it reads the 0xFF poison."""
    maker = dict(CASES[sym])[label]
    got, ref = run_case(maker(), gate_stream, escape=True)
    written = [k for k in ref if not k.startswith("input ")]
    assert any(not np.array_equal(got[k], ref[k]) for k in written), "%s ran on the null stream behind a closed gate and still matched: the gate does not gate" % sym


# ---------------------------------------------------------------- first use on a created stream, in a fresh process
LEGS = ["norm2sq", "batch_reduce", "mr_dots", "apply_norm2", "basis_dot", "plaquette", "wilson_loops", "slice_norms", "loops", "thread"]
_first_use = {"dead": None}


@pytest.mark.parametrize("leg", LEGS)
def test_first_use_on_a_created_stream(leg):
    """The named call is the first compute call of a fresh process (leg `thread`: of a second host thread while the main thread idles), on a
    created stream behind a gate; the worker repeats it on the synchronised null stream and holds both results to the numpy twin of the entry
    point at the tolerance of its own test.  The two results must be the same bits."""
    assert _first_use["dead"] is None, "leg %s ended by signal or at its time limit: the remaining legs do not run" % _first_use["dead"]
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "stream_first_use_worker.py")
    try:
        out = subprocess.run([sys.executable, worker, leg], capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        _first_use["dead"] = leg
        raise
    if out.returncode < 0:
        _first_use["dead"] = leg
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = dict(line.split(" ", 1) for line in out.stdout.splitlines() if line.startswith(("stream ", "null ", "gate ", "twin ")))
    assert lines.get("gate") == "closed", out.stdout[-2000:]
    assert lines["stream"] == lines["null"], out.stdout[-2000:]
    assert lines.get("twin") == "ok", out.stdout[-2000:]
