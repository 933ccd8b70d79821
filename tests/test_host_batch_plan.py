"""CPU-side checks behind tests/test_gpu_batch_routes.py (no GPU: qmg_batch_plan is host code and makes no HIP call).

1. The reference of the route tests is validated before it judges a kernel: batch_numpy against plain complex128 numpy statements of every
   operation, elementwise under the bound the kernels are held to, and its reductions against the oracle's (ol.dot, ol.norm2sq,
   ol.diffnorm2sq).
2. Every row's expected plan is what qmg_batch_plan answers.
3. Coverage: qmg_batch_plan is enumerated over a finite domain of requests, and every distinct pass found there must be the expected pass of
   at least one row of the route table (per storage: a multi-axpy pass is the same launch whether qmg_batch_multi_caxpy_t or the GCR update
   asked for it); every pass that launches nothing must be on the explicit list NOTHING_BECAUSE.  A retune that creates a route no row runs
   fails here until a row is added (a new route needs a row).
4. The long-vector forms begin exactly at BATCH_LONG_BYTES, for both storages.
"""
import ctypes as C
import importlib
import itertools

import numpy as np
import pytest

import batch_numpy as bn
import oracle_lib as ol
import test_gpu_batch_routes as routes

qmg = importlib.import_module("quantum-mg_amd")

C64, C32 = routes.C64, routes.C32


@pytest.fixture(scope="module", autouse=True)
def _built():
    qmg.build()
    yield
    qmg.set_tuning("blas_nt_mb", routes.NT_DEFAULT)


def vec(n, seed, narrow=False):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return bn.r32(v) if narrow else v


def within(got, want, bound):
    return bool(np.all(np.abs(np.asarray(got).astype(bn.CLD) - want) <= bound))


# ---- 1. the reference
@pytest.mark.parametrize("n", [1, 2, 257, 777, 4098])
@pytest.mark.parametrize("narrow", [False, True])
def test_reference_elementwise_operations_match_plain_numpy(n, narrow):
    x, y, z, r, p = (vec(n, s, narrow) for s in range(1, 6))
    a, b = 0.3 - 0.2j, -0.7 + 0.05j
    plain = {bn.ZERO: 0 * z, bn.COPY: x, bn.CAX: a * z, bn.CAXPY: z + a * x, bn.CXPY: z + x, bn.CAXPBYZ: a * x + b * y,
             bn.CAXY: a * x, bn.CXPAY: x + a * z, bn.CAXPBY: a * x + b * z, bn.CXPYZ: x + y}
    for op, ref in plain.items():
        want, S, terms = bn.blas(op, a, b, x, y, z)
        assert within(ref, want, bn.elementwise_bound(terms, S)), op
    # multi-axpy: a zero coefficient's vector is not read, whatever it holds
    xs = [vec(n, 10 + j, narrow) for j in range(5)]
    cf = np.array([0.1 - 0.3j, 0.0, 0.7 + 0.2j, 0.0, -0.4j])
    poisoned = [np.full(n, complex(np.nan, np.inf)) if c == 0 else v for c, v in zip(cf, xs)]
    want, S, terms, P = bn.multi_axpy(cf, poisoned, y, narrow)
    assert terms == 3 and not np.any(P) and np.all(np.isfinite(want.astype(np.complex128)))
    ref = y + sum(c * v for c, v in zip(cf, xs) if c != 0)
    assert within(ref, want, bn.elementwise_bound(terms, S))
    # the GCR update; narrow storage rounds w before it enters r
    wn, Sw, tw, Pw, rn, Sr, tr, slack = bn.gcr_update(cf, poisoned, z, a, r, narrow)
    assert within(ref - y + z, wn, bn.elementwise_bound(tw, Sw))
    w_stored = bn.r32(ref - y + z) if narrow else ref - y + z
    assert within(r + a * w_stored, rn, bn.elementwise_bound(tr, Sr, None, slack if narrow else None))
    # more than 8 vector sets in narrow storage: the partial result behind each pass of 8 is rounded to complex<float>, P is its magnitude
    many = [vec(n, 30 + j, narrow) for j in range(17)]
    cm = np.array([0.2 + 0.05 * j - 0.1j for j in range(17)])
    want, S, terms, P = bn.multi_axpy(cm, many, y, narrow)
    step = y
    for j0 in (0, 8, 16):
        step = step + sum(c * v for c, v in zip(cm[j0:j0 + 8], many[j0:j0 + 8]))
        if narrow and j0 < 16:
            step = bn.r32(step)
    assert terms == 17 and bool(np.any(P)) == narrow
    assert within(step, want, bn.elementwise_bound(terms, S, None, P if narrow else None))
    # multi-shift CG, one (system, shift) pair
    xn, Sx, tx, pn, Sp, tp = bn.cgm_update(0.31, -0.55, 0.42, x, p, r)
    assert within(x + 0.31 * p, xn, bn.elementwise_bound(tx, Sx)) and within(-0.55 * r + 0.42 * p, pn, bn.elementwise_bound(tp, Sp))
    # MR: alpha = omega <p,r> / <p,p>, both XSET forms, and the breakdown
    pr, pp, _, _ = bn.mr_dots(r, p)
    alpha = bn.mr_alpha(0.85, pr, pp)
    al = 0.85 * np.vdot(p, r) / np.vdot(p, p).real
    assert abs(complex(alpha) - al) <= 1e-14 * abs(al)
    for xset in (False, True):
        xn, Sx, tx, rn, Sr, tr = bn.mr_update(alpha, x, r, p, xset)
        assert within((0 if xset else x) + al * r, xn, bn.elementwise_bound(tx, Sx) + 1e-14 * np.abs(al * r))
        assert within(r - al * p, rn, bn.elementwise_bound(tr, Sr) + 1e-14 * np.abs(al * p))
    assert bn.mr_alpha(0.85, pr, bn.LD(0)) == 0
    x0, _, _, r0, _, _ = bn.mr_update(0, x, r, 0 * p, False)
    assert np.array_equal(x0.astype(np.complex128), x) and np.array_equal(r0.astype(np.complex128), r)


@pytest.mark.parametrize("n", [1, 2, 257, 777, 4098, 300001])
def test_reference_reductions_match_numpy_and_the_oracle(n):
    x, y = vec(n, 1), vec(n, 2)
    scale = float(np.sqrt(bn.norm2(x) * bn.norm2(y)))
    want, s = bn.reduce(bn.NORM2, x, None)
    assert abs(complex(want) - np.vdot(x, x)) <= bn.RTOL_RED * float(s) and abs(complex(want).real - ol.norm2sq(x)) <= bn.RTOL_RED * float(s)
    want, s = bn.reduce(bn.DOT, x, y)
    assert float(s) == pytest.approx(scale)
    assert abs(complex(want) - np.vdot(x, y)) <= bn.RTOL_RED * scale and abs(complex(want) - ol.dot(x, y)) <= bn.RTOL_RED * scale
    want, s = bn.reduce(bn.DIFFNORM2, x, y)
    assert abs(complex(want).real - np.linalg.norm(x - y) ** 2) <= bn.RTOL_RED * scale and abs(complex(want).real - ol.diffnorm2sq(x, y)) <= bn.RTOL_RED * scale
    xs = [vec(n, 10 + j) for j in range(3)]
    wants, scales = bn.multidot(xs, y)
    for j in range(3):
        assert abs(complex(wants[j]) - ol.dot(xs[j], y)) <= bn.RTOL_RED * float(scales[j])
    pr, pp, _, _ = bn.mr_dots(x, y)   # (r = x, p = y): <p,r>, <p,p>
    assert abs(complex(pr) - ol.dot(y, x)) <= bn.RTOL_RED * scale and abs(float(pp) - ol.norm2sq(y)) <= bn.RTOL_RED * float(bn.norm2(y))


# ---- 2. the table
def test_route_table_plans_are_what_the_library_answers():
    """every row's expected plan, asked here without a GPU"""
    for r in routes.ROUTES:
        with routes.tuned(r):
            assert routes.planned(r) == r["plans"], routes.route_id(r)


# ---- 3. coverage
ENTRIES = ("blas", "maxpy", "gcr", "cgm", "reduce", "multidot", "mr_dots", "mr_update")
BE = {"blas": qmg.BE_BLAS, "maxpy": qmg.BE_MULTI_CAXPY, "gcr": qmg.BE_GCR_UPDATE, "cgm": qmg.BE_CGM_UPDATE, "reduce": qmg.BE_REDUCE, "multidot": qmg.BE_MULTIDOT,
      "mr_dots": qmg.BE_MR_DOTS, "mr_update": qmg.BE_MR_UPDATE}
NT_MBS = (0, 1, 256)
NRHS = (1, 2, 16)
MAX_PASSES = 8


def domain_n(st):
    thr = routes.LONG_N[st]
    return (0, 1, 2, 777, 4096, thr - 2, thr, thr + 2)


def variants(entry, nrhs):
    """(op, nj, shift_masks, flags) of an entry point over the domain"""
    if entry == "blas":
        return [(op, 0, None, 0) for op in range(10)]
    if entry == "reduce":
        return [(op, 0, None, 0) for op in range(3)]
    if entry == "maxpy":
        return [(0, nj, None, 0) for nj in range(0, 34)]
    if entry == "gcr":
        return [(0, nj, None, zn) for nj in range(0, 34) for zn in (0, 1)]
    if entry == "multidot":
        return [(0, nj, None, 0) for nj in range(1, 33)]
    if entry == "cgm":   # per-system counts 0 .. cap of every launch (cap = 0: nothing iterates), and every pair iterating
        return [(0, ns, tuple(sm), 0) for ns in range(1, 17) for sm in [routes.stair(ns, nrhs, cap) for cap in range(0, 9)] + [[0xFFFF] * ns]]
    if entry == "mr_dots":
        return [(0, 0, None, 0)]
    return [(0, 0, None, f) for f in range(4)]


# why a pass launches nothing: (reason, predicate of (entry, n, mask, nj, shifts of the pass or None))
NOTHING_BECAUSE = [
    ("no active system", lambda e, n, mask, nj, sm: mask == 0),
    ("n = 0 in an elementwise entry point", lambda e, n, mask, nj, sm: n == 0 and e in ("blas", "maxpy", "gcr", "cgm", "mr_update")),
    ("no vector set in a multi-axpy", lambda e, n, mask, nj, sm: e == "maxpy" and nj == 0),
    ("a multi-shift launch none of whose shifts is iterated by an active system", lambda e, n, mask, nj, sm: e == "cgm" and all((mask & m) == 0 for m in sm)),
]


def test_every_pass_in_the_domain_has_a_row():
    expected = {(r["st"], p) for r in routes.ROUTES for p in r["plans"] if p != routes.NOTHING}
    L = qmg.lib()
    out = (C.c_int * (qmg.BATCH_PLAN_INTS * MAX_PASSES))()
    found, unlisted, listed_but_launched, asked = {}, [], [], 0
    try:
        for mb in NT_MBS:
            qmg.set_tuning("blas_nt_mb", mb)
            for entry, st, al, nrhs in itertools.product(ENTRIES, (C64, C32), (1, 0), NRHS):
                for op, nj, sm, flags in variants(entry, nrhs):
                    smp = (C.c_uint * len(sm))(*sm) if sm is not None else None
                    for n, pad, nact in itertools.product(domain_n(st), (0, 1), range(0, nrhs + 1)):
                        mask = (1 << nact) - 1
                        assert L.qmg_batch_plan(BE[entry], routes.DTYPE[st], op, C.c_size_t(n), C.c_size_t(n + pad), nrhs, C.c_uint(mask), nj, smp, flags, al, out,
                                                MAX_PASSES) == 0, (entry, st, n, nrhs, nj)
                        asked += 1
                        passes = [tuple(out[5 * i:5 * i + 5]) for i in range(MAX_PASSES) if out[5 * i] >= 0]
                        for i, p in enumerate(passes):
                            launch = sm[8 * i:8 * i + 8] if entry == "cgm" else None
                            listed = any(pred(entry, n, mask, nj, launch) for _, pred in NOTHING_BECAUSE)
                            if p == routes.NOTHING:
                                if not listed:
                                    unlisted.append((entry, st, n, nrhs, mask, nj, sm))
                            else:
                                assert p[0] != qmg.BF_NOTHING
                                if listed:
                                    listed_but_launched.append((entry, st, n, nrhs, mask, nj, sm))
                                found.setdefault((st, p), (entry, n, pad, nrhs, mask, nj, sm, flags, al, mb))
    finally:
        qmg.set_tuning("blas_nt_mb", routes.NT_DEFAULT)
    per_entry = {"blas": 10, "reduce": 3, "maxpy": 34, "gcr": 68, "multidot": 32, "cgm": 160, "mr_dots": 1, "mr_update": 4}
    assert asked == 3 * 2 * 2 * sum(per_entry.values()) * 8 * 2 * sum(k + 1 for k in NRHS)          # no case skipped
    assert not unlisted, unlisted[:5]
    assert not listed_but_launched, listed_but_launched[:5]
    left_out = {k: v for k, v in found.items() if k not in expected}
    assert not left_out, "passes without a row in test_gpu_batch_routes.ROUTES (pass: first request that gave it): %r" % left_out


# ---- 4. the threshold
@pytest.mark.parametrize("st", [C64, C32])
def test_long_vector_forms_begin_at_the_named_constant(st):
    dt, thr, W = routes.DTYPE[st], routes.LONG_N[st], 2 if st == C32 else 1
    assert thr * (8 if st == C32 else 16) == qmg.BATCH_LONG_BYTES
    one = lambda n, nj: qmg.batch_plan(qmg.BE_MULTI_CAXPY, dt, n, n, 1, 1, nj=nj)
    two = lambda n, nj: qmg.batch_plan(qmg.BE_MULTI_CAXPY, dt, n, n, 2, 0b11, nj=nj)
    W1 = 1   # thr - 1 is odd
    assert two(thr - 1, 11) == [routes.SMALL(W1, 0, 8), routes.SMALL(W1, 0, 3)]
    assert two(thr, 11) == [routes.LONG(W, 0, 8), routes.LONG(W, 0, 3)]
    assert one(thr - 1, 11) == [routes.SMALL(W1, 0, 8), routes.SMALL(W1, 0, 3)]
    assert one(thr, 11) == ([routes.SINGLE(0)] if st == C64 else [routes.LONG(W, 0, 8), routes.LONG(W, 0, 3)])
    # the GCR update: all but the last chunk through the multi-axpy below the threshold, every chunk from it on
    gcr = lambda n, nrhs: qmg.batch_plan(qmg.BE_GCR_UPDATE, dt, n, n, nrhs, (1 << nrhs) - 1, nj=11, flags=qmg.BPV_ZNEXT)
    assert gcr(thr - 1, 2) == [routes.SMALL(W1, 0, 8), routes.GCR(W1, 0, 3, 1)]
    assert gcr(thr, 2) == [routes.LONG(W, 0, 8), routes.LONG(W, 0, 3), routes.GCR(W, 0, 0, 1)]
    assert gcr(thr, 1) == ([routes.SINGLE(0)] if st == C64 else [routes.LONG(W, 0, 8), routes.LONG(W, 0, 3)]) + [routes.GCR(W, 0, 0, 1)]
    # no other entry point looks at the threshold
    for n in (thr - 2, thr, thr + 2):
        assert qmg.batch_plan(qmg.BE_BLAS, dt, n, n, 2, 0b11, op=bn.CAXPY) == [routes.BLAS(W, 0, bn.CAXPY)]
        assert qmg.batch_plan(qmg.BE_CGM_UPDATE, dt, n, n, 2, 0b11, nj=2, shift_masks=[3, 1]) == [routes.CGM(W, 0, 2, 2)]


def test_plan_query_rejects_what_the_entry_points_reject():
    out = (C.c_int * 40)()
    L = qmg.lib()
    invalid = 1
    ask = lambda entry, dtype, op, n, nrhs, mask, nj, sm, flags, max_passes=8: L.qmg_batch_plan(entry, dtype, op, C.c_size_t(n), C.c_size_t(n), nrhs, C.c_uint(mask), nj, sm, flags,
                                                                                                  1, out, max_passes)
    assert ask(8, 0, 0, 8, 1, 1, 0, None, 0) == invalid                       # entry
    assert ask(qmg.BE_BLAS, 2, 0, 8, 1, 1, 0, None, 0) == invalid             # dtype
    assert ask(qmg.BE_BLAS, 0, 10, 8, 1, 1, 0, None, 0) == invalid            # op
    assert ask(qmg.BE_REDUCE, 0, 3, 8, 1, 1, 0, None, 0) == invalid
    assert ask(qmg.BE_BLAS, 0, 0, 8, 17, 1, 0, None, 0) == invalid            # more than 16 systems
    assert ask(qmg.BE_MULTIDOT, 0, 0, 8, 1, 1, 33, None, 0) == invalid        # more than 32 dots
    assert ask(qmg.BE_MULTIDOT, 0, 0, 8, 1, 1, 0, None, 0) == invalid
    assert ask(qmg.BE_CGM_UPDATE, 0, 0, 8, 1, 1, 2, None, 0) == invalid       # no shift masks
    assert ask(qmg.BE_CGM_UPDATE, 0, 0, 8, 1, 1, 17, (C.c_uint * 17)(), 0) == invalid
    assert ask(qmg.BE_MR_UPDATE, 0, 0, 8, 1, 1, 0, None, 4) == invalid        # flags
    assert ask(qmg.BE_MULTI_CAXPY, 0, 0, 8, 1, 1, 9, None, 0, max_passes=1) == invalid   # two passes do not fit
    assert ask(qmg.BE_MULTI_CAXPY, 0, 0, 8, 1, 1, 9, None, 0, max_passes=2) == 0
    assert list(out[:10]) == list(routes.SMALL(1, 0, 8)) + list(routes.SMALL(1, 0, 1))
