"""CPU-side checks behind tests/test_gpu_transfer_routes.py (no GPU: qmg_transfer_plan is host code and makes no HIP call).

1. The reference of the route tests is validated before any GPU run: the oracle's restrict / prolong against transfer_numpy on the
   fp64 rows of the route table, with the elementwise bound the kernels are held to.
2. Coverage: qmg_transfer_plan is enumerated over a finite domain of requests, and every distinct plan found there must be the
   expected plan of at least one row of the route table; every refused request must match the explicit list of refusals.  A retune
   that creates a plan no row runs fails here until a row is added (a new route needs a row).
"""
import importlib
import itertools

import numpy as np
import pytest

import coordspace as cs
import oracle_lib as ol
import test_gpu_transfer_routes as routes
import transfer_numpy as tn

qmg = importlib.import_module("quantum-mg_amd")

R, P = routes.R, routes.P


@pytest.fixture(scope="module", autouse=True)
def _built():
    qmg.build()


FP64_SHAPES = sorted({(row[0], row[2], row[3]) for row in routes.ROUTES if row[1] == "c64"})


@pytest.mark.parametrize("op,fd,cd", FP64_SHAPES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_oracle_matches_numpy_reference(op, fd, cd):
    """ol.restrict / ol.prolong (accumulating into non-zero vectors) against the long-double coordinate-grid reference, elementwise."""
    fsize, csize = fd[0] * fd[1] * fd[2], cd[0] * cd[1] * cd[2]
    nv, fine, coarse = cs.gaussian_cvec(cd[2] * fsize, 1), cs.gaussian_cvec(fsize, 2), cs.gaussian_cvec(csize, 3)
    if op == R:
        got = ol.restrict(nv, fine, fd, cd, coarse=coarse.copy())
        want, S = tn.restrict(nv, fine, fd, cd, coarse)
    else:
        got = ol.prolong(nv, coarse, fd, cd, fine=fine.copy())
        want, S = tn.prolong(nv, coarse, fd, cd, fine)
    err = np.abs(got.astype(tn.CLD) - want)
    assert np.all(err <= tn.elementwise_bound(op, fd, cd, S)), float(np.max(err / tn.elementwise_bound(op, fd, cd, S)))
    assert float(np.linalg.norm(err) / np.linalg.norm(want)) < routes.TOL64


def test_numpy_reference_restrict_is_the_adjoint_of_prolong():
    """<R f, c> = <f, P c> with both forms started from zero: the two einsums state one operator."""
    fd, cd = (12, 8, 3), (4, 2, 5)
    fsize, csize = 12 * 8 * 3, 4 * 2 * 5
    nv, f, c = cs.gaussian_cvec(5 * fsize, 1), cs.gaussian_cvec(fsize, 2), cs.gaussian_cvec(csize, 3)
    Rf, _ = tn.restrict(nv, f, fd, cd, np.zeros(csize))
    Pc, _ = tn.prolong(nv, c, fd, cd, np.zeros(fsize))
    assert abs(np.vdot(Rf, c.astype(tn.CLD)) - np.vdot(f.astype(tn.CLD), Pc)) < 1e-15 * fsize


def test_route_table_plans_are_what_the_library_answers():
    """every row's expected plan, asked here without a GPU"""
    for row in routes.ROUTES:
        assert routes.planned(row) == row[6], routes.route_id(row)


# ---- the coverage domain
OPS = (R, P)
STORAGES = ("c64", "c32", "nv32")
N_ACTIVE = range(1, 17)
NVECS = (2, 4, 6, 8, 12, 13, 14, 16, 20, 24, 32, 40)
FNCS = (1, 2, 3, 8, 24)
BLOCKS = ((2, 1), (2, 2), (4, 4), (4, 2), (2, 4), (8, 8), (3, 4))
CLXS = (2, 4, 6)
CLY = 2
ALIGNED = (True, False)

# the requests the library refuses (all of them on the nv32 entry points), as predicates of (op, storage, fnc, bx, aligned)
REFUSALS = [
    ("complex<float> null vectors under complex<double> vectors: odd fnc", lambda op, st, fnc, bx, al: st == "nv32" and fnc % 2 == 1),
    ("... null vectors not 16-byte aligned", lambda op, st, fnc, bx, al: st == "nv32" and not al),
    ("... restrict with an odd block width", lambda op, st, fnc, bx, al: st == "nv32" and op == R and bx % 2 == 1),
]


def test_every_plan_in_the_domain_has_a_row():
    expected = {(row[0], row[1], plan) for row in routes.ROUTES for plan in row[6] if plan != routes.REFUSED}
    found, refused_unlisted, listed_not_refused, asked = {}, [], [], 0
    for op, st, n, nvec, fnc, (bx, by), cLx, al in itertools.product(OPS, STORAGES, N_ACTIVE, NVECS, FNCS, BLOCKS, CLXS, ALIGNED):
        fd, cd = (bx * cLx, by * CLY, fnc), (cLx, CLY, nvec)
        plans = qmg.transfer_plan(qmg.XFER_RESTRICT if op == R else qmg.XFER_PROLONG, qmg.C32 if st == "c32" else qmg.C64, st == "nv32", nvec, fd, cd, n, al)
        asked += 1
        assert len(plans) in (1, 2)
        listed = any(pred(op, st, fnc, bx, al) for _, pred in REFUSALS)
        for plan in plans:
            if plan == routes.REFUSED:
                if not listed:
                    refused_unlisted.append((op, st, fd, cd, n, al))
            else:
                assert plan[0] != qmg.XF_UNSUPPORTED
                if listed:
                    listed_not_refused.append((op, st, fd, cd, n, al))
                found.setdefault((op, st, plan), (fd, cd, n, al))
    assert asked == 2 * 3 * 16 * 12 * 5 * 7 * 3 * 2          # no case skipped
    assert not refused_unlisted, refused_unlisted[:5]
    assert not listed_not_refused, listed_not_refused[:5]
    left_out = {k: v for k, v in found.items() if k not in expected}
    assert not left_out, "plans without a row in test_gpu_transfer_routes.ROUTES (plan: first request that gave it): %r" % left_out


def test_plan_query_rejects_what_the_entry_points_reject():
    import ctypes as C
    out = (C.c_int * 16)()
    L = qmg.lib()
    invalid = 1
    assert L.qmg_transfer_plan(2, 0, 0, 8, 8, 8, 2, 2, 2, 8, 1, 1, out, 16) == invalid      # op
    assert L.qmg_transfer_plan(0, 1, 1, 8, 8, 8, 2, 2, 2, 8, 1, 1, out, 16) == invalid      # nv32 with complex<float> vectors
    assert L.qmg_transfer_plan(0, 0, 0, 8, 8, 8, 2, 3, 2, 8, 1, 1, out, 16) == invalid      # 8 is no multiple of 3
    assert L.qmg_transfer_plan(0, 0, 0, 9, 8, 8, 2, 2, 2, 8, 1, 1, out, 16) == invalid      # nvec > cnc
    assert L.qmg_transfer_plan(0, 0, 0, 8, 8, 8, 2, 2, 2, 8, 17, 1, out, 16) == invalid     # more than 16 systems
    assert L.qmg_transfer_plan(0, 0, 0, 8, 8, 8, 2, 2, 2, 8, 9, 1, out, 8) == invalid       # two passes do not fit
    assert L.qmg_transfer_plan(0, 0, 0, 8, 8, 8, 2, 2, 2, 8, 9, 1, out, 16) == 0
    assert list(out) == list(routes.SMALL(8, 8)) + list(routes.SMALL(2, 8))
