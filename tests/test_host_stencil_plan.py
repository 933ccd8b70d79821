"""CPU-side checks behind tests/test_gpu_stencil_routes.py (no GPU: qmg_stencil_plan is host code and makes no HIP call).

1. The reference of the route tests is validated before any GPU run: the oracle's stencil apply against stencil_numpy on the fp64 requests
   of the route table, with the elementwise bound the kernels are held to, every single piece bit, and two identities of the reference with
   itself (the pieces add up to the full apply; <y, M x> = <M^dagger y, x> with M^dagger built on the grid).
2. Coverage: qmg_stencil_plan is enumerated over a finite domain of requests (REQUEST BLOCKS below), and every distinct non-slab
   instantiation found there must be the expected plan of at least one row of the route table; every refused request must match the explicit
   list of refusals.  A retune that creates a plan no row runs fails here until a row is added (a new route needs a row).
"""
import importlib
import itertools

import numpy as np
import pytest

import coordspace as cs
import oracle_lib as ol
import stencil_numpy as sn
import test_gpu_stencil_routes as routes

qmg = importlib.import_module("quantum-mg_amd")


@pytest.fixture(scope="module", autouse=True)
def _built():
    qmg.build()
    yield
    routes.set_knobs({})


# ---- 1. the reference
SHIFTS = (0.3 - 0.1j, -0.2 + 0.05j, 0.15 - 0.25j)
FP64_REQUESTS = sorted({(row[2], routes.PIECES[row[5]], "noclover" in row[6], "nohopping" in row[6]) for row in routes.ROUTES
                        if row[1] == "c64" and row[2][0] * row[2][1] <= 4096 and routes.expected_family(row) not in (qmg.SF_INVALID, qmg.SF_UNSUPPORTED)})
SINGLE_BITS = [1 << b for b in range(14)]


def fields(dims, noclover=False, nohopping=False):
    Lx, Ly, nc = dims
    vol = Lx * Ly * nc * nc
    return (None if noclover else cs.gaussian_cvec(vol, 1)), (None if nohopping else cs.gaussian_cvec(4 * vol, 2))


def oracle_against_reference(dims, pieces, noclover, nohopping):
    Lx, Ly, nc = dims
    clover, hopping = fields(dims, noclover, nohopping)
    shifts = SHIFTS if nc % 2 == 0 else SHIFTS[:2] + (0.0,)
    rhs, lhs0 = cs.gaussian_cvec(Lx * Ly * nc, 3), cs.gaussian_cvec(Lx * Ly * nc, 4)
    got = ol.stencil_apply(ol.make_desc(Lx, Ly, nc, clover, hopping, *shifts), rhs, pieces, lhs=lhs0.copy())
    want, S, n = sn.apply(Lx, Ly, nc, clover, hopping, *shifts, pieces, rhs, lhs0)
    err = np.abs(got.astype(sn.CLD) - want)
    bound = sn.elementwise_bound(S, n)
    assert np.all(err <= bound), float(np.max(err / np.where(bound > 0, bound, 1)))
    assert float(np.linalg.norm(err)) <= routes.TOL64 * float(np.linalg.norm(want))
    # a parity no piece touches, and every element no term reaches without a ZERO bit: lhs0, bit for bit
    assert np.array_equal(got[np.asarray(n == 0) & (np.asarray(want) == lhs0)], lhs0[np.asarray(n == 0) & (np.asarray(want) == lhs0)])


@pytest.mark.parametrize("dims,pieces,noclover,nohopping", FP64_REQUESTS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_oracle_matches_numpy_reference(dims, pieces, noclover, nohopping):
    """ol.stencil_apply (accumulating into a non-zero lhs, all three shifts set) against the long-double coordinate-grid reference, elementwise"""
    oracle_against_reference(dims, pieces, noclover, nohopping)


@pytest.mark.parametrize("dims", [(6, 4, 3), (2, 2, 2), (4, 2, 1), (2, 6, 4), (1, 1, 4), (1, 1, 3)], ids=lambda d: "x".join(map(str, d)))
def test_oracle_matches_numpy_reference_on_every_single_piece(dims):
    """one bit at a time (each direction of each parity, each clover, shift and zero bit), on the wraps Lx = 2 / Ly = 2 and the 1 x 1 corner"""
    for bit in SINGLE_BITS:
        oracle_against_reference(dims, bit, False, False)
        oracle_against_reference(dims, bit | qmg.P_ZERO, False, False)


def test_numpy_reference_pieces_add_up_to_the_full_apply():
    """apply(P_ALL) from zero = sum over the twelve single pieces from zero: the same set of terms (n adds up exactly, the values to long-double
    rounding of the different order)"""
    Lx, Ly, nc = 6, 4, 4
    clover, hopping = fields((Lx, Ly, nc))
    rhs, zero = cs.gaussian_cvec(Lx * Ly * nc, 3), np.zeros(Lx * Ly * nc)
    full, S, n = sn.apply(Lx, Ly, nc, clover, hopping, *SHIFTS, qmg.P_ALL, rhs, zero)
    parts = [sn.apply(Lx, Ly, nc, clover, hopping, *SHIFTS, 1 << b, rhs, zero) for b in range(12)]
    assert np.array_equal(sum(p[2] for p in parts), n)
    assert np.all(np.abs(sum(p[0] for p in parts) - full) <= 2.0 ** -60 * S)
    assert np.all(np.abs(sum(p[1] for p in parts) - S) <= 2.0 ** -60 * S)


def test_numpy_reference_adjoint_identity():
    """<y, M x> = <M^dagger y, x>, M^dagger from stencil_numpy.dagger_fields (C(x)^H; H_{-mu}(x + mu)^H): a wrong direction, parity or roll in
    either statement breaks it"""
    for Lx, Ly, nc in ((6, 4, 3), (2, 4, 2), (4, 2, 2)):
        clover, hopping = fields((Lx, Ly, nc))
        dcl, dhop = sn.dagger_fields(Lx, Ly, nc, clover, hopping)
        x, y, zero = cs.gaussian_cvec(Lx * Ly * nc, 3), cs.gaussian_cvec(Lx * Ly * nc, 4), np.zeros(Lx * Ly * nc)
        pieces = qmg.P_CLOVER | qmg.P_HOPPING
        Mx, S, _ = sn.apply(Lx, Ly, nc, clover, hopping, 0, 0, 0, pieces, x, zero)
        Mdy, _, _ = sn.apply(Lx, Ly, nc, dcl, dhop, 0, 0, 0, pieces, y, zero)
        lhs, rhs = np.vdot(y.astype(sn.CLD), Mx), np.vdot(Mdy, x.astype(sn.CLD))
        assert abs(lhs - rhs) <= 2.0 ** -58 * float(np.sum(np.abs(y) * S))


# ---- 2. the plan
def test_route_table_plans_are_what_the_library_answers():
    """every row's expected plan, asked here without a GPU"""
    for row in routes.ROUTES:
        try:
            routes.set_knobs(row[7])
            assert [routes.instantiation(p) for p in routes.planned(row)] == row[8], routes.route_id(row)
        finally:
            routes.set_knobs({})


def test_tall_rows_walk_rows_beyond_the_grid():
    for row in routes.ROUTES:
        if "tall" in row[6]:
            try:
                routes.set_knobs(row[7])
                assert all(p[10] == 65535 for p in routes.planned(row)), routes.route_id(row)
            finally:
                routes.set_knobs({})


# ---- the coverage domain
NCS = (1, 2, 3, 4, 6, 7, 8, 12, 16, 24, 32, 48)
HRS = (1, 2, 3, 5, 6, 8, 17, 260)
LY = 4
STORAGES = ("c64", "c32", "m32", "m16", "m16v32")
SYSTEMS = [(n, h) for n in range(1, 17) for h in (False, True)] + [(n, False) for n in (17, 18, 19)]
# operator forms: (pieces, flags) spanning the site kernel's shapes (1: clover + four hops, 2: four hops, 0: anything else), zero / accumulate,
# one / both parities, a missing field, and no work at all
FORMS = [("M0", ""), ("M+", ""), ("EO0", ""), ("HOP0", ""), ("M0", "noclover"), ("M0", "nohopping"), ("DIAG0", ""), ("XPYM+", ""), ("MIX0", ""), ("NONE", ""),
         ("HOP+", "")]
KNOBS = [{}, {"stencil_site": 7}, {"stencil_site": 0}, {"stencil_pair": 0}, {"stencil_mfma": 2}, {"stencil_mfma": 0}, {"pair_prefetch": 0}]


def request_blocks():
    """(knobs, iterator of (entry, storage, (Lx, Ly, nc), n_active, holes, pieces name, flags)) -- the finite domain, block by block"""
    grid = [(2 * hr, LY, nc) for nc in NCS for hr in HRS]
    for knobs in KNOBS:
        # plain applies: every form at the default knobs and at stencil_site = 7 (kernel S in fp64: every shape, zero and accumulate, one system
        # and batch), the first four under each other knob setting
        forms = FORMS if not knobs or knobs == {"stencil_site": 7} else FORMS[:4]
        yield knobs, (("masked" if (st != "c64" or h or n <= 16) else "apply", st, d, n, h, pc, fl)
                      for d, st, (n, h), (pc, fl) in itertools.product(grid, STORAGES, SYSTEMS, forms))
    # lhs == rhs: one parity from hops alone, and (refused nowhere, but another route) both parities
    yield {}, (("masked", st, d, n, h, pc, "inplace") for d, st, (n, h), pc in itertools.product(grid, STORAGES, SYSTEMS[:32], ("EO0", "OE+", "HOP0")))
    yield {"stencil_pair": 0}, (("masked", "c64", d, n, h, pc, "inplace") for d, (n, h), pc in itertools.product(grid, SYSTEMS[:32], ("EO0", "OE+")))
    # the fused norm
    for knobs in ({}, {"pair_prefetch": 0}):
        yield knobs, (("norm2", "c64", d, n, False, pc, fl) for d, n, (pc, fl) in itertools.product(grid, range(1, 17), FORMS[:6]))
    yield {}, (("norm2", "c64", d, 2, False, "M0", "inplace") for d in grid)
    # the epilogue, with and without the dots, on system 0 and on another
    yield {}, (("epi", st, d, 1, h, pc, fl) for d, st, h, pc, fl in itertools.product(grid, STORAGES, (False, True), ("M0", "EO0", "M+"), ("", "dots")))
    # the 16-bit site entry
    yield {}, (("h16", "h16", d, n, h, pc, fl) for d, (n, h), (pc, fl) in itertools.product(grid, SYSTEMS, FORMS))
    # the 1 x 1 lattice
    yield {}, (("masked", st, (1, 1, nc), n, h, pc, "") for nc, st, (n, h), pc in itertools.product(NCS, ("c64", "c32"), SYSTEMS[:32], ("M0", "M+", "HOP0", "HOP+", "NONE")))
    # slabs (their plans need no row: test_gpu_slab.py holds them bit-for-bit to the single-domain kernels)
    yield {}, (("slab%d" % rows, st, d, n, False, pc, "") for d, st, n, pc, rows in itertools.product(grid, STORAGES + ("h16",), (1, 3, 5, 16), ("M0", "EO0"), (0, 1, 2)))


N_REQUESTS = (12 * 8 * 5 * 35 * (11 + 11 + 5 * 4) + 12 * 8 * 5 * 32 * 3 + 12 * 8 * 32 * 2 + 2 * 12 * 8 * 16 * 6 + 12 * 8 + 12 * 8 * 5 * 2 * 3 * 2
              + 12 * 8 * 35 * 11 + 12 * 2 * 32 * 5 + 12 * 8 * 6 * 4 * 2 * 3)

FINE = (1, 2, 4)
# the requests the library refuses, as predicates of (entry, storage, (Lx, Ly, nc), n, holes, pieces name, flags) with their reasons
REFUSALS = [
    ("more than 16 systems behind a mask", lambda e, st, d, n, h, pc, fl: e in ("masked", "h16") and n > 16),
    ("complex<float> matrices under complex<double> vectors: the Galerkin levels only", lambda e, st, d, n, h, pc, fl: st == "m32" and d[2] in FINE),
    ("complex<half> matrices: nc a multiple of 4 above 4 (kernels B32 / C)", lambda e, st, d, n, h, pc, fl: st in ("m16", "m16v32") and (d[2] % 4 or d[2] == 4) and d[0] > 1
     and not (e.startswith("slab") and st == "m16v32" and d[2] == 2)),   # (a slab at nc = 2 with these two is kernel S's 16-bit form)
    ("complex<half> matrices on a slab at nc = 2 come with complex<float> vectors (its own 16-bit form)", lambda e, st, d, n, h, pc, fl: e.startswith("slab") and st == "m16" and d[2] == 2),
    ("complex<float> matrices under complex<double> vectors on a slab at nc = 2", lambda e, st, d, n, h, pc, fl: e.startswith("slab") and st == "m32" and d[2] == 2),
    ("the 16-bit site entry: nc = 2", lambda e, st, d, n, h, pc, fl: e == "h16" and d[2] != 2),
    ("16-bit site storage on a slab: nc = 2 or the Galerkin levels", lambda e, st, d, n, h, pc, fl: e.startswith("slab") and st == "h16" and d[2] != 2 and (d[2] % 4 or d[2] == 4)),
    ("narrow matrices under fp64 vectors on a slab: the Galerkin levels, nc > 4", lambda e, st, d, n, h, pc, fl: e.startswith("slab") and st == "m32" and d[2] <= 4),
    ("slabs of a generic nc: all rows in one launch", lambda e, st, d, n, h, pc, fl: e in ("slab1", "slab2") and d[2] != 2),
    ("the fused norm: kernel A2, nc = 1 or 2", lambda e, st, d, n, h, pc, fl: e == "norm2" and d[2] not in (1, 2)),
    ("the fused norm: every site written", lambda e, st, d, n, h, pc, fl: e == "norm2" and pc in ("EO0", "NONE")),
    ("the fused norm: lhs != rhs", lambda e, st, d, n, h, pc, fl: e == "norm2" and "inplace" in fl),
    ("the epilogue: kernels B / B32, not nc = 1, 2, 4", lambda e, st, d, n, h, pc, fl: e == "epi" and d[2] in FINE),
    ("the epilogue: the processed parities are overwritten", lambda e, st, d, n, h, pc, fl: e == "epi" and pc == "M+"),
]


def test_every_plan_in_the_domain_has_a_row():
    expected = {routes.kernel_of(p) for row in routes.ROUTES for p in row[8]}
    found, refused_unlisted, listed_not_refused, asked = {}, [], [], 0
    try:
        for knobs, block in request_blocks():
            routes.set_knobs(knobs)
            for req in block:
                entry, st, d, n, h, pc, fl = req
                asked += 1
                listed = any(pred(*req) for _, pred in REFUSALS)
                try:
                    plans = routes.plan_of(entry, st, d, n, h, pc, fl)
                except qmg.QmgError:
                    plans = [(qmg.SF_INVALID,) + (0,) * 11]
                for p in plans:
                    if p[0] in (qmg.SF_UNSUPPORTED, qmg.SF_INVALID):
                        if not listed:
                            refused_unlisted.append((req, knobs))
                    else:
                        if listed:
                            listed_not_refused.append((req, knobs))
                        if not entry.startswith("slab"):
                            found.setdefault(routes.kernel_of(routes.instantiation(p)), (req, knobs))
    finally:
        routes.set_knobs({})
    assert asked == N_REQUESTS          # no case skipped
    assert not refused_unlisted, refused_unlisted[:5]
    assert not listed_not_refused, listed_not_refused[:5]
    left_out = {k: v for k, v in found.items() if k not in expected}
    assert not left_out, "plans without a row in test_gpu_stencil_routes.ROUTES (plan: first request that gave it): %r" % left_out


def test_plan_query_rejects_what_the_entry_points_reject():
    import ctypes as C
    out = (C.c_int * 24)()
    L = qmg.lib()
    ask = lambda *a: L.qmg_stencil_plan(*a, out, 24)
    invalid, M0 = 1, qmg.P_ALL | qmg.P_ZERO
    #          entry          mat v32 Lx Ly nc pieces n holes inplace clover hopping epi rows
    assert ask(qmg.SE_APPLY, 0, 1, 8, 8, 3, M0, 1, 0, 0, 1, 1, 0, 0) == invalid        # complex<float> vectors with complex<double> matrices
    assert ask(qmg.SE_APPLY, 1, 1, 8, 8, 3, M0, 1, 0, 0, 1, 1, 0, 0) == invalid        # qmg_stencil_apply is fp64
    assert ask(qmg.SE_MASKED, 0, 0, 8, 8, 3, M0, 17, 0, 0, 1, 1, 0, 0) == invalid      # more than 16 systems behind a mask
    assert ask(qmg.SE_H16, 2, 0, 8, 8, 2, M0, 1, 0, 0, 1, 1, 0, 0) == invalid          # the 16-bit entry has complex<float> vectors
    assert ask(qmg.SE_NORM2, 0, 0, 8, 8, 2, M0, 17, 0, 0, 1, 1, 0, 0) == invalid
    assert ask(qmg.SE_EPI, 0, 0, 8, 8, 3, M0, 2, 0, 0, 1, 1, 1, 0) == invalid          # the epilogue serves one system
    assert ask(qmg.SE_EPI, 0, 0, 8, 8, 3, M0, 1, 0, 0, 1, 1, 0, 0) == invalid          # ... and needs one
    assert ask(qmg.SE_MASKED, 0, 0, 8, 8, 3, M0, 1, 0, 0, 1, 1, 1, 0) == invalid
    assert ask(qmg.SE_SLAB, 0, 0, 8, 8, 3, M0, 1, 0, 0, 1, 1, 0, 3) == invalid         # rows
    assert ask(qmg.SE_SLAB, 0, 0, 8, 8, 3, M0, 1, 0, 1, 1, 1, 0, 0) == invalid         # a slab in place: one parity from hops alone
    assert L.qmg_stencil_plan(qmg.SE_APPLY, 0, 0, 8, 8, 8, M0, 19, 0, 0, 1, 1, 0, 0, out, 12) == invalid   # two passes do not fit
    for dims, status in (((7, 8, 3), qmg.SF_INVALID), ((8, 0, 3), qmg.SF_INVALID), ((8, 8, 0), qmg.SF_INVALID)):          # odd / empty extents, no colour
        assert ask(qmg.SE_APPLY, 0, 0, *dims, M0, 1, 0, 0, 1, 1, 0, 0) == 0 and out[0] == status
    assert ask(qmg.SE_EPI, 0, 0, 8, 8, 3, qmg.P_ALL, 1, 0, 0, 1, 1, 1, 0) == 0 and out[0] == qmg.SF_INVALID   # accumulate + epilogue
    assert ask(qmg.SE_EPI, 0, 0, 8, 8, 3, M0, 1, 0, 1, 1, 1, 1, 0) == 0 and out[0] == qmg.SF_INVALID          # lhs == rhs
    assert ask(qmg.SE_MASKED, 1, 1, 8, 8, 300, M0, 1, 0, 0, 1, 1, 0, 0) == 0 and out[0] == qmg.SF_UNSUPPORTED  # nc beyond a block
    assert ask(qmg.SE_MASKED, 1, 0, 8, 8, 56, M0, 1, 0, 0, 1, 1, 0, 0) == 0 and out[0] == qmg.SF_UNSUPPORTED   # declined by B32 (7 pairs per thread), beyond B's registers
    assert ask(qmg.SE_APPLY, 0, 0, 8, 8, 8, M0, 19, 0, 0, 1, 1, 0, 0) == 0
    assert [routes.instantiation(tuple(out[12 * p:12 * p + 12])) for p in (0, 1)] == [routes.C(0, 8, 2, 16), routes.C(0, 8, 1, 3, pair=True)]
