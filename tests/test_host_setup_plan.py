"""CPU-side checks behind tests/test_gpu_setup_routes.py (no GPU: qmg_setup_plan is host code and makes no HIP call).

a. The reference of the GPU rows, setup_numpy, is held to the oracle (1e-12) function by function before any GPU run: a failing GPU row then
   has a known side.
b. Every row of test_gpu_setup_routes.ROUTES gets from qmg_setup_plan the plan the row states.
c. Coverage: qmg_setup_plan is enumerated over fnc x block shape x nvec / cnc x coarse extents x "setup_fused" (and the rows' own requests, which
   add the two grid-stride shapes and the LDS-overflow shape); every distinct (family, TPB, groups, opt-in, idle group, outputs per thread,
   strided) found must be the expectation of a row, and the launch geometry of every served request covers its blocks within the LDS of a
   workgroup.
d. Refusals and the plan_out / plan_len contract, as in tests/test_host_dwf.py.
e. The conditions the GPU rows' tolerances rest on, asserted on the reference alone: condition number <= 50 of every orthonormalisation tile
   and of every matrix to invert, a row exchange at every elimination step but the last for the Jacobi inputs, and the Galerkin term counts
   in closed form.
"""
import ctypes as C
import importlib
import itertools

import numpy as np
import pytest

import coordspace as cs
import oracle_lib as ol
import setup_numpy as su
import test_gpu_setup_routes as routes

qmg = importlib.import_module("quantum-mg_amd")

ORACLE_TOL = 1e-12


@pytest.fixture(scope="module", autouse=True)
def _built():
    qmg.build()
    ol.build()
    yield
    qmg.set_tuning("setup_fused", 1)


def rel(a, b):
    return cs.rel_l2(np.asarray(a).astype(np.complex128), np.asarray(b).astype(np.complex128))


# ---- a. the reference against the oracle
SMALL = [((8, 8, 2), (4, 2, 4)), ((12, 8, 3), (4, 2, 5)), ((4, 12, 1), (2, 2, 2))]   # blocks 2 x 4, 3 x 4 (odd), 2 x 6; cLx = 2, cLy = 2
IDS = ["-".join("x".join(map(str, d)) for d in s) for s in SMALL]


@pytest.mark.parametrize("fdims,cdims", SMALL, ids=IDS)
def test_block_qr_is_the_oracles_block_orthonormalize(fdims, cdims):
    nvec, fsize = cdims[2], fdims[0] * fdims[1] * fdims[2]
    nv = cs.gaussian_cvec(nvec * fsize, 3)
    chol = np.zeros(cdims[0] * cdims[1] * nvec * nvec, dtype=np.complex128)
    want1 = ol.block_orthonormalize(nv.copy(), fdims, cdims, cholesky=chol)
    want2 = ol.block_orthonormalize(want1.copy(), fdims, cdims)
    for passes, want in ((1, want1), (2, want2)):
        got, Rf, cond = su.block_qr(nv, fdims, cdims, passes)
        assert rel(got, want) < ORACLE_TOL and rel(su.coarse_mats_to_eo(Rf), chol) < ORACLE_TOL, passes
        assert cond.shape == cdims[:2] and np.all(cond >= 1)
        # upper triangle, real positive diagonal
        assert not np.any(np.tril(Rf, -1)) and np.all(np.diagonal(Rf, axis1=2, axis2=3).imag == 0) and np.all(np.diagonal(Rf, axis1=2, axis2=3).real > 0)
    # Q R reproduces the input tile: the factor is a QR factor, not only the oracle's numbers
    Q, Rf, _ = su.block_qr(nv, fdims, cdims, 1)
    T0, TQ = su.tiles(nv, nvec, fdims, cdims), su.tiles(Q, nvec, fdims, cdims)
    assert np.max(np.abs(np.einsum("xyji,xyje->xyie", Rf, TQ) - T0)) < 1e-16
    # coarse_mats_to_grid undoes coarse_mats_to_eo
    assert np.array_equal(su.coarse_mats_to_grid(su.coarse_mats_to_eo(Rf), cdims, nvec), Rf)


@pytest.mark.parametrize("fdims,cdims", SMALL, ids=IDS)
def test_bi_ortho_is_the_oracles_block_bi_orthonormalize(fdims, cdims):
    nvec, fsize = cdims[2], fdims[0] * fdims[1] * fdims[2]
    cm = cdims[0] * cdims[1] * nvec * nvec
    pv = cs.gaussian_cvec(nvec * fsize, 3)
    rv = pv + 0.3 * cs.gaussian_cvec(nvec * fsize, 4)
    Lh, Uh = np.zeros(cm, dtype=np.complex128), np.zeros(cm, dtype=np.complex128)
    wp, wr = ol.block_bi_orthonormalize(pv.copy(), rv.copy(), fdims, cdims, Lh, Uh)
    gp, gr, L, U = su.bi_ortho(pv, rv, fdims, cdims)
    assert rel(gp, wp) < ORACLE_TOL and rel(gr, wr) < ORACLE_TOL
    assert rel(su.coarse_mats_to_eo(L), Lh) < ORACLE_TOL and rel(su.coarse_mats_to_eo(U), Uh) < ORACLE_TOL
    G = su.block_gram(rv, pv, fdims, cdims)
    assert np.max(np.abs(np.einsum("xyik,xykj->xyij", L, U) - G)) < 1e-15
    assert np.max(np.abs(su.block_gram(gr, gp, fdims, cdims) - np.eye(nvec))) < 1e-15


@pytest.mark.parametrize("fdims,cdims", SMALL, ids=IDS)
def test_galerkin_is_the_oracles_coarse_build(fdims, cdims):
    fLx, fLy, fnc = fdims
    vol, nvec = fLx * fLy, cdims[2]
    clover, hopping = cs.gaussian_cvec(vol * fnc * fnc, 1), cs.gaussian_cvec(4 * vol * fnc * fnc, 2)
    P = cs.gaussian_cvec(nvec * vol * fnc, 5)
    R = P + 0.2 * cs.gaussian_cvec(nvec * vol * fnc, 6)
    for cl, ho, rvecs in ((clover, hopping, None), (clover, hopping, R), (None, hopping, R), (clover, None, None)):
        od = ol.make_desc(fLx, fLy, fnc, cl, ho, 0.1, 0.02, 0.03)           # the shifts are not part of the build
        cc, ch = ol.coarse_build(od, P, cdims, restrict_vecs=rvecs)
        (gc, gh), (Sc, Sh), (nc_, nh) = su.galerkin(fdims, cdims, cl, ho, P, rvecs)
        assert rel(gc, cc) < ORACLE_TOL, (cl is None, ho is None)
        if ho is None:
            assert not np.any(ch) and not np.any(gh) and not np.any(Sh)
        else:
            assert rel(gh, ch) < ORACLE_TOL, (cl is None, rvecs is None)
        assert np.all(np.abs(gc) <= Sc * (1 + 1e-15)) and np.all(np.abs(gh) <= Sh * (1 + 1e-15))


@pytest.mark.parametrize("fdims,cdims", SMALL, ids=IDS)
def test_clover_inverse_rb_hopping_and_dagger_are_the_oracles(fdims, cdims):
    Lx, Ly, nc = fdims
    vol = Lx * Ly
    clover = cs.gaussian_cvec(vol * nc * nc, 1) + 4.0 * np.tile(np.eye(nc).reshape(-1), vol)
    hopping = cs.gaussian_cvec(4 * vol * nc * nc, 2)
    shifts = (0.2 + 0.1j, 0.03 - 0.02j, 0.05 + 0.01j)
    cinv, rclover, rhopping = ol.build_rbjacobi(ol.make_desc(Lx, Ly, nc, clover, hopping, *shifts))
    got, cond = su.clover_inverse(Lx, Ly, nc, clover, *shifts)
    assert rel(got, cinv) < ORACLE_TOL and cond.shape == (Lx, Ly)
    grh, S = su.rb_hopping(Lx, Ly, nc, hopping, got)
    assert rel(grh, rhopping) < ORACLE_TOL and np.all(np.abs(grh) <= S * (1 + 1e-15))
    # the inverse is an inverse: C X = 1 to long-double rounding
    Cg = su.shifted_clover(Lx, Ly, nc, clover, *shifts)
    Xg = su.sn.to_grid(got, Lx, Ly, nc * nc).reshape(Lx, Ly, nc, nc)
    assert np.max(np.abs(np.einsum("xyrk,xykc->xyrc", Cg, Xg) - np.eye(nc))) < 1e-16
    # without a clover: the diagonal of the three shifts alone
    cinv0, _, _ = ol.build_rbjacobi(ol.make_desc(Lx, Ly, nc, None, hopping, *shifts))
    assert rel(su.clover_inverse(Lx, Ly, nc, None, *shifts)[0], cinv0) < ORACLE_TOL
    dc, dh = ol.build_dagger(clover, hopping, Lx, Ly, nc)
    gdc, gdh = su.dagger(Lx, Ly, nc, clover, hopping)
    assert np.array_equal(gdc, dc) and np.array_equal(gdh, dh)
    assert su.dagger(Lx, Ly, nc, None, hopping)[0] is None and su.dagger(Lx, Ly, nc, clover, None)[1] is None
    assert np.array_equal(su.conjtrans(su.conjtrans(clover, vol, nc), vol, nc), clover)


# ---- b. every row is routed as it states
@pytest.mark.parametrize("fused", [1, 0])
def test_every_row_gets_the_plan_it_states(fused):
    qmg.set_tuning("setup_fused", fused)
    try:
        rows = [r for r in routes.ROUTES if r["fused"] == fused and r["expect"] is not None]
        assert rows
        for r in rows:
            assert routes.combo(routes.requested_plan(r)) == r["expect"], (r["id"], routes.requested_plan(r))
    finally:
        qmg.set_tuning("setup_fused", 1)


def test_route_ids_are_unique_and_cover_the_issue_rows():
    ids = [r["id"] for r in routes.ROUTES]
    assert len(set(ids)) == len(ids)
    expects = {r["expect"] for r in routes.ROUTES}
    for tpb, groups in ((32, 2), (32, 4), (32, 8), (64, 1), (64, 2), (64, 4), (128, 1), (128, 2), (256, 1)):
        assert routes.ORTHO(tpb, groups) in expects, (tpb, groups)
    for e in (routes.ORTHO(32, 8, idle=True), routes.ORTHO(256, 1, optin=True), routes.ORTHO(32, 8, strided=True), routes.PASSES, routes.GAL(1), routes.GAL(2),
              routes.GAL(3), routes.GAL(4), routes.GAL(4, optin=True), routes.GAL(1, strided=True), routes.PROBES, routes.CINV(), routes.CINV(strided=True),
              routes.UNSUPPORTED, routes.INVALID):
        assert e in expects, e


# ---- c. coverage and launch geometry
FNC = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48)
BLOCKS = (2, 3, 4, 8)
NCV = (1, 2, 4, 8, 12, 16, 17, 24, 32, 33)
COARSE = (2, 4, 6)
LDS_PER_WORKGROUP = 160 * 1024   # gfx950


def check_geometry(op, plan, fdims, cdims, ncv, tag):
    """the launch covers the request, within the hardware's limits"""
    family, tpb, groups, wgs, lds, flags, outs, threads = plan
    optin, idle, strided = bool(flags & qmg.SUP_LDS_OPTIN), bool(flags & qmg.SUP_IDLE_GROUP), bool(flags & qmg.SUP_STRIDED)
    if family in (qmg.SUF_ORTHO_PASSES, qmg.SUF_GALERKIN_PROBES, qmg.SUF_UNSUPPORTED, qmg.SUF_INVALID):
        assert plan[1:] == (0,) * 7, tag
        return
    assert 0 < lds <= LDS_PER_WORKGROUP and optin == (lds > 64 * 1024) and 0 < threads <= 256, tag
    if family == qmg.SUF_ORTHO_LDS:
        ncs = cdims[0] * cdims[1]
        nel = (fdims[0] // cdims[0]) * (fdims[1] // cdims[1]) * fdims[2]
        assert tpb in (32, 64, 128, 256) and (tpb >= nel or tpb == 256) and (tpb == 32 or tpb < 2 * nel), tag
        assert threads == tpb * groups and threads % 64 == 0 and groups in (1, 2, 4, 8), tag
        assert lds == 16 * ncv * nel * groups + 64, tag                       # the tiles and two doubles per wavefront of a full workgroup
        assert idle == (ncs % groups != 0) and strided == (wgs * groups < ncs), tag
        assert wgs == min(-(-ncs // groups), 262144) and outs == 0, tag
    elif family == qmg.SUF_GALERKIN:
        ncs = cdims[0] * cdims[1]
        assert threads == 256 and outs * 256 >= ncv * ncv > (outs - 1) * 256 and 1 <= outs <= 4, tag
        assert lds == 16 * (3 * fdims[2] * ncv + fdims[2] ** 2) and wgs == min(ncs, 262144) and strided == (wgs < ncs) and not idle and (tpb, groups) == (0, 0), tag
    else:
        assert family == qmg.SUF_CINV and op == qmg.SETUP_OP_CINV, tag
        vol = fdims[0] * fdims[1]
        assert threads == 256 and lds == 32 * fdims[2] ** 2 and wgs == min(vol, 4096) and strided == (wgs < vol) and not idle and not optin and (tpb, groups, outs) == (0, 0, 0), tag


def test_no_reachable_plan_lacks_a_row():
    expected = {r["expect"] for r in routes.ROUTES if r["expect"] is not None}
    found = {}
    try:
        for fused in (1, 0):
            qmg.set_tuning("setup_fused", fused)
            for fnc, bx, by, ncv, cLx, cLy in itertools.product(FNC, BLOCKS, BLOCKS, NCV, COARSE, COARSE):
                fdims, cdims = (bx * cLx, by * cLy, fnc), (cLx, cLy)
                for op, a in ((qmg.SETUP_OP_ORTHO, 1), (qmg.SETUP_OP_ORTHO, 2), (qmg.SETUP_OP_GALERKIN, 0), (qmg.SETUP_OP_GALERKIN, 1)):
                    plan = qmg.setup_plan(op, fdims, cdims, ncv, a)
                    check_geometry(op, plan, fdims, cdims, ncv, (fused, op, fdims, cdims, ncv, a))
                    found.setdefault(routes.combo(plan), (fused, op, fdims, cdims, ncv, a))
            for (Lx, Ly), nc, clover, shift in itertools.product(((2, 2), (6, 4), (34, 10), (48, 48), (64, 64), (66, 64)), sorted(set(FNC) | set(NCV)), (0, 1), (0, 1)):
                plan = qmg.setup_plan(qmg.SETUP_OP_CINV, (Lx, Ly, nc), a=clover, b=shift)
                check_geometry(qmg.SETUP_OP_CINV, plan, (Lx, Ly, nc), None, 0, (fused, Lx, Ly, nc, clover, shift))
                found.setdefault(routes.combo(plan), (fused, "cinv", Lx, Ly, nc, clover, shift))
            for r in routes.ROUTES:                                   # the rows' own requests: the grid-stride and LDS-overflow shapes lie outside the grid above
                if r["expect"] is not None:
                    plan = routes.requested_plan(r)
                    if "fdims" in r:
                        check_geometry(None, plan, r["fdims"], r["cdims"][:2], r["cdims"][2], r["id"])
                    found.setdefault(routes.combo(plan), r["id"])
    finally:
        qmg.set_tuning("setup_fused", 1)
    left_out = {c: first for c, first in found.items() if c not in expected}
    assert not left_out, "plans without a row in test_gpu_setup_routes.ROUTES (plan: first request that gave it): %r" % left_out
    # and no row expects a plan that its own request would not give under either tuning (b. holds each row to its own)
    assert expected <= set(found)
    assert len(found) >= 24


def test_the_knob_moves_every_block_local_request_to_the_full_lattice_passes():
    try:
        for r in routes.ROUTES:
            if r["expect"] is None or r["op"].startswith("jacobi"):
                continue
            qmg.set_tuning("setup_fused", 0)
            fam = routes.requested_plan(r)[0]
            assert fam in (qmg.SUF_ORTHO_PASSES, qmg.SUF_GALERKIN_PROBES, qmg.SUF_UNSUPPORTED), r["id"]
        qmg.set_tuning("setup_fused", 0)
        assert qmg.setup_plan(qmg.SETUP_OP_CINV, (6, 4, 8), a=1, b=1)[0] == qmg.SUF_CINV      # the knob does not reach the Jacobi build
    finally:
        qmg.set_tuning("setup_fused", 1)


# ---- d. refusals and the output buffer contract
BAD_LATTICES = [(3, 4), (4, 5), (0, 2), (2, 0), (-2, 4)]


def test_plan_refuses_bad_arguments():
    O, G, J = qmg.SETUP_OP_ORTHO, qmg.SETUP_OP_GALERKIN, qmg.SETUP_OP_CINV
    for op in (O, G):
        assert qmg.setup_plan(op, (16, 8, 2), (4, 2), 4, 1 if op == O else 0)[0] in (qmg.SUF_ORTHO_LDS, qmg.SUF_GALERKIN)
        for dims in BAD_LATTICES:
            assert qmg.setup_plan(op, dims + (2,), (2, 2), 4, 1)[0] == qmg.SUF_INVALID, (op, dims)
            assert qmg.setup_plan(op, (16, 8, 2), dims, 4, 1)[0] == qmg.SUF_INVALID, (op, dims)
        assert qmg.setup_plan(op, (16, 8, 2), (6, 2), 4, 1)[0] == qmg.SUF_INVALID       # 16 is no multiple of 6
        assert qmg.setup_plan(op, (16, 8, 2), (4, 6), 4, 1)[0] == qmg.SUF_INVALID
        assert qmg.setup_plan(op, (16, 8, 2), (32, 2), 4, 1)[0] == qmg.SUF_INVALID      # coarser than fine
        for bad in (0, -1):
            assert qmg.setup_plan(op, (16, 8, bad), (4, 2), 4, 1)[0] == qmg.SUF_INVALID
            assert qmg.setup_plan(op, (16, 8, 2), (4, 2), bad, 1)[0] == qmg.SUF_INVALID
    for passes in (0, 3, -1):
        assert qmg.setup_plan(O, (16, 8, 2), (4, 2), 4, passes)[0] == qmg.SUF_INVALID
    for dims in BAD_LATTICES:
        assert qmg.setup_plan(J, dims + (2,), a=1, b=1)[0] == qmg.SUF_INVALID
    assert qmg.setup_plan(J, (6, 4, 0), a=1, b=1)[0] == qmg.SUF_INVALID
    assert qmg.setup_plan(J, (6, 4, 33), a=1, b=1)[0] == qmg.SUF_UNSUPPORTED
    assert qmg.setup_plan(J, (6, 4, 33), a=0, b=0)[0] == qmg.SUF_UNSUPPORTED           # the colour count is looked at first, as the entry point did
    assert qmg.setup_plan(J, (6, 4, 32), a=0, b=0)[0] == qmg.SUF_INVALID               # nothing to invert (stencil_2d.h:1471-1475)
    assert qmg.setup_plan(J, (6, 4, 32), a=0, b=1)[0] == qmg.SUF_CINV and qmg.setup_plan(J, (6, 4, 32), a=1, b=0)[0] == qmg.SUF_CINV
    for op in (-1, 3, 99):
        assert qmg.setup_plan(op, (16, 8, 2), (4, 2), 4, 1) == (qmg.SUF_INVALID,) + (0,) * 7
    # a slab build: served where k_galerkin serves it, unsupported where the probe passes would
    assert qmg.setup_plan(G, (8, 8, 2), (2, 2), 32, 1)[0] == qmg.SUF_GALERKIN and qmg.setup_plan(G, (8, 8, 2), (2, 2), 33, 1)[0] == qmg.SUF_UNSUPPORTED
    assert qmg.setup_plan(G, (8, 8, 2), (2, 2), 33, 0)[0] == qmg.SUF_GALERKIN_PROBES


def test_plan_output_buffer_contract():
    lib = qmg.lib()
    out = (C.c_int * 12)(*([7] * 12))
    assert lib.qmg_setup_plan(qmg.SETUP_OP_ORTHO, 16, 8, 2, 4, 2, 16, 2, 0, out, 12) == 0
    assert list(out[8:]) == [-1] * 4 and tuple(out[:8]) == (qmg.SUF_ORTHO_LDS, 32, 2, 4, 16448, 0, 0, 64)
    assert lib.qmg_setup_plan(qmg.SETUP_OP_ORTHO, 16, 8, 2, 4, 2, 16, 2, 0, out, 7) == 1
    assert lib.qmg_setup_plan(qmg.SETUP_OP_ORTHO, 16, 8, 2, 4, 2, 16, 2, 0, None, 8) == 1
    assert qmg.SETUP_PLAN_INTS == 8


def test_plan_beyond_the_grid_caps_is_walked():
    fam, tpb, groups, wgs, lds, flags, outs, threads = qmg.setup_plan(qmg.SETUP_OP_ORTHO, (4096, 2052, 1), (2048, 1026), 1, 1)
    assert (fam, tpb, groups, wgs, flags) == (qmg.SUF_ORTHO_LDS, 32, 8, 262144, qmg.SUP_STRIDED) and 2048 * 1026 > wgs * groups
    fam, _, _, wgs, _, flags, outs, _ = qmg.setup_plan(qmg.SETUP_OP_GALERKIN, (1024, 1028, 1), (512, 514), 1, 0)
    assert (fam, wgs, flags, outs) == (qmg.SUF_GALERKIN, 262144, qmg.SUP_STRIDED, 1)
    assert qmg.setup_plan(qmg.SETUP_OP_GALERKIN, (1024, 1024, 1), (512, 512), 1, 0)[5] == 0          # exactly 262144 coarse sites: one trip
    assert qmg.setup_plan(qmg.SETUP_OP_CINV, (64, 64, 2), a=1, b=0)[5] == 0 and qmg.setup_plan(qmg.SETUP_OP_CINV, (66, 64, 2), a=1, b=0)[5] == qmg.SUP_STRIDED


# ---- e. the conditions of the GPU rows, on the reference alone
def test_orthonormalisation_rows_have_well_conditioned_tiles():
    for r in routes.ROUTES:
        if r["op"] != "ortho" or not r["fused"]:
            continue                                      # (the unfused rows repeat the fused rows' inputs; a one-column tile, nvec = 1, has condition number 1)
        nvec = r["cdims"][2]
        nel = (r["fdims"][0] // r["cdims"][0]) * (r["fdims"][1] // r["cdims"][1]) * r["fdims"][2]
        assert nvec <= nel // 2 or nvec == 1, r["id"]
        _, Rf, cond = su.block_qr(routes.ortho_inputs(r), r["fdims"], r["cdims"], 1)
        assert cond.max() <= routes.COND_CAP, (r["id"], float(cond.max()))
        assert np.all(np.diagonal(Rf, axis1=2, axis2=3).real > 0)
    r = [r for r in routes.ROUTES if r["op"] == "ortho_strided"]
    assert len(r) == 1 and r[0]["cdims"][2] == 1 and r[0]["cdims"][0] * r[0]["cdims"][1] > 262144 * 8


def pivot_trace(M):
    """the row partial pivoting picks at every step of Gauss-Jordan elimination, per matrix of M[V, nc, nc] (complex128): the first row of
    largest modulus in the column, from the diagonal down"""
    m = M.copy()
    V, nc = m.shape[0], m.shape[1]
    idx = np.arange(V)
    piv = np.zeros((V, nc), dtype=np.int64)
    for k in range(nc):
        best = k + np.argmax(np.abs(m[:, k:, k]) ** 2, axis=1)
        piv[:, k] = best
        rows_k, rows_b = m[idx, k].copy(), m[idx, best].copy()
        m[idx, best], m[idx, k] = rows_k, rows_b
        m[:, k] /= m[:, k, k][:, None]
        f = m[:, :, k].copy()
        f[:, k] = 0
        m -= f[:, :, None] * m[:, k][:, None, :]
    return piv


def test_jacobi_rows_are_well_conditioned_and_exchange_rows_at_every_step():
    seen = 0
    for r in routes.ROUTES:
        if r["op"] != "jacobi":
            continue
        (Lx, Ly), nc = r["dims"], r["nc"]
        clover, _ = routes.jacobi_inputs(r)
        Cg = su.shifted_clover(Lx, Ly, nc, clover, *r["shifts"]).astype(np.complex128)
        cond = np.linalg.cond(Cg)
        assert cond.max() <= routes.COND_CAP, (r["id"], float(cond.max()))
        if clover is not None and nc > 1:
            piv = pivot_trace(Cg.reshape(Lx * Ly, nc, nc))
            assert np.all(piv[:, :nc - 1] != np.arange(nc - 1)[None, :]), r["id"]      # never the diagonal: a row exchange at every step but the last
            seen += 1
    assert seen >= 22


def test_galerkin_term_counts_in_closed_form():
    """n = fnc (the inner product M P) + fnc per (fine site, piece) that reaches the entry: a block has bx by sites, 2 (bx - 1) by + 2 bx (by - 1)
    hops that stay inside it, by hops that leave it in +x and in -x, bx in +y and in -y -- whatever the coarse extents, 2 included"""
    seen = 0
    for r in routes.ROUTES:
        if r["op"] != "galerkin" or not r["fused"] or r["fdims"][2] * r["cdims"][2] > 96:
            continue
        fLx, fLy, fnc = r["fdims"]
        cLx, cLy, cnc = r["cdims"]
        bx, by = fLx // cLx, fLy // cLy
        clover, hopping, P, R = routes.galerkin_inputs(r)
        _, (Sc, Sh), (nc_, nh) = su.galerkin(r["fdims"], r["cdims"], clover, hopping, P, R)
        inside = (2 * (bx - 1) * by + 2 * bx * (by - 1)) if hopping is not None else 0
        assert np.all(nc_ == fnc + fnc * ((bx * by if clover is not None else 0) + inside)), r["id"]
        leave = np.repeat([by, bx, by, bx], cLx * cLy * cnc * cnc) if hopping is not None else 0
        assert np.all(nh == fnc + fnc * leave), r["id"]
        if hopping is None:
            assert not np.any(Sh)
        else:
            assert np.all(Sh > 0) and np.all(Sc > 0)
        seen += 1
    assert seen >= 8
