"""Every multigrid SETUP kernel -- block orthonormalisation and the Galerkin build (csrc/qmg_setup.hip), the right-block-Jacobi inverse and
hops, the dagger build and the batched conjugate transpose (csrc/qmg_fill.hip), the bi-orthonormalisation and the two full-lattice fallbacks
(csrc/qmg_transfer.hip) -- against setup_numpy's long-double statement on coordinate grids, one row per route.

ROUTES is the table.  A row names the entry point (op), the shapes, the tuning knob "setup_fused" and the plan it expects in qmg_setup_plan's
terms, as the tuple (family, TPB, groups, LDS opt-in, idle group, outputs per thread, strided).  A row first asserts that the library routes
the request as the row says, so a retune that moves a shape to another instantiation fails here, and tests/test_host_setup_plan.py fails
when a reachable plan has no row.  Then the entry point runs and EVERY block, site and entry is held to the reference:

  orthonormalisation   per (block, vector) |got - want|_2 <= 1e-12 (the reference vectors have unit block norm; 1e-12 is the project's setup
                       parity tolerance); per block the factor's upper triangle within 1e-12 |R_ref|_F and its strict lower triangle, prefilled
                       with a sentinel, byte-identical; with passes = 2 the factor is that of the first pass; the Gram matrix of the device
                       result, formed in long double, |Q^dag Q - 1|_max <= 1e-13 (the n05 number of test_gpu_parity.py).  Every row runs
                       with passes 1 and 2, with and without a factor buffer.  (Condition, asserted on the reference in the host test: every
                       tile has 2-norm condition number <= 50.)
  Galerkin             every entry of the five coarse blocks of every coarse site: |got - want| <= (n + 1) 2^-50 S
                       (stencil_numpy.elementwise_bound) with S = sum |R| |M| |P| and n = fnc + the number of (x, piece, r) contributions
                       from setup_numpy.galerkin.  Outputs are prefilled with NaN.  Non-zero shifts in the fine descriptor must leave the
                       result bit-identical.  The probe fallback is held to the same constant with n + cnc + bx by fnc: a probe is a unit
                       vector, so its prolongation is one product per element (the other cnc - 1 terms of that sum are exact zeros), the
                       partial fine apply is a sum of fnc terms, the restriction a sum over the bx by fnc elements of the block, and the
                       scatter adds the at most nine probe results of an entry; the flat sum the reference counts has n >= fnc terms, the
                       passes' partial sums add at most cnc + bx by fnc roundings to it.
  inverse              per site |got - want|_F <= 1e-12 |want|_F.  The matrix to invert is Pi_x (G_x + s) with G_x Gaussian, s = 6 + 4 sqrt(nc)
                       and Pi_x a cyclic row shift by one place (no fixed points), so that partial pivoting exchanges rows at every step
                       but the last (condition number <= 50 and the pivot trace are asserted on the reference in the host test).
  rb_hopping           elementwise against the long-double product of the hops with the cinv THE DEVICE LEFT (the kernel is held to what
                       it reads): (nc + 1) 2^-50 S.  rb_clover is the identity bit for bit.
  dagger, conjtrans    bit for bit.
  bi-orthonormalisation  per block |R^dag P - 1|_max <= 1e-12, |L U - G| <= 1e-10 (1 + |G|) with G the Gram matrix of the ORIGINAL vectors,
                       vectors and factors within 1e-11 per (block, vector) / per block.
Read-only operands come back byte-identical, and a second run on the same inputs gives the same bytes.  A refused request leaves its
NaN-prefilled outputs untouched.  The grid-stride orthonormalisation row (more than 262144 workgroups' worth of blocks) compares every block
with an fp64 statement of the reference (its own error, a few 2^-53, is far below the tolerances) and samples the long-double one on 4096
blocks and the first and last block of both grid-stride trips; the grid-stride Galerkin row holds every entry to the long-double reference.

Each row prints its worst error over bound (or over tolerance); profiles/setup_routes.txt holds the lines of a run on an MI355X.
"""
import ctypes as C
import importlib

import numpy as np
import pytest

import coordspace as cs
import setup_numpy as su
import stencil_numpy as sn

qmg = importlib.import_module("quantum-mg_amd")

pytestmark = pytest.mark.gpu

TOL_SETUP = 1e-12     # the project's setup parity tolerance (test_gpu_parity.py)
TOL_GRAM = 1e-13      # n05: P^dag P = 1
TOL_BIORTHO = 1e-11   # test_block_bi_orthonormalize_asymmetric_transfer
COND_CAP = 50.0
SHIFTS = (0.7 + 0.3j, 0.25 - 0.15j, -0.2 + 0.1j)   # shift, eo_shift, dof_shift
SENTINEL = 7.25 - 3.5j


# ---- plans, as the tuple the host test enumerates: (family, TPB, groups, LDS opt-in, idle group, outputs per thread, strided)
def combo(plan):
    family, tpb, groups, _wg, _lds, flags, outs, _threads = plan
    return (family, tpb, groups, bool(flags & qmg.SUP_LDS_OPTIN), bool(flags & qmg.SUP_IDLE_GROUP), outs, bool(flags & qmg.SUP_STRIDED))


def ORTHO(tpb, groups, optin=False, idle=False, strided=False):
    return (qmg.SUF_ORTHO_LDS, tpb, groups, optin, idle, 0, strided)


def GAL(outs, optin=False, strided=False):
    return (qmg.SUF_GALERKIN, 0, 0, optin, False, outs, strided)


def CINV(strided=False):
    return (qmg.SUF_CINV, 0, 0, False, False, 0, strided)


PASSES = (qmg.SUF_ORTHO_PASSES, 0, 0, False, False, 0, False)
PROBES = (qmg.SUF_GALERKIN_PROBES, 0, 0, False, False, 0, False)
UNSUPPORTED = (qmg.SUF_UNSUPPORTED, 0, 0, False, False, 0, False)
INVALID = (qmg.SUF_INVALID, 0, 0, False, False, 0, False)

ROUTES = []


def row(op, name, expect, fused=1, **kw):
    r = dict(op=op, expect=expect, fused=fused, id="%s-%s%s" % (op, name, "" if fused else "-unfused"))
    r.update(kw)
    ROUTES.append(r)


def _shape(fdims, cdims):
    return "%dx%dx%d-%dx%dx%d" % (fdims + cdims)


# ---- block orthonormalisation: (fine, coarse + nvec, plan).  nvec <= nel / 2 keeps a Gaussian tile's condition number near 6.
ORTHO_SHAPES = [
    ((16, 8, 2), (4, 2, 16), ORTHO(32, 2)),
    ((24, 8, 2), (6, 2, 8), ORTHO(32, 4)),
    ((12, 4, 2), (6, 2, 4), ORTHO(32, 8, idle=True)),               # 12 blocks, 8 per workgroup: four groups of the second own none
    ((8, 8, 4), (2, 2, 16), ORTHO(64, 1)),
    ((8, 8, 3), (2, 2, 12), ORTHO(64, 2)),                          # nel = 48, not a multiple of TPB
    ((8, 8, 3), (2, 2, 4), ORTHO(64, 4)),
    ((8, 8, 6), (2, 2, 12), ORTHO(128, 1)),                         # nel = 96
    ((8, 8, 6), (2, 2, 4), ORTHO(128, 2)),
    ((8, 8, 12), (2, 2, 8), ORTHO(256, 1)),                         # nel = 192, 24 KB of tile: no opt-in
    ((16, 16, 24), (4, 4, 24), ORTHO(256, 1, optin=True)),          # nel = 384, 144 KB
    ((8, 8, 8), (2, 2, 33), ORTHO(128, 1, optin=True)),             # nel = 128, 66 KB: the opt-in below 256 threads
    ((8, 8, 2), (4, 4, 1), ORTHO(32, 8)),                           # nvec = 1
    ((4, 8, 2), (2, 2, 4), ORTHO(32, 8, idle=True)),                # blocks 2 x 4; one workgroup, four of its groups idle
    ((16, 4, 2), (2, 2, 8), ORTHO(32, 4)),                          # blocks 8 x 2
    ((4, 24, 1), (2, 6, 2), ORTHO(32, 8, idle=True)),               # cLx = 2 with cLy = 6
    ((24, 4, 1), (6, 2, 2), ORTHO(32, 8, idle=True)),               # cLy = 2 with cLx = 6
]
for _f, _c, _p in ORTHO_SHAPES:
    row("ortho", _shape(_f, _c), _p, fdims=_f, cdims=_c, seed=31)
    row("ortho", _shape(_f, _c), PASSES, fused=0, fdims=_f, cdims=_c, seed=31)
row("ortho", _shape((12, 8, 2), (4, 2, 4)), PASSES, fdims=(12, 8, 2), cdims=(4, 2, 4), seed=32)          # the fallback by odd block width
row("ortho", _shape((16, 16, 24), (4, 4, 32)), PASSES, fdims=(16, 16, 24), cdims=(4, 4, 32), seed=33)    # the fallback by LDS overflow (192 KB)
# more than 262144 * 8 blocks: the first 512 workgroups take a second trip.  134 MB of vectors.
row("ortho_strided", _shape((4096, 2052, 1), (2048, 1026, 1)), ORTHO(32, 8, strided=True), fdims=(4096, 2052, 1), cdims=(2048, 1026, 1), seed=34)

# ---- Galerkin: (fine, coarse + cnc, plan, separate restrictor, clover present, hopping present)
GALERKIN_SHAPES = [
    ((8, 8, 1), (2, 2, 1), GAL(1), False, True, True),              # blocks 4 x 4, nvec = 1
    ((4, 4, 2), (2, 2, 2), GAL(1), True, True, True),               # blocks 2 x 2
    ((4, 8, 2), (2, 2, 16), GAL(1), False, True, True),             # blocks 2 x 4; one output per thread, exactly full
    ((16, 4, 2), (2, 2, 17), GAL(2), True, True, True),             # blocks 8 x 2; two outputs, partial
    ((8, 8, 24), (2, 2, 24), GAL(3), True, True, True),             # three outputs; the loops over nf nc and nf nf above 256
    ((4, 4, 8), (2, 2, 32), GAL(4), False, True, True),             # four outputs, full
    ((8, 8, 48), (2, 2, 32), GAL(4, optin=True), True, True, True),   # 108 KB of LDS
    ((4, 4, 48), (2, 2, 24), GAL(3, optin=True), False, True, True),
    ((4, 4, 48), (2, 2, 17), GAL(2, optin=True), True, True, True),
    ((4, 4, 48), (2, 2, 16), GAL(1, optin=True), False, True, True),
    ((8, 12, 2), (4, 6, 4), GAL(1), True, True, True),              # coarse extents above 2: +mu and -mu neighbours differ
    ((16, 4, 2), (8, 2, 4), GAL(1), True, True, True),              # cLy = 2 alone
    ((8, 8, 2), (4, 2, 4), GAL(1), True, False, True),              # no fine clover
    ((8, 8, 2), (2, 4, 4), GAL(1), True, True, False),              # no fine hopping
]
for _f, _c, _p, _r, _cl, _ho in GALERKIN_SHAPES:
    _n = _shape(_f, _c) + ("-R" if _r else "") + ("" if _cl else "-noclover") + ("" if _ho else "-nohopping")
    row("galerkin", _n, _p, fdims=_f, cdims=_c, sep_r=_r, clover=_cl, hopping=_ho, seed=41)
    row("galerkin", _n, PROBES, fused=0, fdims=_f, cdims=_c, sep_r=_r, clover=_cl, hopping=_ho, seed=41)
row("galerkin", _shape((4, 4, 2), (2, 2, 33)) + "-R", PROBES, fdims=(4, 4, 2), cdims=(2, 2, 33), sep_r=True, clover=True, hopping=True, seed=42)   # cnc beyond GAL_MAXOUT
row("galerkin_refused", _shape((4, 4, 2), (2, 2, 33)) + "-slab", UNSUPPORTED, fdims=(4, 4, 2), cdims=(2, 2, 33))   # a slab build the probes would serve
row("galerkin_strided", _shape((1024, 1028, 1), (512, 514, 1)), GAL(1, strided=True), fdims=(1024, 1028, 1), cdims=(512, 514, 1), seed=43)

# ---- right block Jacobi
for _nc in (1, 2, 3, 8, 16, 17, 24, 32):
    for _L in ((2, 2), (6, 4), (34, 10)):
        row("jacobi", "%dx%dx%d" % (_L + (_nc,)), CINV(), dims=_L, nc=_nc, clover=True, hopping=True, rb_hopping=True, shifts=SHIFTS, seed=51)
row("jacobi", "66x64x2", CINV(strided=True), dims=(66, 64), nc=2, clover=True, hopping=True, rb_hopping=True, shifts=SHIFTS, seed=52)   # 4224 sites, 4096 blocks
row("jacobi", "6x4x2-noclover", CINV(), dims=(6, 4), nc=2, clover=False, hopping=True, rb_hopping=True, shifts=(1.5 + 0.5j, 0.3 - 0.2j, 0.2 + 0.1j), seed=53)
row("jacobi", "6x4x3-noclover", CINV(), dims=(6, 4), nc=3, clover=False, hopping=True, rb_hopping=True, shifts=(1.5 + 0.5j, 0.3 - 0.2j, 0.2 + 0.1j), seed=53)
row("jacobi", "6x4x8-norb", CINV(), dims=(6, 4), nc=8, clover=True, hopping=True, rb_hopping=False, shifts=SHIFTS, seed=54)     # rb_hopping = NULL
row("jacobi", "6x4x8-nohopping", CINV(), dims=(6, 4), nc=8, clover=True, hopping=False, rb_hopping=True, shifts=SHIFTS, seed=54)   # nothing to multiply
row("jacobi_refused", "6x4x33", UNSUPPORTED, dims=(6, 4), nc=33, clover=True, shifts=SHIFTS)
row("jacobi_refused", "6x4x2-noclover-noshift", INVALID, dims=(6, 4), nc=2, clover=False, shifts=(0.0, 0.0, 0.0))

# ---- dagger build and conjugate transpose (no plan: one kernel, k_conjtrans)
for _L in ((2, 2), (2, 6), (6, 2), (34, 10)):
    for _nc in (1, 3, 24):
        row("dagger", "%dx%dx%d" % (_L + (_nc,)), None, dims=_L, nc=_nc, seed=61)

# ---- bi-orthonormalisation (no plan: the full-lattice passes)
for _f, _c in [((16, 16, 2), (4, 4, 8)), ((16, 12, 2), (4, 6, 4)), ((8, 8, 8), (2, 2, 6)), ((16, 8, 1), (4, 4, 2)), ((12, 8, 2), (4, 2, 4)), ((8, 8, 2), (4, 4, 1))]:
    row("biortho", _shape(_f, _c), None, fdims=_f, cdims=_c, seed=71)


def requested_plan(r):
    """qmg_setup_plan's answer to the row's request, under the tuning the library holds at the time of the call"""
    op = r["op"].split("_")[0]
    if op == "ortho":
        return qmg.setup_plan(qmg.SETUP_OP_ORTHO, r["fdims"], r["cdims"][:2], r["cdims"][2], 1)
    if op == "galerkin":
        return qmg.setup_plan(qmg.SETUP_OP_GALERKIN, r["fdims"], r["cdims"][:2], r["cdims"][2], r["op"] == "galerkin_refused")
    if op == "jacobi":
        return qmg.setup_plan(qmg.SETUP_OP_CINV, r["dims"] + (r["nc"],), a=r["clover"], b=any(s != 0 for s in r["shifts"]))
    return None


# ---- inputs: functions of the row alone, so that the host test can assert the rows' conditions on the reference without a GPU
def ortho_inputs(r):
    fLx, fLy, fnc = r["fdims"]
    return cs.gaussian_cvec(r["cdims"][2] * fLx * fLy * fnc, r["seed"])


def galerkin_inputs(r):
    """(clover or None, hopping or None, P, R or None)"""
    fLx, fLy, fnc = r["fdims"]
    vol, cnc = fLx * fLy, r["cdims"][2]
    clover = cs.gaussian_cvec(vol * fnc * fnc, r["seed"]) if r["clover"] else None
    hopping = cs.gaussian_cvec(4 * vol * fnc * fnc, r["seed"] + 100) if r["hopping"] else None
    P = cs.gaussian_cvec(cnc * vol * fnc, r["seed"] + 200)
    R = P + 0.2 * cs.gaussian_cvec(cnc * vol * fnc, r["seed"] + 300) if r["sep_r"] else None
    return clover, hopping, P, R


def jacobi_inputs(r):
    """(clover or None, hopping or None): with a clover, the matrix clover + shifts is Pi_x (G_x + s) per site -- the Gaussian G_x with s on
    its diagonal, its rows shifted cyclically by one place, up on the even sites and down on the odd ones (nc = 1: not at all).  Either way
    the large entry of column k sits below the diagonal at every elimination step but the last: in the last row, or in row k + 1."""
    (Lx, Ly), nc = r["dims"], r["nc"]
    vol = Lx * Ly
    hopping = cs.gaussian_cvec(4 * vol * nc * nc, r["seed"] + 100) if r["hopping"] else None
    if not r["clover"]:
        return None, hopping
    A = cs.gaussian_cvec(vol * nc * nc, r["seed"]).reshape(Lx, Ly, nc, nc) + (6.0 + 4.0 * np.sqrt(nc)) * np.eye(nc)
    xs, ys = np.meshgrid(np.arange(Lx), np.arange(Ly), indexing="ij")
    k = np.where((xs + ys) & 1, nc - 1, 1) if nc > 1 else np.zeros_like(xs)
    rows = (np.arange(nc)[None, None, :] + k[:, :, None]) % nc
    M = np.take_along_axis(A, rows[:, :, :, None], axis=2)
    diag = su.shifted_clover(Lx, Ly, nc, None, *r["shifts"]).astype(np.complex128)
    return cs.grid_to_eo((M - diag).reshape(Lx, Ly, nc * nc), Lx, Ly, nc * nc), hopping


# ---- running a row
@pytest.fixture(scope="module", autouse=True)
def _device():
    qmg.build()
    qmg.init(0)
    yield
    qmg.sync()
    qmg.set_tuning("setup_fused", 1)


def D(a):
    return qmg.DeviceArray.from_host(np.ascontiguousarray(a, dtype=np.complex128))


def nan_array(n):
    return D(np.full(n, np.nan + 1j * np.nan))


def same_bytes(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def report(r, **ratios):
    print("ROUTE %-52s %s" % (r["id"], "  ".join(("%s %d" if isinstance(v, int) else "%s %.3g") % (k, v) for k, v in ratios.items())))


def ortho_check(r, got, chol_got, want_tiles, Rf, passes):
    """(worst vector error / 1e-12, worst Gram defect / 1e-13, worst factor error / (1e-12 |R|_F)) over all blocks; asserts"""
    fdims, cdims = r["fdims"], r["cdims"]
    nvec = cdims[2]
    Tg = su.tiles(got, nvec, fdims, cdims)
    err = np.sqrt(np.sum(np.abs(Tg - want_tiles) ** 2, axis=-1))                    # [X, Y, d]
    gram = np.abs(np.einsum("xyie,xyje->xyij", np.conj(Tg), Tg) - np.eye(nvec))
    assert err.max() <= TOL_SETUP, (r["id"], passes, "vector", np.unravel_index(np.argmax(err), err.shape), float(err.max()))
    assert gram.max() <= TOL_GRAM, (r["id"], passes, "gram", np.unravel_index(np.argmax(gram), gram.shape), float(gram.max()))
    fac = 0.0
    if chol_got is not None:
        F = su.coarse_mats_to_grid(chol_got, cdims, nvec)
        lower = np.tril(np.ones((nvec, nvec), dtype=bool), -1)
        assert same_bytes(F[:, :, lower], np.full(F[:, :, lower].shape, SENTINEL)), (r["id"], passes, "the factor's strict lower triangle was written")
        up = np.where(lower, 0, F).astype(su.CLD)
        ferr = np.sqrt(np.sum(np.abs(up - Rf) ** 2, axis=(2, 3)))
        fnorm = np.sqrt(np.sum(np.abs(Rf) ** 2, axis=(2, 3)))
        assert np.all(ferr <= TOL_SETUP * fnorm), (r["id"], passes, "factor", float((ferr / fnorm).max()))
        fac = float((ferr / fnorm).max() / TOL_SETUP)
    return float(err.max() / TOL_SETUP), float(gram.max() / TOL_GRAM), fac


def run_ortho(r):
    fdims, cdims = r["fdims"], r["cdims"]
    nvec = cdims[2]
    nv = ortho_inputs(r)
    ccm = cdims[0] * cdims[1] * nvec * nvec
    worst = [0.0, 0.0, 0.0]
    first = {}
    for passes in (1, 2):
        want, Rf, cond = su.block_qr(nv, fdims, cdims, passes)
        assert cond.max() <= COND_CAP
        want_tiles = su.tiles(want, nvec, fdims, cdims)
        for with_factor in (True, False):
            dnv = D(nv)
            dchol = D(np.full(ccm, SENTINEL)) if with_factor else None
            qmg.block_orthonormalize_n(dnv, nvec, fdims, cdims[0], cdims[1], cholesky=dchol, passes=passes)
            got = dnv.to_host()
            chol_got = dchol.to_host() if with_factor else None
            res = ortho_check(r, got, chol_got, want_tiles, Rf, passes)
            worst = [max(a, b) for a, b in zip(worst, res)]
            if with_factor:
                first[passes] = (got, chol_got)
            else:
                assert same_bytes(got, first[passes][0]), (r["id"], passes, "the vectors depend on the factor buffer")
    # a second run on the same inputs gives the same bytes
    dnv, dchol = D(nv), D(np.full(ccm, SENTINEL))
    qmg.block_orthonormalize_n(dnv, nvec, fdims, cdims[0], cdims[1], cholesky=dchol, passes=2)
    assert same_bytes(dnv.to_host(), first[2][0]) and same_bytes(dchol.to_host(), first[2][1]), (r["id"], "second run")
    report(r, vec=worst[0], gram=worst[1], factor=worst[2])


def strided_samples(ncs, per_trip, count=4096):
    """linear block numbers: `count` random ones plus the first and last block of both grid-stride trips"""
    rng = np.random.default_rng(5)
    return np.unique(np.concatenate([rng.integers(0, ncs, count), [0, per_trip - 1, per_trip, ncs - 1]]))


def run_ortho_strided(r):
    fdims, cdims = r["fdims"], r["cdims"]
    fLx, fLy, _ = fdims
    cLx, cLy, _ = cdims
    ncs = cLx * cLy
    nv = ortho_inputs(r)
    dnv, dchol = D(nv), D(np.full(ncs, SENTINEL))
    qmg.block_orthonormalize_n(dnv, 1, fdims, cLx, cLy, cholesky=dchol, passes=1)
    got, chol_got = dnv.to_host(), dchol.to_host()
    # every block in fp64: a 4-element block divided by its norm
    T0 = cs.eo_to_grid(nv, fLx, fLy, 1).reshape(cLx, 2, cLy, 2).transpose(0, 2, 1, 3).reshape(cLx, cLy, 4)
    Tg = cs.eo_to_grid(got, fLx, fLy, 1).reshape(cLx, 2, cLy, 2).transpose(0, 2, 1, 3).reshape(cLx, cLy, 4)
    nrm = np.sqrt(np.sum(T0.real ** 2 + T0.imag ** 2, axis=-1))
    err = np.sqrt(np.sum(np.abs(Tg - T0 / nrm[:, :, None]) ** 2, axis=-1))
    F = cs.eo_to_grid(chol_got, cLx, cLy, 1)[:, :, 0]
    assert err.max() <= TOL_SETUP, (np.unravel_index(np.argmax(err), err.shape), float(err.max()))
    assert np.all(np.abs(F - nrm) <= TOL_SETUP * nrm), float((np.abs(F - nrm) / nrm).max())
    gram = np.abs(np.sum(Tg.real ** 2 + Tg.imag ** 2, axis=-1) - 1.0)
    assert gram.max() <= TOL_GRAM, float(gram.max())
    # sampled blocks in long double; block number = Y cLx + X counts the blocks in the order the grid-stride trips take them
    pl = qmg.setup_plan(qmg.SETUP_OP_ORTHO, fdims, cdims[:2], 1, 1)
    s = strided_samples(ncs, pl[3] * pl[2])                             # workgroups x groups blocks per trip
    X, Y = s % cLx, s // cLx
    t0, tg = T0[X, Y].astype(su.CLD), Tg[X, Y].astype(su.CLD)
    n_ld = np.sqrt(np.sum(np.abs(t0) ** 2, axis=-1))
    err_ld = np.sqrt(np.sum(np.abs(tg - t0 / n_ld[:, None]) ** 2, axis=-1))
    assert err_ld.max() <= TOL_SETUP and np.all(np.abs(F[X, Y] - n_ld) <= TOL_SETUP * n_ld)
    report(r, vec=float(err.max() / TOL_SETUP), gram=float(gram.max() / TOL_GRAM), factor=float((np.abs(F - nrm) / nrm).max() / TOL_SETUP), blocks=ncs, sampled=len(s))


def galerkin_device(r, clover, hopping, P, R, shifts):
    """(cclover, chopping) from the device, outputs prefilled with NaN; asserts the inputs come back untouched"""
    fLx, fLy, fnc = r["fdims"]
    cdims = r["cdims"]
    ccm = cdims[0] * cdims[1] * cdims[2] ** 2
    dcl, dho, dP, dR = (None if clover is None else D(clover)), (None if hopping is None else D(hopping)), D(P), (None if R is None else D(R))
    gd = qmg.make_desc(fLx, fLy, fnc, dcl, dho, *shifts)
    gcc, gch = nan_array(ccm), nan_array(4 * ccm)
    qmg.coarse_build(gcc, gch, gd, dP, cdims, restrict_vecs=dR)
    for dev, host in ((dcl, clover), (dho, hopping), (dP, P), (dR, R)):
        assert dev is None or same_bytes(dev.to_host(), host), (r["id"], "a read-only operand changed")
    return gcc.to_host(), gch.to_host()


def run_galerkin(r):
    fdims, cdims = r["fdims"], r["cdims"]
    clover, hopping, P, R = galerkin_inputs(r)
    (wc, wh), (Sc, Sh), (nc_, nh) = su.galerkin(fdims, cdims, clover, hopping, P, R)
    extra = 0 if r["expect"][0] == qmg.SUF_GALERKIN else cdims[2] + (fdims[0] // cdims[0]) * (fdims[1] // cdims[1]) * fdims[2]   # the probe passes' sums
    gc, gh = galerkin_device(r, clover, hopping, P, R, (0.0, 0.0, 0.0))
    worst = 0.0
    for name, got, want, S, n in (("clover", gc, wc, Sc, nc_), ("hopping", gh, wh, Sh, nh)):
        assert np.all(np.isfinite(got)), (r["id"], name, "entries left unwritten or not finite: %d" % np.count_nonzero(~np.isfinite(got)))
        err, bound = np.abs(got - want), sn.elementwise_bound(S, n + extra)
        bad = err > bound
        assert not bad.any(), (r["id"], name, int(np.argmax(bad)), float(err[bad].max()))
        worst = max(worst, float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0))))
    # the descriptor's shifts are not part of the build, and a second run gives the same bytes
    gc2, gh2 = galerkin_device(r, clover, hopping, P, R, SHIFTS)
    assert same_bytes(gc2, gc) and same_bytes(gh2, gh), (r["id"], "the shifts of the fine descriptor changed the build")
    report(r, err_over_bound=worst)


def run_galerkin_refused(r):
    fLx, fLy, fnc = r["fdims"]
    cLx, cLy, cnc = r["cdims"]
    ccm = cLx * cLy * cnc * cnc
    nfs = fLx * fLy * fnc
    dcl, dho, dP = D(cs.gaussian_cvec(fLx * fLy * fnc * fnc, 1)), D(cs.gaussian_cvec(4 * fLx * fLy * fnc * fnc, 2)), D(cs.gaussian_cvec(cnc * nfs, 3))
    halo = D(cs.gaussian_cvec(cnc * fLx * fnc, 4))
    gd = qmg.make_desc(fLx, fLy, fnc, dcl, dho)
    gcc, gch = nan_array(ccm), nan_array(4 * ccm)
    before = (gcc.to_host(), gch.to_host())
    rc = qmg.lib().qmg_coarse_build_slab(qmg._vp(gcc), qmg._vp(gch), C.byref(gd), qmg._vp(dP), None, cLx, cLy, cnc, qmg._vp(halo), qmg._vp(halo), C.c_size_t(fLx * fnc), None)
    assert rc == 3, rc
    qmg.sync()
    assert same_bytes(gcc.to_host(), before[0]) and same_bytes(gch.to_host(), before[1])
    report(r, refused=rc)


def run_galerkin_strided(r):
    """fnc = cnc = 1, 2 x 2 blocks: every coarse entry is a sum of at most 12 products of three numbers.  All of them in long double."""
    fdims, cdims = r["fdims"], r["cdims"]
    vol = fdims[0] * fdims[1]
    clover, hopping, P = cs.gaussian_cvec(vol, r["seed"]), cs.gaussian_cvec(4 * vol, r["seed"] + 100), cs.gaussian_cvec(vol, r["seed"] + 200)
    (wc, wh), (Sc, Sh), (nc_, nh) = su.galerkin(fdims, cdims, clover, hopping, P, None)
    rr = dict(r, sep_r=False)
    gc, gh = galerkin_device(rr, clover, hopping, P, None, SHIFTS)
    worst = 0.0
    for name, got, want, S, n in (("clover", gc, wc, Sc, nc_), ("hopping", gh, wh, Sh, nh)):
        assert np.all(np.isfinite(got)), (name, int(np.count_nonzero(~np.isfinite(got))))
        err, bound = np.abs(got - want), sn.elementwise_bound(S, n)
        assert np.all(err <= bound), (name, int(np.argmax(err > bound)))
        worst = max(worst, float(np.max(err / bound)))
    report(r, err_over_bound=worst, coarse_sites=cdims[0] * cdims[1])


def jacobi_device(r, clover, hopping):
    (Lx, Ly), nc = r["dims"], r["nc"]
    cm = Lx * Ly * nc * nc
    dcl, dho = (None if clover is None else D(clover)), (None if hopping is None else D(hopping))
    gd = qmg.make_desc(Lx, Ly, nc, dcl, dho, *r["shifts"])
    gci, grc, grh = nan_array(cm), nan_array(cm), (nan_array(4 * cm) if r.get("rb_hopping", True) else None)
    rc = qmg.lib().qmg_build_rbjacobi(qmg._vp(gci), qmg._vp(grc), qmg._vp(grh), C.byref(gd), None)
    qmg.sync()
    for dev, host in ((dcl, clover), (dho, hopping)):
        assert dev is None or same_bytes(dev.to_host(), host), (r["id"], "a read-only operand changed")
    return rc, gci.to_host(), grc.to_host(), (None if grh is None else grh.to_host())


def run_jacobi(r):
    (Lx, Ly), nc = r["dims"], r["nc"]
    vol = Lx * Ly
    clover, hopping = jacobi_inputs(r)
    want, cond = su.clover_inverse(Lx, Ly, nc, clover, *r["shifts"])
    assert cond.max() <= COND_CAP
    rc, cinv, rcl, rho = jacobi_device(r, clover, hopping)
    assert rc == 0, rc
    W, G = np.asarray(want).reshape(vol, nc * nc), cinv.reshape(vol, nc * nc).astype(su.CLD)
    err, nrm = np.sqrt(np.sum(np.abs(G - W) ** 2, axis=1)), np.sqrt(np.sum(np.abs(W) ** 2, axis=1))
    assert np.all(err <= TOL_SETUP * nrm), (r["id"], "cinv", int(np.argmax(err / nrm)), float((err / nrm).max()))
    assert same_bytes(rcl, np.tile(np.eye(nc, dtype=np.complex128).reshape(-1), vol)), (r["id"], "rb_clover is not the identity bit for bit")
    hop = 0.0
    if rho is not None and hopping is not None:
        wrh, S = su.rb_hopping(Lx, Ly, nc, hopping, cinv)          # from the cinv the device left
        e, bound = np.abs(rho - wrh), sn.elementwise_bound(S, nc)
        assert np.all(e <= bound), (r["id"], "rb_hopping", int(np.argmax(e > bound)))
        hop = float(np.max(e / bound))
    elif rho is not None:
        assert np.all(np.isnan(rho)), (r["id"], "rb_hopping written without a fine hopping")
    rc2, cinv2, rcl2, rho2 = jacobi_device(r, clover, hopping)
    assert rc2 == 0 and same_bytes(cinv2, cinv) and same_bytes(rcl2, rcl) and (rho is None or same_bytes(rho2, rho)), (r["id"], "second run")
    report(r, cinv=float((err / nrm).max() / TOL_SETUP), rb_hopping=hop, cond=float(cond.max()))


def run_jacobi_refused(r):
    (Lx, Ly), nc = r["dims"], r["nc"]
    clover = cs.gaussian_cvec(Lx * Ly * nc * nc, 1) if r["clover"] else None
    hopping = cs.gaussian_cvec(4 * Lx * Ly * nc * nc, 2)
    rc, cinv, rcl, rho = jacobi_device(dict(r, rb_hopping=True), clover, hopping)
    assert rc == (3 if r["expect"] == UNSUPPORTED else 1), rc
    assert np.all(np.isnan(cinv)) and np.all(np.isnan(rcl)) and np.all(np.isnan(rho)), (r["id"], "a refused build wrote an output")
    report(r, refused=rc)


def run_dagger(r):
    (Lx, Ly), nc = r["dims"], r["nc"]
    vol = Lx * Ly
    clover, hopping = cs.gaussian_cvec(vol * nc * nc, r["seed"]), cs.gaussian_cvec(4 * vol * nc * nc, r["seed"] + 1)
    wc, wh = su.dagger(Lx, Ly, nc, clover, hopping)
    dcl, dho = D(clover), D(hopping)
    out = {}
    for rep in (0, 1):
        gdc, gdh, gct = nan_array(clover.size), nan_array(hopping.size), nan_array(hopping.size)
        qmg.build_dagger(gdc, gdh, dcl, dho, Lx, Ly, nc)
        qmg.cmat_conjtrans(gct, dho, 4 * vol, nc)
        out[rep] = (gdc.to_host(), gdh.to_host(), gct.to_host())
    assert same_bytes(out[0][0], wc) and same_bytes(out[0][1], wh), (r["id"], "build_dagger")
    assert same_bytes(out[0][2], su.conjtrans(hopping, 4 * vol, nc)), (r["id"], "cmat_conjtrans")
    assert all(same_bytes(a, b) for a, b in zip(out[0], out[1])), (r["id"], "second run")
    assert same_bytes(dcl.to_host(), clover) and same_bytes(dho.to_host(), hopping)
    # one field alone: the other output stays as it was
    gdc, gdh = nan_array(clover.size), nan_array(hopping.size)
    qmg.build_dagger(gdc, gdh, None, dho, Lx, Ly, nc)
    assert np.all(np.isnan(gdc.to_host())) and same_bytes(gdh.to_host(), wh)
    gdc, gdh = nan_array(clover.size), nan_array(hopping.size)
    qmg.build_dagger(gdc, gdh, dcl, None, Lx, Ly, nc)
    assert same_bytes(gdc.to_host(), wc) and np.all(np.isnan(gdh.to_host()))
    report(r, bit_for_bit=1)


def run_biortho(r):
    fdims, cdims = r["fdims"], r["cdims"]
    nvec = cdims[2]
    fsize = fdims[0] * fdims[1] * fdims[2]
    cm = cdims[0] * cdims[1] * nvec * nvec
    pv = cs.gaussian_cvec(nvec * fsize, r["seed"])
    rv = pv + 0.3 * cs.gaussian_cvec(nvec * fsize, r["seed"] + 1)
    wp, wr, L, U = su.bi_ortho(pv, rv, fdims, cdims)
    G0 = su.block_gram(rv, pv, fdims, cdims)
    out = {}
    for rep in (0, 1):
        dp, dr, dL, dU = D(pv), D(rv), D(np.full(cm, SENTINEL)), D(np.full(cm, SENTINEL))
        qmg.block_bi_orthonormalize(dp, dr, nvec, fdims, cdims[0], cdims[1], dL, dU)
        out[rep] = (dp.to_host(), dr.to_host(), dL.to_host(), dU.to_host())
    gp, gr, gL, gU = out[0]
    assert all(same_bytes(a, b) for a, b in zip(out[0], out[1])), (r["id"], "second run")
    eye = np.eye(nvec)
    defect = np.abs(su.block_gram(gr, gp, fdims, cdims) - eye)
    assert defect.max() <= TOL_SETUP, (r["id"], "R^dag P", float(defect.max()))
    lower = np.tril(np.ones((nvec, nvec), dtype=bool), -1)
    Lg, Ug = su.coarse_mats_to_grid(gL, cdims, nvec), su.coarse_mats_to_grid(gU, cdims, nvec)
    # what the passes do not write keeps the sentinel; L is conjugated as a whole at the end (transfer.h:763), its unwritten entries included
    assert same_bytes(Lg[:, :, lower.T], np.full(Lg[:, :, lower.T].shape, np.conj(SENTINEL))) and same_bytes(Ug[:, :, lower], np.full(Ug[:, :, lower].shape, SENTINEL))
    Lz, Uz = np.where(lower.T, 0, Lg).astype(su.CLD), np.where(lower, 0, Ug).astype(su.CLD)
    lu = np.abs(np.einsum("xyik,xykj->xyij", Lz, Uz) - G0)
    assert np.all(lu <= 1e-10 * (1 + np.abs(G0))), (r["id"], "L U", float(lu.max()))
    worst = 0.0
    for got, want in ((gp, wp), (gr, wr)):
        Tg, Tw = su.tiles(got, nvec, fdims, cdims), su.tiles(want, nvec, fdims, cdims)
        e, nrm = np.sqrt(np.sum(np.abs(Tg - Tw) ** 2, axis=-1)), np.sqrt(np.sum(np.abs(Tw) ** 2, axis=-1))
        assert np.all(e <= TOL_BIORTHO * nrm), (r["id"], "vectors", float((e / nrm).max()))
        worst = max(worst, float((e / nrm).max() / TOL_BIORTHO))
    for got, want in ((Lz, L), (Uz, U)):
        e, nrm = np.sqrt(np.sum(np.abs(got - want) ** 2, axis=(2, 3))), np.sqrt(np.sum(np.abs(want) ** 2, axis=(2, 3)))
        assert np.all(e <= TOL_BIORTHO * nrm), (r["id"], "factors", float((e / nrm).max()))
        worst = max(worst, float((e / nrm).max() / TOL_BIORTHO))
    report(r, RdagP=float(defect.max() / TOL_SETUP), LU=float(np.max(lu / (1e-10 * (1 + np.abs(G0))))), vec_and_factors=worst)


RUN = dict(ortho=run_ortho, ortho_strided=run_ortho_strided, galerkin=run_galerkin, galerkin_refused=run_galerkin_refused, galerkin_strided=run_galerkin_strided,
           jacobi=run_jacobi, jacobi_refused=run_jacobi_refused, dagger=run_dagger, biortho=run_biortho)


@pytest.mark.parametrize("r", ROUTES, ids=[r["id"] for r in ROUTES])
def test_route(r):
    try:
        qmg.set_tuning("setup_fused", r["fused"])
        if r["expect"] is not None:
            assert combo(requested_plan(r)) == r["expect"], (r["id"], requested_plan(r))
        RUN[r["op"]](r)
    except qmg.QmgError as e:
        pytest.exit("%s: %s -- a failed HIP call ends the session, nothing more is started on the device" % (r["id"], e), returncode=3)
    finally:
        qmg.set_tuning("setup_fused", 1)
