"""Independent statement of the multigrid SETUP operations in np.clongdouble arithmetic on coordinate grids: block orthonormalisation
(transfer/transfer.h:514-607), block bi-orthonormalisation (:610-769), the Galerkin coarse operator (operators/coarse.h:137-444), the
right-block-Jacobi inverse and hops (stencil/stencil_2d.h:1452-1601) and the dagger build (:1080-1139).

Arrays are indexed [x, y, colour].  They come from and go back to the even-odd storage layout through coordspace / stencil_numpy.to_eo
only; a block is a slice of the grid (x = X bx + lx, y = Y by + ly: a reshape), a neighbour is np.roll.  There is no block map and no index
arithmetic shared with the kernels (csrc/qmg_setup.hip, csrc/qmg_fill.hip, csrc/qmg_transfer.hip) or the oracle (oracle/qmg_oracle.cpp).
tests/test_host_setup_plan.py holds every function here to the oracle at 1e-12, so that a failure of a GPU row
(tests/test_gpu_setup_routes.py) has a known side.
"""
import numpy as np

import coordspace as cs
import stencil_numpy as sn

CLD = np.clongdouble
LD = np.longdouble


# ---- layout: flat even-odd arrays <-> grids and block tiles
def vecs_to_grid(v, nvec, fdims):
    """nvec vector-major fine vectors -> V[d, x, y, c] (complex long double)"""
    Lx, Ly, nc = fdims
    v = np.asarray(v).reshape(nvec, Lx * Ly * nc)
    return np.stack([sn.to_grid(v[d], Lx, Ly, nc) for d in range(nvec)])


def grid_to_vecs(V, fdims):
    Lx, Ly, nc = fdims
    return np.concatenate([sn.to_eo(V[d], Lx, Ly, nc) for d in range(V.shape[0])])


def grid_to_tiles(V, fdims, cdims):
    """V[d, x, y, c] -> T[X, Y, d, e]: the nvec x nel tile of every block, e running over (lx, ly, c)"""
    fLx, fLy, fnc = fdims
    cLx, cLy = cdims[0], cdims[1]
    bx, by = fLx // cLx, fLy // cLy
    nvec = V.shape[0]
    return V.reshape(nvec, cLx, bx, cLy, by, fnc).transpose(1, 3, 0, 2, 4, 5).reshape(cLx, cLy, nvec, bx * by * fnc)


def tiles_to_grid(T, fdims, cdims):
    fLx, fLy, fnc = fdims
    cLx, cLy = cdims[0], cdims[1]
    bx, by = fLx // cLx, fLy // cLy
    nvec = T.shape[2]
    return T.reshape(cLx, cLy, nvec, bx, by, fnc).transpose(2, 0, 3, 1, 4, 5).reshape(nvec, fLx, fLy, fnc)


def tiles(v, nvec, fdims, cdims):
    """flat fine vectors -> T[X, Y, d, e]"""
    return grid_to_tiles(vecs_to_grid(v, nvec, fdims), fdims, cdims)


def coarse_mats_to_grid(m, cdims, n):
    """flat coarse field of n x n matrices (eo, y, x, r, c) -> M[X, Y, r, c], keeping m's dtype (a pure permutation)"""
    cLx, cLy = cdims[0], cdims[1]
    pos = np.arange(cLx * cLy * n * n, dtype=np.float64)
    idx = np.rint(cs.eo_to_grid(pos, cLx, cLy, n * n).real).astype(np.int64)
    return np.asarray(m).reshape(-1)[idx].reshape(cLx, cLy, n, n)


def coarse_mats_to_eo(M):
    cLx, cLy, n = M.shape[0], M.shape[1], M.shape[2]
    return sn.to_eo(M.reshape(cLx, cLy, n * n), cLx, cLy, n * n)


def _bdot(a, b):
    """<a, b> per block: sum_e conj(a) b over the last axis"""
    return np.sum(np.conj(a) * b, axis=-1)


# ---- block orthonormalisation
def block_qr(nullvecs, fdims, cdims, passes=1):
    """Modified Gram-Schmidt per block in the reference's order (transfer.h:548-593): for i: for j < i: c = <v_j, v_i> with the CURRENT v_i,
    v_i -= c v_j; then v_i /= |v_i|.  `passes` = 2 runs it twice (:160-174).
    Returns (vectors flat, factor[X, Y, j, i] of the FIRST pass: c at (j, i) for j < i, |v_i| real positive on the diagonal, zero below,
    cond[X, Y]: the 2-norm condition number of every block's nel x nvec tile of the input)."""
    nvec = cdims[2]
    T = tiles(nullvecs, nvec, fdims, cdims).copy()
    cond = np.linalg.cond(np.swapaxes(T.astype(np.complex128), 2, 3))
    Rf = np.zeros(T.shape[:2] + (nvec, nvec), dtype=CLD)
    for p in range(passes):
        for i in range(nvec):
            for j in range(i):
                c = _bdot(T[:, :, j], T[:, :, i])
                if p == 0:
                    Rf[:, :, j, i] = c
                T[:, :, i] = T[:, :, i] - c[:, :, None] * T[:, :, j]
            nrm = np.sqrt(_bdot(T[:, :, i], T[:, :, i]).real)
            if p == 0:
                Rf[:, :, i, i] = nrm
            T[:, :, i] = T[:, :, i] / nrm[:, :, None]
    return grid_to_vecs(tiles_to_grid(T, fdims, cdims), fdims), Rf, cond


def bi_ortho(pvecs, rvecs, fdims, cdims):
    """The asymmetric counterpart (transfer.h:610-769), one pass: afterwards <r_i, p_j> = delta_ij per block.
    Returns (P flat, R flat, L[X, Y, i, j], U[X, Y, j, i]) with L lower and U upper triangular, L U = the block Gram matrix <r_i, p_j> of the
    input."""
    nvec = cdims[2]
    P = tiles(pvecs, nvec, fdims, cdims).copy()
    R = tiles(rvecs, nvec, fdims, cdims).copy()
    L = np.zeros(P.shape[:2] + (nvec, nvec), dtype=CLD)
    U = np.zeros_like(L)
    for i in range(nvec):
        for j in range(i):
            c = _bdot(R[:, :, j], P[:, :, i])            # <r_j, p_i>  (:647)
            U[:, :, j, i] = c
            P[:, :, i] = P[:, :, i] - c[:, :, None] * P[:, :, j]
            c = _bdot(P[:, :, j], R[:, :, i])            # <p_j, r_i>  (:672), stored conjugated (:763)
            L[:, :, i, j] = np.conj(c)
            R[:, :, i] = R[:, :, i] - c[:, :, None] * R[:, :, j]
        d = _bdot(R[:, :, i], P[:, :, i])                # <r_i, p_i>  (:703)
        a = np.abs(d)
        z = d / (a * np.sqrt(a))                         # polar(1 / sqrt|d|, arg d)  (:376-380)
        L[:, :, i, i] = np.conj(1 / z)                   # :712-722, :763
        R[:, :, i] = z[:, :, None] * R[:, :, i]
        U[:, :, i, i] = np.sqrt(a)                       # 1 / |z|  (:736-745)
        P[:, :, i] = P[:, :, i] / np.sqrt(a)[:, :, None]
    back = lambda T: grid_to_vecs(tiles_to_grid(T, fdims, cdims), fdims)
    return back(P), back(R), L, U


def block_gram(rvecs, pvecs, fdims, cdims):
    """G[X, Y, i, j] = <r_i, p_j> per block"""
    nvec = cdims[2]
    R, P = tiles(rvecs, nvec, fdims, cdims), tiles(pvecs, nvec, fdims, cdims)
    return np.einsum("xyie,xyje->xyij", np.conj(R), P)


# ---- the Galerkin coarse operator
def galerkin(fdims, cdims, clover, hopping, P, R=None):
    """C(X) = sum_{x in B_X} R(x)^dag [A(x) P(x) + sum_{mu: x + mu in B_X} H_mu(x) P(x + mu)],
    H_mu(X) = sum_{x in B_X: x + mu not in B_X} R(x)^dag H_mu(x) P(x + mu)          (coarse.h:222-252),
    with periodic neighbours from coordinates; a missing clover or hopping counts as zero; the descriptor's shifts are not part of the
    build (coarse.h:131).  R = None: the restrictor is the prolongator.
    Returns ((clover, hopping), (S_clover, S_hopping), (n_clover, n_hopping)) as flat coarse fields (eo, Y, X, a, b) / (mu, eo, Y, X, a, b):
    the value, the term-magnitude sum S = sum |R| |M| |P| and the term count n = fnc + the number of (x, piece, r) contributions."""
    fLx, fLy, fnc = fdims
    cLx, cLy, cnc = cdims
    bx, by = fLx // cLx, fLy // cLy
    Pg = vecs_to_grid(P, cnc, fdims)
    Rg = Pg if R is None else vecs_to_grid(R, cnc, fdims)
    Cg, Hg = sn.matrix_grids(fLx, fLy, fnc, clover, hopping)
    Rc, aR, aP = np.conj(Rg), np.abs(Rg), np.abs(Pg)
    bsum = lambda K: K.reshape(cLx, bx, cLy, by, cnc, cnc).sum(axis=(1, 3))
    zero = lambda dt: np.zeros((cLx, cLy, cnc, cnc), dtype=dt)
    val = [zero(CLD) for _ in range(5)]
    S = [zero(LD) for _ in range(5)]
    n = [np.full((cLx, cLy, cnc, cnc), fnc, dtype=np.int64) for _ in range(5)]
    xs, ys = np.meshgrid(np.arange(fLx), np.arange(fLy), indexing="ij")
    rmp = lambda Rx, M, Pn: np.einsum("axyr,xyrb->xyab", Rx, np.einsum("xyrc,bxyc->xyrb", M, Pn))   # R(x)^dag [M(x) P(nb)] per fine site
    if Cg is not None:
        val[0] = val[0] + bsum(rmp(Rc, Cg, Pg))
        S[0] = S[0] + bsum(rmp(aR, np.abs(Cg), aP))
        n[0] = n[0] + bx * by * fnc
    if Hg is not None:
        for mu in range(4):
            axis, step = sn.STEP[mu]
            Pn, aPn = np.roll(Pg, step, axis=1 + axis), np.roll(aP, step, axis=1 + axis)
            nx, ny = (xs - step) % fLx if axis == 0 else xs, (ys - step) % fLy if axis == 1 else ys   # the site psi((x, y) + mu) came from
            inside = ((nx // bx == xs // bx) & (ny // by == ys // by))
            K = rmp(Rc, Hg[mu], Pn)
            KS = rmp(aR, np.abs(Hg[mu]), aPn)
            m_in = inside[:, :, None, None]
            val[0] = val[0] + bsum(K * m_in)
            S[0] = S[0] + bsum(KS * m_in)
            val[1 + mu] = val[1 + mu] + bsum(K * ~m_in)
            S[1 + mu] = S[1 + mu] + bsum(KS * ~m_in)
            cnt = inside.reshape(cLx, bx, cLy, by).sum(axis=(1, 3))[:, :, None, None]
            n[0] = n[0] + cnt * fnc
            n[1 + mu] = n[1 + mu] + (bx * by - cnt) * fnc
    pack = lambda A: (coarse_mats_to_eo(A[0]), np.concatenate([coarse_mats_to_eo(A[1 + mu]) for mu in range(4)]))
    return pack(val), pack(S), pack(n)


# ---- right block Jacobi
def shifted_clover(Lx, Ly, nc, clover, shift=0.0, eo_shift=0.0, dof_shift=0.0):
    """C[x, y, r, c] = clover + (shift +- eo_shift (+ even, - odd sites) +- dof_shift (+ r < nc / 2, - else; zero for odd nc)) on the
    diagonal: the sign convention of stencil_2d.h as k_clover_inverse states it"""
    Cg = np.zeros((Lx, Ly, nc, nc), dtype=CLD) if clover is None else sn.to_grid(clover, Lx, Ly, nc * nc).reshape(Lx, Ly, nc, nc).copy()
    xs, ys = np.meshgrid(np.arange(Lx), np.arange(Ly), indexing="ij")
    sg = np.where((xs + ys) & 1, -1.0, 1.0).astype(LD)[:, :, None]
    dg = (np.where(np.arange(nc) < nc // 2, 1.0, -1.0) if nc % 2 == 0 else np.zeros(nc)).astype(LD)[None, None, :]
    diag = CLD(shift) + sg * CLD(eo_shift) + dg * CLD(dof_shift)
    Cg[:, :, np.arange(nc), np.arange(nc)] += diag
    return Cg


def clover_inverse(Lx, Ly, nc, clover, shift=0.0, eo_shift=0.0, dof_shift=0.0):
    """Per site the inverse of the shifted clover: np.linalg.inv in float64, then two Newton steps X <- X (2 - C X) in long double -- quadratic
    convergence from a 1e-15 cond start, independent of any elimination order.  Returns (cinv flat (eo, y, x, r, c), cond[x, y])."""
    Cg = shifted_clover(Lx, Ly, nc, clover, shift, eo_shift, dof_shift)
    C64 = Cg.astype(np.complex128)
    X = np.linalg.inv(C64).astype(CLD)
    two = 2 * np.eye(nc, dtype=CLD)
    for _ in range(2):
        X = np.einsum("xyrk,xykc->xyrc", X, two - np.einsum("xyrk,xykc->xyrc", Cg, X))
    return sn.to_eo(X.reshape(Lx, Ly, nc * nc), Lx, Ly, nc * nc), np.linalg.cond(C64)


def rb_hopping(Lx, Ly, nc, hopping, cinv):
    """rb_mu(x) = H_mu(x) cinv(x + mu) (stencil_2d.h:1556-1581).  Returns (value, S = |H| |cinv|) as flat (mu, eo, y, x, r, c) fields."""
    _, Hg = sn.matrix_grids(Lx, Ly, nc, None, hopping)
    Xg = sn.to_grid(cinv, Lx, Ly, nc * nc).reshape(Lx, Ly, nc, nc)
    val, S = [], []
    for mu in range(4):
        axis, step = sn.STEP[mu]
        Xn = np.roll(Xg, step, axis=axis)
        val.append(sn.to_eo(np.einsum("xyrk,xykc->xyrc", Hg[mu], Xn).reshape(Lx, Ly, nc * nc), Lx, Ly, nc * nc))
        S.append(sn.to_eo(np.einsum("xyrk,xykc->xyrc", np.abs(Hg[mu]), np.abs(Xn)).reshape(Lx, Ly, nc * nc), Lx, Ly, nc * nc))
    return np.concatenate(val), np.concatenate(S)


def dagger(Lx, Ly, nc, clover, hopping):
    """C'(x) = C(x)^H, H'_mu(x) = H_{-mu}(x + mu)^H (stencil_2d.h:1080-1139) in complex128: pure data movement, exact.  A missing field
    gives None."""
    vol = Lx * Ly * nc * nc
    grid = lambda m: cs.eo_to_grid(np.asarray(m, dtype=np.complex128), Lx, Ly, nc * nc).reshape(Lx, Ly, nc, nc)
    back = lambda M: cs.grid_to_eo(np.conj(np.swapaxes(M, 2, 3)).reshape(Lx, Ly, nc * nc), Lx, Ly, nc * nc)
    dc = None if clover is None else back(grid(clover))
    dh = None
    if hopping is not None:
        Hg = [grid(np.asarray(hopping)[mu * vol:(mu + 1) * vol]) for mu in range(4)]
        dh = np.concatenate([back(np.roll(Hg[(mu + 2) % 4], sn.STEP[mu][1], axis=sn.STEP[mu][0])) for mu in range(4)])
    return dc, dh


def conjtrans(m, nsite, nc):
    return np.conj(np.swapaxes(np.asarray(m).reshape(nsite, nc, nc), 1, 2)).reshape(-1)
