"""Independent statement of the stencil apply  lhs (+)= pieces(M) rhs  (stencil/stencil_2d.h:666-936) in np.clongdouble arithmetic on
coordinate grids.

Nothing here shares the even-odd index arithmetic of the device kernels or of the oracle's cshift: vectors and matrix fields are moved to
psi[x, y, c] and M[x, y, r, c] with coordspace.eo_to_grid (a matrix field is a vector of nc * nc numbers per site), a neighbour is np.roll,
and the result goes back through coordspace.grid_to_eo's layout.  With p(x, y) = (x + y) & 1 the parity of the OUTPUT site and the hopping
fields mu = {+x, +y, -x, -y} (include/qmg_hip.h:58):

    out(x, y) = (ZERO_p ? 0 : lhs0(x, y))
              + [CLOVER_p]      C(x, y) rhs(x, y)                                  (clover present)
              + [EO/OE bit mu]  H_mu(x, y) rhs((x, y) + mu)                        (hopping present; the EO bits are the even outputs')
              + [SHIFT_p]       (shift +- eo_shift (+ even, - odd) +- dof_shift (+ c < nc / 2, - else; even nc only)) rhs(x, y)

A parity none of whose bits is set keeps lhs0.  The 1 x 1 lattice is the reference's corner form (stencil_2d.h:870-888): its half-volume
loops run zero times, so clover and hopping do nothing, the one site counts as even, and a ZERO bit of either parity clears it.

Next to the result come, per output element, the term-magnitude sum S = |lhs0| + sum |m| |x| + (|shift| + |eo_shift| + |dof_shift|) |x| and
the number of terms n (nc per matrix, 3 for the shift term): the scale and length of the standard summation bound the route tests
(test_gpu_stencil_routes.py) hold the kernels to.
"""
import numpy as np

import coordspace as cs

CLD = np.clongdouble

P_CLOVER_E, P_EO_XP1, P_OE_XP1, P_SHIFT_E, P_ZERO_E = 1 << 0, 1 << 2, 1 << 6, 1 << 10, 1 << 12   # include/qmg_hip.h; the odd bit is the next one
STEP = ((0, -1), (1, -1), (0, +1), (1, +1))   # mu -> (axis, np.roll shift) that brings psi((x, y) + mu) to (x, y)


def to_grid(v, Lx, Ly, dof):
    return cs.eo_to_grid(np.asarray(v).astype(CLD), Lx, Ly, dof)


def to_eo(psi, Lx, Ly, dof):
    """psi[x, y, dof] -> flat (eo, y, x, dof) array, keeping psi's dtype: grid_to_eo applied to the grid's own flat positions gives the
    permutation (exact: integers far below 2^53)."""
    pos = np.arange(Lx * Ly * dof, dtype=np.float64).reshape(Lx, Ly, dof)
    perm = np.rint(cs.grid_to_eo(pos, Lx, Ly, dof).real).astype(np.int64)
    return psi.reshape(-1)[perm]


def matrix_grids(Lx, Ly, nc, clover, hopping):
    """(C[x, y, r, c] or None, [H_mu[x, y, r, c]] or None) from the flat (eo, y, x, r, c) / (mu, eo, y, x, r, c) fields"""
    vol = Lx * Ly * nc * nc
    Cg = None if clover is None else to_grid(clover, Lx, Ly, nc * nc).reshape(Lx, Ly, nc, nc)
    Hg = None if hopping is None else [to_grid(np.asarray(hopping)[mu * vol:(mu + 1) * vol], Lx, Ly, nc * nc).reshape(Lx, Ly, nc, nc) for mu in range(4)]
    return Cg, Hg


_LAST = []   # the grids of the fields last applied and their magnitudes: a batch row applies the same fields once per system


def _grids_and_magnitudes(Lx, Ly, nc, clover, hopping):
    """(C, [H_mu], |C|, [|H_mu|]) of matrix_grids, kept while the next call passes the same two arrays"""
    if _LAST and _LAST[0] is clover and _LAST[1] is hopping and _LAST[2] == (Lx, Ly, nc):
        return _LAST[3]
    Cg, Hg = matrix_grids(Lx, Ly, nc, clover, hopping)
    _LAST[:] = [clover, hopping, (Lx, Ly, nc), (Cg, Hg, None if Cg is None else np.abs(Cg), None if Hg is None else [np.abs(h) for h in Hg])]
    return _LAST[3]


def apply(Lx, Ly, nc, clover, hopping, shift, eo_shift, dof_shift, pieces, rhs, lhs0):
    """(out, S, n) as flat (eo, y, x, c) arrays: complex long double, long double, int."""
    x = to_grid(rhs, Lx, Ly, nc)
    out = to_grid(lhs0, Lx, Ly, nc).copy()
    shift, eo_shift, dof_shift = CLD(shift), CLD(eo_shift), CLD(dof_shift)
    half = (np.arange(nc) < nc // 2)
    dof_sign = np.where(half, 1.0, -1.0).astype(np.longdouble) if nc % 2 == 0 else np.zeros(nc, dtype=np.longdouble)
    dof_mag = abs(dof_shift) if nc % 2 == 0 else np.longdouble(0)
    if Lx == 1 and Ly == 1:
        if pieces & (P_ZERO_E | (P_ZERO_E << 1)):
            out[:] = 0
        S, n = np.abs(out), np.zeros(out.shape, dtype=np.int64)
        if pieces & P_SHIFT_E:
            out = out + (shift + eo_shift + dof_sign * dof_shift) * x
            S = S + (abs(shift) + abs(eo_shift) + dof_mag) * np.abs(x)
            n = n + 3
        return to_eo(out, 1, 1, nc), to_eo(S, 1, 1, nc), to_eo(n, 1, 1, nc)
    Cg, Hg, Ca, Ha = _grids_and_magnitudes(Lx, Ly, nc, clover, hopping)
    xs, ys = np.meshgrid(np.arange(Lx), np.arange(Ly), indexing="ij")
    parity = (xs + ys) & 1
    for p in (0, 1):
        if pieces & (P_ZERO_E << p):
            out[parity == p] = 0
    S, n = np.abs(out), np.zeros(out.shape, dtype=np.int64)
    ax = np.abs(x)
    for p in (0, 1):
        on = (parity == p)[:, :, None]
        if Cg is not None and pieces & (P_CLOVER_E << p):
            out = out + on * np.einsum("xyrc,xyc->xyr", Cg, x)
            S = S + on * np.einsum("xyrc,xyc->xyr", Ca, ax)
            n = n + on * nc
        for mu in range(4):
            if Hg is not None and pieces & ((P_OE_XP1 if p else P_EO_XP1) << mu):
                axis, step = STEP[mu]
                out = out + on * np.einsum("xyrc,xyc->xyr", Hg[mu], np.roll(x, step, axis=axis))
                S = S + on * np.einsum("xyrc,xyc->xyr", Ha[mu], np.roll(ax, step, axis=axis))
                n = n + on * nc
        if pieces & (P_SHIFT_E << p):
            eo = eo_shift if p == 0 else -eo_shift
            out = out + on * ((shift + eo + dof_sign * dof_shift) * x)
            S = S + on * ((abs(shift) + abs(eo_shift) + dof_mag) * ax)
            n = n + on * 3
    return to_eo(out, Lx, Ly, nc), to_eo(S, Lx, Ly, nc), to_eo(n, Lx, Ly, nc)


def dagger_fields(Lx, Ly, nc, clover, hopping):
    """the flat fields of M^dagger, built on the grid: C'(x) = C(x)^H, H'_mu(x) = H_{-mu}(x + mu)^H"""
    Cg, Hg = matrix_grids(Lx, Ly, nc, clover, hopping)
    dag = lambda M: np.conj(np.swapaxes(M, 2, 3))
    cl = to_eo(dag(Cg).reshape(Lx, Ly, nc * nc), Lx, Ly, nc * nc)
    hp = []
    for mu in range(4):
        axis, step = STEP[mu]
        hp.append(to_eo(dag(np.roll(Hg[(mu + 2) % 4], step, axis=axis)).reshape(Lx, Ly, nc * nc), Lx, Ly, nc * nc))
    return cl, np.concatenate(hp)


def elementwise_bound(S, n, want=None, fp32_arithmetic=False):
    """|got - want| <= (n + 1) 2^-50 S for fp64 accumulation (the standard summation bound n 2^-53 S with the 8x room transfer_numpy grants
    for FMA contraction and the matrix cores' order); kernels that do their arithmetic in fp32: (n + 1) 2^-21 S; complex<float> results
    (want given) add one rounding of the result with a factor 2: 2^-23 |want|."""
    b = (n + 1) * (2.0 ** -21 if fp32_arithmetic else 2.0 ** -50) * S
    if want is not None:
        b = b + 2.0 ** -23 * np.abs(want)
    return b
