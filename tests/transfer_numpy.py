"""Independent statement of restrict and prolong (transfer/transfer.h:455-511) in np.longdouble complex arithmetic on coordinate grids.

Nothing here shares the index arithmetic of the device kernels or of the oracle's coarse map (ol.transfer_build_map is not used): a
vector is moved to psi[x, y, c] with coordspace.eo_to_grid, the blocks are the regular (fLx/cLx) x (fLy/cLy) rectangles cut out by a
reshape, and the result goes back through coordspace.grid_to_eo's layout.  Both forms accumulate, as the kernels do:

    restrict   coarse[X, Y, d] += sum_{(x, y) in block (X, Y), c} conj(null[d][x, y, c]) fine[x, y, c]
    prolong    fine[x, y, c]   += sum_d null[d][x, y, c] coarse[x // bx, y // by, d]

Next to each result comes the term-magnitude sum S = |out0| + sum |n| |v| per output element, the scale of the standard summation
bound that the route tests (test_gpu_transfer_routes.py) hold the kernels to.
"""
import numpy as np

import coordspace as cs

CLD = np.clongdouble


def _to_grid(v, Lx, Ly, nc):
    return cs.eo_to_grid(np.asarray(v).astype(CLD), Lx, Ly, nc)


def _to_eo(psi, Lx, Ly, nc):
    """psi[x, y, c] -> flat (eo, y, x, c) vector, keeping psi's dtype: grid_to_eo applied to the grid's own flat positions gives the
    permutation (exact: integers far below 2^53)."""
    pos = np.arange(Lx * Ly * nc, dtype=np.float64).reshape(Lx, Ly, nc)
    perm = np.rint(cs.grid_to_eo(pos, Lx, Ly, nc).real).astype(np.int64)
    return psi.reshape(-1)[perm]


_LAST = []   # the grids of the null vectors last asked for: a batch row asks once per system with the same array


def _null_grid(nullvecs, nvec, fdims):
    """(null, conj(null), |null|) as [d, x, y, c] grids"""
    if _LAST and _LAST[0] is nullvecs and _LAST[1] == (nvec, fdims):
        return _LAST[2]
    fLx, fLy, fnc = fdims
    fsize = fLx * fLy * fnc
    N = np.stack([_to_grid(nullvecs[d * fsize:(d + 1) * fsize], fLx, fLy, fnc) for d in range(nvec)])
    _LAST[:] = [nullvecs, (nvec, fdims), (N, np.conj(N), np.abs(N))]
    return _LAST[2]


def restrict(nullvecs, fine, fdims, cdims, coarse0):
    """(coarse0 + R fine, S) as flat coarse vectors (complex longdouble, longdouble)."""
    fLx, fLy, fnc = fdims
    cLx, cLy, nvec = cdims
    bx, by = fLx // cLx, fLy // cLy
    _, Nc, Na = (a.reshape(nvec, cLx, bx, cLy, by, fnc) for a in _null_grid(nullvecs, nvec, fdims))
    F = _to_grid(fine, fLx, fLy, fnc).reshape(cLx, bx, cLy, by, fnc)
    C0 = _to_grid(coarse0, cLx, cLy, nvec)
    out = C0 + np.einsum("dxiyjc,xiyjc->xyd", Nc, F)
    S = np.abs(C0) + np.einsum("dxiyjc,xiyjc->xyd", Na, np.abs(F))
    return _to_eo(out, cLx, cLy, nvec), _to_eo(S, cLx, cLy, nvec)


def prolong(nullvecs, coarse, fdims, cdims, fine0):
    """(fine0 + P coarse, S) as flat fine vectors (complex longdouble, longdouble)."""
    fLx, fLy, fnc = fdims
    cLx, cLy, nvec = cdims
    bx, by = fLx // cLx, fLy // cLy
    N, _, Na = _null_grid(nullvecs, nvec, fdims)
    C = np.repeat(np.repeat(_to_grid(coarse, cLx, cLy, nvec), bx, axis=0), by, axis=1)   # coarse[x // bx, y // by, d] on the fine grid
    F0 = _to_grid(fine0, fLx, fLy, fnc)
    out = F0 + np.einsum("dxyc,xyd->xyc", N, C)
    S = np.abs(F0) + np.einsum("dxyc,xyd->xyc", Na, np.abs(C))
    return _to_eo(out, fLx, fLy, fnc), _to_eo(S, fLx, fLy, fnc)


def sum_length(op, fdims, cdims):
    """nel of the elementwise bound: the number of terms in one output element's sum"""
    if op == "restrict":
        return (fdims[0] // cdims[0]) * (fdims[1] // cdims[1]) * fdims[2]
    return cdims[2]


def elementwise_bound(op, fdims, cdims, S, want=None):
    """|got - want| <= (nel + 1) 2^-50 S for fp64 results; complex<float> results (want given) add one rounding of the result with a
    factor 2: 2^-23 |want|.  (The standard summation bound is nel 2^-53 S; 8x over it leaves room for FMA contraction and the matrix
    cores' own order.)"""
    b = (sum_length(op, fdims, cdims) + 1) * 2.0 ** -50 * S
    if want is not None:
        b = b + 2.0 ** -23 * np.abs(want)
    return b
