"""Independent statement of the domain-wall measurements (csrc/qmg_dwf_meas.hip, include/qmg/dwf_measure.hpp) on coordinate grids
psi[x, y, s, sigma] in long double: the wall source, the wall and midpoint projections, the slice norms, the correlators built on them and
the integrated axial Ward identity.  Data enters and leaves through stencil_numpy.to_grid / to_eo; nothing shares the kernels' index
arithmetic.  sigma = 0 is the P_+ component (it hops s -> s+1 and crosses the wall as out(0, 0) += m psi(Ls-1, 0)), sigma = 1 is P_-.

    wall source     B(x; 0, 0) = eta(x, 0),  B(x; Ls-1, 1) = eta(x, 1),  zero elsewhere
    physical q      q(x, 0) = Psi(x; Ls-1, 0),  q(x, 1) = Psi(x; 0, 1)
    midpoint q      q(x, 0) = Psi(x; Ls/2-1, 0),  q(x, 1) = Psi(x; Ls/2, 1)
    slice norms     N(y, s, sigma) = sum_x |Psi(x, y; s, sigma)|^2
    Ward identity   m |q|^2 + |q_mp|^2 = Re <eta, q>      for Psi = D^-1 B, even Ls, real m, on every gauge field
"""
import numpy as np

import stencil_numpy as sn

CLD = sn.CLD


# ---- on grids
def source_grid(eta, Ls):
    """eta[x, y, sigma] -> B[x, y, s, sigma]"""
    B = np.zeros(eta.shape[:2] + (Ls, 2), dtype=eta.dtype)
    B[:, :, 0, 0] = eta[:, :, 0]
    B[:, :, Ls - 1, 1] = eta[:, :, 1]
    return B


def wall_slices(Ls, which):
    """(slice of sigma 0, slice of sigma 1): 'wall', 'mid', or 'wrong' -- the other midpoint pairing, which the identity rejects"""
    return {"wall": (Ls - 1, 0), "mid": (Ls // 2 - 1, Ls // 2), "wrong": (Ls // 2, Ls // 2 - 1)}[which]


def project_grid(psi, which="wall"):
    """psi[x, y, s, sigma] -> q[x, y, sigma]"""
    s0, s1 = wall_slices(psi.shape[2], which)
    return np.stack([psi[:, :, s0, 0], psi[:, :, s1, 1]], axis=-1)


def norms_grid(psi):
    """N[y, s, sigma] in long double"""
    p = psi.astype(CLD)
    return (p.real * p.real + p.imag * p.imag).sum(axis=0)


def ward_grid(eta, psi, m, mid="mid"):
    """(lhs, rhs) = (m |q|^2 + |q_mp|^2, Re <eta, q>)"""
    q, qm = project_grid(psi, "wall"), project_grid(psi, mid)
    return m * np.sum(np.abs(q) ** 2) + np.sum(np.abs(qm) ** 2), np.sum(np.conj(eta) * q).real


def correlators(N):
    """(C_pi[t], C_mp[t], profile[s]) of slice norms N[y, s, sigma] already summed over the source spins; the profile sums to 1"""
    Ls = N.shape[1]
    (w0, w1), (m0, m1) = wall_slices(Ls, "wall"), wall_slices(Ls, "mid")
    prof = N.sum(axis=(0, 2))
    return N[:, w0, 0] + N[:, w1, 1], N[:, m0, 0] + N[:, m1, 1], prof / prof.sum()


# ---- on the flat (eo, y, x, c) arrays the kernels take; the values pass through unchanged, so the result in the input's dtype is exact
def grid5(v, Lx, Ly, Ls):
    return sn.to_grid(v, Lx, Ly, 2 * Ls).reshape(Lx, Ly, Ls, 2)


def wall_source(eta, Lx, Ly, Ls):
    B = source_grid(sn.to_grid(eta, Lx, Ly, 2), Ls)
    return sn.to_eo(B.reshape(Lx, Ly, 2 * Ls), Lx, Ly, 2 * Ls).astype(np.asarray(eta).dtype)


def wall_project(psi, Lx, Ly, Ls, which="wall"):
    return sn.to_eo(project_grid(grid5(psi, Lx, Ly, Ls), which), Lx, Ly, 2).astype(np.asarray(psi).dtype)


def slice_norms(psi, Lx, Ly, Ls):
    return norms_grid(grid5(psi, Lx, Ly, Ls))
