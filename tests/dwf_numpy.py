"""Independent statement of the Shamir domain-wall operator (operators/dwf.h) in np.clongdouble arithmetic on coordinate grids.

A field is psi[x, y, s, sigma]: s = 0 .. Ls-1 the fifth-dimension slice, sigma the spin.  Neighbours are np.roll, the fifth dimension is
written with slices, spin with the Pauli matrices; nothing shares the index arithmetic of csrc/qmg_dwf.hip.  Data enters through
coordspace.eo_to_grid and leaves through coordspace.grid_to_eo's layout (stencil_numpy.to_grid / to_eo); the flat component is
c = 2 s + sigma, i.e. the C-order reshape of the two trailing axes.

With w the Wilson coefficient, m the wall mass, U_mu the links and p(x, y) = (x + y) & 1 the parity of the OUTPUT site:

    out(x) = (ZERO_p ? 0 : lhs0(x))
           + [CLOVER_p]  3 w psi(x)  -  psi(x; s-1, 0) -> (s, 0)  -  psi(x; s+1, 1) -> (s, 1)        (inside 0 .. Ls-1)
                         + m psi(x; Ls-1, 0) -> (0, 0)  +  m psi(x; 0, 1) -> (Ls-1, 1)
           + [EO/OE +x]  1/2 U_x(x) (sigma1 - w) psi(x + x^)          [-x]  1/2 conj U_x(x - x^) (-sigma1 - w) psi(x - x^)
           + [EO/OE +y]  1/2 U_y(x) (sigma2 - w) psi(x + y^)          [-y]  1/2 conj U_y(x - y^) (-sigma2 - w) psi(x - y^)
           + [SHIFT_p]   (shift +- eo_shift (+ even, - odd) +- dof_shift (+ where 2 s + sigma < Ls, - else)) psi(x)

(the domain-wall height M5 is the shift).  Next to the result come, per output element, the term-magnitude sum S and the term count n that
stencil_numpy.elementwise_bound takes: one per nonzero term, 3 for the shift, and one more per hopping term when w != 1 (the entry w/2 U is
itself a rounded product then).
"""
import numpy as np

import stencil_numpy as sn

CLD = np.clongdouble
SIGMA = (np.array([[0, 1], [1, 0]], dtype=CLD), np.array([[0, -1j], [1j, 0]], dtype=CLD))   # sigma1, sigma2
P_CLOVER_E, P_EO_XP1, P_OE_XP1, P_SHIFT_E, P_ZERO_E = sn.P_CLOVER_E, sn.P_EO_XP1, sn.P_OE_XP1, sn.P_SHIFT_E, sn.P_ZERO_E


def link_grids(gauge, Lx, Ly, ctype=CLD):
    """U_x[x, y], U_y[x, y] from the flat (mu, eo, y, x) gauge field"""
    g = np.asarray(gauge)
    V = Lx * Ly
    return (sn.to_grid(g[:V], Lx, Ly, 1)[:, :, 0].astype(ctype), sn.to_grid(g[V:], Lx, Ly, 1)[:, :, 0].astype(ctype))


def hop_terms(Ux, Uy, w, ctype=CLD):
    """mu = +x, +y, -x, -y -> (axis, np.roll step that brings psi(x + mu) to x, link factor[x, y], 2 x 2 spin matrix)"""
    I2 = np.eye(2, dtype=ctype)
    half = ctype(0.5)
    out = []
    for mu in range(4):
        axis, sign = mu % 2, (1 if mu < 2 else -1)
        U = (Ux, Uy)[axis]
        link = U if sign > 0 else np.conj(np.roll(U, +1, axis=axis))
        out.append((axis, -sign, link, half * (sign * SIGMA[axis].astype(ctype) - ctype(w) * I2)))
    return out


def _core(x, lhs0, Ux, Uy, m, w, shift, eo_shift, dof_shift, pieces, ctype):
    """x, lhs0: [x, y, s, sigma, ...] (any trailing axes).  Returns (out, S, n) on the same grid."""
    Lx, Ly, Ls = x.shape[:3]
    rtype = np.longdouble if ctype is CLD else np.float64
    extra = (1,) * (x.ndim - 4)
    ex = lambda a, nd: np.asarray(a).reshape(np.asarray(a).shape + (1,) * (4 - nd) + extra)   # an [x, y] (nd = 2) or [x, y, s, sigma] (nd = 4) array against x
    xs, ys = np.meshgrid(np.arange(Lx), np.arange(Ly), indexing="ij")
    parity = (xs + ys) & 1
    m, shift, eo_shift, dof_shift = ctype(m), ctype(shift), ctype(eo_shift), ctype(dof_shift)
    out = np.array(lhs0, dtype=ctype, copy=True)
    for p in (0, 1):
        if pieces & (P_ZERO_E << p):
            out[parity == p] = 0
    S, n = np.abs(out), np.zeros(out.shape, dtype=np.int64)
    ax = np.abs(x)
    s_idx = np.arange(Ls)[:, None]
    g_idx = np.arange(2)[None, :]
    dof_sign = ex(np.where(2 * s_idx + g_idx < Ls, 1.0, -1.0).astype(rtype)[None, None], 4)
    for p in (0, 1):
        on = ex((parity == p), 2)
        if pieces & (P_CLOVER_E << p):
            t, ts, tn = ctype(3.0 * w) * x, abs(3.0 * w) * ax, np.ones(out.shape, dtype=np.int64)
            t[:, :, 1:, 0] -= x[:, :, :-1, 0]; ts[:, :, 1:, 0] += ax[:, :, :-1, 0]; tn[:, :, 1:, 0] += 1
            t[:, :, :-1, 1] -= x[:, :, 1:, 1]; ts[:, :, :-1, 1] += ax[:, :, 1:, 1]; tn[:, :, :-1, 1] += 1
            if m != 0:
                t[:, :, 0, 0] += m * x[:, :, Ls - 1, 0]; ts[:, :, 0, 0] += abs(m) * ax[:, :, Ls - 1, 0]; tn[:, :, 0, 0] += 1
                t[:, :, Ls - 1, 1] += m * x[:, :, 0, 1]; ts[:, :, Ls - 1, 1] += abs(m) * ax[:, :, 0, 1]; tn[:, :, Ls - 1, 1] += 1
            out, S, n = out + on * t, S + on * ts, n + on * tn
        for mu, (axis, step, link, M) in enumerate(hop_terms(Ux, Uy, w, ctype)):
            if pieces & ((P_OE_XP1 if p else P_EO_XP1) << mu):
                out = out + on * (ex(link, 2) * np.einsum("ab,xysb...->xysa...", M, np.roll(x, step, axis=axis)))
                S = S + on * (ex(np.abs(link), 2) * np.einsum("ab,xysb...->xysa...", np.abs(M), np.roll(ax, step, axis=axis)))
                n = n + on * (2 if w == 1 else 4)
        if pieces & (P_SHIFT_E << p):
            eo = eo_shift if p == 0 else -eo_shift
            out = out + on * ((shift + eo + dof_sign * dof_shift) * x)
            S = S + on * ((abs(shift) + abs(eo_shift) + abs(dof_shift)) * ax)
            n = n + on * 3
    return out, S, n


def apply(Lx, Ly, Ls, gauge, m, w, shift, eo_shift, dof_shift, pieces, rhs, lhs0):
    """(out, S, n) as flat (eo, y, x, c) arrays: complex long double, long double, int."""
    nc = 2 * Ls
    Ux, Uy = link_grids(gauge, Lx, Ly)
    x = sn.to_grid(rhs, Lx, Ly, nc).reshape(Lx, Ly, Ls, 2)
    l0 = sn.to_grid(lhs0, Lx, Ly, nc).reshape(Lx, Ly, Ls, 2)
    out, S, n = _core(x, l0, Ux, Uy, m, w, shift, eo_shift, dof_shift, pieces, CLD)
    flat = lambda a: sn.to_eo(a.reshape(Lx, Ly, nc), Lx, Ly, nc)
    return flat(out), flat(S), flat(n)


def fields(Lx, Ly, Ls, gauge, m, w):
    """The stored form: flat clover (eo, y, x, r, c) and hopping (mu, eo, y, x, r, c) fields of the nc = 2 Ls stencil, complex128 (each entry
    formed in long double and rounded once), zeros included."""
    nc = 2 * Ls
    Ux, Uy = link_grids(gauge, Lx, Ly)
    C = np.zeros((Lx, Ly, Ls, 2, Ls, 2), dtype=CLD)
    for s in range(Ls):
        for g in range(2):
            C[:, :, s, g, s, g] = 3.0 * w
    for s in range(Ls - 1):
        C[:, :, s + 1, 0, s, 0] = -1      # out(s+1, 0) -= psi(s, 0)
        C[:, :, s, 1, s + 1, 1] = -1      # out(s, 1) -= psi(s+1, 1)
    C[:, :, 0, 0, Ls - 1, 0] = CLD(m)     # out(0, 0) += m psi(Ls-1, 0)
    C[:, :, Ls - 1, 1, 0, 1] = CLD(m)     # out(Ls-1, 1) += m psi(0, 1)
    flat = lambda a: sn.to_eo(a.reshape(Lx, Ly, nc * nc), Lx, Ly, nc * nc).astype(np.complex128)
    hops = []
    for axis, step, link, M in hop_terms(Ux, Uy, w):
        H = np.zeros((Lx, Ly, Ls, 2, Ls, 2), dtype=CLD)
        for s in range(Ls):
            H[:, :, s, :, s, :] = link[:, :, None, None] * M[None, None]
        hops.append(flat(H))
    return flat(C), np.concatenate(hops)


def gamma5_grid(x):
    """(Gamma5 psi)(s, sigma) = (-1)^sigma psi(Ls-1-s, sigma) on psi[x, y, s, sigma, ...]"""
    sign = np.array([1.0, -1.0]).reshape((1, 1, 1, 2) + (1,) * (x.ndim - 4))
    return sign * x[:, :, ::-1]


def gamma5_dense(Ls):
    """Gamma5 as the nc x nc matrix on the flat component c = 2 s + sigma"""
    G = np.zeros((Ls, 2, Ls, 2))
    for s in range(Ls):
        G[s, 0, Ls - 1 - s, 0] = 1.0
        G[s, 1, Ls - 1 - s, 1] = -1.0
    return G.reshape(2 * Ls, 2 * Ls)


def dense(Lx, Ly, Ls, gauge, m, w, M5):
    """D and Gamma5 as dense complex128 matrices over the grid ordering (x, y, s, sigma): the formulas above applied to the identity"""
    N = Lx * Ly * Ls * 2
    Ux, Uy = link_grids(gauge, Lx, Ly, np.complex128)
    eye = np.eye(N, dtype=np.complex128).reshape(Lx, Ly, Ls, 2, N)
    pieces = 0xFFF | (P_ZERO_E * 3)
    Dm, _, _ = _core(eye, np.zeros_like(eye), Ux, Uy, m, w, M5, 0.0, 0.0, pieces, np.complex128)
    return Dm.reshape(N, N), gamma5_grid(eye).reshape(N, N)
