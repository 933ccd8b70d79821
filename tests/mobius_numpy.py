"""Independent statement of the Moebius domain-wall operator and of its dagger in np.clongdouble arithmetic on coordinate grids.

A field is psi[x, y, s, sigma] as in dwf_numpy: neighbours are np.roll, the fifth dimension is written with slices, spin with the Pauli
matrices; nothing shares the index arithmetic of csrc/qmg_mobius.hip.  With w the Wilson coefficient, m the wall mass, M5 the domain-wall
height, d_w = 2 w + M5, alpha = b5 d_w + 1, kappa = c5 d_w - 1 and

    (L psi)(s, 0) = psi(s-1, 0)  (s >= 1),     (L psi)(0, 0)    = -m psi(Ls-1, 0)
    (L psi)(s, 1) = psi(s+1, 1)  (s <= Ls-2),  (L psi)(Ls-1, 1) = -m psi(0, 1)
    (H psi)(x) = sum_mu link_mu(x) M_mu psi(x + mu),   M_{+-x} = (+-sigma1 - w) / 2,  M_{+-y} = (+-sigma2 - w) / 2     (dwf_numpy.hop_terms)

the operator is D = D_W (b5 + c5 L) + (1 - L) with D_W = d_w + H:

    D psi        = alpha psi + kappa L psi + H chi,                    chi = b5 psi + c5 L psi
    D^dagger psi = alpha psi + kappa L^+ psi + b5 g + c5 L^+ g,        g = H^+ psi

    (L^+ psi)(s, 0) = psi(s+1, 0)  (s <= Ls-2),  (L^+ psi)(Ls-1, 0) = -conj(m) psi(0, 0)
    (L^+ psi)(s, 1) = psi(s-1, 1)  (s >= 1),     (L^+ psi)(0, 1)    = -conj(m) psi(Ls-1, 1)
    (H^+ psi)(x) = sum_mu link_mu(x) M_mu^- psi(x + mu),   M_mu^- = M_mu with sigma -> -sigma

(H^+ has the links of H: the conjugate of the link of the opposite hop is the link itself).  The descriptor's shifts are added to the
diagonal afterwards, shift +- eo_shift (+ even, - odd) +- dof_shift (+ where 2 s + sigma < Ls), conjugated for the dagger.  Both operators
are written out term by term; dense() builds the matrix of D another way, from Kronecker products.

Next to the result come the term-magnitude sum S and the term count n of stencil_numpy.elementwise_bound.  A term is one product
coefficient x psi of the expanded sum; it counts once, plus once for every rounded product inside its coefficient or on its way (alpha and
kappa; -m kappa; b5 or c5 on the way through chi or g; -m c5; w/2 U when w != 1), plus 3 for the shift.
"""
import fractions

import numpy as np

import dwf_numpy as dn
import stencil_numpy as sn

CLD = np.clongdouble
P_SHIFT_E, P_ZERO_E = sn.P_SHIFT_E, sn.P_ZERO_E

# what the two solve tests (tests/test_host_mobius.py, tests/test_gpu_mobius.py) share: the system, eps and the gate
SOLVE = dict(dims=(4, 4), Ls=4, m=0.05, w=1.0, M5=-1.0, b5=1.5, c5=0.5, eps=1e-10, gauge_seed=31, rhs_seed=32)
# |x_cg - x_dense| / |x_dense| of the numpy CG at eps = 1e-10: 1.509e-10 after 63 iterations (cond D = 26.5; printed by
# test_numpy_cg_fixes_the_solve_gate, which holds it to SOLVE_REACH); the GPU solve is gated at ten times SOLVE_REACH
SOLVE_REACH = 1.6e-10


def coefficients(w, M5, b5, c5, ctype=CLD):
    rt = np.longdouble if ctype is CLD else np.float64
    d_w = rt(2.0) * rt(w) + rt(M5)
    return rt(b5) * d_w + rt(1.0), rt(c5) * d_w - rt(1.0)      # alpha, kappa


def hop_terms_dagger(Ux, Uy, w, ctype=CLD):
    """dwf_numpy.hop_terms with sigma -> -sigma in the spin matrices"""
    I2 = np.eye(2, dtype=ctype)
    out = []
    for axis, step, link, M in dn.hop_terms(Ux, Uy, w, ctype):
        out.append((axis, step, link, -M - ctype(w) * I2))     # (s sigma - w)/2 -> (-s sigma - w)/2
    return out


def _L(x, m, dagger):
    """(L x, |L| |x| with the magnitudes of the coefficients, 1 where the coefficient is the wall's -m) on [x, y, s, sigma, ...]"""
    Ls = x.shape[2]
    out = np.zeros_like(x)
    wall = np.zeros(x.shape, dtype=np.int64)
    lo, hi = (1, 0) if dagger else (0, 1)       # the spin that takes slice s-1, and the one that takes s+1
    mm = np.conj(m) if dagger else m
    out[:, :, 1:, lo] = x[:, :, :-1, lo]
    out[:, :, 0, lo] = -mm * x[:, :, Ls - 1, lo]
    out[:, :, :-1, hi] = x[:, :, 1:, hi]
    out[:, :, Ls - 1, hi] = -mm * x[:, :, 0, hi]
    wall[:, :, 0, lo] = 1
    wall[:, :, Ls - 1, hi] = 1
    return out, wall


def _Labs(ax, m, dagger):
    """|L| applied to magnitudes"""
    out, _ = _L(ax, -abs(m), dagger)
    return out


def _hops(terms, x, ax, ex):
    """(H x, |H| |x|)"""
    g, gs = np.zeros_like(x), np.zeros_like(ax)
    for axis, step, link, M in terms:
        g = g + ex(link) * np.einsum("ab,xysb...->xysa...", M, np.roll(x, step, axis=axis))
        gs = gs + ex(np.abs(link)) * np.einsum("ab,xysb...->xysa...", np.abs(M), np.roll(ax, step, axis=axis))
    return g, gs


def _core(x, lhs0, Ux, Uy, m, w, M5, b5, c5, shift, eo_shift, dof_shift, pieces, dagger, ctype):
    """x, lhs0: [x, y, s, sigma, ...].  The full operator on both parities (+ SHIFT_p, ZERO_p of `pieces`).  Returns (out, S, n)."""
    Lx, Ly, Ls = x.shape[:3]
    rtype = np.longdouble if ctype is CLD else np.float64
    extra = (1,) * (x.ndim - 4)
    ex2 = lambda a: np.asarray(a).reshape(np.asarray(a).shape + (1, 1) + extra)
    ex4 = lambda a: np.asarray(a).reshape(np.asarray(a).shape + extra)
    xs, ys = np.meshgrid(np.arange(Lx), np.arange(Ly), indexing="ij")
    parity = (xs + ys) & 1
    m, shift, eo_shift, dof_shift = ctype(m), ctype(shift), ctype(eo_shift), ctype(dof_shift)
    if dagger:
        shift, eo_shift, dof_shift = np.conj(shift), np.conj(eo_shift), np.conj(dof_shift)
    alpha, kappa = coefficients(w, M5, b5, c5, ctype)
    b5, c5 = rtype(b5), rtype(c5)
    out = np.array(lhs0, dtype=ctype, copy=True)
    for p in (0, 1):
        if pieces & (P_ZERO_E << p):
            out[parity == p] = 0
    S = np.abs(out)
    ax = np.abs(x)
    ones = np.ones(x.shape, dtype=np.int64)
    hw = 0 if w == 1 else 1                                  # w/2 U is a rounded product
    # the site-local part
    Lx_, wall = _L(x, m, dagger)
    out = out + alpha * x + kappa * Lx_
    S = S + abs(alpha) * ax + abs(kappa) * _Labs(ax, m, dagger)
    n = 2 * ones + (2 + wall)                                # alpha psi; kappa L psi (-m kappa at the wall)
    # the hops: 2 spin entries per direction, through b5 (the slice itself) and through c5 (its fifth-dimension partner)
    per_dir = 2 * ((2 + hw) + (2 + hw))
    if not dagger:
        chi = b5 * x + c5 * Lx_
        chis = abs(b5) * ax + abs(c5) * _Labs(ax, m, False)
        g, gs = _hops(dn.hop_terms(Ux, Uy, w, ctype), chi, chis, ex2)
        out, S = out + g, S + gs
        n = n + 4 * per_dir + 4 * 2 * 1                      # (the partner may be the wall's: one more product, counted for every slice)
    else:
        g, gs = _hops(hop_terms_dagger(Ux, Uy, w, ctype), x, ax, ex2)
        Lg, _ = _L(g, m, True)
        out = out + b5 * g + c5 * Lg
        S = S + abs(b5) * gs + abs(c5) * _Labs(gs, m, True)
        n = n + 4 * per_dir + 4 * 2 * 1
    # the shifts
    s_idx, g_idx = np.arange(Ls)[:, None], np.arange(2)[None, :]
    dof_sign = ex4(np.where(2 * s_idx + g_idx < Ls, 1.0, -1.0).astype(rtype)[None, None])
    for p in (0, 1):
        if pieces & (P_SHIFT_E << p):
            on = ex2(parity == p)
            eo = eo_shift if p == 0 else -eo_shift
            out = out + on * ((shift + eo + dof_sign * dof_shift) * x)
            S = S + on * ((abs(shift) + abs(eo_shift) + abs(dof_shift)) * ax)
            n = n + on * 3
    return out, S, n


def apply(Lx, Ly, Ls, gauge, m, w, M5, b5, c5, shift, eo_shift, dof_shift, pieces, rhs, lhs0, dagger=False, ctype=CLD):
    """(out, S, n) as flat (eo, y, x, c) arrays.  pieces: P_ALL with any of P_SHIFT_E / _O, P_ZERO_E / _O taken out."""
    nc = 2 * Ls
    Ux, Uy = dn.link_grids(gauge, Lx, Ly, ctype)
    x = sn.to_grid(rhs, Lx, Ly, nc).reshape(Lx, Ly, Ls, 2)
    l0 = sn.to_grid(lhs0, Lx, Ly, nc).reshape(Lx, Ly, Ls, 2)
    out, S, n = _core(x, l0, Ux, Uy, m, w, M5, b5, c5, shift, eo_shift, dof_shift, pieces, dagger, ctype)
    flat = lambda a: sn.to_eo(np.asarray(a).reshape(Lx, Ly, nc), Lx, Ly, nc)
    return flat(out), flat(S), flat(n)


def grid_operator(Lx, Ly, Ls, gauge, m, w, M5, b5, c5, dagger=False):
    """the grid formula applied to the identity: D (or D^dagger) as a complex128 matrix over the ordering (x, y, s, sigma)"""
    N = Lx * Ly * Ls * 2
    Ux, Uy = dn.link_grids(gauge, Lx, Ly, np.complex128)
    eye = np.eye(N, dtype=np.complex128).reshape(Lx, Ly, Ls, 2, N)
    Dm, _, _ = _core(eye, np.zeros_like(eye), Ux, Uy, m, w, M5, b5, c5, 0.0, 0.0, 0.0, P_ZERO_E * 3, dagger, np.complex128)
    return Dm.reshape(N, N)


# ---- the dense matrix, written independently of the grid form: Kronecker products of L, the spin blocks and the site shifts
def L_dense(Ls, m):
    """L on the component c = 2 s + sigma"""
    L0 = np.zeros((Ls, Ls), dtype=np.complex128)       # sigma 0: slice s takes slice s-1
    for s in range(1, Ls):
        L0[s, s - 1] = 1.0
    L0[0, Ls - 1] = -m
    L1 = np.zeros((Ls, Ls), dtype=np.complex128)       # sigma 1: slice s takes slice s+1
    for s in range(Ls - 1):
        L1[s, s + 1] = 1.0
    L1[Ls - 1, 0] = -m
    P0, P1 = np.diag([1.0, 0.0]), np.diag([0.0, 1.0])
    return np.kron(L0, P0) + np.kron(L1, P1)


def site_shift(Lx, Ly, axis, step):
    """T with (T f)(x) = f(x + step along axis) on the site ordering (x, y), periodic"""
    V = Lx * Ly
    T = np.zeros((V, V))
    for x in range(Lx):
        for y in range(Ly):
            xn, yn = ((x + step) % Lx, y) if axis == 0 else (x, (y + step) % Ly)
            T[x * Ly + y, xn * Ly + yn] = 1.0
    return T


def hops_dense(Lx, Ly, Ls, gauge, w, B=None):
    """H (I x B): sum over the four directions of diag(link) T x (I_Ls x M)"""
    Ux, Uy = dn.link_grids(gauge, Lx, Ly, np.complex128)
    s1 = np.array([[0, 1], [1, 0]], dtype=np.complex128)
    s2 = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)
    I2 = np.eye(2)
    H = 0
    for axis, U, sig in ((0, Ux, s1), (1, Uy, s2)):
        Tf, Tb = site_shift(Lx, Ly, axis, +1), site_shift(Lx, Ly, axis, -1)
        fwd = np.diag(U.reshape(-1)) @ Tf                               # U(x) f(x + mu)
        bwd = np.diag((Tb @ U.reshape(-1)).conj()) @ Tb                  # conj U(x - mu) f(x - mu)
        H = H + np.kron(fwd, np.kron(np.eye(Ls), 0.5 * (sig - w * I2))) + np.kron(bwd, np.kron(np.eye(Ls), 0.5 * (-sig - w * I2)))
    return H


def dense(Lx, Ly, Ls, gauge, m, w, M5, b5, c5):
    """(D, A, B, H, Gamma5) as dense complex128 matrices over (x, y, s, sigma): D = A + H B, A = alpha + kappa L, B = b5 + c5 L"""
    V, nc = Lx * Ly, 2 * Ls
    alpha, kappa = coefficients(w, M5, b5, c5, np.complex128)
    L = np.kron(np.eye(V), L_dense(Ls, m))
    I = np.eye(V * nc)
    A = alpha * I + kappa * L
    B = b5 * I + c5 * L
    H = hops_dense(Lx, Ly, Ls, gauge, w)
    G5 = np.kron(np.eye(V), dn.gamma5_dense(Ls))
    return A + H @ B, A, B, H, G5


# ---- the stored form
def _exact_round(fr):
    """a Fraction rounded once to the nearest double"""
    return fr.numerator / fr.denominator      # int / int true division is correctly rounded


def fields(Lx, Ly, Ls, gauge, m, w, M5, b5, c5):
    """flat clover (eo, y, x, r, c) and hopping (mu, eo, y, x, r, c) fields of the nc = 2 Ls stencil, complex128, zeros included: every
    entry is its exact value rounded once.  The entries with a real coefficient are formed in long double, where the products of two or
    three doubles that occur are exact or far inside the last place of the rounding to double; the wall entries of the hopping field,
    -m c5 (w/2) U (sigma - w): a complex product whose parts can cancel, are formed in rational arithmetic."""
    nc = 2 * Ls
    F = fractions.Fraction
    m = complex(m)
    Ux, Uy = dn.link_grids(gauge, Lx, Ly)
    alpha, kappa = coefficients(w, M5, b5, c5)
    C = np.zeros((Lx, Ly, Ls, 2, Ls, 2), dtype=CLD)
    Bc = np.zeros((Ls, 2, Ls), dtype=CLD)               # B[(sr, g), sc]: the real-coefficient part, and where the wall sits
    wall = np.zeros((Ls, 2, Ls), dtype=bool)
    for s in range(Ls):
        for g in range(2):
            C[:, :, s, g, s, g] = alpha
            Bc[s, g, s] = b5
    for s in range(Ls - 1):
        C[:, :, s + 1, 0, s, 0] = kappa
        C[:, :, s, 1, s + 1, 1] = kappa
        Bc[s + 1, 0, s] = c5
        Bc[s, 1, s + 1] = c5
    C[:, :, 0, 0, Ls - 1, 0] = -CLD(m) * kappa
    C[:, :, Ls - 1, 1, 0, 1] = -CLD(m) * kappa
    if c5 != 0:
        wall[0, 0, Ls - 1] = True
        wall[Ls - 1, 1, 0] = True
    flat = lambda a: sn.to_eo(a.reshape(Lx, Ly, nc * nc), Lx, Ly, nc * nc)
    hops = []
    cr, ci = -F(m.real) * F(c5), -F(m.imag) * F(c5)
    for axis, step, link, M in dn.hop_terms(Ux, Uy, w):
        Hm = np.zeros((Lx, Ly, Ls, 2, Ls, 2), dtype=CLD)
        Hw = np.zeros((Lx, Ly, Ls, 2, Ls, 2), dtype=np.complex128)
        for sr in range(Ls):
            for sc in range(Ls):
                for gc in range(2):
                    if wall[sr, gc, sc]:
                        # (cr + i ci) link M[:, gc], exactly; M's entries are (a + i b) / 2 with a, b in {0, +-1, -w}
                        for gr in range(2):
                            e = complex(M[gr, gc])
                            er, ei = F(float(e.real)), F(float(e.imag))
                            for ix in range(Lx):
                                for iy in range(Ly):
                                    u = complex(link[ix, iy])
                                    ur, ui = F(float(u.real)), F(float(u.imag))
                                    tr, ti = ur * er - ui * ei, ur * ei + ui * er
                                    Hw[ix, iy, sr, gr, sc, gc] = complex(_exact_round(cr * tr - ci * ti), _exact_round(cr * ti + ci * tr))
                    elif Bc[sr, gc, sc] != 0:
                        Hm[:, :, sr, :, sc, gc] = Bc[sr, gc, sc] * link[:, :, None] * M[None, None, :, gc]
        hops.append(flat(Hm).astype(np.complex128) + flat(Hw))
    return flat(C).astype(np.complex128), np.concatenate(hops)


def cg_normal(apply_D, apply_Ddag, b, eps, max_iter):
    """CG on D^dagger D x = D^dagger b from x = 0 in complex128, stopped at |r| <= eps |D^dagger b| (minv_vector_cg's rule): (x, iterations)"""
    rhs = apply_Ddag(b)
    x = np.zeros_like(rhs)
    r = rhs.copy()
    p = r.copy()
    rr = np.vdot(r, r).real
    stop = eps * eps * np.vdot(rhs, rhs).real
    it = 0
    while it < max_iter and rr > stop:
        Ap = apply_Ddag(apply_D(p))
        a = rr / np.vdot(p, Ap).real
        x = x + a * p
        r = r - a * Ap
        rr_new = np.vdot(r, r).real
        p = r + (rr_new / rr) * p
        rr = rr_new
        it += 1
    return x, it
