"""Independent statement of the even-odd domain-wall operations (csrc/qmg_dwf_eo.hip) in np.clongdouble arithmetic on psi[x, y, s, sigma].

D = A + H.  The hops H come from dwf_numpy; the site-local block A_p = clover + shift is written with slices here (d_p = 3 w + shift +-
eo_shift on the diagonal, + on even sites, - on odd; dof_shift = 0), and its inverse is the Ls x Ls per-spin matrix that Gauss-Jordan
elimination in long double gives for A_p applied to the unit vectors -- not the closed form the kernels scan with.

    inv5        out_p = alpha A_p^-1 rhs_p                                        (kernel I; overwrites the named parities)
    hops_inv5   out_p = (ZERO_p ? 0 : lhs0_p) + alpha A_p^-1 H_{p,1-p} [G5] rhs    (kernel K)
    schur       out_p = [G5] (A_p [G5] rhs_p + H_{p,1-p} t),  t = -A_{1-p}^-1 H_{1-p,p} [G5] rhs_p   (= [G5] M_p [G5] rhs_p)

Next to every result come the term-magnitude sum S and the term count n of stencil_numpy.elementwise_bound:
    S = |alpha| |A^-1| S_hop (+ |lhs0|),   n = n_hop + 2 Ls + 2
-- one per term of a row of A^-1, one more per term because each entry of A^-1 (a power of 1 / d_p) is itself rounded, and 2 for alpha and
the accumulation into lhs0.  For kernel I S_hop = |rhs| and n_hop = 0.  The Schur complement composes two such sums: with t known to
(n_t + 1) u S_t, the second stage's n_2 terms give (n_2 + n_t + 2) u (S_A + |H| S_t), so S = S_A + |H| S_t and n = n_2 + n_t + 1.
"""
import numpy as np

import dwf_numpy as dn
import stencil_numpy as sn

CLD = np.clongdouble
LD = np.longdouble
G5_IN, G5_OUT = 1, 2
P_CLOVER_E, P_EO, P_OE, P_ZERO_E = sn.P_CLOVER_E, 0xF << 2, 0xF << 6, sn.P_ZERO_E


def diag(w, shift, eo_shift, p, ctype=CLD):
    """d_p = 3 w + shift +- eo_shift"""
    return ctype(3.0 * w) + ctype(shift) + (ctype(-eo_shift) if p else ctype(eo_shift))


def apply_A(x, d, m):
    """A x on [..., s, sigma] arrays (the two trailing axes), d and m scalars: the diagonal, the shift along s, the wall"""
    Ls = x.shape[-2]
    out = d * x
    out[..., 1:, 0] -= x[..., :-1, 0]            # out(s+1, 0) -= psi(s, 0)
    out[..., :-1, 1] -= x[..., 1:, 1]            # out(s, 1) -= psi(s+1, 1)
    out[..., 0, 0] += m * x[..., Ls - 1, 0]      # the wall
    out[..., Ls - 1, 1] += m * x[..., 0, 1]
    return out


def abs_A(ax, d, m):
    """the term-magnitude sum of apply_A and its term count (2 for the diagonal: d is itself a rounded sum)"""
    Ls = ax.shape[-2]
    S = abs(d) * ax
    n = np.full(ax.shape, 2, dtype=np.int64)
    S[..., 1:, 0] += ax[..., :-1, 0]; n[..., 1:, 0] += 1
    S[..., :-1, 1] += ax[..., 1:, 1]; n[..., :-1, 1] += 1
    if m != 0:
        S[..., 0, 0] += abs(m) * ax[..., Ls - 1, 0]; n[..., 0, 0] += 1
        S[..., Ls - 1, 1] += abs(m) * ax[..., 0, 1]; n[..., Ls - 1, 1] += 1
    return S, n


def gauss_jordan(A):
    """the inverse of a small square matrix by Gauss-Jordan elimination with partial pivoting, in A's (long double) arithmetic"""
    n = A.shape[0]
    M = np.concatenate([np.array(A, copy=True), np.eye(n, dtype=A.dtype)], axis=1)
    for c in range(n):
        piv = c + int(np.argmax(np.abs(M[c:, c])))
        if piv != c:
            M[[c, piv]] = M[[piv, c]]
        M[c] = M[c] / M[c, c]
        for r in range(n):
            if r != c:
                M[r] = M[r] - M[r, c] * M[c]
    return M[:, n:]


def a_blocks(Ls, d, m, ctype=CLD):
    """(A0, A1): the Ls x Ls matrices of A on sigma = 0 and 1, from apply_A on the unit vectors"""
    eye = np.zeros((Ls, Ls, 2), dtype=ctype)       # [column, s, sigma]
    out = []
    for g in (0, 1):
        e = eye.copy()
        e[np.arange(Ls), np.arange(Ls), g] = 1
        out.append(apply_A(e, ctype(d), ctype(m))[:, :, g].T.copy())
    return out


def inv_blocks(Ls, w, m, shift, eo_shift, p):
    """(B0, B1) = the inverses of A_p's two spin blocks, long double Gauss-Jordan"""
    return [gauss_jordan(A) for A in a_blocks(Ls, diag(w, shift, eo_shift, p), m)]


def _parity(Lx, Ly):
    xs, ys = np.meshgrid(np.arange(Lx), np.arange(Ly), indexing="ij")
    return (xs + ys) & 1


def _grid(v, Lx, Ly, Ls, dtype=None):
    g = sn.to_grid(v, Lx, Ly, 2 * Ls).reshape(Lx, Ly, Ls, 2)
    return g if dtype is None else g.astype(dtype)


def _flat(a, Lx, Ly, Ls):
    return sn.to_eo(a.reshape(Lx, Ly, 2 * Ls), Lx, Ly, 2 * Ls)


def _inv5_grid(h, Sh, nh, l0, par, on, Ls, w, m, shift, eo_shift, alpha, zero, blocks=inv_blocks):
    """out, S, n on the grid: the sites with on[p] get (zero[p] ? 0 : l0) + alpha A_p^-1 h, every other site keeps l0"""
    out, S, n = np.array(l0, copy=True), np.abs(l0).astype(LD), np.zeros(l0.shape, dtype=np.int64)
    for p in (0, 1):
        if not on[p]:
            continue
        B = blocks(Ls, w, m, shift, eo_shift, p)
        y, Sy = np.empty_like(h), np.empty_like(Sh)
        for g in (0, 1):
            y[:, :, :, g] = np.einsum("st,xyt->xys", B[g], h[:, :, :, g])
            Sy[:, :, :, g] = np.einsum("st,xyt->xys", np.abs(B[g]), Sh[:, :, :, g])
        sel = par == p
        base = np.zeros_like(out[sel]) if zero[p] else out[sel]
        out[sel] = base + CLD(alpha) * y[sel]
        S[sel] = np.abs(base) + abs(alpha) * Sy[sel]
        n[sel] = nh[sel] + 2 * Ls + 2
    return out, S, n


def inv5(Lx, Ly, Ls, m, w, shift, eo_shift, pieces, alpha, rhs, lhs0):
    """kernel I.  (out, S, n) as flat (eo, y, x, c) arrays."""
    h, l0 = _grid(rhs, Lx, Ly, Ls), _grid(lhs0, Lx, Ly, Ls)
    on = [bool(pieces & (P_CLOVER_E << p)) for p in (0, 1)]
    out, S, n = _inv5_grid(h, np.abs(h), np.zeros(h.shape, dtype=np.int64), l0, _parity(Lx, Ly), on, Ls, w, m, shift, eo_shift, alpha, [True, True])
    return _flat(out, Lx, Ly, Ls), _flat(S, Lx, Ly, Ls), _flat(n, Lx, Ly, Ls)


def _hops(x, Ux, Uy, w, hop_pieces):
    """(H x, S, n) on the grid for the hop bits given, overwriting"""
    return dn._core(x, np.zeros_like(x), Ux, Uy, 0.0, w, 0.0, 0.0, 0.0, hop_pieces | (P_ZERO_E * 3), CLD)


def hops_inv5(Lx, Ly, Ls, gauge, m, w, shift, eo_shift, pieces, alpha, flags, rhs, lhs0):
    """kernel K.  (out, S, n) as flat arrays."""
    Ux, Uy = dn.link_grids(gauge, Lx, Ly)
    x, l0 = _grid(rhs, Lx, Ly, Ls), _grid(lhs0, Lx, Ly, Ls)
    if flags & G5_IN:
        x = dn.gamma5_grid(x)
    h, Sh, nh = _hops(x, Ux, Uy, w, pieces & (P_EO | P_OE))
    on = [bool(pieces & (P_EO, P_OE)[p]) for p in (0, 1)]
    zero = [bool(pieces & (P_ZERO_E << p)) for p in (0, 1)]
    out, S, n = _inv5_grid(h, Sh, nh, l0, _parity(Lx, Ly), on, Ls, w, m, shift, eo_shift, alpha, zero)
    return _flat(out, Lx, Ly, Ls), _flat(S, Lx, Ly, Ls), _flat(n, Lx, Ly, Ls)


def schur(Lx, Ly, Ls, gauge, m, w, shift, eo_shift, parity, flags, rhs, lhs0, tmp0):
    """[G5] M_p [G5] rhs_p.  (out, S, n, tmp, S_tmp, n_tmp) as flat arrays: out = lhs0 and tmp = tmp0 outside the halves written."""
    Ux, Uy = dn.link_grids(gauge, Lx, Ly)
    par = _parity(Lx, Ly)
    p, o = parity, 1 - parity
    x, l0, t0 = _grid(rhs, Lx, Ly, Ls), _grid(lhs0, Lx, Ly, Ls), _grid(tmp0, Lx, Ly, Ls)
    if flags & G5_IN:
        x = dn.gamma5_grid(x)
    x = np.where((par == p)[:, :, None, None], x, 0)          # only the p half of rhs is read
    # stage 1: t_o = -A_o^-1 H_{o,p} x
    h, Sh, nh = _hops(x, Ux, Uy, w, (P_EO, P_OE)[o])
    on, zero = [o == 0, o == 1], [True, True]
    t, St, nt = _inv5_grid(h, Sh, nh, t0, par, on, Ls, w, m, shift, eo_shift, -1.0, zero)
    tz = np.where((par == o)[:, :, None, None], t, 0)
    Stz = np.where((par == o)[:, :, None, None], St, 0)
    # stage 2: A_p x + H_{p,o} t
    d = diag(w, shift, eo_shift, p)
    Ax = apply_A(x, d, CLD(m))
    SA, nA = abs_A(np.abs(x), d, CLD(m))
    Ht, _, nH = _hops(tz, Ux, Uy, w, (P_EO, P_OE)[p])
    _, SH, _ = _hops(Stz.astype(CLD), Ux, Uy, w, (P_EO, P_OE)[p])     # |H| S_t: _core's magnitude sum of the input S_t
    res, S, n = Ax + Ht, SA + SH, nA + nH + int(np.max(nt)) + 1
    if flags & G5_OUT:
        res, S, n = dn.gamma5_grid(res), S[:, :, ::-1], n[:, :, ::-1]
    sel = par == p
    out, So, no = np.array(l0, copy=True), np.abs(l0).astype(LD), np.zeros(l0.shape, dtype=np.int64)
    out[sel], So[sel], no[sel] = res[sel], S[sel], n[sel]
    f = lambda a: _flat(a, Lx, Ly, Ls)
    return f(out), f(So), f(no), f(t), f(St), f(nt)


# ---- the same inverse as the kernels form it, for tests/test_host_dwf_eo.py: closed form, any complex dtype
def closed_form_blocks(Ls, w, m, shift, eo_shift, p, ctype=np.complex128):
    """B0[s, s'] = [s >= s'] d^-(s-s'+1) - m d^-(s+1) d^-(Ls-s') / (1 + m d^-Ls),  B1[s, s'] = B0[Ls-1-s, Ls-1-s']"""
    d, m = diag(w, shift, eo_shift, p, ctype), ctype(m)
    pw = np.array([(1 / d) ** k for k in range(Ls + 1)], dtype=ctype)
    q = m / (1 + m * pw[Ls])
    B0 = np.zeros((Ls, Ls), dtype=ctype)
    for s in range(Ls):
        for t in range(Ls):
            B0[s, t] = (pw[s - t + 1] if s >= t else 0) - q * pw[s + 1] * pw[Ls - t]
    return [B0, B0[::-1, ::-1].copy()]


def forward_substitution(h, Ls, w, m, shift, eo_shift, p, ctype=np.complex128):
    """A_p^-1 h on [..., s, sigma] by the recurrence g_s = (h_s + g_{s-1}) / d and the wall correction, in ctype"""
    d, m = diag(w, shift, eo_shift, p, ctype), ctype(m)
    inv = 1 / d
    h = h.astype(ctype)
    g = np.zeros_like(h)
    for s in range(Ls):                       # sigma 0 from below
        g[..., s, 0] = (h[..., s, 0] + (g[..., s - 1, 0] if s else 0)) * inv
    for s in range(Ls - 1, -1, -1):           # sigma 1 from above
        g[..., s, 1] = (h[..., s, 1] + (g[..., s + 1, 1] if s + 1 < Ls else 0)) * inv
    pw = np.array([inv ** k for k in range(Ls + 1)], dtype=ctype)
    q = m / (1 + m * pw[Ls])
    y = np.empty_like(g)
    y[..., 0] = g[..., 0] - q * pw[1:] * g[..., Ls - 1:Ls, 0]
    y[..., 1] = g[..., 1] - q * pw[1:][::-1] * g[..., 0:1, 1]
    return y
