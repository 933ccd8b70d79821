"""Independent statement of the even-odd Moebius operations (csrc/qmg_mobius_eo.hip) in np.clongdouble arithmetic on psi[x, y, s, sigma].

D = A + H B (mobius_numpy).  The hops H come from dwf_numpy; the site-local blocks A_p = alpha_p + kappa L (alpha_p = alpha + shift +- eo_shift,
+ on even sites, - on odd; dof_shift = 0) and B = b5 + c5 L are written with slices here, and A_p^-1 is the Ls x Ls per-spin matrix that the
long-double Gauss-Jordan elimination of dwf_eo_numpy gives for A_p applied to the unit vectors -- not the twisted-circulant closed form the
kernels take their tables from.  The primed blocks of the dagger are the same formulas with conj(m) and the conjugated shifts.

    inv5        out_p = scale S rhs_p                                              S = A_p^-1 or A_p^-1 B; overwrites the named parities
    hops_inv5   out_p = (ZERO_p ? 0 : lhs0_p) + scale S H_{p,1-p} (R [G5] rhs)     S in {1, A_p^-1, A_p^-1 B}, R in {1, B}
    schur op 0  out_p = A_p x_p + H (B t),                t = -A_o^-1 H (B x_p)           (= M_p x_p)
    schur op 1  out_p = G5 [A'_p G5 x_p + B' (H t)],      t = -(A'_o^-1 B') H (G5 x_p)    (= M_p^dagger x_p)

Next to every result come the term-magnitude sum S and the term count n of stencil_numpy.elementwise_bound, composed as dwf_eo_numpy does it:
a vector known to (n_v + 1) u S_v that goes through a further sum of n_2 terms is known to (n_2 + n_v + 2) u |sum| S_v.
    B on a vector     S = |B| S_v,   n = n_v + N_LIN + 1     N_LIN = 4: two for the diagonal (a rounded sum in A; counted for B too), one for the
                                                             partner along s and one more because its coefficient across the wall (-m c5, -m kappa)
                                                             is a rounded product
    H on a vector     S = |H| S_v,   n = n_v + n_hop + 1     n_hop: dwf_numpy's count
    a table S         S = |scale| |S| S_v (+ |lhs0|),   n = n_v + 2 Ls + 2      one per term of a row, one more per term because each entry of the
                                                             table is itself rounded, 2 for the scale and the accumulation (dwf_eo_numpy's count)
"""
import numpy as np

import dwf_eo_numpy as de
import dwf_numpy as dn
import mobius_numpy as mn
import stencil_numpy as sn

CLD = np.clongdouble
LD = np.longdouble
S_ONE, S_AINV, S_AINV_B = range(3)
R_ONE, R_B = range(2)
G5_IN = 1
P_CLOVER_E, P_EO, P_OE, P_ZERO_E = de.P_CLOVER_E, de.P_EO, de.P_OE, de.P_ZERO_E
N_LIN = 4
# |x - x_dense| / |x_dense| of the numpy CG on M^dagger M at mobius_numpy.SOLVE's system and eps (prepare, CG, reconstruct): 5.658e-11 after 39
# iterations, against 63 on D^dagger D (printed by test_numpy_cg_on_the_schur_complement_fixes_the_solve_gate, which holds it to SOLVE_REACH);
# the GPU solve is gated at ten times SOLVE_REACH
SOLVE_REACH = 6.0e-11


def alpha_p(w, M5, b5, c5, shift, eo_shift, p, dagger=False):
    """(alpha_p, kappa): alpha + shift +- eo_shift (conjugated shifts for the dagger), kappa"""
    alpha, kappa = mn.coefficients(w, M5, b5, c5)
    sh, eo = CLD(shift), CLD(eo_shift)
    if dagger:
        sh, eo = np.conj(sh), np.conj(eo)
    return CLD(alpha) + sh + (-eo if p else eo), kappa


def lin(x, d, k, m):
    """(d + k L) x on [..., s, sigma] arrays (the two trailing axes), d, k, m scalars: the diagonal, the shift along s, the wall"""
    Ls = x.shape[-2]
    out = d * x
    out[..., 1:, 0] += k * x[..., :-1, 0]             # (L x)(s, 0) = x(s-1, 0)
    out[..., :-1, 1] += k * x[..., 1:, 1]             # (L x)(s, 1) = x(s+1, 1)
    out[..., 0, 0] += (-m * k) * x[..., Ls - 1, 0]    # the wall
    out[..., Ls - 1, 1] += (-m * k) * x[..., 0, 1]
    return out


def lin_abs(ax, d, k, m):
    """|d + k L| on magnitudes"""
    return lin(ax, abs(d), abs(k), -abs(m))


def lin_blocks(Ls, d, k, m):
    """(M0, M1): the Ls x Ls matrices of d + k L on sigma = 0 and 1, from lin on the unit vectors"""
    out = []
    for g in (0, 1):
        e = np.zeros((Ls, Ls, 2), dtype=CLD)           # [column, s, sigma]
        e[np.arange(Ls), np.arange(Ls), g] = 1
        out.append(lin(e, CLD(d), CLD(k), CLD(m))[:, :, g].T.copy())
    return out


def table_blocks(Ls, table, m, w, M5, b5, c5, shift, eo_shift, p, dagger=False):
    """the per-spin matrices of S on parity p: 1, A_p^-1 (long double Gauss-Jordan) or A_p^-1 B"""
    if table == S_ONE:
        return [np.eye(Ls, dtype=CLD), np.eye(Ls, dtype=CLD)]
    mm = np.conj(CLD(m)) if dagger else CLD(m)
    ap, kappa = alpha_p(w, M5, b5, c5, shift, eo_shift, p, dagger)
    inv = [de.gauss_jordan(A) for A in lin_blocks(Ls, ap, kappa, mm)]
    if table == S_AINV:
        return inv
    B = lin_blocks(Ls, LD(b5), LD(c5), mm)
    return [inv[g] @ B[g] for g in (0, 1)]


def _mask(a, par, p):
    return np.where((par == p)[:, :, None, None], a, 0)


def _table_grid(h, Sh, nh, l0, par, on, Ls, blocks_of, scale, zero):
    """dwf_eo_numpy._inv5_grid with the matrices of S in place of A^-1: (out, S, n) on the grid"""
    return de._inv5_grid(h, Sh, nh, l0, par, on, Ls, None, None, None, None, scale, zero, blocks=lambda Ls_, w_, m_, s_, e_, p: blocks_of(p))


def inv5(Lx, Ly, Ls, m, w, M5, b5, c5, shift, eo_shift, pieces, table, scale, rhs, lhs0):
    """lhs_p = scale S rhs_p.  (out, S, n) as flat (eo, y, x, c) arrays."""
    h, l0 = de._grid(rhs, Lx, Ly, Ls), de._grid(lhs0, Lx, Ly, Ls)
    on = [bool(pieces & (P_CLOVER_E << p)) for p in (0, 1)]
    blocks_of = lambda p: table_blocks(Ls, table, m, w, M5, b5, c5, shift, eo_shift, p)
    out, S, n = _table_grid(h, np.abs(h), np.zeros(h.shape, dtype=np.int64), l0, de._parity(Lx, Ly), on, Ls, blocks_of, scale, [True, True])
    return de._flat(out, Lx, Ly, Ls), de._flat(S, Lx, Ly, Ls), de._flat(n, Lx, Ly, Ls)


def _hops_of(v, Sv, nv, Ux, Uy, w, hop_pieces):
    """(H v, |H| S_v, n_v + n_hop + 1) for a vector known to (n_v + 1) u S_v (n_v = -1: exact input)"""
    h, _, nh = de._hops(v, Ux, Uy, w, hop_pieces)
    _, Sh, _ = de._hops(Sv.astype(CLD), Ux, Uy, w, hop_pieces)      # |H| S_v: _core's magnitude sum of the input S_v
    return h, Sh.real.astype(LD) if np.iscomplexobj(Sh) else Sh, nh + nv + 1


def hops_inv5(Lx, Ly, Ls, gauge, m, w, M5, b5, c5, shift, eo_shift, pieces, table, source, scale, flags, rhs, lhs0):
    """lhs_p (+)= scale S H_{p,1-p} (R [G5] rhs).  (out, S, n) as flat arrays."""
    Ux, Uy = dn.link_grids(gauge, Lx, Ly)
    x, l0 = de._grid(rhs, Lx, Ly, Ls), de._grid(lhs0, Lx, Ly, Ls)
    if flags & G5_IN:
        x = dn.gamma5_grid(x)
    Sx, nx = np.abs(x), -1
    if source == R_B:
        x, Sx, nx = lin(x, CLD(b5), CLD(c5), CLD(m)), lin_abs(Sx, b5, c5, m), N_LIN
    h, Sh, nh = _hops_of(x, Sx, nx, Ux, Uy, w, pieces & (P_EO | P_OE))
    on = [bool(pieces & (P_EO, P_OE)[p]) for p in (0, 1)]
    zero = [bool(pieces & (P_ZERO_E << p)) for p in (0, 1)]
    blocks_of = lambda p: table_blocks(Ls, table, m, w, M5, b5, c5, shift, eo_shift, p)
    out, S, n = _table_grid(h, Sh, nh, l0, de._parity(Lx, Ly), on, Ls, blocks_of, scale, zero)
    return de._flat(out, Lx, Ly, Ls), de._flat(S, Lx, Ly, Ls), de._flat(n, Lx, Ly, Ls)


def schur(Lx, Ly, Ls, gauge, m, w, M5, b5, c5, shift, eo_shift, parity, op, rhs, lhs0, tmp0):
    """M_p rhs_p (op 0) or M_p^dagger rhs_p (op 1).  (out, S, n, tmp, S_tmp, n_tmp) as flat arrays: out = lhs0 and tmp = tmp0 outside the
    halves written."""
    Ux, Uy = dn.link_grids(gauge, Lx, Ly)
    par = de._parity(Lx, Ly)
    p, o = parity, 1 - parity
    dag = bool(op)
    mm = np.conj(CLD(m)) if dag else CLD(m)
    x, l0, t0 = de._grid(rhs, Lx, Ly, Ls), de._grid(lhs0, Lx, Ly, Ls), de._grid(tmp0, Lx, Ly, Ls)
    if dag:
        x = dn.gamma5_grid(x)
    x = _mask(x, par, p)                                        # only the p half of rhs is read
    ax = np.abs(x)
    on, zero = [o == 0, o == 1], [True, True]
    hop_o, hop_p = (P_EO, P_OE)[o], (P_EO, P_OE)[p]
    ap, kappa = alpha_p(w, M5, b5, c5, shift, eo_shift, p, dag)
    Ax, SA, nA = lin(x, ap, CLD(kappa), mm), lin_abs(ax, ap, kappa, mm), N_LIN
    if not dag:
        # stage 1: t_o = -A_o^-1 H_{o,p} (B x)
        h, Sh, nh = _hops_of(lin(x, CLD(b5), CLD(c5), mm), lin_abs(ax, b5, c5, mm), N_LIN, Ux, Uy, w, hop_o)
        blocks_of = lambda q: table_blocks(Ls, S_AINV, m, w, M5, b5, c5, shift, eo_shift, q)
        t, St, nt = _table_grid(h, Sh, nh, t0, par, on, Ls, blocks_of, -1.0, zero)
        tz, Stz, ntm = _mask(t, par, o), _mask(St, par, o), int(np.max(nt))
        # stage 2: A_p x + H_{p,o} (B t)
        Ht, SH, nH = _hops_of(lin(tz, CLD(b5), CLD(c5), mm), lin_abs(Stz, b5, c5, mm), ntm + N_LIN + 1, Ux, Uy, w, hop_p)
        res, S, n = Ax + Ht, SA + SH, nA + nH + 1
    else:
        # stage 1: t_o = -(A'_o^-1 B') H_{o,p} x,  x = G5 rhs
        h, Sh, nh = _hops_of(x, ax, -1, Ux, Uy, w, hop_o)
        blocks_of = lambda q: table_blocks(Ls, S_AINV_B, m, w, M5, b5, c5, shift, eo_shift, q, True)
        t, St, nt = _table_grid(h, Sh, nh, t0, par, on, Ls, blocks_of, -1.0, zero)
        tz, Stz, ntm = _mask(t, par, o), _mask(St, par, o), int(np.max(nt))
        # stage 2: G5 [A'_p x + B' (H_{p,o} t)]
        g, Sg, ng = _hops_of(tz, Stz, ntm, Ux, Uy, w, hop_p)
        res, S, n = Ax + lin(g, CLD(b5), CLD(c5), mm), SA + lin_abs(Sg, b5, c5, mm), nA + ng + N_LIN + 2
        res, S, n = dn.gamma5_grid(res), S[:, :, ::-1], n[:, :, ::-1]
    sel = par == p
    out, So, no = np.array(l0, copy=True), np.abs(l0).astype(LD), np.zeros(l0.shape, dtype=np.int64)
    out[sel], So[sel], no[sel] = res[sel], S[sel], n[sel]
    f = lambda a: de._flat(a, Lx, Ly, Ls)
    return f(out), f(So), f(no), f(t), f(St), f(nt)


# ---- the solve, on flat vectors: prepare, M, M^dagger, reconstruct with the even half as the system
def full_ops(Lx, Ly, Ls, gauge, m, w, M5, b5, c5, shift=0.0, eo_shift=0.0):
    """closures on flat complex vectors of the whole lattice in the twin's arithmetic: (M, Mdag, prepare, reconstruct) for parity 0"""
    zeros = lambda: np.zeros(Lx * Ly * 2 * Ls, dtype=CLD)
    args = (Lx, Ly, Ls, gauge, m, w, M5, b5, c5, shift, eo_shift)
    M = lambda x: schur(*args, 0, 0, x, zeros(), zeros())[0]
    Mdag = lambda x: schur(*args, 0, 1, x, zeros(), zeros())[0]

    def prepare(b):
        """b'_e = b_e - H_eo B A_o^-1 b_o on the even half; the odd half keeps b_o"""
        t = inv5(Lx, Ly, Ls, m, w, M5, b5, c5, shift, eo_shift, P_CLOVER_E << 1, S_AINV, 1.0, b, zeros())[0]
        return hops_inv5(*args, P_EO, S_ONE, R_B, -1.0, 0, t, np.asarray(b, dtype=CLD))[0]

    def reconstruct(x_e, b):
        """x_o = A_o^-1 (b_o - H_oe B x_e); returns the full x"""
        n = b.size
        v = np.concatenate([np.asarray(x_e, dtype=CLD)[:n // 2], np.asarray(b, dtype=CLD)[n // 2:]])
        r = hops_inv5(*args, P_OE, S_ONE, R_B, -1.0, 0, v, v)[0]                      # r_o = b_o - H_oe B x_e
        xo = inv5(Lx, Ly, Ls, m, w, M5, b5, c5, shift, eo_shift, P_CLOVER_E << 1, S_AINV, 1.0, r, zeros())[0]
        return np.concatenate([v[:n // 2], xo[n // 2:]])
    return M, Mdag, prepare, reconstruct


# ---- the tables as the kernels take them, for tests/test_host_mobius_eo.py: the twisted-circulant closed form, any complex dtype
def closed_form_table(Ls, table, m, w, M5, b5, c5, shift, eo_shift, p, ctype=np.complex128):
    """f_k, k < Ls:  A_p^-1: r^k / (alpha_p (1 + m r^Ls)), r = -kappa / alpha_p;  A_p^-1 B: b5 f_k + c5 f_{k-1}, g_0 = b5 f_0 - m c5 f_{Ls-1}"""
    if table == S_ONE:
        return np.array([1] + [0] * (Ls - 1), dtype=ctype)
    ap, kappa = alpha_p(w, M5, b5, c5, shift, eo_shift, p)
    ap, kappa, m = ctype(ap), ctype(kappa), ctype(m)
    r = -kappa / ap
    f = np.array([r ** k for k in range(Ls)], dtype=ctype) / (ap * (1 + m * r ** Ls))
    if table == S_AINV:
        return f
    g = ctype(b5) * f + ctype(c5) * np.roll(f, 1)
    g[0] = ctype(b5) * f[0] - m * ctype(c5) * f[Ls - 1]
    return g


def circulant_blocks(f, m):
    """the per-spin matrices of sum_k f_k L^k: sigma 0  C[s, s-k] = f_k (s >= k), C[s, s-k+Ls] = -m f_k (s < k); sigma 1 the mirror"""
    Ls = len(f)
    C0 = np.zeros((Ls, Ls), dtype=f.dtype)
    for s in range(Ls):
        for k in range(Ls):
            if s >= k:
                C0[s, s - k] = f[k]
            else:
                C0[s, s - k + Ls] = -f.dtype.type(m) * f[k]
    return [C0, C0[::-1, ::-1].copy()]
