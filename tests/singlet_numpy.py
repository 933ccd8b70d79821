"""Independent numpy statement of the flavour-singlet measurement (csrc/qmg_singlet.hip, include/qmg/singlet.hpp): the counter-based Z4
noise, the dilution classes, the loops S, P, N from a DENSE inverse of the Wilson operator, and `combine`.  No product code: the operator is
coordspace.wilson_apply on unit vectors, the inverse numpy.linalg.solve.

Layout: element i = site * nc + c, site = (y + p * Ly) * hr + j, hr = Lx / 2, p the parity half.
Noise:  h = splitmix64(seed * 0xD1342543DE82EF95 + 2 i) (mod 2^64), eta_i = i^(h >> 62).
Class:  d(i) = ((y mod nt) * ncs + (spin ? c : 0)) * neo + (eo ? p : 0), ncs = spin ? nc : 1, neo = eo ? 2 : 1.
Gamma:  g(i) = +1 for c < nc / 2, -1 otherwise (mode 0);  -1 on the odd half (mode 1).

Signs and normalisation of `combine` (stated once, the product follows them): with S(y) = sum_d S_d(y), P(y) = sum_d P_d(y) per noise,
  condensate = Re sum_y S(y) / (Lx Ly)                       (mean over noises; error = standard error of that mean)
  q5         = sum_y Re P(y)
  Ddisc(t)   = 1 / (Nn (Nn - 1) Ly) sum_{a != b} sum_{y0} Re P_a(y0) Re P_b((y0 + t) mod Ly)
  Cpi(t)     = 1 / (Nn Ly) sum_a sum_{t0} sum_{d: class row = t0} N_d((t0 + t) mod Ly)         (nt == Ly only)
  Ceta(t)    = Cpi(t) - N_f Ddisc(t)
"""
import numpy as np

import coordspace as cs

M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def splitmix64(z):
    """The hash on an array of uint64 (arithmetic mod 2^64)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def z4_power(seed, n):
    """q_i of eta_i = i^q_i for the elements 0 .. n-1."""
    i = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        s = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) * np.uint64(0xD1342543DE82EF95)
        h = splitmix64(s + np.uint64(2) * i)
    return (h >> np.uint64(62)).astype(np.int64)


Z4 = np.array([complex(1.0, 0.0), complex(0.0, 1.0), complex(-1.0, 0.0), complex(0.0, -1.0)])   # (-1j is -0 - 1j: the zeros here are +0)


def noise_z4(seed, n):
    return Z4[z4_power(seed, n)]


def coords(Lx, Ly, nc):
    """(y, c, p) of every element."""
    hr = Lx // 2
    i = np.arange(Lx * Ly * nc)
    site, c = i // nc, i % nc
    row = site // hr
    p = row // Ly
    return row - p * Ly, c, p


def n_classes(nc, dil):
    nt, spin, eo = dil
    return nt * (nc if spin else 1) * (2 if eo else 1)


def class_map(Lx, Ly, nc, dil):
    nt, spin, eo = dil
    assert nt >= 1 and Ly % nt == 0 and spin in (0, 1) and eo in (0, 1)
    y, c, p = coords(Lx, Ly, nc)
    ncs, neo = (nc if spin else 1), (2 if eo else 1)
    return ((y % nt) * ncs + (c if spin else 0)) * neo + (p if eo else 0)


def class_row(d, nc, dil):
    """y mod nt of class d."""
    nt, spin, eo = dil
    return d // ((nc if spin else 1) * (2 if eo else 1))


def diluted(seed, Lx, Ly, nc, dil, d):
    eta = noise_z4(seed, Lx * Ly * nc)
    return np.where(class_map(Lx, Ly, nc, dil) == d, eta, 0.0)


def gamma_sign(Lx, Ly, nc, g5_mode):
    y, c, p = coords(Lx, Ly, nc)
    if g5_mode == 0:
        assert nc % 2 == 0
        return np.where(c < nc // 2, 1.0, -1.0)
    return np.where(p == 1, -1.0, 1.0)


def loops(psi, seed, Lx, Ly, nc, dil, d, g5_mode):
    """out[y] = (Re S, Im S, Re P, Im P, N) of one solution psi = D^-1 eta^(d) (any vector, for the kernel tests)."""
    n = Lx * Ly * nc
    psi = np.asarray(psi, dtype=np.complex128)[:n]
    eta = noise_z4(seed, n)
    y, _, _ = coords(Lx, Ly, nc)
    hit = class_map(Lx, Ly, nc, dil) == d
    g = gamma_sign(Lx, Ly, nc, g5_mode)
    s = np.where(hit, np.conj(eta) * psi, 0.0)
    out = np.zeros((Ly, 5))
    out[:, 0] = np.bincount(y, weights=s.real, minlength=Ly)
    out[:, 1] = np.bincount(y, weights=s.imag, minlength=Ly)
    out[:, 2] = np.bincount(y, weights=g * s.real, minlength=Ly)
    out[:, 3] = np.bincount(y, weights=g * s.imag, minlength=Ly)
    out[:, 4] = np.bincount(y, weights=np.abs(psi) ** 2, minlength=Ly)
    return out


def row_abs_sum(psi, Lx, Ly, nc):
    """sum_{i in row y} |psi_i|: the scale of the summation-order gate."""
    y, _, _ = coords(Lx, Ly, nc)
    return np.bincount(y, weights=np.abs(np.asarray(psi)[:Lx * Ly * nc]), minlength=Ly)


def support_sizes(Lx, Ly, nc, dil, d):
    """|support_d(y)| per row."""
    y, _, _ = coords(Lx, Ly, nc)
    return np.bincount(y[class_map(Lx, Ly, nc, dil) == d], minlength=Ly)


def wilson_dense(Ux, Uy, mass):
    """D in the even-odd layout, column by column from coordspace.wilson_apply on unit vectors."""
    Lx, Ly = Ux.shape
    n = Lx * Ly * 2
    D = np.zeros((n, n), dtype=np.complex128)
    for j in range(n):
        e = np.zeros(n, dtype=np.complex128)
        e[j] = 1.0
        D[:, j] = cs.grid_to_eo(cs.wilson_apply(cs.eo_to_grid(e, Lx, Ly, 2), Ux, Uy, mass), Lx, Ly, 2)
    return D


def exact_traces(Dinv, Lx, Ly, nc, g5_mode=0):
    """(Tr_y[D^-1], Tr_y[gamma5 D^-1]) per row, complex."""
    y, _, _ = coords(Lx, Ly, nc)
    dg = np.diag(Dinv)
    g = gamma_sign(Lx, Ly, nc, g5_mode)
    tr = np.bincount(y, weights=dg.real, minlength=Ly) + 1j * np.bincount(y, weights=dg.imag, minlength=Ly)
    tr5 = np.bincount(y, weights=(g * dg).real, minlength=Ly) + 1j * np.bincount(y, weights=(g * dg).imag, minlength=Ly)
    return tr, tr5


def measure(D, seed, Lx, Ly, nc, dil, g5_mode=0):
    """One noise through the dense operator: {"S": [D, Ly] complex, "P": [D, Ly] complex, "N": [D, Ly], "psi": [D, n]}."""
    nd = n_classes(nc, dil)
    B = np.stack([diluted(seed, Lx, Ly, nc, dil, d) for d in range(nd)], axis=1)
    X = np.linalg.solve(D, B)
    S = np.zeros((nd, Ly), dtype=np.complex128)
    P = np.zeros((nd, Ly), dtype=np.complex128)
    N = np.zeros((nd, Ly))
    for d in range(nd):
        o = loops(X[:, d], seed, Lx, Ly, nc, dil, d, g5_mode)
        S[d], P[d], N[d] = o[:, 0] + 1j * o[:, 1], o[:, 2] + 1j * o[:, 3], o[:, 4]
    return {"S": S, "P": P, "N": N, "psi": X.T.copy()}


def combine(noises, Lx, Ly, nc, dil, n_f=2):
    """The observables of a list of measure()-shaped noises (signs and normalisation: the module docstring)."""
    nn = len(noises)
    S = np.array([m["S"].sum(axis=0) for m in noises])   # [noise, y]
    P = np.array([m["P"].sum(axis=0) for m in noises])
    cond = S.real.sum(axis=1) / (Lx * Ly)
    out = {"S": S, "P": P, "condensate_per_noise": cond, "condensate": float(cond.mean()),
           "condensate_err": float(cond.std(ddof=1) / np.sqrt(nn)) if nn > 1 else 0.0, "q5": P.real.sum(axis=1)}
    if nn >= 2:
        dd = np.zeros(Ly)
        for t in range(Ly):
            for a in range(nn):
                for b in range(nn):
                    if a != b:
                        dd[t] += np.dot(P[a].real, np.roll(P[b].real, -t))
        out["Ddisc"] = dd / (nn * (nn - 1) * Ly)
    if dil[0] == Ly:
        cpi = np.zeros(Ly)
        for m in noises:
            for d in range(m["N"].shape[0]):
                cpi += np.roll(m["N"][d], -class_row(d, nc, dil))
        out["Cpi"] = cpi / (nn * Ly)
        if nn >= 2:
            out["Ceta"] = out["Cpi"] - n_f * out["Ddisc"]
    return out
