"""Independent numpy statement of the U(1) field tools (u1/u1_utils.h:241-383, 545-603) on (x, y) grids with np.roll.

A helper, not a test.  Like coordspace.py, on which it builds, it shares nothing with the even-odd index algebra of
csrc/qmg_u1.hip: fields are U[mu][x, y] grids and only coordspace's layout functions move them in and out.
tests/test_host_u1_tools.py pins these statements by their identities before tests/test_gpu_u1_tools.py judges the device by them."""
import numpy as np

import coordspace as cs

NEW_SYMBOLS = ["qmg_u1_hot_gauge", "qmg_u1_gauss_gauge", "qmg_u1_random_trans", "qmg_u1_gauge_transform", "qmg_u1_ape_smear",
               "qmg_u1_instanton", "qmg_u1_noncompact_instanton"]
NEW_BINDINGS = ["u1_hot_gauge", "u1_gauss_gauge", "u1_random_trans", "u1_gauge_transform", "u1_ape_smear", "u1_instanton", "u1_noncompact_instanton"]


def plaquette(Ux, Uy):
    """(volume average of U_x(x) U_y(x+xhat) U_x^*(x+yhat) U_y^*(x), topological charge sum arg / 2 pi)"""
    p = Ux * cs.fwd(Uy, 0) * np.conj(cs.fwd(Ux, 1)) * np.conj(Uy)
    return p.mean(), np.angle(p).sum() / (2 * np.pi)


def gauge_transform(Ux, Uy, g):
    """U_mu(x) <- g(x) U_mu(x) conj g(x + mu)   (u1_utils.h:241-272)"""
    return g * Ux * np.conj(cs.fwd(g, 0)), g * Uy * np.conj(cs.fwd(g, 1))


def project(z):
    """P[z] = exp(i arg z); np.angle(0) = 0, so P[0] = 1   (arg_vector + polar, u1_utils.h:371-372)"""
    return np.exp(1j * np.angle(z))


def ape_iteration(Ux, Uy, alpha):
    """One iteration, both directions from the previous iterate, no (1 - alpha) factor   (u1_utils.h:292-375)"""
    up_x = Uy * cs.fwd(Ux, 1) * np.conj(cs.fwd(Uy, 0))
    lo_x = np.conj(cs.bwd(Uy, 1)) * cs.bwd(Ux, 1) * cs.bwd(cs.fwd(Uy, 0), 1)
    up_y = Ux * cs.fwd(Uy, 0) * np.conj(cs.fwd(Ux, 1))
    lo_y = np.conj(cs.bwd(Ux, 0)) * cs.bwd(Uy, 0) * cs.bwd(cs.fwd(Ux, 1), 0)
    return project(Ux + alpha * (up_x + lo_x)), project(Uy + alpha * (up_y + lo_y))


def ape_smear(Ux, Uy, alpha, n_iter):
    for _ in range(n_iter):
        Ux, Uy = ape_iteration(Ux, Uy, alpha)
    return Ux, Uy


def instanton(Ux, Uy, Q, x0, y0):
    """create_instanton_u1 (u1_utils.h:545-572), with its centring arithmetic"""
    Lx, Ly = Ux.shape
    x, y = np.arange(Lx)[:, None], np.arange(Ly)[None, :]
    rx, ry = x - Lx // 2 + 0.5 + 0 * y, y - Ly // 2 + 0.5 + 0 * x
    r2 = rx * rx + ry * ry
    tx, ty = (x - Lx // 2 + x0 + 3 * Lx) % Lx + 0 * y, (y - Ly // 2 + y0 + 3 * Ly) % Ly + 0 * x
    Ux, Uy = Ux.copy(), Uy.copy()
    Ux[tx, ty] = Ux[tx, ty] * np.exp(1j * Q * ry / r2)
    Uy[tx, ty] = Uy[tx, ty] * np.exp(-1j * Q * rx / r2)
    return Ux, Uy


def noncompact_instanton(Ax, Ay, Q):
    """create_noncompact_instanton_u1 (u1_utils.h:575-603), with the reference's literal for pi"""
    Lx, Ly = Ax.shape
    x, y = np.arange(Lx)[:, None], np.arange(Ly)[None, :]
    Ax = Ax + (-Q * 3.1415926535 * y / (Lx * Ly)) + 0.0 * x
    Ay = Ay.copy()
    Ay[:, Ly - 1] += Q * 3.1415926535 * np.arange(Lx) / Lx
    return Ax, Ay


def gaussian_links(L, beta, seed, Ly=None):
    rng = np.random.default_rng(seed)
    ph = rng.normal(0.0, 1.0 / np.sqrt(beta), size=(L, Ly or L, 2))
    return np.exp(1j * ph[:, :, 0]), np.exp(1j * ph[:, :, 1])


def random_transform(Lx, Ly, seed):
    return np.exp(1j * np.random.default_rng(seed).uniform(-np.pi, np.pi, size=(Lx, Ly)))


def grid_to_eo_real(A, Lx, Ly):
    return cs.grid_to_eo(A[:, :, None].astype(complex), Lx, Ly, 1).real.copy()


def eo_gauge_to_links(g, Lx, Ly):
    V = Lx * Ly
    return cs.eo_to_grid(g[:V], Lx, Ly, 1)[:, :, 0], cs.eo_to_grid(g[V:], Lx, Ly, 1)[:, :, 0]
