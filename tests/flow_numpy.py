"""Independent numpy statement of the Wilson flow and of planar Wilson / Polyakov loops for compact U(1) on (x, y) grids with np.roll.

A helper, not a test.  Like u1_numpy.py and hmc_numpy.py it builds on coordspace.py and shares nothing with the even-odd index algebra or the
two-register Runge-Kutta form of csrc/qmg_flow.hip: phases are (thx, thy) pairs of [x, y] grids, the step is Luescher's scheme in its textbook
three-Z form, and a Wilson loop is an explicit walk around its perimeter.  tests/test_host_flow.py pins these statements (finite differences
of the action, the order of the integrator, monotonicity, the exact loops of the two-dimensional torus) before tests/test_gpu_flow.py
judges the device by them.

  d theta / dt = -dS_w/d theta,   S_w = sum_x (1 - cos P(x)),   P(x) = theta_x(x) + theta_y(x+xhat) - theta_x(x+yhat) - theta_y(x)
"""
import numpy as np

import coordspace as cs

NEW_SYMBOLS = ["qmg_u1_flow_stage", "qmg_u1_flow", "qmg_u1_wilson_loops", "qmg_u1_polyakov"]
NEW_BINDINGS = ["u1_flow_stage", "u1_flow", "u1_wilson_loops", "u1_polyakov"]


def plaquette_angle(th):
    return th[0] + cs.fwd(th[1], 0) - cs.fwd(th[0], 1) - th[1]


def action(th):
    """S_w = sum_x (1 - cos P(x))"""
    return float(np.sum(1.0 - np.cos(plaquette_angle(th))))


def force(th):
    """dS_w/dtheta_mu(x): a link sits in two plaquettes"""
    s = np.sin(plaquette_angle(th))
    return s - cs.bwd(s, 1), -s + cs.bwd(s, 0)


def Z(th, eps):
    f = force(th)
    return -eps * f[0], -eps * f[1]


def rk3_step(th, eps):
    """Luescher, JHEP 08 (2010) 071, (C.1), for commuting generators, every Z kept:
    W1 = exp(Z0/4) W0,  W2 = exp(8/9 Z1 - 17/36 Z0) W1,  V(t + eps) = exp(3/4 Z2 - 8/9 Z1 + 17/36 Z0) W2,  Z_i = eps Z(W_i)"""
    z0 = Z(th, eps)
    w1 = (th[0] + z0[0] / 4.0, th[1] + z0[1] / 4.0)
    z1 = Z(w1, eps)
    w2 = tuple(w1[m] + (8.0 / 9.0) * z1[m] - (17.0 / 36.0) * z0[m] for m in range(2))
    z2 = Z(w2, eps)
    return tuple(w2[m] + 0.75 * z2[m] - (8.0 / 9.0) * z1[m] + (17.0 / 36.0) * z0[m] for m in range(2))


def flow(th, eps, n_steps):
    th = (th[0].copy(), th[1].copy())
    for _ in range(n_steps):
        th = rk3_step(th, eps)
    return th


def rk3_stages_two_register(th, eps):
    """The form the device uses (A = Z; A = 8/9 Z - 17/36 A; A = 3/4 Z - A): the phases and the accumulator after each of the three stages.
    Only test_host_flow.py (numpy against itself) and the per-stage device comparison use it."""
    out = []
    a = Z(th, eps)
    th = (th[0] + a[0] / 4.0, th[1] + a[1] / 4.0)
    out.append((th, a))
    z = Z(th, eps)
    a = tuple((8.0 / 9.0) * z[m] - (17.0 / 36.0) * a[m] for m in range(2))
    th = (th[0] + a[0], th[1] + a[1])
    out.append((th, a))
    z = Z(th, eps)
    a = tuple(0.75 * z[m] - a[m] for m in range(2))
    th = (th[0] + a[0], th[1] + a[1])
    out.append((th, a))
    return out


def links(th):
    return np.exp(1j * th[0]), np.exp(1j * th[1])


def topo(th):
    """sum_x arg exp(i P(x)) / 2 pi, the geometric charge qmg_u1_plaquette returns"""
    return float(np.angle(np.exp(1j * plaquette_angle(th))).sum() / (2 * np.pi))


def wilson_loop(Ux, Uy, R, T):
    """Lattice average of the R x T loop by a walk around the perimeter from every site at once: R links along +x, T along +y, R back along
    -x (conjugated), T back along -y."""
    w = np.ones_like(Ux)
    for k in range(R):                     # (x + k, y) -> (x + k + 1, y)
        w = w * np.roll(Ux, -k, axis=0)
    for k in range(T):                     # (x + R, y + k) -> (x + R, y + k + 1)
        w = w * np.roll(np.roll(Uy, -R, axis=0), -k, axis=1)
    for k in range(R - 1, -1, -1):         # (x + k + 1, y + T) -> (x + k, y + T)
        w = w * np.conj(np.roll(np.roll(Ux, -k, axis=0), -T, axis=1))
    for k in range(T - 1, -1, -1):         # (x, y + k + 1) -> (x, y + k)
        w = w * np.conj(np.roll(Uy, -k, axis=1))
    return complex(w.mean())


def wilson_loops(Ux, Uy, r_max, t_max):
    return np.array([[wilson_loop(Ux, Uy, R, T) for T in range(1, t_max + 1)] for R in range(1, r_max + 1)])


def polyakov(Ux, Uy):
    """(prod_x U_x(x, y) averaged over y, prod_y U_y(x, y) averaged over x)"""
    return complex(np.prod(Ux, axis=0).mean()), complex(np.prod(Uy, axis=1).mean())


def creutz(W, R, T):
    """chi(R, T) = -log[ W(R,T) W(R-1,T-1) / (W(R-1,T) W(R,T-1)) ] of a real table W[R-1, T-1], W(0,.) = W(.,0) = 1"""
    w = lambda r, t: 1.0 if r == 0 or t == 0 else W[r - 1][t - 1]
    return float(-np.log(w(R, T) * w(R - 1, T - 1) / (w(R - 1, T) * w(R, T - 1))))


def bessel_i(n, x, terms=60):
    """I_n(x) by its power series (n >= 0 integer), as the I1/I0 of the HMC tests"""
    k = np.arange(terms)
    logs = (2 * k + n) * np.log(x / 2.0) - np.array([np.sum(np.log(np.arange(1, j + 1))) + np.sum(np.log(np.arange(1, j + n + 1))) for j in k])
    return float(np.sum(np.exp(logs)))


def torus_wilson_loop(beta, V, area, n_max=30):
    """<W> of a loop of `area` plaquettes for compact pure-gauge U(1) with the Wilson action on a periodic lattice of V plaquettes:
    sum_n I_n^(V - area) I_(n+1)^area / sum_n I_n^V  (character expansion; the sum over n is the sum over the flux through the torus)."""
    try:
        from scipy.special import iv
        I = {n: float(iv(abs(n), beta)) for n in range(-n_max - 1, n_max + 2)}
    except ImportError:
        I = {n: bessel_i(abs(n), beta) for n in range(-n_max - 1, n_max + 2)}
    i0 = I[0]
    num = sum((I[n] / i0) ** (V - area) * (I[n + 1] / i0) ** area for n in range(-n_max, n_max + 1))
    den = sum((I[n] / i0) ** V for n in range(-n_max, n_max + 1))
    return num / den


def hmc_loops_pure_gauge(L, beta, tau, n_steps, n_therm, n_meas, seed, pairs=((1, 1), (1, 2), (2, 2))):
    """hmc_numpy.hmc_pure_gauge's run (cold start, same random stream and decisions) with the loops `pairs` measured on every trajectory after
    thermalisation; (means of Re W in the order of `pairs`, acceptance)"""
    import hmc_numpy as hn
    rng = np.random.default_rng(seed)
    th = (np.zeros((L, L)), np.zeros((L, L)))
    meas, acc = [], 0
    for t in range(n_therm + n_meas):
        pi = (rng.standard_normal((L, L)), rng.standard_normal((L, L)))
        th1, _, dH = hn.md_dH(th, pi, beta, tau, n_steps)
        ok = rng.uniform() < np.exp(-dH)
        if ok:
            th = th1
        if t >= n_therm:
            acc += ok
            Ux, Uy = links(th)
            meas.append([wilson_loop(Ux, Uy, R, T).real for R, T in pairs])
    return np.mean(np.array(meas), axis=0), acc / n_meas


# ---- gates of the ensemble tests (CPU and GPU): five standard deviations of the run's mean over 12 seeds (measured in test_host_flow.py::test_torus_wilson_loops_from_the_twin_hmc) ----
SIGMA_W = {(1, 1): 0.00277, (1, 2): 0.00418, (2, 2): 0.00347}
GATE_W = {k: 5.0 * v for k, v in SIGMA_W.items()}


def chi22_gate(beta=2.0, V=256):
    """chi(2,2) = -log W22 - log W11 + 2 log W12: the three loop gates propagated linearly at the exact values, in quadrature"""
    w = {k: torus_wilson_loop(beta, V, k[0] * k[1]) for k in GATE_W}
    return float(np.sqrt((GATE_W[(2, 2)] / w[(2, 2)]) ** 2 + (GATE_W[(1, 1)] / w[(1, 1)]) ** 2 + (2.0 * GATE_W[(1, 2)] / w[(1, 2)]) ** 2))


def uniform_field(Lx, Ly, Q):
    """theta_x = -F y, theta_y = F Ly x on the last row, F = 2 pi Q / V: every plaquette angle is F (mod 2 pi), the charge is Q"""
    F = 2.0 * np.pi * Q / (Lx * Ly)
    x, y = np.meshgrid(np.arange(Lx), np.arange(Ly), indexing="ij")
    return -F * y * 1.0, np.where(y == Ly - 1, F * Ly * x, 0.0) * 1.0


def gaussian_phases(Lx, Ly, beta, seed):
    ph = np.random.default_rng(seed).normal(0.0, 1.0 / np.sqrt(beta), size=(Lx, Ly, 2))
    return ph[:, :, 0].copy(), ph[:, :, 1].copy()


# ---- layout: grids <-> the (mu, eo, y, x) device fields ----
def field_to_eo(th):
    Lx, Ly = th[0].shape
    return np.concatenate([cs.grid_to_eo(t[:, :, None].astype(complex), Lx, Ly, 1).real for t in th])


def eo_to_field(v, Lx, Ly):
    V = Lx * Ly
    v = np.asarray(v, dtype=np.float64).astype(np.complex128)
    return cs.eo_to_grid(v[:V], Lx, Ly, 1)[:, :, 0].real.copy(), cs.eo_to_grid(v[V:], Lx, Ly, 1)[:, :, 0].real.copy()


def file_phases(path, Lx, Ly):
    """the reference's text format (x outer, y, mu inner) as a (thx, thy) pair"""
    ph = np.loadtxt(path).reshape(Lx, Ly, 2)
    return ph[:, :, 0].copy(), ph[:, :, 1].copy()
