"""Independent numpy statement of two-flavour Wilson HMC for the Schwinger model on (x, y) grids with np.roll.

A helper, not a test.  Like u1_numpy.py it builds on coordspace.py and shares nothing with the even-odd index algebra of csrc/qmg_hmc.hip:
phases, momenta and forces are (thx, thy) pairs of [x, y] grids, spinors psi[x, y, 2], and only coordspace's layout functions move them in
and out.  tests/test_host_hmc.py pins these statements (finite differences of the action, gauge covariance, reversibility and the dt^2 law
of leapfrog) before tests/test_gpu_hmc.py judges the device by them.

  H = 1/2 sum pi^2 + S_g + S_f,   S_g = beta sum_x (1 - cos P(x)),   S_f = phi^dag (D^dag D)^-1 phi,   D = coordspace.wilson_apply (w = 1)
  P(x) = theta_x(x) + theta_y(x+xhat) - theta_x(x+yhat) - theta_y(x)
"""
import numpy as np

import coordspace as cs

NEW_SYMBOLS = ["qmg_hmc_momentum_update", "qmg_hmc_link_update", "qmg_hmc_momentum_refresh", "qmg_hmc_stream_seed"]
NEW_BINDINGS = ["hmc_momentum_update", "hmc_link_update", "hmc_momentum_refresh", "hmc_stream_seed"]

S1 = np.array([[0, 1], [1, 0]], dtype=np.complex128)
S2 = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)
G5 = np.array([1.0, -1.0])


def links(th):
    return np.exp(1j * th[0]), np.exp(1j * th[1])


def plaquette_angle(th):
    return th[0] + cs.fwd(th[1], 0) - cs.fwd(th[0], 1) - th[1]


def gauge_action(th, beta):
    return float(beta * np.sum(1.0 - np.cos(plaquette_angle(th))))


def gauge_force(th, beta):
    s = np.sin(plaquette_angle(th))
    return beta * (s - cs.bwd(s, 1)), beta * (-s + cs.bwd(s, 0))


def D(psi, th, mass):
    Ux, Uy = links(th)
    return cs.wilson_apply(psi, Ux, Uy, mass)


def Ddag(psi, th, mass):
    """D^dag = gamma5 D gamma5 (real mass)"""
    return G5 * D(G5 * psi, th, mass)


def dense_D(th, mass):
    """D as a (2V x 2V) matrix on the flattened [x, y, spin] index, column by column"""
    Lx, Ly = th[0].shape
    n = 2 * Lx * Ly
    M = np.empty((n, n), dtype=np.complex128)
    for j in range(n):
        e = np.zeros(n, dtype=np.complex128)
        e[j] = 1.0
        M[:, j] = D(e.reshape(Lx, Ly, 2), th, mass).reshape(-1)
    return M


def solve_dense(phi, th, mass):
    """X = (D^dag D)^-1 phi by LU"""
    M = dense_D(th, mass)
    return np.linalg.solve(M.conj().T @ M, phi.reshape(-1)).reshape(phi.shape)


def make_cg(eps, max_iter=100000, iters=None):
    """X = (D^dag D)^-1 phi by plain CG from zero, stopped like the library's: recursive |r| < eps |phi|.  iters: a list that collects counts."""
    def solve(phi, th, mass):
        x = np.zeros_like(phi)
        r = phi.copy()
        p = r.copy()
        rsq = np.vdot(r, r).real
        stop = eps * eps * rsq
        k = 0
        while rsq >= stop and k < max_iter:
            Ap = Ddag(D(p, th, mass), th, mass)
            a = rsq / np.vdot(p, Ap).real
            x += a * p
            r -= a * Ap
            new = np.vdot(r, r).real
            p = r + (new / rsq) * p
            rsq = new
            k += 1
        if iters is not None:
            iters.append(k)
        return x
    return solve


def fermion_action(th, phi, mass, solve=solve_dense):
    return float(np.vdot(phi, solve(phi, th, mass)).real)


def fermion_force_xy(th, X, Y):
    """Ff_mu(x) = 2 Im[ U_mu(x) Y(x)^dag Hp_mu X(x+mu) - conj(U_mu(x)) Y(x+mu)^dag Hm_mu X(x) ] for ANY pair of spinor fields X, Y"""
    out = []
    I2 = np.eye(2)
    for mu, (U, sig) in enumerate(zip(links(th), (S1, S2))):
        Hp, Hm = 0.5 * (-I2 + sig), 0.5 * (-I2 - sig)
        a = np.einsum("xyr,rc,xyc->xy", np.conj(Y), Hp, cs.fwd(X, mu))
        b = np.einsum("xyr,rc,xyc->xy", np.conj(cs.fwd(Y, mu)), Hm, X)
        out.append(2.0 * np.imag(U * a - np.conj(U) * b))
    return out[0], out[1]


def fermion_force(th, phi, mass, solve=solve_dense):
    X = solve(phi, th, mass)
    return fermion_force_xy(th, X, D(X, th, mass))


def action(th, beta, phi=None, mass=0.0, solve=solve_dense):
    return gauge_action(th, beta) + (fermion_action(th, phi, mass, solve) if phi is not None else 0.0)


def force(th, beta, phi=None, mass=0.0, solve=solve_dense):
    fx, fy = gauge_force(th, beta)
    if phi is not None:
        gx, gy = fermion_force(th, phi, mass, solve)
        fx, fy = fx + gx, fy + gy
    return fx, fy


def hamiltonian(th, pi, beta, phi=None, mass=0.0, solve=solve_dense):
    return 0.5 * float(np.sum(pi[0] ** 2) + np.sum(pi[1] ** 2)) + action(th, beta, phi, mass, solve)


def leapfrog(th, pi, beta, tau, n_steps, phi=None, mass=0.0, solve=solve_dense):
    """Half step of the momenta, n_steps - 1 times (full link step, full momentum step), a last link step and half momentum step."""
    dt = tau / n_steps
    th = (th[0].copy(), th[1].copy())
    pi = (pi[0].copy(), pi[1].copy())

    def kick(e):
        f = force(th, beta, phi, mass, solve)
        return pi[0] - e * f[0], pi[1] - e * f[1]

    pi = kick(0.5 * dt)
    for k in range(n_steps):
        th = (th[0] + dt * pi[0], th[1] + dt * pi[1])
        pi = kick(dt if k + 1 < n_steps else 0.5 * dt)
    return th, pi


def md_dH(th, pi, beta, tau, n_steps, phi=None, mass=0.0, solve=solve_dense):
    """(end phases, end momenta, H_end - H_start)"""
    h0 = hamiltonian(th, pi, beta, phi, mass, solve)
    th1, pi1 = leapfrog(th, pi, beta, tau, n_steps, phi, mass, solve)
    return th1, pi1, hamiltonian(th1, pi1, beta, phi, mass, solve) - h0


def gauge_shift(th, a):
    """theta_mu(x) += a(x) - a(x + mu): the links become g(x) U_mu(x) conj g(x + mu) with g = exp(i a)"""
    return th[0] + a - cs.fwd(a, 0), th[1] + a - cs.fwd(a, 1)


def hmc_pure_gauge(L, beta, tau, n_steps, n_therm, n_meas, seed):
    """Pure-gauge HMC from a cold start; (mean plaquette over the measured trajectories, acceptance over them)"""
    rng = np.random.default_rng(seed)
    th = (np.zeros((L, L)), np.zeros((L, L)))
    plaq, acc = [], 0
    for t in range(n_therm + n_meas):
        pi = (rng.standard_normal((L, L)), rng.standard_normal((L, L)))
        th1, _, dH = md_dH(th, pi, beta, tau, n_steps)
        ok = rng.uniform() < np.exp(-dH)
        if ok:
            th = th1
        if t >= n_therm:
            acc += ok
            plaq.append(np.cos(plaquette_angle(th)).mean())
    return float(np.mean(plaq)), acc / n_meas


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
