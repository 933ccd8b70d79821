"""Independent numpy statement of staggered HMC (two tastes) and rooted RHMC (one taste) for the Schwinger model with even-odd pseudofermions.

A helper, not a test.  Everything is an [x, y] grid moved with np.roll; vectors on the even sites are full grids that vanish on the odd ones.
Nothing here shares the even-odd index algebra of csrc/qmg_hmc.hip or include/qmg/hmc_staggered.hpp; only coordspace's layout functions move
data in and out.  tests/test_host_stag_hmc.py pins these statements (the oracle's staggered apply, finite differences of the dense action,
gauge covariance, reversibility, the heatbath identities) before tests/test_gpu_stag_hmc.py judges the device by them.

  D = m + H,   H psi(x) = s/2 sum_mu eta_mu(x) [U_mu(x) psi(x+mu) - conj(U_mu(x-mu)) psi(x-mu)],   eta_x = 1, eta_y = (-1)^x,   s = SIGN
  A = D^dag D = m^2 - H^2 (block diagonal in parity),   eps(x) = (-1)^(x+y)
  two tastes:  S_f = phi_e^dag A_ee^-1 phi_e,  phi_e = (D^dag eta)_e
  one taste:   S_pf = phi_e^dag r(A_ee) phi_e,  r = Zolotarev's approximation of y^(-1/2) on [m^2, m^2 + 4] (rhmc_numpy.zolotarev(n, m, sqrt(m^2 + 4)))
  force:       W = X_e (+) (H X_e)_o,  dS/dtheta_mu(x) = -s eta_mu(x) eps(x) Im[U_mu(x) conj(W(x)) W(x+mu)]
"""
import numpy as np

import coordspace as cs
import hmc_numpy as hn
import rhmc_numpy as rn

NEW_SYMBOLS = ["qmg_hmc_momentum_update_staggered"]
NEW_BINDINGS = ["hmc_momentum_update_staggered"]
SIGN = -1.0   # the project's stencil apply of the reference's -0.5 U / +0.5 U^dag fill; pinned against the CPU oracle in test_host_stag_hmc.py


def eta(Lx, Ly):
    x = np.arange(Lx)[:, None]
    return np.ones((Lx, Ly)), (1.0 - 2.0 * (x % 2)) * np.ones((Lx, Ly))


def eps(Lx, Ly):
    return 1.0 - 2.0 * ((np.arange(Lx)[:, None] + np.arange(Ly)[None, :]) % 2)


def even(Lx, Ly):
    return eps(Lx, Ly) > 0


def H(psi, th, sign=SIGN):
    Lx, Ly = psi.shape
    out = np.zeros_like(psi)
    for mu, (U, e) in enumerate(zip(hn.links(th), eta(Lx, Ly))):
        out = out + 0.5 * sign * e * (U * cs.fwd(psi, mu) - np.conj(cs.bwd(U, mu)) * cs.bwd(psi, mu))
    return out


def D(psi, th, mass, sign=SIGN):
    return mass * psi + H(psi, th, sign)


def A(psi, th, mass, sign=SIGN):
    """m^2 - H^2; keeps a vector on the even sites there"""
    return mass * mass * psi - H(H(psi, th, sign), th, sign)


def dense(fn, Lx, Ly):
    """the matrix of a linear map on [x, y] grids over the flattened index"""
    n = Lx * Ly
    M = np.empty((n, n), dtype=np.complex128)
    for j in range(n):
        e = np.zeros(n, dtype=np.complex128)
        e[j] = 1.0
        M[:, j] = fn(e.reshape(Lx, Ly)).reshape(-1)
    return M


def dense_A_ee(th, mass, sign=SIGN):
    """A restricted to the even sites (row-major order of the even sites of the [x, y] grid)"""
    Lx, Ly = th[0].shape
    ev = even(Lx, Ly).reshape(-1)
    return dense(lambda v: A(v, th, mass, sign), Lx, Ly)[np.ix_(ev, ev)]


# ---- solvers on the even sites: each returns [(A_ee + sigma)^-1 phi for sigma in shifts] as full grids ----
def solve_dense(phi, th, mass, shifts=(0.0,), sign=SIGN):
    Lx, Ly = phi.shape
    ev = even(Lx, Ly)
    M = dense_A_ee(th, mass, sign)
    out = []
    for s in shifts:
        x = np.zeros_like(phi)
        x[ev] = np.linalg.solve(M + s * np.eye(M.shape[0]), phi[ev])
        out.append(x)
    return out


def make_cg(eps_, max_iter=100000, iters=None, op=None):
    """Multi-shift CG from zero (plain CG for one shift), anchored on the smallest shift; shift s stops when zeta_s |r| < eps |phi|, the run
    when the smallest has.  op(p, th, mass, sign): the operator, A by default.  iters: a list that collects counts."""
    def solve(phi, th, mass, shifts=(0.0,), sign=SIGN):
        apply = op if op is not None else A
        shifts = np.asarray(shifts, dtype=np.float64)
        ns = len(shifts)
        base = int(np.argmin(shifts))
        ds = shifts - shifts[base]
        xs = [np.zeros_like(phi) for _ in range(ns)]
        ps = [phi.copy() for _ in range(ns)]
        r = phi.copy()
        rsq = np.vdot(r, r).real
        bn = np.sqrt(rsq)
        zeta, zeta_old = np.ones(ns), np.ones(ns)
        alpha_old, beta_old = 1.0, 0.0
        live = np.ones(ns, dtype=bool)
        k = 0
        while live[base] and k < max_iter:
            p = ps[base]
            Ap = apply(p, th, mass, sign) + shifts[base] * p
            alpha = rsq / np.vdot(p, Ap).real
            r = r - alpha * Ap
            new = np.vdot(r, r).real
            beta = new / rsq
            for s in range(ns):
                if not live[s]:
                    continue
                ratio = zeta_old[s] * alpha_old / (alpha * beta_old * (zeta_old[s] - zeta[s]) + zeta_old[s] * alpha_old * (1.0 + ds[s] * alpha))
                zeta_old[s], zeta[s] = zeta[s], zeta[s] * ratio
                xs[s] = xs[s] + alpha * ratio * ps[s]
                ps[s] = zeta[s] * r + beta * ratio * ratio * ps[s]
                if zeta[s] * np.sqrt(new) < eps_ * bn:
                    live[s] = False
            alpha_old, beta_old, rsq = alpha, beta, new
            k += 1
        if iters is not None:
            iters.append(k)
        return xs
    return solve


# ---- the action, its force ----
def rational(n, mass):
    return rn.zolotarev(n, mass, np.sqrt(mass * mass + 4.0))


def force_W(th, W, sign=SIGN):
    """-s eta_mu(x) eps(x) Im[U_mu(x) conj(W(x)) W(x+mu)] for ANY full-lattice W"""
    Lx, Ly = W.shape
    e = eps(Lx, Ly)
    return tuple(-sign * et * e * np.imag(U * np.conj(W) * cs.fwd(W, mu)) for mu, (U, et) in enumerate(zip(hn.links(th), eta(Lx, Ly))))


def make_W(X, th, sign=SIGN):
    """X_e (+) (H X_e)_o"""
    return X + H(X, th, sign)


def poles(z):
    """(shifts, weights, constant) of S = const phi^dag phi + sum_j weights_j phi^dag (A_ee + shifts_j)^-1 phi; z = None: two tastes"""
    if z is None:
        return np.array([0.0]), np.array([1.0]), 0.0
    return z.mu2, z.c0 * z.rho, z.c0


def fermion_action(th, phi, mass, z=None, solve=solve_dense, sign=SIGN):
    sh, w, c = poles(z)
    X = solve(phi, th, mass, sh, sign)
    return float(c * np.vdot(phi, phi).real + sum(wj * np.vdot(phi, x).real for wj, x in zip(w, X)))


def fermion_force(th, phi, mass, z=None, solve=solve_dense, sign=SIGN):
    sh, w, _ = poles(z)
    X = solve(phi, th, mass, sh, sign)
    fx, fy = np.zeros(phi.shape), np.zeros(phi.shape)
    for wj, x in zip(w, X):
        gx, gy = force_W(th, make_W(x, th, sign), sign)
        fx, fy = fx + wj * gx, fy + wj * gy
    return fx, fy


def apply_rational(z, v, th, mass, solve=solve_dense, sign=SIGN):
    """r(A_ee) v = c0 (v + sum_j rho_j (A_ee + mu_j^2)^-1 v)"""
    X = solve(v, th, mass, z.mu2, sign)
    return z.c0 * (v + sum(rho * x for rho, x in zip(z.rho, X)))


def action(th, beta, phi=None, mass=0.0, z=None, solve=solve_dense, sign=SIGN):
    return hn.gauge_action(th, beta) + (fermion_action(th, phi, mass, z, solve, sign) if phi is not None else 0.0)


def force(th, beta, phi=None, mass=0.0, z=None, solve=solve_dense, sign=SIGN):
    fx, fy = hn.gauge_force(th, beta)
    if phi is not None:
        gx, gy = fermion_force(th, phi, mass, z, solve, sign)
        fx, fy = fx + gx, fy + gy
    return fx, fy


def hamiltonian(th, pi, beta, phi=None, mass=0.0, z=None, solve=solve_dense, sign=SIGN):
    return 0.5 * float(np.sum(pi[0] ** 2) + np.sum(pi[1] ** 2)) + action(th, beta, phi, mass, z, solve, sign)


def leapfrog(th, pi, beta, tau, n_steps, phi=None, mass=0.0, z=None, solve=solve_dense, sign=SIGN):
    """hmc_numpy.leapfrog with the staggered force"""
    dt = tau / n_steps
    th = (th[0].copy(), th[1].copy())
    pi = (pi[0].copy(), pi[1].copy())

    def kick(e):
        f = force(th, beta, phi, mass, z, solve, sign)
        return pi[0] - e * f[0], pi[1] - e * f[1]

    pi = kick(0.5 * dt)
    for k in range(n_steps):
        th = (th[0] + dt * pi[0], th[1] + dt * pi[1])
        pi = kick(dt if k + 1 < n_steps else 0.5 * dt)
    return th, pi


def md_dH(th, pi, beta, tau, n_steps, phi=None, mass=0.0, z=None, solve=solve_dense, sign=SIGN):
    """(end phases, end momenta, H_end - H_start)"""
    h0 = hamiltonian(th, pi, beta, phi, mass, z, solve, sign)
    th1, pi1 = leapfrog(th, pi, beta, tau, n_steps, phi, mass, z, solve, sign)
    return th1, pi1, hamiltonian(th1, pi1, beta, phi, mass, z, solve, sign) - h0


# ---- heatbaths: eta on the full lattice, phi on the even sites ----
def heatbath_two(th, eta_full, mass, sign=SIGN):
    """phi_e = (D^dag eta)_e = m eta_e - (H eta)_e"""
    Lx, Ly = eta_full.shape
    return np.where(even(Lx, Ly), mass * eta_full - H(eta_full, th, sign), 0.0)


def primed(z, mass):
    """(mu'_j, nu'_j, s'_j): A + nu^2 = K^2 + nu'^2 with K = i H"""
    mup, nup = np.sqrt(mass * mass + z.mu2), np.sqrt(mass * mass + z.nu2)
    sp = np.empty(z.n)
    for j in range(z.n):
        o = np.arange(z.n) != j
        sp[j] = np.prod(mup - nup[j]) / np.prod(nup[o] - nup[j])
    return mup, nup, sp


def solve_K2_dense(eta_full, th, shifts, sign=SIGN):
    Lx, Ly = eta_full.shape
    M = -np.linalg.matrix_power(dense(lambda v: H(v, th, sign), Lx, Ly), 2)
    return [np.linalg.solve(M + s * np.eye(Lx * Ly), eta_full.reshape(-1)).reshape(Lx, Ly) for s in shifts]


def make_cg_K2(eps_, iters=None):
    """multi-shift CG on -H^2 over the full lattice, in the call shape of solve_K2_dense"""
    cg = make_cg(eps_, iters=iters, op=lambda p, th, mass, sign: -H(H(p, th, sign), th, sign))
    return lambda eta_full, th, shifts, sign=SIGN: cg(eta_full, th, 0.0, shifts, sign)


def heatbath_full(z, th, eta_full, mass, solve=solve_K2_dense, sign=SIGN):
    """B eta on the full lattice, B = c0^(-1/2) [1 + sum_j i s'_j (K - i nu'_j)(K^2 + nu'_j^2)^-1], K = i H:
    c0^(-1/2) [eta - H (sum_j s'_j Z_j) + sum_j s'_j nu'_j Z_j], Z_j = (-H^2 + nu'_j^2)^-1 eta"""
    mup, nup, sp = primed(z, mass)
    Z = solve(eta_full, th, nup ** 2, sign)
    w = sum(s * zj for s, zj in zip(sp, Z))
    v = sum(s * n * zj for s, n, zj in zip(sp, nup, Z))
    return (eta_full - H(w, th, sign) + v) / np.sqrt(z.c0)


def heatbath_one(z, th, eta_full, mass, solve=solve_K2_dense, sign=SIGN):
    """the even half of B eta"""
    Lx, Ly = eta_full.shape
    return np.where(even(Lx, Ly), heatbath_full(z, th, eta_full, mass, solve, sign), 0.0)


def dense_B(z, th, mass, sign=SIGN):
    Lx, Ly = th[0].shape
    return dense(lambda v: heatbath_full(z, th, v, mass, solve_K2_dense, sign), Lx, Ly)


def dense_r_full(z, th, mass, sign=SIGN):
    """r(A) on the full lattice by an eigendecomposition"""
    Lx, Ly = th[0].shape
    M = dense(lambda v: A(v, th, mass, sign), Lx, Ly)
    lam, vec = np.linalg.eigh(0.5 * (M + M.conj().T))
    return (vec * rn.r_product(z, lam)[None, :]) @ vec.conj().T


# ---- a whole run, for the plaquette of the driver test ----
def hmc_run(L, beta, mass, n_tastes, n_steps, n_therm, n_meas, seed, degree=8, tau=1.0):
    """HMC from a cold start with dense solves; (mean plaquette, acceptance, mean exp(-dH)) over the measured trajectories"""
    rng = np.random.default_rng(seed)
    z = rational(degree, mass) if n_tastes == 1 else None
    th = (np.zeros((L, L)), np.zeros((L, L)))
    plaq, w, acc = [], [], 0
    for t in range(n_therm + n_meas):
        pi = (rng.standard_normal((L, L)), rng.standard_normal((L, L)))
        e = (rng.standard_normal((L, L)) + 1j * rng.standard_normal((L, L))) / np.sqrt(2.0)
        phi = heatbath_one(z, th, e, mass) if n_tastes == 1 else heatbath_two(th, e, mass)
        th1, _, dH = md_dH(th, pi, beta, tau, n_steps, phi, mass, z)
        ok = rng.uniform() < np.exp(-dH)
        if ok:
            th = th1
        if t >= n_therm:
            acc += ok
            w.append(np.exp(-dH))
            plaq.append(np.cos(hn.plaquette_angle(th)).mean())
    return float(np.mean(plaq)), acc / n_meas, float(np.mean(w))


# ---- layout: even-site grids <-> the device's half vectors ----
def grid_to_eo(v):
    Lx, Ly = v.shape
    return cs.grid_to_eo(v[:, :, None], Lx, Ly, 1)


def eo_to_grid(v, Lx, Ly):
    return cs.eo_to_grid(np.asarray(v, dtype=np.complex128), Lx, Ly, 1)[:, :, 0].copy()


def even_to_half(v):
    """the first half (the even sites) of the device layout"""
    return grid_to_eo(v)[: v.size // 2].copy()


def half_to_even(h, Lx, Ly):
    return eo_to_grid(np.concatenate([np.asarray(h, dtype=np.complex128), np.zeros(Lx * Ly // 2, dtype=np.complex128)]), Lx, Ly)
