"""Independent numpy / scipy statement of one-flavour RHMC for the Schwinger model, on top of hmc_numpy.py (which it does not change).

A helper, not a test.  Q = gamma5 D is Hermitian and Q^2 = D^dag D.  One flavour is the weight det D = det (Q^2)^(1/2), i.e. the pseudofermion
action S_pf = phi^dag r(Q^2) phi with r(y) ~ y^(-1/2) Zolotarev's optimal rational function of degree n on [ra^2, rb^2]:

  eps = (ra/rb)^2, k^2 = 1 - eps, K = K(k);  a_r = cn^2(r K/(2n+1), k) / sn^2(r K/(2n+1), k), r = 1 .. 2n (decreasing)
  r0(y) = A prod_j (y + a_{2j-1}) / (y + a_{2j}) on y in [eps, 1],  A = 2 / (max + min) of sqrt(y) prod(...),  delta = max |sqrt(y) r0(y) - 1|
  r(Q^2) = c0 prod_j (Q^2 + nu_j^2)/(Q^2 + mu_j^2) = c0 (1 + sum_j rho_j (Q^2 + mu_j^2)^-1),  nu_j^2 = rb^2 a_{2j-1}, mu_j^2 = rb^2 a_{2j}, c0 = A / rb
  heatbath: phi = c0^(-1/2) prod_j (Q + i mu_j)(Q + i nu_j)^-1 eta = c0^(-1/2) [eta + sum_j i s_j (Q - i nu_j)(Q^2 + nu_j^2)^-1 eta]

Here the elliptic functions are scipy's and A, delta come from a dense log grid; the C++ (include/qmg/rational.hpp) computes its own by the
arithmetic-geometric mean and takes the extrema at the end points.  tests/test_host_rhmc.py pins both against each other and these statements
against dense linear algebra before tests/test_gpu_rhmc.py judges the device by them.
"""
import numpy as np
from scipy import special

import hmc_numpy as hn

NEW_SYMBOLS = ["qmg_hmc_momentum_update_poles"]
NEW_BINDINGS = ["hmc_momentum_update_poles"]
# (n, eps, A, delta) as computed independently with scipy.special.ellipj on a 200001-point log grid
TABLE = [(4, 1e-2, 0.261413, 2.3426e-05), (6, 1e-3, 0.237074, 7.0073e-06), (8, 1e-3, 0.181292, 1.1866e-07), (10, 1e-4, 0.181636, 1.2311e-07),
         (12, 1e-4, 0.152575, 4.5654e-09)]


class Rational(object):
    pass


def zolotarev_a(n, eps):
    """a_r, r = 1 .. 2n, on the scaled interval [eps, 1]"""
    m = 1.0 - eps
    K = special.ellipk(m)
    sn, cn, _, _ = special.ellipj(np.arange(1, 2 * n + 1) * K / (2 * n + 1), m)
    return (cn / sn) ** 2


def scaled_product(y, a):
    """prod_j (y + a_{2j-1}) / (y + a_{2j}) for an array y"""
    y = np.asarray(y, dtype=np.float64)[..., None]
    return np.prod((y + a[0::2]) / (y + a[1::2]), axis=-1)


def zolotarev(n, ra, rb, grid=200001):
    """The coefficients of r(y) ~ y^(-1/2) on [ra^2, rb^2]; A and delta from a log grid of `grid` points over [eps, 1]"""
    z = Rational()
    eps = (ra / rb) ** 2
    a = zolotarev_a(n, eps)
    y = np.exp(np.linspace(np.log(eps), 0.0, grid))
    f = np.sqrt(y) * scaled_product(y, a)
    A = 2.0 / (f.max() + f.min())
    z.n, z.ra, z.rb, z.eps, z.a, z.A = n, ra, rb, eps, a, A
    z.delta = float(np.abs(A * f - 1.0).max())
    z.c0 = A / rb
    z.nu2, z.mu2 = rb * rb * a[0::2], rb * rb * a[1::2]
    nu, mu = np.sqrt(z.nu2), np.sqrt(z.mu2)
    z.rho, z.s = np.empty(n), np.empty(n)
    for j in range(n):
        o = np.arange(n) != j
        z.rho[j] = np.prod(z.nu2 - z.mu2[j]) / np.prod(z.mu2[o] - z.mu2[j])
        z.s[j] = np.prod(mu - nu[j]) / np.prod(nu[o] - nu[j])
    return z


def from_coefficients(n, ra, rb, c0, delta, mu2, nu2, rho, s):
    """the same object from numbers computed elsewhere (the C++ function's)"""
    z = Rational()
    z.n, z.ra, z.rb, z.eps, z.c0, z.delta = n, ra, rb, (ra / rb) ** 2, c0, delta
    z.mu2, z.nu2, z.rho, z.s = (np.asarray(v, dtype=np.float64) for v in (mu2, nu2, rho, s))
    z.A = c0 * rb
    z.a = np.empty(2 * n)
    z.a[0::2], z.a[1::2] = z.nu2 / (rb * rb), z.mu2 / (rb * rb)
    return z


def r_product(z, y):
    """r(y), product form, for y in [ra^2, rb^2]"""
    y = np.asarray(y, dtype=np.float64)[..., None]
    return z.c0 * np.prod((y + z.nu2) / (y + z.mu2), axis=-1)


def r_poles(z, y):
    """r(y), partial fractions"""
    y = np.asarray(y, dtype=np.float64)[..., None]
    return z.c0 * (1.0 + np.sum(z.rho / (y + z.mu2), axis=-1))


# ---- dense statements ----
def dense_Q(th, mass):
    """Q = gamma5 D on the flattened [x, y, spin] index; Hermitian"""
    M = hn.dense_D(th, mass)
    g5 = np.tile(hn.G5, M.shape[0] // 2)
    return g5[:, None] * M


def spectrum_Q2(th, mass):
    """(eigenvalues of Q^2 ascending, eigenvectors as columns)"""
    Q = dense_Q(th, mass)
    lam, vec = np.linalg.eigh(0.5 * (Q + Q.conj().T))
    o = np.argsort(lam * lam)
    return (lam * lam)[o], vec[:, o]


def dense_r(z, th, mass):
    """r(Q^2) as a matrix, by an eigendecomposition of Q"""
    Q = dense_Q(th, mass)
    lam, vec = np.linalg.eigh(0.5 * (Q + Q.conj().T))
    return (vec * r_product(z, lam * lam)[None, :]) @ vec.conj().T


def solve_shifts_dense(phi, th, mass, shifts):
    """[(D^dag D + sigma)^-1 phi for sigma in shifts] by LU"""
    M = hn.dense_D(th, mass)
    A = M.conj().T @ M
    return [np.linalg.solve(A + s * np.eye(A.shape[0]), phi.reshape(-1)).reshape(phi.shape) for s in shifts]


def make_cg_m(eps, max_iter=100000, iters=None):
    """Multi-shift CG from zero in CG's own notation, anchored on the smallest shift; shift s stops when zeta_s |r| < eps |phi| (its recurrence
    residual), the run when the smallest has.  iters: a list that collects counts."""
    def solve(phi, th, mass, shifts):
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
            Ap = hn.Ddag(hn.D(p, th, mass), th, mass) + shifts[base] * p
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
                if zeta[s] * np.sqrt(new) < eps * bn:
                    live[s] = False
            alpha_old, beta_old, rsq = alpha, beta, new
            k += 1
        if iters is not None:
            iters.append(k)
        return xs
    return solve


def apply_Q(psi, th, mass):
    return hn.G5 * hn.D(psi, th, mass)


def apply_rational(z, v, th, mass, solve=solve_shifts_dense):
    """r(Q^2) v = c0 (v + sum_j rho_j (Q^2 + mu_j^2)^-1 v)"""
    X = solve(v, th, mass, z.mu2)
    return z.c0 * (v + sum(rho * x for rho, x in zip(z.rho, X)))


def pf_action(z, th, phi, mass, solve=solve_shifts_dense):
    X = solve(phi, th, mass, z.mu2)
    return float(z.c0 * (np.vdot(phi, phi).real + sum(rho * np.vdot(phi, x).real for rho, x in zip(z.rho, X))))


def pf_force(z, th, phi, mass, solve=solve_shifts_dense):
    """dS_pf/dtheta = c0 sum_j rho_j Ff(X_j, D X_j)"""
    X = solve(phi, th, mass, z.mu2)
    fx, fy = np.zeros(th[0].shape), np.zeros(th[0].shape)
    for rho, x in zip(z.rho, X):
        gx, gy = hn.fermion_force_xy(th, x, hn.D(x, th, mass))
        fx, fy = fx + z.c0 * rho * gx, fy + z.c0 * rho * gy
    return fx, fy


def heatbath(z, th, eta, mass, solve=solve_shifts_dense):
    """phi = B eta with B B^dag = r(Q^2)^-1: phi = c0^(-1/2) [eta + Q (sum_j i s_j Z_j) + sum_j s_j nu_j Z_j], Z_j = (Q^2 + nu_j^2)^-1 eta"""
    Z = solve(eta, th, mass, z.nu2)
    nu = np.sqrt(z.nu2)
    w = sum(1j * s * zj for s, zj in zip(z.s, Z))
    v = sum(s * n * zj for s, n, zj in zip(z.s, nu, Z))
    return (eta + apply_Q(w, th, mass) + v) / np.sqrt(z.c0)


def range_check(z, th, xi, mass, solve=solve_shifts_dense):
    """(|xi^dag (r Q^2 r - 1) xi| / xi^dag xi, the bound 2 delta + delta^2): the ratio cannot exceed the bound while the spectrum of Q^2 is
    inside [ra^2, rb^2]"""
    w = apply_rational(z, xi, th, mass, solve)
    qw = apply_Q(w, th, mass)
    n = np.vdot(xi, xi).real
    return abs(np.vdot(qw, qw).real - n) / n, 2.0 * z.delta + z.delta ** 2


def action(z, th, beta, phi, mass, solve=solve_shifts_dense):
    return hn.gauge_action(th, beta) + pf_action(z, th, phi, mass, solve)


def force(z, th, beta, phi, mass, solve=solve_shifts_dense):
    fx, fy = hn.gauge_force(th, beta)
    gx, gy = pf_force(z, th, phi, mass, solve)
    return fx + gx, fy + gy


def hamiltonian(z, th, pi, beta, phi, mass, solve=solve_shifts_dense):
    return 0.5 * float(np.sum(pi[0] ** 2) + np.sum(pi[1] ** 2)) + action(z, th, beta, phi, mass, solve)


def leapfrog(z, th, pi, beta, tau, n_steps, phi, mass, solve=solve_shifts_dense):
    """hmc_numpy.leapfrog with the rational force"""
    dt = tau / n_steps
    th = (th[0].copy(), th[1].copy())
    pi = (pi[0].copy(), pi[1].copy())

    def kick(e):
        f = force(z, th, beta, phi, mass, solve)
        return pi[0] - e * f[0], pi[1] - e * f[1]

    pi = kick(0.5 * dt)
    for k in range(n_steps):
        th = (th[0] + dt * pi[0], th[1] + dt * pi[1])
        pi = kick(dt if k + 1 < n_steps else 0.5 * dt)
    return th, pi


def md_dH(z, th, pi, beta, tau, n_steps, phi, mass, solve=solve_shifts_dense):
    """(end phases, end momenta, H_end - H_start)"""
    h0 = hamiltonian(z, th, pi, beta, phi, mass, solve)
    th1, pi1 = leapfrog(z, th, pi, beta, tau, n_steps, phi, mass, solve)
    return th1, pi1, hamiltonian(z, th1, pi1, beta, phi, mass, solve) - h0
