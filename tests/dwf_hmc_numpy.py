"""Independent numpy statement of two-flavour domain-wall HMC for the Schwinger model with Pauli-Villars fields on even-site pseudofermions.

A helper, not a test.  A field is psi[x, y, s, sigma] (any trailing axes) on coordinate grids; a vector "on the even sites" is a full grid that
vanishes on the odd ones.  The hops and Gamma5 come from dwf_numpy, the blocks of the site-local A from dwf_eo_numpy (inverted by its long double
Gauss-Jordan), gauge action, gauge force and the Wilson force bilinear from hmc_numpy.  Nothing here shares the even-odd index algebra of
csrc/qmg_hmc.hip or include/qmg/hmc_dwf.hpp; only coordspace's layout functions move data in and out.  tests/test_host_dwf_hmc.py pins these
statements before tests/test_gpu_dwf_hmc.py judges the device by them.

  D(m) = A(m) + H,   A = (3 + M5) - (shift along s) + m (wall),   H: the Wilson hops on every slice (w = 1)
  M(m) = A_ee - H_eo A_oo^-1 H_oe,   det D = det A_oo det M,   Gamma5 M Gamma5 = M^dag,   P = M(1)
  S_f = phi^dag P (M^dag M)^-1 P^dag phi;   heatbath phi = P (P^dag P)^-1 M^dag eta,  S_f(phi) = |eta|^2
  chi = P^dag phi,  X = (M^dag M)^-1 chi,  Y = M X,  and on the full lattice
     X5  = X (+) -A_oo(m)^-1 H_oe X       Y5  = Gamma5 [G5Y   (+) -A_oo(m)^-1 H_oe G5Y],    G5Y   = Gamma5 Y
     X5' = X (+) -A_oo(1)^-1 H_oe X       Y5' = Gamma5 [G5phi (+) -A_oo(1)^-1 H_oe G5phi],  G5phi = Gamma5 phi
  dS_f/dtheta_mu(x) = sum_s [Ff_mu(x; X5(s), Y5(s)) - Ff_mu(x; X5'(s), Y5'(s))],   Ff = hmc_numpy.fermion_force_xy
"""
import numpy as np

import coordspace as cs
import dwf_eo_numpy as de
import dwf_numpy as dn
import hmc_numpy as hn

NEW_SYMBOLS = ["qmg_hmc_momentum_update_dwf", "qmg_hmc_dwf_plan"]
NEW_BINDINGS = ["hmc_momentum_update_dwf", "hmc_momentum_update_dwf_status", "hmc_dwf_plan", "hmc_dwf_plan_status"]
M5 = -1.0


def even(Lx, Ly):
    return ((np.arange(Lx)[:, None] + np.arange(Ly)[None, :]) % 2) == 0


def _on(mask, psi):
    """mask[x, y] against psi[x, y, s, sigma, ...]"""
    return mask.reshape(mask.shape + (1,) * (psi.ndim - 2))


def keep(psi, parity):
    """psi on the sites of one parity, zero elsewhere"""
    Lx, Ly = psi.shape[:2]
    return np.where(_on(even(Lx, Ly) == (parity == 0), psi), psi, 0.0)


def hops(psi, th):
    """H psi"""
    Ux, Uy = hn.links(th)
    out = np.zeros_like(psi)
    for axis, step, link, mat in dn.hop_terms(Ux, Uy, 1.0, np.complex128):
        out = out + _on(link, psi) * np.einsum("ab,xysb...->xysa...", mat, np.roll(psi, step, axis=axis))
    return out


def apply_A(psi, m, m5=M5):
    """A(m) psi: the diagonal 3 + M5, the shift along s, the wall (dwf_eo_numpy.apply_A's statement with room for trailing axes)"""
    Ls = psi.shape[2]
    out = (3.0 + m5) * psi
    out[:, :, 1:, 0] -= psi[:, :, :-1, 0]
    out[:, :, :-1, 1] -= psi[:, :, 1:, 1]
    out[:, :, 0, 0] += m * psi[:, :, Ls - 1, 0]
    out[:, :, Ls - 1, 1] += m * psi[:, :, 0, 1]
    return out


def apply_A_inv(psi, m, m5=M5):
    """A(m)^-1 psi through the Ls x Ls spin blocks, inverted by Gauss-Jordan elimination in long double"""
    Ls = psi.shape[2]
    blocks = [de.gauss_jordan(a).astype(np.complex128) for a in de.a_blocks(Ls, de.diag(1.0, m5, 0.0, 0), m)]
    out = np.empty_like(psi)
    for g in (0, 1):
        out[:, :, :, g] = np.einsum("st,xyt...->xys...", blocks[g], psi[:, :, :, g])
    return out


def D(psi, th, m, m5=M5):
    return apply_A(psi, m, m5) + hops(psi, th)


def fill_odd(v, th, m, m5=M5):
    """v_e (+) -A_oo(m)^-1 H_oe v_e"""
    ve = keep(v, 0)
    return ve - keep(apply_A_inv(hops(ve, th), m, m5), 1)


def M(v, th, m, m5=M5):
    """M(m) v on the even sites: A v - H A^-1 H v"""
    ve = keep(v, 0)
    return apply_A(ve, m, m5) - keep(hops(apply_A_inv(hops(ve, th), m, m5), th), 0)


def Mdag(v, th, m, m5=M5):
    return dn.gamma5_grid(M(dn.gamma5_grid(v), th, m, m5))


def MdagM(v, th, m, m5=M5):
    return Mdag(M(v, th, m, m5), th, m, m5)


# ---- dense matrices over the flattened [x, y, s, sigma] index ----
def dense(fn, Lx, Ly, Ls):
    """the matrix of a linear map on psi[x, y, s, sigma, ...] grids: the map applied to all unit vectors at once"""
    n = Lx * Ly * Ls * 2
    return fn(np.eye(n, dtype=np.complex128).reshape(Lx, Ly, Ls, 2, n)).reshape(n, n)


def even_index(Lx, Ly, Ls):
    return np.broadcast_to(even(Lx, Ly)[:, :, None, None], (Lx, Ly, Ls, 2)).reshape(-1)


def dense_M(th, m, Ls, m5=M5):
    """M(m) restricted to the even sites"""
    Lx, Ly = th[0].shape
    ev = even_index(Lx, Ly, Ls)
    return dense(lambda v: M(v, th, m, m5), Lx, Ly, Ls)[np.ix_(ev, ev)]


def logdets(th, m, Ls, m5=M5):
    """(log |det D|, log |det A_oo| + log |det M|)"""
    Lx, Ly = th[0].shape
    od = ~even_index(Lx, Ly, Ls)
    Dm = dense(lambda v: D(v, th, m, m5), Lx, Ly, Ls)
    Am = dense(lambda v: apply_A(v, m, m5), Lx, Ly, Ls)[np.ix_(od, od)]
    return np.linalg.slogdet(Dm)[1], np.linalg.slogdet(Am)[1] + np.linalg.slogdet(dense_M(th, m, Ls, m5))[1]


# ---- solvers on the even sites: X = (M(m)^dag M(m))^-1 b as a full grid ----
def solve_dense(b, th, m, m5=M5):
    Lx, Ly, Ls = b.shape[:3]
    ev = even_index(Lx, Ly, Ls)
    Mm = dense_M(th, m, Ls, m5)
    x = np.zeros(b.size, dtype=np.complex128)
    x[ev] = np.linalg.solve(Mm.conj().T @ Mm, b.reshape(-1)[ev])
    return x.reshape(b.shape)


def make_cg(eps, max_iter=100000, iters=None):
    """plain CG from zero, stopped like the library's: recursive |r| < eps |b|.  iters: a list that collects counts."""
    def solve(b, th, m, m5=M5):
        x = np.zeros_like(b)
        r = keep(b, 0)
        p = r.copy()
        rsq = np.vdot(r, r).real
        stop = eps * eps * rsq
        k = 0
        while rsq >= stop and k < max_iter:
            Ap = MdagM(p, th, m, m5)
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


# ---- the action, its force, the heatbath ----
def fermion_action(th, phi, m, solve=solve_dense, m5=M5):
    chi = Mdag(phi, th, 1.0, m5)
    return float(np.vdot(chi, solve(chi, th, m, m5)).real)


def force_pairs(th, X, Y, weights, g5_y=False):
    """sum_j weights[j] sum_s Ff(X[j](.; s), Y[j](.; s)) for ANY full-lattice fields; g5_y: every Y[j] is read as Gamma5 Y[j]"""
    Lx, Ly = th[0].shape
    fx, fy = np.zeros((Lx, Ly)), np.zeros((Lx, Ly))
    for w, x, y in zip(weights, X, Y):
        if g5_y:
            y = dn.gamma5_grid(y)
        for s in range(x.shape[2]):
            gx, gy = hn.fermion_force_xy(th, x[:, :, s], y[:, :, s])
            fx, fy = fx + w * gx, fy + w * gy
    return fx, fy


def force_fields(th, phi, m, solve=solve_dense, m5=M5):
    """(X5, X5'), (Gamma5 Y5, Gamma5 Y5'): the fields of the kick, the second list as the device passes it (to be read through Gamma5)"""
    chi = Mdag(phi, th, 1.0, m5)
    X = solve(chi, th, m, m5)
    g5y, g5phi = dn.gamma5_grid(M(X, th, m, m5)), dn.gamma5_grid(keep(phi, 0))
    return (fill_odd(X, th, m, m5), fill_odd(X, th, 1.0, m5)), (fill_odd(g5y, th, m, m5), fill_odd(g5phi, th, 1.0, m5))


def fermion_force(th, phi, m, solve=solve_dense, m5=M5):
    X, Z = force_fields(th, phi, m, solve, m5)
    return force_pairs(th, X, Z, (1.0, -1.0), g5_y=True)


def heatbath(th, eta, m, solve=solve_dense, m5=M5):
    """phi = P (P^dag P)^-1 M^dag eta on the even sites"""
    return M(solve(Mdag(eta, th, m, m5), th, 1.0, m5), th, 1.0, m5)


def action(th, beta, phi=None, m=0.0, solve=solve_dense):
    return hn.gauge_action(th, beta) + (fermion_action(th, phi, m, solve) if phi is not None else 0.0)


def force(th, beta, phi=None, m=0.0, solve=solve_dense):
    fx, fy = hn.gauge_force(th, beta)
    if phi is not None:
        gx, gy = fermion_force(th, phi, m, solve)
        fx, fy = fx + gx, fy + gy
    return fx, fy


def hamiltonian(th, pi, beta, phi=None, m=0.0, solve=solve_dense):
    return 0.5 * float(np.sum(pi[0] ** 2) + np.sum(pi[1] ** 2)) + action(th, beta, phi, m, solve)


def leapfrog(th, pi, beta, tau, n_steps, phi=None, m=0.0, solve=solve_dense):
    """hmc_numpy.leapfrog with the domain-wall force"""
    dt = tau / n_steps
    th = (th[0].copy(), th[1].copy())
    pi = (pi[0].copy(), pi[1].copy())

    def kick(e):
        f = force(th, beta, phi, m, solve)
        return pi[0] - e * f[0], pi[1] - e * f[1]

    pi = kick(0.5 * dt)
    for k in range(n_steps):
        th = (th[0] + dt * pi[0], th[1] + dt * pi[1])
        pi = kick(dt if k + 1 < n_steps else 0.5 * dt)
    return th, pi


def md_dH(th, pi, beta, tau, n_steps, phi=None, m=0.0, solve=solve_dense):
    """(end phases, end momenta, H_end - H_start)"""
    h0 = hamiltonian(th, pi, beta, phi, m, solve)
    th1, pi1 = leapfrog(th, pi, beta, tau, n_steps, phi, m, solve)
    return th1, pi1, hamiltonian(th1, pi1, beta, phi, m, solve) - h0


def gauge_rotate(psi, a):
    """psi(x) -> exp(i a(x)) psi(x), the companion of hmc_numpy.gauge_shift"""
    return _on(np.exp(1j * a), psi) * psi


# ---- a whole run, for the acceptance band of the driver test ----
def hmc_run(L, Ls, beta, m, n_steps, n_therm, n_meas, seed, tau=1.0):
    """HMC from a cold start with dense solves; (mean plaquette, acceptance, mean exp(-dH)) over the measured trajectories"""
    rng = np.random.default_rng(seed)
    th = (np.zeros((L, L)), np.zeros((L, L)))
    plaq, w, acc = [], [], 0
    for t in range(n_therm + n_meas):
        pi = (rng.standard_normal((L, L)), rng.standard_normal((L, L)))
        e = keep((rng.standard_normal((L, L, Ls, 2)) + 1j * rng.standard_normal((L, L, Ls, 2))) / np.sqrt(2.0), 0)
        phi = heatbath(th, e, m)
        th1, _, dH = md_dH(th, pi, beta, tau, n_steps, phi, m)
        ok = rng.uniform() < np.exp(-dH)
        if ok:
            th = th1
        if t >= n_therm:
            acc += ok
            w.append(np.exp(-dH))
            plaq.append(np.cos(hn.plaquette_angle(th)).mean())
    return float(np.mean(plaq)), acc / n_meas, float(np.mean(w))


# ---- layout: psi[x, y, s, sigma] <-> the device's nc = 2 Ls vectors (c = 2 s + sigma), whole and even half ----
def grid_to_eo(psi):
    Lx, Ly, Ls = psi.shape[:3]
    return cs.grid_to_eo(psi.reshape(Lx, Ly, 2 * Ls), Lx, Ly, 2 * Ls)


def eo_to_grid(v, Lx, Ly, Ls):
    return cs.eo_to_grid(np.asarray(v, dtype=np.complex128), Lx, Ly, 2 * Ls).reshape(Lx, Ly, Ls, 2).copy()


def even_to_half(psi):
    """the first half (the even sites) of the device layout"""
    return grid_to_eo(psi)[: psi.size // 2].copy()


def half_to_even(h, Lx, Ly, Ls):
    return eo_to_grid(np.concatenate([np.asarray(h, dtype=np.complex128), np.zeros(Lx * Ly * Ls, dtype=np.complex128)]), Lx, Ly, Ls)


def slices_to_eo(psi):
    """the Ls slices of psi as separate nc = 2 device vectors (what qmg_hmc_momentum_update_poles takes)"""
    Lx, Ly, Ls = psi.shape[:3]
    return [cs.grid_to_eo(psi[:, :, s], Lx, Ly, 2) for s in range(Ls)]
