"""Independent numpy statement of stout-smeared Wilson fermions in the Schwinger-model HMC, on top of hmc_numpy.py and rhmc_numpy.py (which
it does not change): (x, y) grids with np.roll, no even-odd index algebra.

A helper, not a test.  Link fields (phases, momenta, forces) are (Fx, Fy) pairs of [x, y] grids, plaquette fields single grids.

  curl       (C F)(x) = F_x(x) + F_y(x+xhat) - F_x(x+yhat) - F_y(x)                 -- P = C theta
  transpose  (C^T g)_x(x) = g(x) - g(x-yhat),  (C^T g)_y(x) = -g(x) + g(x-xhat)     -- dS_w/dtheta = C^T sin P,  S_w = sum_x (1 - cos P)
  one level  theta^(k+1) = theta^(k) - rho C^T sin P^(k)                            -- an Euler step of the Wilson flow of length rho
  Jacobian   J_k = 1 - rho C^T diag(cos P^(k)) C                                    -- symmetric

The fermions live on V = theta^(n), the gauge action on the thin links theta^(0):
  S = beta sum_x (1 - cos P^(0)) + S_f[theta^(n)],   dS_f/dtheta^(0) = J_0 J_1 .. J_(n-1) (dS_f/dV)
with S_f the two-flavour action of hmc_numpy or, with a rational function z (rhmc_numpy.Rational), the pole-list action of rhmc_numpy.
tests/test_host_stout.py pins these statements (finite differences, symmetry, covariance, reversibility, the dt^2 law) before
tests/test_gpu_stout.py judges the device (csrc/qmg_stout.hip, include/qmg/stout.hpp) by them.
"""
import numpy as np

import coordspace as cs
import hmc_numpy as hn
import rhmc_numpy as rn

NEW_SYMBOLS = ["qmg_u1_stout_smear", "qmg_hmc_fermion_force", "qmg_u1_stout_force_level", "qmg_hmc_momentum_update_stout"]
NEW_BINDINGS = ["u1_stout_smear", "hmc_fermion_force", "u1_stout_force_level", "hmc_momentum_update_stout"]


def curl(F):
    return F[0] + cs.fwd(F[1], 0) - cs.fwd(F[0], 1) - F[1]


def curl_T(g):
    return g - cs.bwd(g, 1), -g + cs.bwd(g, 0)


def smear_level(th, rho):
    d = curl_T(np.sin(curl(th)))
    return th[0] - rho * d[0], th[1] - rho * d[1]


def levels(th, rho, n_levels):
    """[theta^(0), .., theta^(n)]"""
    out = [(th[0], th[1])]
    for _ in range(n_levels):
        out.append(smear_level(out[-1], rho))
    return out


def smear(th, rho, n_levels):
    return levels(th, rho, n_levels)[-1]


def jacobian_apply(th_k, F, rho):
    """J_k F with the phases of level k"""
    d = curl_T(np.cos(curl(th_k)) * curl(F))
    return F[0] - rho * d[0], F[1] - rho * d[1]


def pull_back(lv, F, rho):
    """J_0 J_1 .. J_(n-1) F for the levels lv = levels(th, rho, n)"""
    for k in range(len(lv) - 2, -1, -1):
        F = jacobian_apply(lv[k], F, rho)
    return F


def _solver(z, solve):
    return solve if solve is not None else (hn.solve_dense if z is None else rn.solve_shifts_dense)


def fermion_action(th, phi, mass, rho, n_levels, z=None, solve=None):
    V = smear(th, rho, n_levels)
    return hn.fermion_action(V, phi, mass, _solver(z, solve)) if z is None else rn.pf_action(z, V, phi, mass, _solver(z, solve))


def fermion_force(th, phi, mass, rho, n_levels, z=None, solve=None):
    """dS_f[V(theta)]/dtheta: the thin-link expression on V, pulled back through the levels"""
    lv = levels(th, rho, n_levels)
    F = hn.fermion_force(lv[-1], phi, mass, _solver(z, solve)) if z is None else rn.pf_force(z, lv[-1], phi, mass, _solver(z, solve))
    return pull_back(lv, F, rho)


def action(th, beta, phi, mass, rho, n_levels, z=None, solve=None):
    return hn.gauge_action(th, beta) + (fermion_action(th, phi, mass, rho, n_levels, z, solve) if phi is not None else 0.0)


def force(th, beta, phi, mass, rho, n_levels, z=None, solve=None):
    fx, fy = hn.gauge_force(th, beta)
    if phi is not None:
        gx, gy = fermion_force(th, phi, mass, rho, n_levels, z, solve)
        fx, fy = fx + gx, fy + gy
    return fx, fy


def hamiltonian(th, pi, beta, phi, mass, rho, n_levels, z=None, solve=None):
    return 0.5 * float(np.sum(pi[0] ** 2) + np.sum(pi[1] ** 2)) + action(th, beta, phi, mass, rho, n_levels, z, solve)


def leapfrog(th, pi, beta, tau, n_steps, phi, mass, rho, n_levels, z=None, solve=None):
    """hmc_numpy.leapfrog with the smeared force"""
    dt = tau / n_steps
    th = (th[0].copy(), th[1].copy())
    pi = (pi[0].copy(), pi[1].copy())

    def kick(e):
        f = force(th, beta, phi, mass, rho, n_levels, z, solve)
        return pi[0] - e * f[0], pi[1] - e * f[1]

    pi = kick(0.5 * dt)
    for k in range(n_steps):
        th = (th[0] + dt * pi[0], th[1] + dt * pi[1])
        pi = kick(dt if k + 1 < n_steps else 0.5 * dt)
    return th, pi


def md_dH(th, pi, beta, tau, n_steps, phi, mass, rho, n_levels, z=None, solve=None):
    """(end phases, end momenta, H_end - H_start)"""
    h0 = hamiltonian(th, pi, beta, phi, mass, rho, n_levels, z, solve)
    th1, pi1 = leapfrog(th, pi, beta, tau, n_steps, phi, mass, rho, n_levels, z, solve)
    return th1, pi1, hamiltonian(th1, pi1, beta, phi, mass, rho, n_levels, z, solve) - h0
