"""Independent numpy statement of the molecular-dynamics schemes of HmcCore::set_integrator on (x, y) grids.

A helper, not a test.  It knows nothing of any action: phases and momenta are (x-link, y-link) pairs of [x, y] grids and the two forces are callables
`force(th) -> (fx, fy)`, so that the forces of hmc_numpy, stout_numpy, rhmc_numpy, stag_hmc_numpy and dwf_hmc_numpy plug in unchanged, e.g.
    force_gauge = lambda th: hn.gauge_force(th, beta);   force_fermion = lambda th: hn.fermion_force(th, phi, mass, solve)
force_fermion = None is a run without fermions.  tests/test_host_md_schemes.py pins these statements (hn.leapfrog, reversibility, the dt^2 law,
nesting without fermions) before tests/test_gpu_md_schemes.py judges the device by them.

One step of length h, K a kick of the momenta (pi -= e F) and D a drift of the phases (th += e pi):
    leapfrog   K(h/2) D(h) K(h/2)
    omelyan    K(lam h) D(h/2) K((1 - 2 lam) h) D(h/2) K(lam h)                 (second-order minimum norm)
n steps are the n lists in a row with every two adjacent kicks made one: n + 1 kicks for leapfrog, 2 n + 1 for Omelyan.
n_gauge = 0: one scale, F the sum of both forces.  n_gauge >= 1: two scales -- the kicks of the list carry the fermion force alone (none when there
are no fermions) and every drift D(e) of the list is n_gauge steps of the same scheme, of length e / n_gauge, under the gauge force alone.
"""
import numpy as np

NEW_SYMBOLS = ["qmg_hmc_gauge_step"]
NEW_BINDINGS = ["hmc_gauge_step"]

LEAPFROG, OMELYAN ="leapfrog", "omelyan"
LAMBDA = 0.1931833275037836


def one_step(scheme, h, lam=LAMBDA):
    """[(kind, length)] of one step: kind 'K' or 'D'"""
    if scheme == LEAPFROG:
        return [("K", 0.5 * h), ("D", h), ("K", 0.5 * h)]
    if scheme == OMELYAN:
        return [("K", lam * h), ("D", 0.5 * h), ("K", (1.0 - 2.0 * lam) * h), ("D", 0.5 * h), ("K", lam * h)]
    raise ValueError("unknown scheme %r" % (scheme,))


def sequence(scheme, n_steps, h, lam=LAMBDA):
    """n_steps steps of length h in a row, adjacent kicks merged"""
    ops = []
    for _ in range(n_steps):
        for kind, e in one_step(scheme, h, lam):
            if kind == "K" and ops and ops[-1][0] == "K":
                ops[-1] = ("K", ops[-1][1] + e)
            else:
                ops.append((kind, e))
    return ops


def n_fermion_forces(scheme, n_steps):
    return sum(1 for kind, _ in sequence(scheme, n_steps, 1.0) if kind == "K")


def integrate(th, pi, force_gauge, force_fermion, tau, n_steps, scheme=LEAPFROG, n_gauge=0, lam=LAMBDA):
    """(end phases, end momenta) after n_steps steps of `scheme` over tau; the inputs are left alone"""
    th = (th[0].copy(), th[1].copy())
    pi = (pi[0].copy(), pi[1].copy())

    def kick(e, f):
        return pi[0] - e * f[0], pi[1] - e * f[1]

    def drift(e):
        return th[0] + e * pi[0], th[1] + e * pi[1]

    for kind, e in sequence(scheme, n_steps, tau / n_steps, lam):
        if kind == "K":
            if n_gauge == 0:
                f = force_gauge(th)
                if force_fermion is not None:
                    g = force_fermion(th)
                    f = (f[0] + g[0], f[1] + g[1])
                pi = kick(e, f)
            elif force_fermion is not None:
                pi = kick(e, force_fermion(th))
        elif n_gauge == 0:
            th = drift(e)
        else:
            for inner, ei in sequence(scheme, n_gauge, e / n_gauge, lam):
                if inner == "K":
                    pi = kick(ei, force_gauge(th))
                else:
                    th = drift(ei)
    return th, pi


def md_dH(th, pi, hamiltonian, force_gauge, force_fermion, tau, n_steps, scheme=LEAPFROG, n_gauge=0, lam=LAMBDA):
    """(end phases, end momenta, H_end - H_start); hamiltonian(th, pi) is the caller's"""
    h0 = hamiltonian(th, pi)
    th1, pi1 = integrate(th, pi, force_gauge, force_fermion, tau, n_steps, scheme, n_gauge, lam)
    return th1, pi1, hamiltonian(th1, pi1) - h0
