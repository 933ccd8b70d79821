"""CPU side of the Wilson flow and the Wilson loops: (i) the numpy statement tests/flow_numpy.py is pinned by what any correct statement must
obey -- its force is the derivative of its action, the Runge-Kutta step is of third order, the action never rises along the flow, a uniform
field strength is a fixed point with loops exp(i F R T), and the loops of a pure-gauge ensemble are the exact ones of the two-dimensional
torus -- before it judges the device in test_gpu_flow.py; the numbers measured here are the device gates; (ii) the drop-in boundary: every
new entry point is exported by libqmg_hip.so, declared in include/qmg_hip.h and bound in Python."""
import importlib
import os
import re

import numpy as np
import pytest

import coordspace as cs
import flow_numpy as fn
import u1_numpy as un

qmg = importlib.import_module("quantum-mg_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GATE_W, chi22_gate, uniform_field = fn.GATE_W, fn.chi22_gate, fn.uniform_field


def max_abs(a, b):
    return max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max())


def rel_l2(a, b):
    a, b = np.concatenate([np.ravel(a[0]), np.ravel(a[1])]), np.concatenate([np.ravel(b[0]), np.ravel(b[1])])
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


gaussian_phases = fn.gaussian_phases


@pytest.mark.parametrize("Lx,Ly", [(6, 4), (4, 6)])
def test_force_is_the_derivative_of_the_action(Lx, Ly):
    """Central differences at h = 1e-4 on every link; the gate of test_host_hmc.py, 1e-6 absolute (O(h^2) error ~1e-8)."""
    rng = np.random.default_rng(11)
    th = (rng.uniform(-np.pi, np.pi, (Lx, Ly)), rng.uniform(-np.pi, np.pi, (Lx, Ly)))
    f = fn.force(th)
    h, worst = 1e-4, 0.0
    for mu in range(2):
        for x in range(Lx):
            for y in range(Ly):
                up, dn = (th[0].copy(), th[1].copy()), (th[0].copy(), th[1].copy())
                up[mu][x, y] += h
                dn[mu][x, y] -= h
                worst = max(worst, abs((fn.action(up) - fn.action(dn)) / (2 * h) - f[mu][x, y]))
    fmax = max(np.abs(f[0]).max(), np.abs(f[1]).max())
    print("%dx%d: max |F - FD| = %.2e, max |F| = %.2f" % (Lx, Ly, worst, fmax))
    assert fmax > 1.0
    assert worst < 1e-6


def test_flow_force_is_the_hmc_gauge_force_at_beta_one():
    import hmc_numpy as hn
    th = gaussian_phases(6, 4, 1.0, 3)
    assert max_abs(fn.force(th), hn.gauge_force(th, 1.0)) == 0.0


def test_rk3_is_of_third_order(golden_dir):
    """The 32^2 beta-6.0 fixture flowed to t = 0.5 with eps = 0.05, 0.025, 0.0125 against eps = 0.5/320: the global error (max abs over the phases)
    falls by 8.94 and 8.47 per halving (4.2e-5, 4.7e-6, 5.6e-7; from eps = 0.1 the ratio is 9.9, from t = 1 they are 9.2 and 8.6): third order,
    approached from above.  Band [7, 10]."""
    th = fn.file_phases(os.path.join(golden_dir, "l32t32b60_heatbath.dat"), 32, 32)
    ref = fn.flow(th, 0.5 / 320, 320)
    err = [max_abs(fn.flow(th, 0.5 / n, n), ref) for n in (10, 20, 40)]
    print("global error at t = 0.5:", err, "ratios", err[0] / err[1], err[1] / err[2])
    assert 7.0 <= err[0] / err[1] <= 10.0 and 7.0 <= err[1] / err[2] <= 10.0


def test_two_register_form_is_the_textbook_step(golden_dir):
    """numpy against itself: the two-register form the device uses against the three-Z form, 1 and 20 steps at eps 0.01 and 0.05.  Measured on
    the three fixtures and the 2 x 2, 6 x 4, 34 x 10 Gaussian fields: at most 4.2e-16 relative l2 in the phases, 6.2e-16 in the links -- under a
    tenth of 1e-12, so the device gate of test_gpu_flow.py stays 1e-12."""
    worst = 0.0
    fields = [fn.file_phases(os.path.join(golden_dir, "l32t32b60_heatbath.dat"), 32, 32)] + [gaussian_phases(Lx, Ly, 6.0, 100 + Lx) for Lx, Ly in ((2, 2), (6, 4), (34, 10))]
    for th in fields:
        for eps in (0.01, 0.05):
            for n in (1, 20):
                a, b = fn.flow(th, eps, n), (th[0].copy(), th[1].copy())
                for _ in range(n):
                    b = fn.rk3_stages_two_register(b, eps)[-1][0]
                worst = max(worst, rel_l2(b, a), rel_l2(fn.links(b), fn.links(a)))
    print("two-register vs three-Z: worst relative l2 %.2e" % worst)
    assert worst < 1e-13


def test_action_never_rises_along_the_flow(golden_dir):
    """200 steps of eps = 0.05 on the 32^2 beta-6.0 fixture (S_w 87.12 -> 2.75 at t = 1 -> 0.089 at t = 10) and on a rough Gaussian field"""
    for th in (fn.file_phases(os.path.join(golden_dir, "l32t32b60_heatbath.dat"), 32, 32), gaussian_phases(32, 32, 1.0, 7)):
        S = [fn.action(th)]
        for _ in range(200):
            th = fn.rk3_step(th, 0.05)
            S.append(fn.action(th))
        assert all(S[i + 1] <= S[i] for i in range(200))
        assert S[-1] < 0.1 * S[0]


def test_flowed_charge_settles():
    """The geometric charge of a periodic field is an integer at every t (the plaquette angles sum to zero), but on a rough field it is not
    stable: the Gaussian beta = 1 field (32^2, seed 7) has Q = -8 at t = 0, -3 at t = 0.5 and -5 from t = 1.0 on (every 10 steps of eps = 0.05 to
    t = 10).  The fixture l32t32b60 has Q = 0 throughout.  test_gpu_flow.py holds the device to these numbers: settled from T_SETTLED = 1.0."""
    th = gaussian_phases(32, 32, 1.0, 7)
    Q = [fn.topo(th)]
    for _ in range(20):
        th = fn.flow(th, 0.05, 10)
        Q.append(fn.topo(th))
    print("Q(t), t = 0, 0.5, ..:", [round(q, 3) for q in Q])
    assert all(abs(q - round(q)) < 1e-9 for q in Q)
    assert [round(q) for q in Q[:3]] == [-8, -3, -5] and all(round(q) == -5 for q in Q[2:])


def test_uniform_field_is_a_fixed_point_and_the_reference_instanton_is_not():
    """A uniform field strength F = 2 pi Q / V is a fixed point to rounding and has W(R,T) = exp(i F R T), Polyakov loops of modulus 1.
    create_instanton_u1 with the reference's centring arithmetic is NOT such a field: on the unit field at 16^2, Q = 1, its plaquette angles run
    from -1.6 to 2.28 (uniform would be 0.0245), 20 steps of eps = 0.05 move its phases by 0.75, and W(1,1) = 0.98100 + 0.02276 i instead of
    0.99970 + 0.02454 i; a charge-2 one has geometric charge 3.  So the instanton identities are asserted on the uniform field built here, and
    the reference's instanton only through numpy's own loops of it (test_gpu_flow.py)."""
    for Lx, Ly, Q in ((16, 16, 1), (12, 8, -2)):
        th = uniform_field(Lx, Ly, Q)
        F = 2.0 * np.pi * Q / (Lx * Ly)
        assert np.abs(np.angle(np.exp(1j * (fn.plaquette_angle(th) - F)))).max() < 1e-14
        assert abs(fn.topo(th) - Q) < 1e-12
        assert max_abs(fn.flow(th, 0.05, 20), th) < 1e-13
        W = fn.wilson_loops(*fn.links(th), Lx // 2, Ly // 2)
        R, T = np.meshgrid(np.arange(1, Lx // 2 + 1), np.arange(1, Ly // 2 + 1), indexing="ij")
        assert np.abs(W - np.exp(1j * F * R * T)).max() < 1e-13
    one = np.ones((16, 16), dtype=complex)
    Ux, Uy = un.instanton(one, one, 1.0, 8, 8)
    P = np.angle(Ux * cs.fwd(Uy, 0) * np.conj(cs.fwd(Ux, 1)) * np.conj(Uy))
    th = (np.angle(Ux), np.angle(Uy))
    moved = max_abs(fn.flow(th, 0.05, 20), th)
    print("reference instanton 16^2: P in [%.3f, %.3f], flow moves it by %.3f, W(1,1) = %s" % (P.min(), P.max(), moved, fn.wilson_loop(Ux, Uy, 1, 1)))
    assert P.max() - P.min() > 1.0 and moved > 0.1


def test_loops_by_perimeter_walks_obey_their_identities():
    """W(1,1) is the plaquette; loops are gauge invariant; a cold field gives 1; Polyakov loops are gauge invariant and 1 on a cold field"""
    Lx, Ly = 6, 4
    Ux, Uy = un.gaussian_links(Lx, 6.0, 5, Ly=Ly)
    assert abs(fn.wilson_loop(Ux, Uy, 1, 1) - un.plaquette(Ux, Uy)[0]) < 1e-15
    g = un.random_transform(Lx, Ly, 9)
    Gx, Gy = un.gauge_transform(Ux, Uy, g)
    assert np.abs(fn.wilson_loops(Gx, Gy, 3, 2) - fn.wilson_loops(Ux, Uy, 3, 2)).max() < 1e-14
    assert max(abs(a - b) for a, b in zip(fn.polyakov(Gx, Gy), fn.polyakov(Ux, Uy))) < 1e-14
    one = np.ones((Lx, Ly), dtype=complex)
    assert np.array_equal(fn.wilson_loops(one, one, 3, 2), np.ones((3, 2))) and fn.polyakov(one, one) == (1.0, 1.0)


def test_torus_formula():
    """<W(R,T)> = sum_n I_n^(V-RT) I_(n+1)^RT / sum_n I_n^V: the area law (I1/I0)^RT up to finite-volume terms that vanish at 16^2, beta = 2"""
    r = fn.bessel_i(1, 2.0) / fn.bessel_i(0, 2.0)
    assert abs(r - 0.697774657964008) < 1e-14
    for area in (1, 2, 4):
        assert abs(fn.torus_wilson_loop(2.0, 256, area) - r ** area) < 1e-14
    assert abs(fn.torus_wilson_loop(2.0, 4, 1) - r) > 1e-3          # on 2 x 2 the other flux sectors are visible
    W = [[fn.torus_wilson_loop(2.0, 256, R * T) for T in (1, 2)] for R in (1, 2)]
    assert abs(fn.creutz(W, 2, 2) + np.log(r)) < 1e-13


def test_torus_wilson_loops_from_the_twin_hmc():
    """16^2, beta 2, tau 1, 10 steps, cold start, 100 + 300 trajectories (the run of test_host_hmc.py), W(1,1), W(1,2), W(2,2) on every measured
    trajectory.  Exact: 0.697775, 0.486889, 0.237061.  Over seeds 1..12 the means of this run are 0.69769, 0.48672, 0.23751 with standard
    deviations 0.00277, 0.00418, 0.00347 (largest deviation of a seed from the exact value: 2.4 sigma); chi(2,2) from the means has mean 0.3574
    and standard deviation 0.0103 against the exact -log(I1/I0) = 0.359859.  Gates of the GPU ensemble test: five standard deviations, 0.0139,
    0.0209, 0.0174, and for chi(2,2) the three propagated linearly in quadrature, 0.115 (five times its own spread would be 0.051)."""
    means, acc = fn.hmc_loops_pure_gauge(16, 2.0, 1.0, 10, 100, 300, 1)
    print("twin HMC loops:", means, "acceptance", acc)
    for (R, T), m in zip(((1, 1), (1, 2), (2, 2)), means):
        assert abs(m - fn.torus_wilson_loop(2.0, 256, R * T)) <= GATE_W[(R, T)]
    chi = -np.log(means[2] * means[0] / means[1] ** 2)
    assert abs(chi22_gate() - 0.115) < 0.001
    assert abs(chi + np.log(fn.bessel_i(1, 2.0) / fn.bessel_i(0, 2.0))) <= chi22_gate()
    assert 0.8 < acc < 1.0


def test_layout_round_trip():
    th = gaussian_phases(6, 4, 6.0, 16)
    back = fn.eo_to_field(fn.field_to_eo(th), 6, 4)
    assert np.array_equal(back[0], th[0]) and np.array_equal(back[1], th[1])


def test_new_entry_points_are_exported_declared_and_bound():
    qmg.build()
    lib = qmg.lib()
    header = open(os.path.join(ROOT, "include", "qmg_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in fn.NEW_SYMBOLS:
        assert hasattr(lib, name), "libqmg_hip.so does not export %s" % name
        assert re.search(r"\b%s\s*\(" % name, header), "include/qmg_hip.h does not declare %s" % name
        assert name in qmg.ABI_SYMBOLS
    for name in fn.NEW_BINDINGS:
        assert callable(getattr(qmg, name, None)), "the Python module does not bind %s" % name
