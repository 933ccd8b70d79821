"""Wilson flow and Wilson / Polyakov loops on the device (csrc/qmg_flow.hip, include/qmg/u1.hpp, drivers/u1_flow_measure.cpp).

The yardstick is the numpy statement tests/flow_numpy.py (np.roll on (x, y) grids, the Runge-Kutta step in its three-Z form, loops by
perimeter walks; pinned in test_host_flow.py), never the code under test:
  * every stage and the full flow against numpy, 1 and 20 steps at eps 0.01 and 0.05, relative l2 <= 1e-12 in phases (modulo 2 pi) and links
    (numpy's two forms of the step differ by 6.2e-16, under a tenth of the gate, so it stands), | |U| - 1 | <= 1e-15;
  * eps = 0 and n_steps = 0 bit for bit, covariance under qmg_u1_gauge_transform to 1e-13;
  * the action non-increasing step by step, Q(t) equal to numpy's, settled where numpy's is;
  * loops against numpy to 1e-12, W(1,1) against qmg_u1_plaquette to 1e-14, gauge invariance to 1e-13, uniform fields, the cold field;
  * a pure-gauge ensemble against the exact loops of the torus within the gates fixed on the CPU; the driver.
Measured on an MI355X: phases 4.3e-16, links 6.2e-16, accumulator 3.7e-15, | |U| - 1 | 2.2e-16; covariance 6.7e-16; loops 4.4e-16, Polyakov
1.2e-16, W(1,1) - plaquette 4.4e-16; ensemble W11 0.697706, W12 0.489158, W22 0.242003, chi(2,2) 0.3486, acceptance 0.897."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import coordspace as cs
import flow_numpy as fn
import u1_numpy as un
from flow_numpy import GATE_W, chi22_gate, gaussian_phases, uniform_field

qmg = importlib.import_module("quantum-mg_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVERS = os.path.join(ROOT, "quantum-mg_amd", "drivers")
STORED = [("l32t32b60", 32), ("l64t64b60", 64), ("l128t128b60", 128)]
TOL = 1e-12
T_SETTLED = 1.0     # test_host_flow.py::test_flowed_charge_settles


@pytest.fixture(scope="module", autouse=True)
def _device():
    qmg.build()
    subprocess.check_call(["make", "-C", DRIVERS, "-j4"], stdout=subprocess.DEVNULL)
    qmg.init(0)
    yield
    qmg.sync()


def fields(golden_dir):
    """(name, Lx, Ly, (thx, thy)): the three stored configurations and Gaussian beta = 6 phases on 2 x 2, 2 x 6, 6 x 2, 6 x 4 and 34 x 10"""
    out = [(name, L, L, fn.file_phases(os.path.join(golden_dir, name + "_heatbath.dat"), L, L)) for name, L in STORED]
    for Lx, Ly in ((2, 2), (2, 6), (6, 2), (6, 4), (34, 10)):
        out.append(("%dx%d" % (Lx, Ly), Lx, Ly, gaussian_phases(Lx, Ly, 6.0, 100 + Lx)))
    return out


def rel_l2(a, b):
    return float(np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(np.ravel(b)))


def eo_links(th):
    Lx, Ly = th[0].shape
    return cs.links_to_eo_gauge(*fn.links(th), Lx, Ly)


def upload(th):
    """(device phases, device links exp(i theta))"""
    return qmg.DeviceArray.from_host(fn.field_to_eo(th)), qmg.DeviceArray.from_host(eo_links(th))


def phase_error(got, want):
    """relative l2 of the phases compared modulo 2 pi"""
    d = np.angle(np.exp(1j * (got - want)))
    return float(np.linalg.norm(d) / np.linalg.norm(want))


def device_flow(th, eps, n_steps):
    Lx, Ly = th[0].shape
    dth, dg = upload(th)
    qmg.u1_flow(dth, dg, Lx, Ly, eps, n_steps)
    return dth.to_host(), dg.to_host()


@pytest.mark.parametrize("eps", [0.01, 0.05])
def test_stages_match_numpy(golden_dir, eps):
    """one step, stage by stage through qmg_u1_flow_stage with the caller's ping-pong: phases, accumulator and links after each stage"""
    for name, Lx, Ly, th in fields(golden_dir):
        n = 2 * Lx * Ly
        dth, dg = upload(th)
        dacc, dtmp = qmg.DeviceArray(n, np.float64), qmg.DeviceArray(n)
        bufs = [dg, dtmp]
        for stage, (w_th, w_acc) in enumerate(fn.rk3_stages_two_register(th, eps), start=1):
            qmg.u1_flow_stage(dth, dacc, bufs[stage & 1], bufs[(stage - 1) & 1], Lx, Ly, eps, stage)
            U = bufs[stage & 1].to_host()
            e_th, e_acc, e_u = phase_error(dth.to_host(), fn.field_to_eo(w_th)), rel_l2(dacc.to_host(), fn.field_to_eo(w_acc)), rel_l2(U, eo_links(w_th))
            mod = float(np.abs(np.abs(U) - 1.0).max())
            print("%s eps %.2f stage %d: phases %.2e acc %.2e links %.2e | |U| - 1 | %.2e" % (name, eps, stage, e_th, e_acc, e_u, mod))
            assert e_th <= TOL and e_acc <= TOL and e_u <= TOL and mod <= 1e-15, name
        # the three stages are the textbook step
        assert phase_error(dth.to_host(), fn.field_to_eo(fn.rk3_step(th, eps))) <= TOL, name


@pytest.mark.parametrize("eps", [0.01, 0.05])
@pytest.mark.parametrize("n_steps", [1, 20])
def test_flow_matches_numpy(golden_dir, eps, n_steps):
    for name, Lx, Ly, th in fields(golden_dir):
        want = fn.flow(th, eps, n_steps)
        got_th, got_u = device_flow(th, eps, n_steps)
        e_th, e_u, mod = phase_error(got_th, fn.field_to_eo(want)), rel_l2(got_u, eo_links(want)), float(np.abs(np.abs(got_u) - 1.0).max())
        print("%s eps %.2f n %d: phases %.2e links %.2e | |U| - 1 | %.2e" % (name, eps, n_steps, e_th, e_u, mod))
        assert e_th <= TOL and e_u <= TOL and mod <= 1e-15, name
        assert rel_l2(got_u, np.exp(1j * got_th)) <= 1e-15, name            # the links are exp(i theta) of the phases beside them


def test_zero_step_and_zero_steps_return_the_inputs_bit_for_bit(golden_dir):
    for name, Lx, Ly, th in fields(golden_dir):
        th0, u0 = fn.field_to_eo(th), eo_links(th)
        for eps, n_steps in ((0.0, 5), (0.05, 0), (0.0, 0)):
            got_th, got_u = device_flow(th, eps, n_steps)
            assert np.array_equal(got_th.view(np.uint64), th0.view(np.uint64)), name
            assert np.array_equal(got_u.view(np.uint64), u0.view(np.uint64)), name


def test_flow_is_gauge_covariant(golden_dir):
    """flow(U^g) = (flow U)^g with the device's own transform, relative l2 of the links <= 1e-13"""
    for name, Lx, Ly, th in fields(golden_dir):
        n = 2 * Lx * Ly
        dt = qmg.DeviceArray(Lx * Ly)
        qmg.u1_random_trans(dt, Lx, Ly, 77)
        # plain: flow, then transform
        dth, dg = upload(th)
        qmg.u1_flow(dth, dg, Lx, Ly, 0.05, 20)
        qmg.u1_gauge_transform(dg, dt, Lx, Ly)
        # transformed: transform, take the phases of the transformed links, flow
        _, dg2 = upload(th)
        qmg.u1_gauge_transform(dg2, dt, Lx, Ly)
        dth2 = qmg.DeviceArray(n, np.float64)
        qmg.u1_gauge_to_phase(dth2, dg2, n)
        qmg.u1_flow(dth2, dg2, Lx, Ly, 0.05, 20)
        e = rel_l2(dg2.to_host(), dg.to_host())
        print("%s: flow o transform against transform o flow %.2e" % (name, e))
        assert e <= 1e-13, name


def test_action_is_monotone_and_the_charge_is_numpys(golden_dir):
    """32^2 beta-6.0 fixture, 200 steps of eps = 0.05 one at a time: E(t) from qmg_u1_plaquette never rises and Q(t) is numpy's (0 throughout).
    Gaussian beta = 1 field (seed 7): Q(t) is numpy's at every measured t (every 10 steps) and -5 from T_SETTLED = 1.0 on."""
    L = 32
    th = fn.file_phases(os.path.join(golden_dir, "l32t32b60_heatbath.dat"), L, L)
    dth, dg = upload(th)
    ref = th
    e_prev = 1.0 - qmg.u1_plaquette(dg, L, L)[0].real
    for step in range(200):
        qmg.u1_flow(dth, dg, L, L, 0.05, 1)
        ref = fn.rk3_step(ref, 0.05)
        p, q = qmg.u1_plaquette(dg, L, L)
        e = 1.0 - p.real
        assert e <= e_prev, step
        assert abs(e * L * L - fn.action(ref)) <= 1e-10 * max(1.0, fn.action(th))
        assert abs(q - fn.topo(ref)) < 1e-9 and abs(q) < 1e-9, step
        e_prev = e
    rough = gaussian_phases(L, L, 1.0, 7)
    dth, dg = upload(rough)
    ref = rough
    for k in range(21):
        t = 0.5 * k
        q = qmg.u1_plaquette(dg, L, L)[1]
        print("rough field t = %.1f: Q device %.6f numpy %.6f" % (t, q, fn.topo(ref)))
        assert abs(q - fn.topo(ref)) < 1e-9
        if t >= T_SETTLED:
            assert abs(q + 5.0) < 1e-9
        qmg.u1_flow(dth, dg, L, L, 0.05, 10)
        ref = fn.flow(ref, 0.05, 10)


def test_wilson_and_polyakov_loops_match_numpy(golden_dir):
    """every (R, T) up to Lx/2, Ly/2, max abs difference <= 1e-12; W(1,1) is the plaquette of qmg_u1_plaquette to 1e-14; invariant under a
    random gauge transform to 1e-13"""
    for name, Lx, Ly, th in fields(golden_dir):
        r_max, t_max = Lx // 2, Ly // 2
        Ux, Uy = fn.links(th)
        _, dg = upload(th)
        W = qmg.u1_wilson_loops(dg, Lx, Ly, r_max, t_max)
        want = fn.wilson_loops(Ux, Uy, r_max, t_max)
        d = float(np.abs(W - want).max())
        px, py = qmg.u1_polyakov(dg, Lx, Ly)
        wx, wy = fn.polyakov(Ux, Uy)
        plaq = qmg.u1_plaquette(dg, Lx, Ly)[0]
        print("%s: loops %.2e (r_max %d t_max %d), Polyakov %.2e %.2e, W(1,1) - plaquette %.2e" % (name, d, r_max, t_max, abs(px - wx), abs(py - wy), abs(W[0, 0] - plaq)))
        assert d <= 1e-12 and abs(px - wx) <= 1e-12 and abs(py - wy) <= 1e-12, name
        assert abs(W[0, 0] - plaq) <= 1e-14, name
        dt = qmg.DeviceArray(Lx * Ly)
        qmg.u1_random_trans(dt, Lx, Ly, 4242)
        qmg.u1_gauge_transform(dg, dt, Lx, Ly)
        Wg = qmg.u1_wilson_loops(dg, Lx, Ly, r_max, t_max)
        gx, gy = qmg.u1_polyakov(dg, Lx, Ly)
        assert np.abs(Wg - W).max() <= 1e-13 and abs(gx - px) <= 1e-13 and abs(gy - py) <= 1e-13, name
    # a rectangular table that is not the full one
    th = gaussian_phases(34, 10, 6.0, 134)
    assert np.abs(qmg.u1_wilson_loops(upload(th)[1], 34, 10, 3, 5) - fn.wilson_loops(*fn.links(th), 3, 5)).max() <= 1e-12


@pytest.mark.parametrize("rows", ["all", "tail"])
def test_loops_past_the_cap_of_the_partial_sum_grid(rows):
    """516 x 512 = 264 192 sites against the 1024 blocks x 256 lanes = 262 144 of k_wilson_loop's grid: lanes 0 .. 2047 take a second site,
    even-odd index >= 262 144, i.e. the odd sites from row 504 on.  "all": Gaussian beta = 6 phases on every link; "tail": on the links of the
    rows y >= 509 alone, so that half of the loops that differ from 1 are summed on a second trip.  Loops up to (2, 2) and the Polyakov loops
    against numpy at the 1e-12 of the test above; a second run returns the same bits."""
    Lx, Ly = 516, 512
    assert Lx * Ly > 1024 * 256
    th = gaussian_phases(Lx, Ly, 6.0, 516)
    if rows == "tail":
        th = tuple(np.where(np.arange(Ly)[None, :] >= 509, t, 0.0) for t in th)
    Ux, Uy = fn.links(th)
    _, dg = upload(th)
    W, want = qmg.u1_wilson_loops(dg, Lx, Ly, 2, 2), fn.wilson_loops(Ux, Uy, 2, 2)
    (px, py), (wx, wy) = qmg.u1_polyakov(dg, Lx, Ly), fn.polyakov(Ux, Uy)
    print("516 x 512 %s: loops %.2e, Polyakov %.2e %.2e" % (rows, np.abs(W - want).max(), abs(px - wx), abs(py - wy)))
    assert np.abs(W - want).max() <= 1e-12 and abs(px - wx) <= 1e-12 and abs(py - wy) <= 1e-12
    assert np.abs(want - 1.0).min() > 1e-4                                        # the rows of the tail alone move every loop far beyond the gate
    assert np.array_equal(qmg.u1_wilson_loops(dg, Lx, Ly, 2, 2), W) and qmg.u1_polyakov(dg, Lx, Ly) == (px, py)


def test_loops_of_uniform_instanton_and_cold_fields():
    """Uniform field strength F = 2 pi Q / V: W(R,T) = exp(i F R T) and a fixed point of the flow to rounding (test_host_flow.py).  The
    reference's create_instanton_u1 is not uniform (plaquette angles from -1.6 to 2.28 on the unit field), so for it numpy's own loops of the
    field the DEVICE made are asserted.  A cold field gives exactly 1."""
    for Lx, Ly, Q in ((16, 16, 1), (12, 8, -2)):
        th = uniform_field(Lx, Ly, Q)
        F = 2.0 * np.pi * Q / (Lx * Ly)
        dth, dg = upload(th)
        R, T = np.meshgrid(np.arange(1, Lx // 2 + 1), np.arange(1, Ly // 2 + 1), indexing="ij")
        assert np.abs(qmg.u1_wilson_loops(dg, Lx, Ly, Lx // 2, Ly // 2) - np.exp(1j * F * R * T)).max() <= 1e-13
        u0 = dg.to_host()
        qmg.u1_flow(dth, dg, Lx, Ly, 0.05, 20)
        assert np.abs(np.angle(dg.to_host() * np.conj(u0))).max() <= 1e-13
    L = 16
    one = np.ones((L, L), dtype=complex)
    dg = qmg.DeviceArray.from_host(cs.links_to_eo_gauge(one, one, L, L))
    W = qmg.u1_wilson_loops(dg, L, L, L // 2, L // 2)
    assert np.array_equal(W, np.ones((L // 2, L // 2), dtype=complex))
    assert qmg.u1_polyakov(dg, L, L) == (1.0, 1.0)
    qmg.u1_instanton(dg, L, L, 1.0, L // 2, L // 2)
    Ux, Uy = un.eo_gauge_to_links(dg.to_host(), L, L)
    W = qmg.u1_wilson_loops(dg, L, L, L // 2, L // 2)
    assert np.abs(W - fn.wilson_loops(Ux, Uy, L // 2, L // 2)).max() <= 1e-12
    assert abs(W[0, 0] - (0.9809963328011999 + 0.022758191634532205j)) <= 1e-12       # numpy's value, test_host_flow.py


def test_invalid_arguments_are_refused():
    L = 8
    n = 2 * L * L
    th, acc, g, g2 = qmg.DeviceArray.zeros(n, np.float64), qmg.DeviceArray.zeros(n, np.float64), qmg.DeviceArray.zeros(n), qmg.DeviceArray.zeros(n)
    for call in (lambda: qmg.u1_flow_stage(th, acc, g, g, L, L, 0.01, 1), lambda: qmg.u1_flow_stage(th, acc, g2, g, L, L, 0.01, 0),
                 lambda: qmg.u1_flow_stage(th, acc, g2, g, L, L, 0.01, 4), lambda: qmg.u1_flow_stage(th, None, g2, g, L, L, 0.01, 1),
                 lambda: qmg.u1_flow_stage(th, acc, g2, g, L, 7, 0.01, 1), lambda: qmg.u1_flow(th, g, L, L, 0.01, -1), lambda: qmg.u1_flow(None, g, L, L, 0.01, 1),
                 lambda: qmg.u1_flow(th, g, L, L, float("nan"), 1), lambda: qmg.u1_wilson_loops(g, L, L, L // 2 + 1, 1), lambda: qmg.u1_wilson_loops(g, L, L, 1, 0),
                 lambda: qmg.u1_wilson_loops(None, L, L, 1, 1), lambda: qmg.u1_polyakov(g, L, 5)):
        with pytest.raises(qmg.QmgError, match="invalid"):
            call()


def test_pure_gauge_ensemble_has_the_exact_loops_of_the_torus():
    """16^2, beta 2, tau 1, 10 leapfrog steps, cold start, 100 + 300 trajectories -- the run of test_gpu_hmc.py's pure-gauge check, driven from here
    through the molecular-dynamics entries so that W(1,1), W(1,2), W(2,2) can be measured on every trajectory.  Exact (torus formula): 0.697775,
    0.486889, 0.237061; gates 0.0139, 0.0209, 0.0174 (five standard deviations of the numpy run over 12 seeds, test_host_flow.py);
    chi(2,2) = -log(I1(2)/I0(2)) = 0.359859 within the propagated 0.115."""
    L, beta, n_steps, n_therm, n_meas = 16, 2.0, 10, 100, 300
    V, n = L * L, 2 * L * L
    dt = 1.0 / n_steps
    theta, saved, pi, gauge = qmg.DeviceArray.zeros(n, np.float64), qmg.DeviceArray(n, np.float64), qmg.DeviceArray(n, np.float64), qmg.DeviceArray(n)
    qmg.u1_phase_to_gauge(gauge, theta, n)
    rng = np.random.default_rng(4242)

    def hamiltonian():
        return 0.5 * qmg.norm2sq(pi, n // 2) + beta * V * (1.0 - qmg.u1_plaquette(gauge, L, L)[0].real)

    def kick(e):
        qmg.hmc_momentum_update(pi, gauge, None, None, L, L, beta, e, qmg.HMC_GAUGE_ONLY)

    meas, acc = [], 0
    for traj in range(n_therm + n_meas):
        qmg.copy_vector(saved, theta, n // 2)
        qmg.hmc_momentum_refresh(pi, n, 4242, traj)
        h0 = hamiltonian()
        kick(0.5 * dt)
        for k in range(n_steps):
            qmg.hmc_link_update(theta, gauge, pi, n, dt)
            kick(dt if k + 1 < n_steps else 0.5 * dt)
        ok = rng.uniform() < np.exp(-(hamiltonian() - h0))
        if not ok:
            qmg.copy_vector(theta, saved, n // 2)
            qmg.u1_phase_to_gauge(gauge, theta, n)
        if traj >= n_therm:
            acc += ok
            W = qmg.u1_wilson_loops(gauge, L, L, 2, 2)
            meas.append([W[0, 0].real, W[0, 1].real, W[1, 1].real])
    m = np.mean(np.array(meas), axis=0)
    exact = [fn.torus_wilson_loop(beta, V, a) for a in (1, 2, 4)]
    chi = -np.log(m[2] * m[0] / m[1] ** 2)
    print("ensemble: W11 %.6f W12 %.6f W22 %.6f (exact %.6f %.6f %.6f), chi(2,2) %.6f (exact %.6f), acceptance %.3f"
          % (m[0], m[1], m[2], exact[0], exact[1], exact[2], chi, -np.log(exact[0]), acc / n_meas))
    for got, want, key in zip(m, exact, ((1, 1), (1, 2), (2, 2))):
        assert abs(got - want) <= GATE_W[key], key
    assert abs(chi + np.log(exact[0])) <= chi22_gate()
    assert 0.8 < acc / n_meas < 1.0


def test_u1_flow_measure_driver(tmp_path, golden_dir):
    """the t = 0 row is qmg_u1_plaquette's and numpy's; every row is numpy's flow; the flowed file reads back with the last printed plaquette"""
    L, out_cfg = 32, str(tmp_path / "flowed.dat")
    cfg = os.path.join(golden_dir, "l32t32b60_heatbath.dat")
    out = subprocess.run([os.path.join(DRIVERS, "u1_flow_measure"), cfg, str(L), "0.05", "20", "10", "3", "4", out_cfg], capture_output=True, text=True, timeout=300)
    print(out.stdout[-4000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    def numbers(line):
        vals = []
        for tok in line.split()[1:]:
            try:
                vals.append(float(tok))
            except ValueError:
                pass                                   # the labels t, E, plaq, Q, P, W, chi
        return vals

    rows = [numbers(line) for line in out.stdout.splitlines() if line.startswith("[FLOW] ")]
    assert len(rows) == 3 and all(len(r) == 4 + 4 + 12 + 12 for r in rows)
    th = fn.file_phases(cfg, L, L)
    dg = upload(th)[1]
    plaq, q = qmg.u1_plaquette(dg, L, L)
    assert rows[0][0] == 0.0 and abs(rows[0][2] - plaq.real) <= 1e-12 and abs(rows[0][1] - (1.0 - plaq.real)) <= 1e-12 and abs(rows[0][3] - q) <= 1e-9
    for k, row in enumerate(rows):
        ref = fn.flow(th, 0.05, 10 * k)
        Ux, Uy = fn.links(ref)
        W = fn.wilson_loops(Ux, Uy, 3, 4).real
        assert abs(row[0] - 0.5 * k) <= 1e-12
        assert abs(row[2] - un.plaquette(Ux, Uy)[0].real) <= 1e-11 and abs(row[3] - fn.topo(ref)) <= 1e-9
        px, py = fn.polyakov(Ux, Uy)
        assert np.abs(np.array(row[4:8]) - np.array([px.real, px.imag, py.real, py.imag])).max() <= 1e-11
        assert np.abs(np.array(row[8:20]).reshape(3, 4) - W).max() <= 1e-11
        chi = np.array([[fn.creutz(W, R, T) for T in range(1, 5)] for R in range(1, 4)])
        assert np.abs(np.array(row[20:32]).reshape(3, 4) - chi).max() <= 1e-8
    Ux, Uy = cs.phases_to_links(np.loadtxt(out_cfg), L, L)
    assert abs(un.plaquette(Ux, Uy)[0].real - rows[-1][2]) <= 1e-11
    back = re.search(r"\[FLOW-READBACK\] plaq (\S+) Q (\S+)", out.stdout)
    assert back and abs(float(back.group(1)) - rows[-1][2]) <= 1e-11
