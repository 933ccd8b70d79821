"""Pins tests/krylov_batch_numpy.py, the reference of tests/test_gpu_krylov_batch.py, and keeps that test from being vacuous: the dense
matrices are the oracle's stencils, both operators are as well conditioned as the derived bars assume, the CPU twins solve every one of the six
right-hand sides alone to the two bars, and the batch is UNEVEN -- a condition on the inputs, checked here with the twins alone:
  * the iteration counts of slots 0, 3 and 5 take three distinct values, and slot 5 stops at least 5 iterations after the first of them;
  * in a case cut by max_iter at least one slot converges and at least one does not.
Runs without a GPU.  `twin` and `twin_table` are shared with the GPU test."""
import numpy as np
import pytest

import krylov_batch_numpy as kb
import oracle_lib as ol

_DESC = {}


def descs():
    """the oracle's stencil descriptors of the same links: name -> (desc, dagger desc or None)"""
    if _DESC:
        return _DESC
    ops = kb.operators()
    w = ops["wilson16"]
    gauge = ol.phases_to_gauge_u1(w.phases, w.Lx, w.Ly)
    wc, wh = ol.wilson_fill(gauge, w.Lx, w.Ly)
    dc, dh = ol.build_dagger(wc, wh, w.Lx, w.Ly, 2)
    _DESC["wilson16"] = (ol.make_desc(w.Lx, w.Ly, 2, wc, wh, w.mass), ol.make_desc(w.Lx, w.Ly, 2, dc, dh, w.mass))
    _DESC["normal16"] = _DESC["wilson16f"] = _DESC["wilson16"]
    h = ops["wilson16h"]
    _DESC["wilson16h"] = (ol.make_desc(h.Lx, h.Ly, 2, wc, wh, h.mass), None)
    lp = ops["laplace34x10"]
    gauge = ol.phases_to_gauge_u1(lp.phases, lp.Lx, lp.Ly)
    lc, lh = ol.laplace_fill(gauge, lp.Lx, lp.Ly)
    _DESC["laplace34x10"] = (ol.make_desc(lp.Lx, lp.Ly, 1, lc, lh, lp.mass), None)
    return _DESC


def twin(case, k, b, x0, max_iter, tol):
    """the CPU twin of `case` on ONE system: (converged, iterations, x, resSq)"""
    op = kb.operators()[case.op]
    d, dag = descs()[case.op]
    if case.core == "mr":
        return ol.krylov_solve(ol.KRYLOV_MR, d, b, max_iter, tol, param_d=kb.OMEGA, x0=x0)[:4]
    if case.core == "bicg":
        return ol.krylov_solve(ol.KRYLOV_BICGSTAB_L, d, b, max_iter, tol, param_i=case.pi, x0=x0)[:4]
    if case.core == "gcr" and not case.pre:
        return ol.krylov_solve(ol.KRYLOV_GCR, d, b, max_iter, tol, param_i=case.pi, x0=x0)[:4]
    if case.core == "gcr":
        return kb.fgcr_dense(op.A, b, x0, max_iter, tol, case.pi, lambda r: kb.mr_dense(op.A, r, 4, kb.OMEGA))
    if case.pi > 0:
        return kb.cg_restart_dense(op.A, b, x0, max_iter, tol, case.pi)
    return ol.krylov_solve(ol.KRYLOV_CG, d, b, max_iter, tol, x0=x0, dagger_desc=dag if op.kind == "normal" else None, normal=op.kind == "normal")[:4]


_TABLE = {}


def twin_table():
    """(case name, precision) -> (case with max_iter resolved, [per slot (converged, iterations, x, resSq)]); every twin runs once"""
    if _TABLE:
        return _TABLE
    sets = {name: kb.rhs_sets(op) for name, op in kb.operators().items()}
    conv_iters = {}
    for case in kb.case_table():
        b0, bg, g = sets[case.op]
        for prec in ("f64", "f32"):
            max_iter = case.max_iter
            if max_iter < 0:   # cut where the converging case of the same solver stops slot 0
                max_iter = conv_iters[(case.core, case.op, case.pi, case.eps_ps, prec)]
            rows = []
            for k in range(kb.NRHS):
                b = bg[k] if case.guess else b0[k]
                rows.append(twin(case, k, b, g[k] if case.guess else None, max_iter, kb.case_eps(case, prec, k)))
            if case.converging and not case.guess and not case.pre:
                conv_iters.setdefault((case.core, case.op, case.pi, case.eps_ps, prec), rows[0][1])
            _TABLE[(case.name, prec)] = (case._replace(max_iter=max_iter), rows)
    return _TABLE


def test_dense_matrices_are_the_oracles_stencils():
    ops = kb.operators()
    for name in ("wilson16", "wilson16h", "laplace34x10"):
        op, (d, dag) = ops[name], descs()[name]
        for seed in (1, 2):
            v = np.random.default_rng(seed).standard_normal(op.n) + 1j * np.random.default_rng(seed + 10).standard_normal(op.n)
            want = ol.stencil_apply(d, v)
            assert np.linalg.norm(op.A @ v - want) <= 1e-13 * np.linalg.norm(want)
            if dag is not None:
                want = ol.stencil_apply(dag, ol.stencil_apply(d, v))
                assert np.linalg.norm(ops["normal16"].A @ v - want) <= 1e-13 * np.linalg.norm(want)


def test_operators_are_well_conditioned_and_hermitian_where_cg_needs_it():
    for op in kb.operators().values():
        assert op.smin > 0 and op.smax / op.smin <= kb.COND_MAX, (op.name, op.smax / op.smin)
        if op.hermitian:
            assert np.abs(op.A - op.A.conj().T).max() <= 1e-14 * op.smax
            assert np.linalg.eigvalsh(op.A)[0] > 0
    assert kb.operators()["wilson16"].smax / kb.operators()["wilson16"].smin <= 10.0   # cond(M^dag M) = cond(M)^2


def test_the_right_hand_sides_are_what_the_table_says():
    for op in kb.operators().values():
        b0, bg, g = kb.rhs_sets(op)
        assert not b0[1].any() and not bg[1].any() and g[1].any()                 # a zero rhs with a non-zero guess
        assert (b0[4] == kb.SCALE * b0[0]).all() and (g[4] == kb.SCALE * g[0]).all() and (bg[4] == b0[4]).all()
        assert np.linalg.norm(bg[3] - op.A @ g[3]) <= 1e-13 * np.linalg.norm(bg[3])
        


def test_fp32_storage_stays_inside_the_derived_margin():
    """the float bar is the double one because rounding a stored x moves the relative residual by 2^-24 |A| |x| / |b|, far under 0.5 eps:
    that needs every x the solver stores, the guess and the solution, to be of the size cond |b| / |A| at most -- a condition on the inputs"""
    for op in kb.operators().values():
        b0, bg, g = kb.rhs_sets(op)
        for b, x0 in ((b0, np.zeros_like(g)), (bg, g)):
            for k in range(kb.NRHS):
                if not b[k].any():
                    continue
                size = max(np.linalg.norm(x0[k]), np.linalg.norm(kb.dense_solution(op.A, b[k])))
                assert kb.UNIT["f32"] * op.smax * size / np.linalg.norm(b[k]) <= kb.FP32_PREMISE * kb.EPS["f32"], (op.name, k)


def test_dense_solution_refines_to_rounding():
    for op in kb.operators().values():
        b = kb.rhs_sets(op)[0][0]
        x = kb.dense_solution(op.A, b)
        assert kb.residual_norm(op.A, x, b) <= 1e-14 * op.smax / op.smin * np.linalg.norm(b)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_the_batches_are_uneven(prec):
    table = twin_table()
    for case in kb.case_table():
        c, rows = table[(case.name, prec)]
        its = [r[1] for r in rows]
        if case.converging:
            assert all(r[0] for r in rows), (case.name, prec, its)
            assert len({its[0], its[3], its[5]}) == 3, (case.name, prec, its)
            assert its[5] >= min(its[0], its[3], its[5]) + 5, (case.name, prec, its)
        elif c.max_iter > 0 and not case.fixed:
            assert rows[3][0] and not rows[5][0], (case.name, prec, [r[0] for r in rows], its)
        assert rows[1][0] and its[1] == 0 and not rows[1][2].any()                 # a zero rhs: x = 0, whatever the guess
        assert its[4] == its[0] and rows[4][0] == rows[0][0]                       # the scaled copy stops where slot 0 does


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_the_twins_solutions_meet_the_two_bars(prec):
    table = twin_table()
    ref = {}
    for case in kb.case_table():
        c, rows = table[(case.name, prec)]
        op = kb.operators()[case.op]
        b0, bg, g = kb.rhs_sets(op)
        for k, (conv, it, x, rsq) in enumerate(rows):
            b = bg[k] if case.guess else b0[k]
            if not conv or not b.any():
                continue
            key = (case.op, case.guess, k)
            if key not in ref:
                ref[key] = kb.dense_solution(op.A, b)
            kb.check_bars(op, x, b, kb.case_eps(case, prec, k), ref[key])
