"""The lock-step batch cores of include/qmg/krylov.hpp (bmr_core, bbicgstab_l_core, bgcr_core, bcg_core) on UNEVEN batches, held to dense numpy
solves (tests/krylov_batch_numpy.py; the inputs are pinned and shown uneven in tests/test_host_krylov_batch.py).  drivers/krylov_batch_parity.cpp
runs every case in double and float, with the systems n and n + 37 elements apart, under the masks 0x3F and 0x3B, each system also alone, and
bgcr_core once on 16 systems under 0xA5A5.  For every run:
  1. the equation: a system reported `success` meets the two derived bars (true residual <= 1.5 eps |b|, error <= residual / sigma_min) against
     the dense matrix; one reported not converged stopped at max_iter; sqrt(resSq) < eps |b| exactly when success; in the cut and fixed-iteration
     cases sqrt(resSq) is the numpy true residual of the dumped x to RES_AGREE * |b|;
  2. iteration counts equal the CPU twins' and the system's alone within the slacks of tests/test_gpu_krylov.py (1; BiCGStab(L): L; CG on M^dag M: 2);
  3. slot 4 = 2^-40 slot 0 has slot 0's iter, ops and success and, bit for bit, 2^-40 times its solution;
  4. the masks the solver hands to the operator: subsets of the call's mask, ops_count[k] = the number of calls with bit k (exact), nothing for
     a zero right-hand side or a system converged at its guess after the opening residual, nothing at all under max_iter = 0, and (MR,
     BiCGStab, GCR) a bit that left never returns;
  5. untouched: the rhs allocation byte for byte, the padding still NaN, a masked-out slot's x byte for byte its NaN fill, nothing non-finite elsewhere;
  6. a zero right-hand side ends with x == 0 exactly, success, iter 0, resSq 0 -- from a non-zero guess too.
RES_AGREE: MR and GCR return a recurrence that is re-anchored on a true norm every 8 orders of magnitude: 1e-8.  CG and BiCGStab return a
computed norm: 1e-12 in double = 90 cond 2^-53 at cond = 100.  In float the vectors carry 2^-24, every scalar stays fp64: 90 cond 2^-24 = 5.4e-4
for all four (the recurrence's own 1e-8 is below it)."""
import os
import subprocess

import numpy as np
import pytest

import krylov_batch_numpy as kb
import test_host_krylov_batch as host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVERS = os.path.join(ROOT, "quantum-mg_amd", "drivers")
CASES = kb.case_table()
PRECS = ("f64", "f32")
RES_AGREE = {"f64": {"mr": 1e-8, "gcr": 1e-8, "cg": 1e-12, "bicg": 1e-12}, "f32": dict.fromkeys(("mr", "gcr", "cg", "bicg"), 90 * kb.COND_MAX * kb.UNIT["f32"])}


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    assert os.path.exists(os.path.join(DRIVERS, "krylov_batch_parity")), "drivers/krylov_batch_parity is not built"
    tmp = str(tmp_path_factory.mktemp("krylov_batch"))
    table = host.twin_table()
    kb.write_case_dir(tmp, [(c, table[(c.name, "f64")][0].max_iter, table[(c.name, "f32")][0].max_iter) for c in CASES])
    out = subprocess.run([os.path.join(DRIVERS, "krylov_batch_parity"), tmp], cwd=DRIVERS, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "[QMG-ERROR]" not in out.stdout and "[FAIL]" not in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
    return kb.parse_output(out.stdout), tmp, out.stdout


_REF = {}


def reference(op, set_tag, prec, k, b):
    key = (op.name, set_tag, prec, k)
    if key not in _REF:
        _REF[key] = kb.dense_solution(op.A, b)
    return _REF[key]


def load_rhs(tmp, case, prec):
    op = kb.operators()[case.op]
    tag = "g" if case.guess else "0"
    return np.fromfile(os.path.join(tmp, "rhs_%s_%s_%s.bin" % (op.name, tag, prec)), dtype=kb.NP_DTYPE[prec]).reshape(kb.NRHS, op.n).astype(np.complex128), tag


def check_masks(case, r, mask, max_iter):
    """4: the masks the solver handed out"""
    for name in ("ops", "pre"):
        calls = r[name]
        assert all(m & ~mask == 0 for m in calls), (name, [hex(m) for m in calls])
        if case.core != "cg":
            gone = 0
            for m in calls:
                assert m & gone == 0, ("a frozen system returned", name, [hex(c) for c in calls])
                gone |= mask & ~m
    for s in r["sys"]:
        assert s.ops == sum(1 for m in r["ops"] if (m >> s.k) & 1), (s, [hex(m) for m in r["ops"]])
    # what a system's ops_count may be, given its iteration count, from the statement of each method alone: an opening residual from a guess,
    # one apply per MR / GCR / CG iteration and two per BiCG step, one true residual per GCR restart or CG cycle the system STARTS -- a
    # system that has stopped takes no further apply (a converged system that is restarted once more shows here and nowhere else)
    g = 1 if case.guess else 0
    for s in r["sys"]:
        if s.slot < 0 or s.slot == 1:
            continue
        rf = case.pi if case.pi > 0 else max(max_iter, 1)
        if case.core == "mr":
            allowed = {s.iter + g}
        elif case.core == "bicg":
            allowed = {2 * s.iter + g}
        elif case.core == "gcr":   # restarts at every multiple of rf below iter; at iter itself only if the recurrence had not stopped it there
            done = (s.iter - 1) // rf if s.iter > 0 else 0
            allowed = {s.iter + g + done} | ({s.iter + g + done + 1} if s.iter > 0 and s.iter % rf == 0 else set())
        else:                      # cycles started: ceil(iter / rf), one more where a cycle ended unconverged and the next began converged
            starts = {-(-s.iter // rf)} | ({s.iter // rf + 1} if s.iter % rf == 0 else set()) if s.iter > 0 else {1}
            allowed = {s.iter + n - (1 - g) for n in starts}
        assert s.ops in allowed, (s, allowed)
    later = r["ops"][1:] if case.guess else r["ops"]
    quiet = [s.k for s in r["sys"] if s.slot == 1 or (case.guess and s.slot == 3)]
    assert all(not (m >> k) & 1 for m in later for k in quiet), [hex(m) for m in r["ops"]]
    assert all(not (m >> s.k) & 1 for m in r["ops"] for s in r["sys"] if s.slot == 1)       # a zero rhs takes part in no apply at all
    if max_iter == 0:
        assert len(r["ops"]) == (1 if case.guess else 0) and not r["pre"]


def check_systems(case, prec, r, x, b, set_tag, max_iter, twins, alone=None):
    """1, 2, 6 for the active systems of one run; x: (nrhs, stride) as stored, b: the six right-hand sides in complex128"""
    op = kb.operators()[case.op]
    for s in r["sys"]:
        if s.slot < 0:
            assert not s.success and s.iter == 0 and s.ops == 0
            continue
        bk, xk = b[s.slot], x[s.k, :op.n].astype(np.complex128)
        eps, bn = kb.case_eps(case, prec, s.slot), np.linalg.norm(b[s.slot])
        if s.slot == 1:
            assert s.success and s.iter == 0 and s.res_sq == 0.0 and s.ops == 0 and not x[s.k, :op.n].any(), s
            continue
        assert np.isfinite(x[s.k, :op.n]).all()
        assert (np.sqrt(s.res_sq) < eps * bn) == s.success, s
        if s.success:
            kb.check_bars(op, xk, bk, eps, reference(op, set_tag, prec, s.slot, bk))
        elif case.core == "bicg":
            assert max_iter <= s.iter < max_iter + case.pi, s
        else:
            assert s.iter == max_iter, s
        if not case.converging:
            true = kb.residual_norm(op.A, xk, bk)
            assert abs(np.sqrt(s.res_sq) - true) <= RES_AGREE[prec][case.core] * bn, (s, true, np.sqrt(s.res_sq))
        else:
            assert s.success, s
        conv, it = twins[s.slot][:2]
        assert abs(s.iter - it) <= case.slack, ("twin", s, it)
        if alone is not None:
            assert abs(s.iter - alone[s.slot].iter) <= case.slack and s.success == alone[s.slot].success, ("alone", s, alone[s.slot])


def check_untouched(r, x, n, mask, dtype):
    """5"""
    assert r["rhs"] == 1
    nrhs, stride = x.shape
    fill = kb.nan_fill(stride, dtype).tobytes()
    for k in range(nrhs):
        if (mask >> k) & 1:
            assert np.isfinite(x[k, :n]).all(), k
            assert x[k, n:].tobytes() == fill[:(stride - n) * x.itemsize], ("padding", k)
        else:
            assert x[k].tobytes() == fill, ("masked-out slot", k)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_uneven_batch_against_dense_solves(run, case):
    runs, tmp, _ = run
    op = kb.operators()[case.op]
    for prec in PRECS:
        dtype = kb.NP_DTYPE[prec]
        resolved, twins = host.twin_table()[(case.name, prec)]
        b, set_tag = load_rhs(tmp, case, prec)
        alone = None
        if case.converging:
            alone = []
            for k in range(kb.NRHS):
                tag = "%s_%s_a%d" % (case.name, prec, k)
                xa = np.fromfile(os.path.join(tmp, "x_%s.bin" % tag), dtype=dtype).reshape(1, op.n)
                ra = dict(runs[tag], sys=[s._replace(slot=k) for s in runs[tag]["sys"]])
                check_masks(case, ra, 1, resolved.max_iter)
                check_systems(case, prec, ra, xa, b, set_tag, resolved.max_iter, twins)
                check_untouched(ra, xa, op.n, 1, dtype)
                alone.append(ra["sys"][0])
        for p, stride in enumerate((op.n, op.n + kb.STRIDE_PAD)):
            for mask in (kb.FULL, kb.PARTIAL):
                tag = "%s_%s_s%d_%x" % (case.name, prec, p, mask)
                r = runs[tag]
                x = np.fromfile(os.path.join(tmp, "x_%s.bin" % tag), dtype=dtype).reshape(kb.NRHS, stride)
                check_masks(case, r, mask, resolved.max_iter)
                check_systems(case, prec, r, x, b, set_tag, resolved.max_iter, twins, alone)
                check_untouched(r, x, op.n, mask, dtype)
                # 3: exact scale covariance of slot 4 against slot 0
                s0, s4 = r["sys"][0], r["sys"][4]
                assert (s4.iter, s4.ops, s4.success) == (s0.iter, s0.ops, s0.success), (s0, s4)
                assert np.array_equal(x[4, :op.n], x[0, :op.n] * dtype(kb.SCALE)), tag


def test_gcr_on_sixteen_systems_under_a_sparse_mask(run):
    runs, tmp, _ = run
    case = next(c for c in CASES if c.name == "gcr8")
    op = kb.operators()[case.op]
    mask, nrhs, stride = 0xA5A5, 16, op.n + kb.STRIDE_PAD
    for prec in PRECS:
        dtype = kb.NP_DTYPE[prec]
        resolved, twins = host.twin_table()[(case.name, prec)]
        b, set_tag = load_rhs(tmp, case, prec)
        tag = "gcr8_%s_s1_a5a5" % prec
        r = runs[tag]
        x = np.fromfile(os.path.join(tmp, "x_%s.bin" % tag), dtype=dtype).reshape(nrhs, stride)
        assert [s.slot for s in r["sys"]] == [0, -1, 1, -1, -1, 2, -1, 3, 4, -1, 5, -1, -1, 0, -1, 1]
        check_masks(case, r, mask, resolved.max_iter)
        check_systems(case, prec, r, x, b, set_tag, resolved.max_iter, twins)
        check_untouched(r, x, op.n, mask, dtype)
        assert np.array_equal(x[8, :op.n], x[0, :op.n] * dtype(kb.SCALE)) and np.array_equal(x[13, :op.n], x[0, :op.n])


def iteration_table(runs):
    """the observed per-slot iteration counts of the full-mask batches (profiles/krylov_batch_cases.txt)"""
    lines = ["# case precision max_iter : iterations of slots 0..5 (batch, stride n, mask 0x3f) | the CPU twins alone | success of the batch"]
    for case in CASES:
        for prec in PRECS:
            resolved, twins = host.twin_table()[(case.name, prec)]
            r = runs["%s_%s_s0_3f" % (case.name, prec)]
            lines.append("%-16s %s %3d : %s | %s | %s" % (case.name, prec, resolved.max_iter, " ".join("%3d" % s.iter for s in r["sys"]),
                                                        " ".join("%3d" % t[1] for t in twins), " ".join(str(int(s.success)) for s in r["sys"])))
    return "\n".join(lines) + "\n"
