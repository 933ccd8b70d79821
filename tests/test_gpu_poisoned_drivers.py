"""Every driver twice: plain, and with QMG_MALLOC_POISON=1.

Under the key every qmg_malloc, every block that leaves VecPool::get or ArrayStorageMG::check_out -- recycled ones included -- and the
library's own scratch where it is created or grown hold 0xFF, a NaN in every storage.  A solver that reads a vector before it writes it
then computes with NaN instead of with the previous solve's plausible numbers.  Each driver runs on the smallest command line its own test
uses; the result lines those tests parse -- iteration counts, alleged and check tolerances, [KRYLOV], [QMG-MRHS] and [QMG-MRHS-VERIFY] rows, the multi-shift [BATCH] rows, OPS / ITER stats,
[HMC] rows with plaquette, acceptance and exp_mdH, correlator rows, the self-tests' verdict lines -- must be EQUAL AS STRINGS in the two
runs, and "nan" must not appear.  Timing lines are not compared.
"""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVERS = os.path.join(ROOT, "quantum-mg_amd", "drivers")

RESULT = re.compile(r"^(\[BATCH0?\] rhs .*|\[GUESS\] .*|\[STATE\] .*|\[QMG-ERROR\].*|Multigrid (converged|failed to converge) in .*|Check tolerance .*|\[KRYLOV\] .*|\[QMG-MRHS\]: rhs \d+ .*|\[QMG-MRHS-VERIFY\]: rhs \d+ .*|\[QMG-OPS-STATS\].*|\[QMG-ITER-STATS\].*"
                    r"|\[HMC\] .*|\[HMC-FINAL\] .*|\[HMC-READBACK\] .*|\[RHMC\] .*|\[RHMC-CHECK\] .*|\[FLOW\] .*|\[FLOW-READBACK\] .*|\[QMG-DWF\] .*|\[QMG-DWF-EO\] .*"
                    r"|\[QMG-WARD\]: .*|\[QMG-MRES\]: .*|\[QMG-COARSEST-EVALS\]: .*|\[QMG-SLAB\]: world .*|\[ OK \] .*|\[FAIL\] .*|\[SELFTEST \w+\].*)$")


def result_lines(stdout):
    """the lines the drivers' own tests parse, in order; the rows between [QMG-BEGIN-x] and [QMG-END-x] (dwf_measure's correlators) with them"""
    out, block = [], None
    for ln in stdout.splitlines():
        if ln.startswith("[QMG-BEGIN-"):
            block = ln
        if block is not None or RESULT.match(ln):
            out.append(re.sub(r" ; single-path solve \S+ s$", "", ln))      # (a [QMG-MRHS-VERIFY] row ends in a timing)
        if ln.startswith("[QMG-END-"):
            block = None
    return out


def undefined_effective_masses(stdout):
    """The rows of a [QMG-BEGIN-PION-EFFMASS] block that have no real value: m(t) = acosh((C(t+1) + C(t-1)) / (2 C(t))) where the printed
    correlator of the [QMG-BEGIN-PION] block gives an argument below 1 (one 8 x 8 configuration is not convex around its midpoint).  The
    plain run prints "-nan" there, as the reference's drivers do; it is arithmetic on finite, printed numbers, not a vector read before it
    was written -- every other "nan" is."""
    lines = stdout.splitlines()
    block = lambda name: [ln.split() for ln in lines[lines.index("[QMG-BEGIN-%s]" % name) + 1:lines.index("[QMG-END-%s]" % name)]] if "[QMG-BEGIN-%s]" % name in lines else []
    pion = [float(v) for _, v in block("PION")]
    assert all(np.isfinite(pion))
    return {"%s %s" % (t, v) for t, v in block("PION-EFFMASS") if (pion[int(t) + 1] + pion[int(t) - 1]) / (2.0 * pion[int(t)]) < 1.0}


def gauge(L):
    return os.path.join(ROOT, "tests", "golden", "l%dt%db60_heatbath.dat" % (L, L))


def small_cfg(tmp):
    """test_gpu_dwf_meas.py's 8 x 8 file"""
    path = os.path.join(tmp, "cfg8.dat")
    with open(path, "w") as f:
        f.write("".join("%.17g\n" % p for p in 0.4 * np.random.default_rng(11).standard_normal(128)))
    return path


Q = {"QMG_QUIET": "1"}
# (id, program, arguments (TMP: a fresh directory of the run), environment, minimum number of result lines, timeout in seconds)
CASES = [
    ("n13", "n13_wilson_kcycle", ["32", "-0.03", "6.0", "1", "4", gauge(32), "32"], Q, 3, 300),
    ("n13_mrhs5_point_f32", "n13_wilson_kcycle_mrhs", ["64", "-0.07", "6.0", "2", "8", gauge(64), "64", "5", "verify", "f32"], dict(Q, QMG_MRHS_POINT="1"), 10, 300),
    ("n19_schur", "n19_wilson_kcycle_precond", ["64", "2", gauge(64), "64"], Q, 2, 150),
    ("n22", "n22_wilson_kcycle_adaptive", ["64", "-0.07", "6.0", "2", "1", gauge(64), "64"], Q, 8, 150),
    ("n22_schur", "n22_wilson_kcycle_adaptive", ["64", "-0.07", "6.0", "2", "1", gauge(64), "64", "schur"], Q, 8, 150),
    ("krylov_parity", "krylov_parity", ["32", "0.05", gauge(32), "TMP"], {}, 8, 200),
    ("multishift_parity", "multishift_parity", ["32", gauge(32), "TMP", "staggered", "0.04,0.06,0.08,0.1"], {}, 8, 300),
    # the gauged Laplace operator: the run that prints the [BATCH] / [BATCH0] rows of three systems by four shifts, and one refused non-zero guess
    ("multishift_parity_laplace", "multishift_parity", ["32", gauge(32), "TMP", "laplace", "0.001,0.01,0.1,1.0"], {}, 32, 300),
    ("facade_selftest", "facade_selftest", [gauge(32)], {}, 86, 150),
    ("dwf_selftest", "dwf_selftest", ["8", "6", "0.05", "7"], {}, 8, 300),
    ("dwf_eo_selftest", "dwf_eo_selftest", ["8", "6", "0.05", "7"], {}, 9, 300),
    ("dwf_measure", "dwf_measure", ["8", "CFG8", "0.05", "4", "-1", "1e-12"], {}, 10, 300),
    ("hmc_two_flavours", "schwinger_hmc", ["8", "4.0", "0.1", "2", "3", "0", "4", "99", "TMP/a.dat", "heatbath"], {}, 4, 120),
    ("hmc_one_flavour", "schwinger_hmc", ["8", "4.0", "0.1", "1", "3", "0", "4", "99", "TMP/a.dat", "heatbath", "8", "0.1"], {}, 4, 120),
    ("hmc_staggered", "schwinger_hmc", ["8", "4.0", "0.2", "2", "3", "0", "4", "99", "TMP/a.dat", "heatbath", "staggered"], {}, 4, 120),
    ("dwf_hmc", "dwf_hmc", ["8", "4", "2.0", "0.2", "2", "40", "10", "10", "77", "TMP/dwf.dat", "cold"], {}, 51, 300),
    ("u1_flow_measure", "u1_flow_measure", [gauge(32), "32", "0.05", "20", "10", "3", "4", "TMP/flowed.dat"], {}, 4, 300),
    ("n13_deflated", "n13_wilson_kcycle", ["128", "-0.06", "6.0", "2", "8", gauge(128), "128"], dict(Q, QMG_COARSEST_TYPE="mmd", QMG_DEFLATE="16"), 19, 300),
    # two ranks emulated by host threads, each with its own stream and its own VecPool: the ranks print in any order, so the lines are compared as a sorted list
    ("n13_slab_2_ranks", "n13_wilson_kcycle_slab", ["128", "-0.05", "6.0", "2", "8", gauge(64), "64"], dict(Q, QMG_NULL_BATCH="1", QMG_COMM_EMULATE="2"), 3, 600),
]
UNORDERED = ("n13_slab_2_ranks",)
EXPECTED_ERRORS = {"multishift_parity_laplace": 1}      # "[QMG-ERROR]: CG-M: non-zero initial guess", asked for by the driver (test_gpu_multishift.py)


def run_case(case, tmp, poison):
    name, prog, args, extra, _, timeout = case
    os.makedirs(tmp, exist_ok=True)
    args = [small_cfg(tmp) if a == "CFG8" else a.replace("TMP", tmp) for a in args]
    env = dict(os.environ)
    for k in ("QMG_MALLOC_POISON", "QMG_TUNING", "QMG_DEFLATE", "QMG_DEFLATE_USE", "QMG_COARSEST_TYPE", "QMG_DUMP_DIR", "QMG_F32_KCYCLE", "QMG_COARSE_F32", "QMG_MRHS_POINT"):
        env.pop(k, None)
    env.update(extra)
    if poison:
        env["QMG_MALLOC_POISON"] = "1"
    return subprocess.run([os.path.join(DRIVERS, prog)] + args, cwd=DRIVERS, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=timeout)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_a_driver_prints_the_same_results_under_malloc_poison(case, tmp_path):
    assert os.path.exists(os.path.join(DRIVERS, case[1])), "drivers/%s is not built" % case[1]
    plain = run_case(case, str(tmp_path / "plain"), False)
    poisoned = run_case(case, str(tmp_path / "poisoned"), True)
    for tag, out in (("plain", plain), ("poisoned", poisoned)):
        assert out.returncode == 0, (tag, out.stdout[-3000:] + out.stderr[-2000:])
        assert out.stdout.count("[QMG-ERROR]") == EXPECTED_ERRORS.get(case[0], 0), (tag, out.stdout[-3000:])
        nans = [ln for ln in out.stdout.splitlines() if re.search(r"(?<![a-z])nan(?![a-z])", ln, re.I)]      # nan, -nan, NaN; not "dominant"
        assert set(nans) <= undefined_effective_masses(out.stdout), (tag, nans[:5])
    a, b = result_lines(plain.stdout), result_lines(poisoned.stdout)
    if case[0] in UNORDERED:
        a, b = sorted(a), sorted(b)
    assert len(a) >= case[4], (len(a), plain.stdout[-3000:])
    differ = [(x, y) for x, y in zip(a, b) if x != y]
    assert len(a) == len(b) and not differ, differ[:5]
