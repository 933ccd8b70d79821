"""The three stream-taking entry points of the even-odd Moebius unit (qmg_mobius_inv5, qmg_mobius_hops_inv5, qmg_mobius_schur_apply) in the
case table of tests/test_gpu_streams.py, and through its protocol.

tests/test_host_stream_binding.py holds that table to include/qmg_hip.h: every prototype that ends in `void* stream` has a case.  This
module adds the cases for the three entries to the table when it is imported -- which pytest does while it collects the tests directory,
before any test runs -- with the table's own `case` decorator, and runs them through the table's own protocol (`run_case`: a synchronised
null-stream reference, a decoy run, then the call enqueued on a created stream behind a closed gate; every output and its copy must equal the
reference byte for byte), as tests/test_gpu_streams_mobius.py does for the operator.  The cases are the Shamir even-odd ones of the table on
the same lattice and vectors, in both precisions as masked batches of three; the Schur apply runs both ops (two launches each on the stream).
"""
import numpy as np
import pytest

import test_gpu_streams as streams
from test_gpu_streams import gate_stream      # the module's created stream and gate length (a fixture)  # noqa: F401

qmg = streams.qmg
P = qmg
pytestmark = pytest.mark.gpu

MOB = dict(w=1.0, M5=-1.0, b5=1.5, c5=0.5)
DW, DLS, DMASS, DSTRIDE = streams.DW, streams.DLS, streams.DMASS, streams.DSTRIDE
MINE = ("qmg_mobius_inv5", "qmg_mobius_hops_inv5", "qmg_mobius_schur_apply")
NRHS, MASK = 3, 0b101
INV_P, HOP_P = P.P_CLOVER_E | P.P_CLOVER_O, P.P_OE | P.P_ZERO_O
E_FULL = P.P_CLOVER_E | P.P_EO | P.P_SHIFT_E | P.P_ZERO_E


def desc():
    return qmg.make_desc(DW[0], DW[1], 2 * DLS, None, None, 0.0)


def mobius_eo_case(sym, dtype, op=0):
    vdt = streams.NPT[dtype]

    def call(b, s):
        if sym == "qmg_mobius_inv5":
            qmg.mobius_inv5(dtype, desc(), DLS, DMASS, b.lhs, b.rhs, INV_P, qmg.MOBIUS_S_AINV_B, 0.7 - 0.2j, nrhs=NRHS, vec_stride=DSTRIDE, mask=MASK, stream=s, **MOB)
        elif sym == "qmg_mobius_hops_inv5":
            qmg.mobius_hops_inv5(dtype, desc(), b.g, DLS, DMASS, b.lhs, b.rhs, HOP_P, qmg.MOBIUS_S_AINV, qmg.MOBIUS_R_B, 0.7 - 0.2j, qmg.DWF_G5_IN, nrhs=NRHS,
                                 vec_stride=DSTRIDE, mask=MASK, stream=s, **MOB)
        else:
            qmg.mobius_schur_apply(dtype, desc(), b.g, DLS, DMASS, b.lhs, b.rhs, b.tmp, 0, op, nrhs=NRHS, vec_stride=DSTRIDE, mask=MASK, stream=s, **MOB)

    def reach():
        n = bin(MASK).count("1")
        if sym == "qmg_mobius_inv5":
            assert qmg.mobius_eo_plan(dtype, DW, DLS, qmg.MEK_INV5, INV_P, qmg.MOBIUS_S_AINV_B, 0, n)[0] == qmg.MEF_MIX
        elif sym == "qmg_mobius_hops_inv5":
            assert qmg.mobius_eo_plan(dtype, DW, DLS, qmg.MEK_HOPS_INV5, HOP_P, qmg.MOBIUS_S_AINV, qmg.MOBIUS_R_B, n)[0] == qmg.MEF_HOPS_MIX
        else:
            assert qmg.mobius_eo_plan(dtype, DW, DLS, qmg.MEK_HOPS_INV5, HOP_P, 2 if op else 1, 0 if op else 1, n)[0] == qmg.MEF_HOPS_MIX
            assert qmg.mobius_eo_plan(dtype, DW, DLS, qmg.MEK_SCHUR2_DAGGER if op else qmg.MEK_SCHUR2, E_FULL, 0, 0, n)[0] == (
                qmg.MEF_SCHUR2_DAGGER if op else qmg.MEF_SCHUR2)
    ins = {"rhs": streams.dwf_vec(2, vdt, NRHS)}
    if sym != "qmg_mobius_inv5":
        ins["g"] = streams.links(*DW, 1, vdt)
    return streams.Case(call, ins=ins, inout={"lhs": streams.dwf_vec(3, vdt, NRHS)},
                        outs={"tmp": (vdt, DSTRIDE * NRHS)} if sym == "qmg_mobius_schur_apply" else {}, reach=reach)


for _dt in (streams.C64, streams.C32):
    for _sym in MINE[:2]:
        streams.case(_sym, label=streams.TAG[_dt])(lambda y=_sym, d=_dt: mobius_eo_case(y, d))
    for _op in (0, 1):
        streams.case(MINE[2], label="%s-op%d" % (streams.TAG[_dt], _op))(lambda d=_dt, o=_op: mobius_eo_case(MINE[2], d, o))

ALL = [(sym, label, maker) for sym in MINE for label, maker in streams.CASES[sym]]
IDS = [sym[4:] + ("-" + label if label else "") for sym, label, _ in ALL]


def test_the_table_has_the_cases():
    assert [len(streams.CASES[s]) for s in MINE] == [2, 2, 4] and len(set(IDS)) == 8


@pytest.mark.parametrize("sym,label,maker", ALL, ids=IDS)
def test_call_stays_on_its_stream(sym, label, maker, gate_stream):
    got, ref = streams.run_case(maker(), gate_stream)
    assert sorted(got) == sorted(ref)
    for k in ref:
        assert np.array_equal(got[k], ref[k]), "%s %s: `%s` differs from the synchronised null-stream run in %d of %d bytes" % (
            sym, label, k, int(np.count_nonzero(got[k] != ref[k])), ref[k].size)


def test_escaped_call_is_caught(gate_stream):
    """The negative control on an LDS kernel (the dagger's two launches both exchange along s): the call goes to the null stream while its
    inputs are still behind the gate; it reads the 0xFF poison."""
    maker = dict(streams.CASES["qmg_mobius_schur_apply"])["c64-op1"]
    got, ref = streams.run_case(maker(), gate_stream, escape=True)
    written = [k for k in ref if not k.startswith("input ")]
    assert any(not np.array_equal(got[k], ref[k]) for k in written), "the call ran on the null stream behind a closed gate and still matched"
