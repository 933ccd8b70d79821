"""The two stream-taking entry points of the Moebius operator (qmg_mobius_fill, qmg_mobius_apply_direct) in the case table of
tests/test_gpu_streams.py, and through its protocol.

tests/test_host_stream_binding.py holds that table to include/qmg_hip.h: every prototype that ends in `void* stream` has a case.  This
module adds the cases for the Moebius entries to the table when it is imported -- which pytest does while it collects the tests directory,
before any test runs -- with the table's own `case` decorator, and runs them through the table's own protocol (`run_case`: a synchronised
null-stream reference, a decoy run, then the call enqueued on a created stream behind a closed gate; every output and its copy must equal the
reference byte for byte).  The cases are the Shamir ones of the table on the same lattice and vectors: the fill, and both ops of the apply in
both precisions as masked batches of three (op 0 mixes on the load, op 1 through LDS).
"""
import numpy as np
import pytest

import test_gpu_streams as streams
from test_gpu_streams import gate_stream      # the module's created stream and gate length (a fixture)  # noqa: F401

qmg = streams.qmg
pytestmark = pytest.mark.gpu

MOB = dict(w=1.0, M5=-1.0, b5=1.5, c5=0.5)
DW, DLS, DMASS, DSTRIDE = streams.DW, streams.DLS, streams.DMASS, streams.DSTRIDE
MINE = ("qmg_mobius_fill", "qmg_mobius_apply_direct")


@streams.case("qmg_mobius_fill")
def _fill():
    cm = DW[0] * DW[1] * (2 * DLS) ** 2
    return streams.Case(lambda b, s: qmg.mobius_fill(b.cl, b.ho, b.g, DW[0], DW[1], DLS, DMASS, stream=s, **MOB), ins={"g": streams.links(*DW, 1)},
                        outs={"cl": (streams.c128, cm), "ho": (streams.c128, 4 * cm)})


def mobius_apply_case(dtype, op, nrhs, mask, pieces):
    vdt = streams.NPT[dtype]

    def reach():
        assert qmg.mobius_plan(dtype, DW, DLS, op, pieces, bin(mask).count("1"))[0] == (qmg.MF_RESULT if op else qmg.MF_LOAD)
    return streams.Case(lambda b, s: qmg.mobius_apply_direct(dtype, streams.dwf_desc(), b.g, DLS, DMASS, b.lhs, b.rhs, pieces, op=op, nrhs=nrhs, vec_stride=DSTRIDE,
                                                             mask=mask, stream=s, **MOB),
                        ins={"g": streams.links(*DW, 1, vdt), "rhs": streams.dwf_vec(2, vdt, nrhs)}, inout={"lhs": streams.dwf_vec(3, vdt, nrhs)}, reach=reach)


for _dt in (streams.C64, streams.C32):
    for _op in (0, 1):
        streams.case("qmg_mobius_apply_direct", label="%s-op%d" % (streams.TAG[_dt], _op))(
            lambda d=_dt, o=_op: mobius_apply_case(d, o, 3, 0b101, streams.MP if o else streams.M0))

ALL = [(sym, label, maker) for sym in MINE for label, maker in streams.CASES[sym]]
IDS = [sym[4:] + ("-" + label if label else "") for sym, label, _ in ALL]


def test_the_table_has_the_cases():
    assert [len(streams.CASES[s]) for s in MINE] == [1, 4] and len(set(IDS)) == 5


@pytest.mark.parametrize("sym,label,maker", ALL, ids=IDS)
def test_call_stays_on_its_stream(sym, label, maker, gate_stream):
    got, ref = streams.run_case(maker(), gate_stream)
    assert sorted(got) == sorted(ref)
    for k in ref:
        assert np.array_equal(got[k], ref[k]), "%s %s: `%s` differs from the synchronised null-stream run in %d of %d bytes" % (
            sym, label, k, int(np.count_nonzero(got[k] != ref[k])), ref[k].size)


def test_escaped_call_is_caught(gate_stream):
    """The negative control on op 1: the call goes to the null stream while its inputs are still behind the gate; it reads the 0xFF poison."""
    maker = dict(streams.CASES["qmg_mobius_apply_direct"])["c64-op1"]
    got, ref = streams.run_case(maker(), gate_stream, escape=True)
    written = [k for k in ref if not k.startswith("input ")]
    assert any(not np.array_equal(got[k], ref[k]) for k in written), "the call ran on the null stream behind a closed gate and still matched"
