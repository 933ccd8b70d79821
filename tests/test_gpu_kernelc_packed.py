"""Kernel C, MODE 1, where the last row tile is packed (nc % 16 == 8: nc = 24 and the one-site nc = 8 form): the eight left-over
matrix rows feed ONE MFMA whose tile rows 0-7 carry Re M and rows 8-15 Im M, and the epilogue takes P and Q from the two halves of one
accumulator (forms with narrow-stored matrices; with complex<double> matrices the packed form was slower and the c64 cases below run the unpacked
one).  A wrong P / Q pairing, a swapped half or a wrong exchange lane puts another row's or another system's numbers into an output, so
every row of every site must be distinguishable: the matrices and vectors are the unsymmetric Gaussian fields of tests/test_gpu_stencil_routes.py.

Each case is a row of that file's table and goes through its check_route: the plan query must answer kernel C, MODE 1, with the systems of the
call in one pass; padded strides, a non-zero initial lhs (the accumulate cases add to it), all three shifts set with the dof shift splitting
the two halves of the rows; every active system against stencil_numpy's long-double reference at that file's tolerances (relative L2 1e-13 for
fp64 results, 3e-7 for complex<float> results, elementwise (n + 1) 2^-50 S or (n + 1) 2^-21 S on the f32 matrix pipe); frozen systems and
padding bit-identical; a second run the same bytes.

Then the batch is applied again as two smaller batches that still route to MODE 1 (they overlap where the batch is too small to halve: MODE 1
starts at 4 systems for nc = 24 and at 5 for nc = 8, so a batch of 5 at nc = 8 has no smaller one and is left out of this part).  The number of
systems only changes how many MFMA columns are fed, not a column's arithmetic: every system must come out with the same bytes.

Cases: lattices 12 x 4 and 6 x 4 at nc = 24, 6 x 4 at nc = 8 (an odd half-row: the plan answers the one-site form, not PAIR); storages c64, m32
(fp64 vectors), c32 (the f32 pipe) and m16; the full operator, the hops alone, one parity, and the full operator accumulated; 5 systems,
8 systems, and 8 with 6 active.  The batch shapes rotate over the other three axes so that each meets every storage, piece set and lattice.
"""
import importlib

import pytest

import coordspace as cs
import test_gpu_stencil_routes as tr

qmg = importlib.import_module("quantum-mg_amd")

pytestmark = pytest.mark.gpu

SHAPES = ((12, 4, 24), (6, 4, 24), (6, 4, 8))
STORAGES = (("c64", 0), ("m32", tr.M32), ("c32", tr.C32BITS), ("m16", tr.M32 | tr.M16))
PIECE_SETS = ("M0", "HOP0", "EVEN0", "M+")
BATCHES = ((5, 0b11111), (8, 0xff), (8, 0b10111101))
MODE1_FROM = {24: 4, 8: 5}     # the fewest systems the plan gives to kernel C (MODE 1 up to 8)


def rows():
    out = []
    for si, (storage, bits) in enumerate(STORAGES):
        for li, dims in enumerate(SHAPES):
            for pi, pieces in enumerate(PIECE_SETS):
                nrhs, mask = BATCHES[(si + li + pi) % 3]
                out.append(("masked", storage, dims, nrhs, mask, pieces, "", {}, [tr.C(bits, dims[2], 1, len(tr.active(mask, nrhs)))]))
    return out


ROWS = rows()


@pytest.fixture(scope="module", autouse=True)
def _device():
    qmg.build()
    qmg.init(0)
    tr.set_knobs({})
    yield
    tr.set_knobs({})
    qmg.sync()


def test_the_cases_cover_what_they_claim():
    for axis, values in ((1, [s for s, _ in STORAGES]), (2, SHAPES), (5, PIECE_SETS)):
        for v in values:
            assert {(r[3], r[4]) for r in ROWS if r[axis] == v} == set(BATCHES), (axis, v)
    assert all(d[0] // 2 % 2 == 1 for d in SHAPES if d[2] == 8)      # nc = 8 on an odd half-row: no PAIR form


@pytest.mark.parametrize("row", ROWS, ids=tr.route_id)
def test_packed_tile_against_numpy_reference(row):
    assert tr.planned(row)[0][5] & qmg.SPF_PAIR == 0
    tr.check_route(row)


def sub_batches(act, fewest):
    """two smaller sets of systems that cover `act`, each large enough for MODE 1; None if there is no smaller batch"""
    if len(act) <= fewest:
        return None
    k = max(fewest, (len(act) + 1) // 2)
    return act[:k], act[-k:]


@pytest.mark.parametrize("row", [r for r in ROWS if sub_batches(tr.active(r[4], r[3]), MODE1_FROM[r[2][2]])], ids=tr.route_id)
def test_a_batch_equals_its_sub_batches_bit_for_bit(row):
    entry, storage, dims, nrhs, mask, pieces, flags, knobs, plans = row
    Lx, Ly, nc = dims
    act = tr.active(mask, nrhs)
    mdtype, vdtype, _, vec32 = tr.STORAGE[storage]
    stride = Lx * Ly * nc + tr.PAD
    clover, hopping = tr.operator(dims, mdtype)
    rhs0, lhs0 = cs.gaussian_cvec(nrhs * stride, 3), cs.gaussian_cvec(nrhs * stride, 4)
    dcl, dhop = tr.to_device(clover, mdtype), tr.to_device(hopping, mdtype)
    desc = qmg.make_desc(Lx, Ly, nc, dcl, dhop, *tr.SHIFTS)
    dr = tr.to_device(rhs0, vdtype)

    def run(systems):
        m = sum(1 << k for k in systems)
        sub = (entry, storage, dims, nrhs, m, pieces, flags, knobs, [tr.C(plans[0][1], nc, 1, len(systems))])
        got = tr.planned(sub)
        assert [tr.instantiation(p) for p in got] == sub[8] and got[0][11] == len(systems)     # kernel C, MODE 1, one pass
        dl = tr.to_device(lhs0, vdtype)
        tr.call(sub, desc, dl, dr, stride, {})
        out = dl.to_host().reshape(nrhs, stride)
        dl.free()
        return out

    whole = run(act)
    for part in sub_batches(act, MODE1_FROM[nc]):
        assert len(part) < len(act)
        out = run(list(part))
        for k in part:
            assert out[k].tobytes() == whole[k].tobytes(), (k, part)
    for d in (dcl, dhop, dr):
        d.free()
