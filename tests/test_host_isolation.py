"""tests/isolation.py without a device.

  * the byte helpers: 0xFF is a NaN in all three storages, a band keeps the operand's alignment or misalignment;
  * the parity and ZERO rules against the REFERENCES (stencil_numpy.apply, dwf_numpy.apply, dwf_eo_numpy: the grid formulas), not against
    kernel code: with the inputs poisoned by the rule a reference returns, on every element the call writes, exactly the numbers it returns
    on clean inputs and no NaN -- for every piece set and flag combination the route tables use -- and poisoning ONE more element that the rule
    says is read puts a NaN into the result: the rule is tight, not merely safe;
  * the comparison logic against deliberately leaky numpy stand-ins (a batched apply that adds 0 * frozen_system, one that reads padding, one
    that loads the lhs it clears, one that writes a frozen system): check_isolation must flag each, and pass the honest one;
  * coverage over the tables: every served row has poisoned bytes in every operand it passes, every kernel family and storage the plans name
    occurs in a row with a hole in its mask, and the GPU module parametrises over the whole of each table.
"""
import importlib

import numpy as np
import pytest

import dwf_eo_numpy as de
import dwf_numpy as dn
import isolation as iso
import stencil_numpy as sn
import test_gpu_dwf as tdw
import test_gpu_dwf_eo as tde
import test_gpu_isolation as gi
import test_gpu_stencil_routes as tr
import test_gpu_transfer_routes as tx
import test_gpu_wilson_routes as tw

qmg = importlib.import_module("quantum-mg_amd")


@pytest.fixture(scope="module", autouse=True)
def _library():
    qmg.build()      # the plan queries of the coverage tests are host code of the library


def cvec(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


# ---------------------------------------------------------------- bytes
def test_the_poison_is_a_nan_in_every_storage():
    keep = np.array([True, False, True, False])
    for dtype in (np.complex128, np.complex64):
        a = iso.poisoned(np.arange(1, 5).astype(dtype), keep)
        assert np.isnan(a.real[~keep]).all() and np.isnan(a.imag[~keep]).all()
        assert a[keep].tolist() == [1, 3]
    h = iso.poisoned(np.arange(1, 9).astype(np.float16), np.repeat(keep, 2))       # complex<half> as interleaved float16 pairs
    assert np.isnan(h[~np.repeat(keep, 2)]).all() and h[np.repeat(keep, 2)].tolist() == [1, 2, 5, 6]
    src = np.ones(3, dtype=np.complex64)
    iso.poisoned(src, np.zeros(3, dtype=bool))
    assert src.tolist() == [1, 1, 1]                                               # a copy: the operand itself is left alone


def test_a_band_keeps_the_alignment_and_owns_what_surrounds_the_operand():
    a = np.arange(10).astype(np.complex64)
    for lead in (0, 1):
        image, offset = iso.band(a, lead)
        assert offset % 16 == (8 * lead) % 16 and iso.GUARD % 16 == 0
        assert image.size == iso.GUARD + lead * 8 + a.nbytes + iso.GUARD
        assert np.all(image[:offset] == 0xFF) and np.all(image[offset + a.nbytes:] == 0xFF)
        assert iso.unband(image, offset, a).tobytes() == a.tobytes()


# ---------------------------------------------------------------- the rules against the references
def hold_reference(reference, roles, clean, aliases=()):
    """reference({role: array}) -> {role: result}: exact on the written elements under the rule's poison, a NaN from one more element"""
    ops = iso.operands_of(roles, clean, aliases)
    shared = {b: a for a, b in aliases}

    def inputs(extra=None):
        bufs = {}
        for name, op in ops.items():
            keep = op.reads.copy()
            if extra is not None and extra[0] == name:
                keep[extra[1]] = False
            bufs[name] = iso.poisoned(op.clean, keep)
        return {role: bufs[shared.get(role, role)] for role in roles}

    want = reference({role: ops[shared.get(role, role)].clean for role in roles})
    got = reference(inputs())
    written = 0
    for name, op in ops.items():
        if op.writes.any():
            w = op.writes
            written += int(w.sum())
            assert not np.isnan(got[name][w]).any(), (name, "the rule poisons an element the reference reads")
            assert np.array_equal(got[name][w], want[name][w]), name      # (not tobytes: a long double carries six bytes of padding)
    # tight: one more poisoned element of every contiguous run the rule says is read reaches a written element
    for name, op in ops.items():
        idx = np.flatnonzero(op.reads)
        if idx.size == 0:
            continue
        starts = idx[np.concatenate([[True], np.diff(idx) > 1])]
        half = op.reads.size // 2
        probes = set(int(s) for s in starts) | ({int(idx[idx >= half][0])} if (idx >= half).any() else set())
        for i in sorted(probes):
            out = reference(inputs((name, i)))
            assert any(np.isnan(out[n][o.writes]).any() for n, o in ops.items() if o.writes.any()), (name, i, "the rule says read; the reference does not read it")
    return written


def stencil_combinations():
    """(pieces name, noclover, nohopping, inplace) over the stored-stencil and Wilson tables"""
    seen = set()
    for row in tr.ROUTES:
        seen.add((row[5], "noclover" in row[6], "nohopping" in row[6], "inplace" in row[6]))
    for row in tw.ROUTES:
        if gi.wilson_served(row):
            seen.add((row[5], row[0].startswith("hops"), False, "inplace" in row[6].split()))
    return sorted(seen)


def test_every_piece_set_of_the_tables_is_exercised():
    assert {c[0] for c in stencil_combinations()} == set(tr.PIECES)


@pytest.mark.parametrize("dims", [(4, 4, 2), (2, 2, 3), (1, 1, 2)], ids=lambda d: "%dx%dx%d" % d)
@pytest.mark.parametrize("combo", stencil_combinations(), ids=lambda c: "%s%s%s%s" % (c[0], "-noclover" * c[1], "-nohopping" * c[2], "-inplace" * c[3]))
def test_stencil_rule_against_stencil_numpy(combo, dims):
    name, noclover, nohopping, inplace = combo
    Lx, Ly, nc = dims
    size, pc = Lx * Ly * nc, tr.PIECES[name]
    clover = None if noclover else cvec(Lx * Ly * nc * nc, 1)
    hopping = None if nohopping else cvec(4 * Lx * Ly * nc * nc, 2)
    shifts = tr.SHIFTS if nc % 2 == 0 else tr.SHIFTS[:2] + (0.0,)
    roles = iso.stencil_reads("masked", dims, 1, size, 1, pc, "", not noclover, not nohopping)
    rhs = cvec(size, 3)
    clean = {"rhs": rhs, "lhs": rhs if inplace else cvec(size, 4)}
    reference = lambda v: {"lhs": sn.apply(Lx, Ly, nc, clover, hopping, *shifts, pc, v["rhs"], v["lhs"])[0], "rhs": None}
    if inplace:
        assert not (roles["rhs"][0] & roles["lhs"][1]).any()      # an in-place row reads one half and writes the other
    hold_reference(reference, roles, clean, [("lhs", "rhs")] if inplace else [])


DWF_DIMS, DWF_LS = (4, 4), 3


@pytest.mark.parametrize("call", gi.DWF_CALLS + [("direct", p, 0, 0) for p in tdw.SERVED] + [("hops", p, 0, f) for p in tde.K_PIECES for f in (0, 1)]
                         + [("inv5", P, 0, 0) for P in (sn.P_CLOVER_E,)] + [("schur", 0, p, f) for p in (0, 1) for f in range(4)],
                         ids=lambda c: "%s-%x-p%d-g%d" % c)
def test_dwf_rules_against_the_grid_formulas(call):
    entry, pieces, parity, flags = call
    (Lx, Ly), Ls = DWF_DIMS, DWF_LS
    n = Lx * Ly * 2 * Ls
    g = tde.gauge(Lx, Ly)
    roles = iso.dwf_reads(entry, n, 1, n, 1, pieces, parity)
    clean = {role: cvec(n, seed) for role, seed in (("rhs", 1), ("lhs", 2), ("tmp", 3)) if role in roles}
    if entry == "direct":
        reference = lambda v: {"lhs": dn.apply(Lx, Ly, Ls, g, tdw.M, tdw.W, *tdw.SHIFTS, pieces, v["rhs"], v["lhs"])[0]}
    elif entry == "inv5":
        reference = lambda v: {"lhs": de.inv5(Lx, Ly, Ls, tde.M, tde.W, tde.SHIFT, tde.EO_SHIFT, pieces, tde.ALPHA, v["rhs"], v["lhs"])[0]}
    elif entry == "hops":
        reference = lambda v: {"lhs": de.hops_inv5(Lx, Ly, Ls, g, tde.M, tde.W, tde.SHIFT, tde.EO_SHIFT, pieces, tde.ALPHA, flags, v["rhs"], v["lhs"])[0]}
    else:
        def reference(v):
            out = de.schur(Lx, Ly, Ls, g, tde.M, tde.W, tde.SHIFT, tde.EO_SHIFT, parity, flags, v["rhs"], v["lhs"], v["tmp"])
            return {"lhs": out[0], "tmp": out[3]}
        assert not roles["tmp"][0].any() and not roles["lhs"][0].any()      # scratch and an overwritten lhs: poisoned everywhere
    assert hold_reference(reference, roles, clean) > 0


# ---------------------------------------------------------------- the comparison logic against leaky stand-ins
NRHS, MASK, SIZE, STRIDE = 3, 0b101, 8, 10


def stand_in(leak):
    """check_isolation's `execute` for a numpy batched apply  lhs_k = (ZERO even half ? 0 : lhs_k) + 2 rhs_k  with pieces EO0-like semantics:
    even half overwritten, odd half untouched; `leak` names what it does wrong"""
    def execute(images):
        v = {name: iso.unband(im, off, np.empty((im.size - 2 * iso.GUARD) // 16, dtype=np.complex128)) for name, (im, off) in images.items()}
        rhs, lhs = v["rhs"], v["lhs"]
        for k in iso.active(MASK, NRHS):
            even = slice(k * STRIDE, k * STRIDE + SIZE // 2)
            odd = slice(k * STRIDE + SIZE // 2, k * STRIDE + SIZE)
            out = 2 * rhs[odd]
            if leak == "frozen":
                out = out + 0 * rhs[1 * STRIDE + SIZE // 2:1 * STRIDE + SIZE]
            if leak == "padding":
                out = out + 0 * rhs[k * STRIDE + SIZE]
            if leak == "lhs":
                out = out + 0 * lhs[even]
            if leak == "parity":
                out = out + 0 * rhs[even]
            lhs[even] = out
        if leak == "writes":
            lhs[1 * STRIDE] = 1.0
        if leak == "band":
            images["lhs"][0][3] = 0
        after = {}
        for name, (im, off) in images.items():
            im = im.copy()
            im[off:off + v[name].nbytes] = v[name].view(np.uint8)
            after[name] = im
        norms = np.array([np.vdot(lhs[k * STRIDE:k * STRIDE + SIZE // 2], lhs[k * STRIDE:k * STRIDE + SIZE // 2]).real for k in iso.active(MASK, NRHS)])
        if leak == "norms":
            norms = norms + 0 * lhs[1 * STRIDE].real
        return after, norms.tobytes()
    return execute


def stand_in_operands():
    pieces = tr.PIECES["EO0"]
    roles = iso.stencil_reads("masked", (2, 2, 2), NRHS, STRIDE, MASK, pieces)
    return iso.operands_of(roles, {"rhs": cvec(NRHS * STRIDE, 5), "lhs": cvec(NRHS * STRIDE, 6)})


def test_an_honest_stand_in_passes():
    counts = iso.check_isolation(stand_in_operands(), stand_in(None))
    assert counts == {"rhs": 16 * (NRHS * STRIDE - 2 * SIZE // 2), "lhs": 16 * NRHS * STRIDE}       # rhs: two odd halves kept; lhs: nothing is read


@pytest.mark.parametrize("leak", ["frozen", "padding", "lhs", "parity", "writes", "band", "norms"])
def test_a_leaky_stand_in_is_flagged(leak):
    with pytest.raises(iso.Leak):
        iso.check_isolation(stand_in_operands(), stand_in(leak))


def test_a_refusal_must_leave_every_byte():
    def refusing(images):
        return {name: im.copy() for name, (im, _) in images.items()}, b""

    def scribbling(images):
        after = {name: im.copy() for name, (im, _) in images.items()}
        after["lhs"][iso.GUARD] ^= 1
        return after, b""

    iso.check_isolation(stand_in_operands(), refusing, served=False)
    with pytest.raises(iso.Leak):
        iso.check_isolation(stand_in_operands(), scribbling, served=False)


# ---------------------------------------------------------------- coverage over the tables
TABLES = {
    "stencil": (tr.ROUTES, lambda row: gi.stencil_case(row, data=False), gi.stencil_served, lambda row: (row[8][0][0], row[8][0][1]),
                lambda row: len(tr.active(row[4], row[3])) < row[3]),
    "wilson": (tw.ROUTES, lambda row: gi.wilson_case(row, data=False)[0], gi.wilson_served, lambda row: (row[8][0], row[1]),
               lambda row: len(tw.active(row[4], row[3])) < row[3]),
    "transfer": (gi.TRANSFER_ROWS, lambda row: gi.transfer_case(row, data=False), gi.transfer_served, lambda row: (row[6][0][0], row[1]),
                 lambda row: len(tx.active(row[5], row[4])) < row[4]),
}


@pytest.mark.parametrize("table", sorted(TABLES))
def test_every_served_row_is_poisoned_in_every_operand(table):
    rows, case, served, family, hole = TABLES[table]
    totals, n_served = {}, 0
    for row in rows:
        ops = case(row)
        for name, op in ops.items():
            if served(row):
                assert op.poisoned_bytes() > 0, (row[:7], name)
            totals[name] = totals.get(name, 0) + op.poisoned_bytes()
        n_served += bool(served(row))
    # (the figures DESIGN 10.12 quotes: run with -s)
    print("%s: %d rows, %d served; poisoned bytes per operand class, guard bands not counted: %s" % (table, len(rows), n_served, totals))
    assert n_served > 0


@pytest.mark.parametrize("table", sorted(TABLES))
def test_every_kernel_family_and_storage_meets_a_mask_with_a_hole(table):
    rows, case, served, family, hole = TABLES[table]
    named = {family(row) for row in rows if served(row)}
    holed = {family(row) for row in rows if served(row) and hole(row)}
    missing = named - holed
    if table == "stencil":
        missing = {m for m in missing if m[0] != qmg.SF_NOTHING}      # nothing is launched
    assert not missing, missing


def test_no_row_is_skipped():
    for fn, rows in ((gi.test_stencil_route_reads_nothing_it_must_not, tr.ROUTES), (gi.test_wilson_route_reads_nothing_it_must_not, tw.ROUTES),
                     (gi.test_transfer_route_reads_nothing_it_must_not, gi.TRANSFER_ROWS)):
        marks = [m for m in fn.pytestmark if m.name == "parametrize"]
        assert len(marks) == 1 and marks[0].args[1] is rows
        assert not [m for m in fn.pytestmark if m.name in ("skip", "skipif", "xfail")]
    assert gi.TRANSFER_ROWS[:len(tx.ROUTES)] == tx.ROUTES      # the whole table, and the rows the module adds to it
