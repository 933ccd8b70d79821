"""What a call must not read, poisoned: every served row of the three route tables, the masked batches of the domain-wall
entries and the batched dwf_meas entries run twice -- on the clean operands of their own test files and on copies in which every byte the
call may not read (tests/isolation.py: frozen systems, stride padding, a misaligned operand's leading element, the rhs parity no piece takes
as a source, the lhs halves a ZERO piece clears or no piece touches, scratch, and 4096-byte guard bands around every operand) is 0xFF, a NaN in
every storage.  Then

  * every element the call writes has the same bytes in both runs;
  * every other byte of every operand of the poisoned run, read-only operands and guard bands included, is what was uploaded;
  * fused norms and MR dots of the active systems have the same bits, and the MR slots of the other systems are as the caller left them;
  * a row whose plan refuses leaves every operand untouched.

No tolerance: the clean run is what test_gpu_stencil_routes.py, test_gpu_wilson_routes.py, test_gpu_transfer_routes.py, test_gpu_dwf.py,
test_gpu_dwf_eo.py and test_gpu_dwf_meas.py hold to the long-double references.  The route modules are imported as modules and nothing in
them is edited; the rows, plans, calls, operators and seeds are theirs.  The builders below (`*_case`) are host-only, so that
tests/test_host_isolation.py can assert the coverage of the tables without a device.
"""
import importlib

import numpy as np
import pytest

import coordspace as cs
import isolation as iso
import test_gpu_dwf as tdw
import test_gpu_dwf_eo as tde
import test_gpu_stencil_routes as tr
import test_gpu_transfer_routes as tx
import test_gpu_wilson_routes as tw

qmg = importlib.import_module("quantum-mg_amd")

pytestmark = pytest.mark.gpu

DWF_CASES = [((2, 2), 3), ((4, 6), 6), ((130, 2), 12), ((16, 8), 32)]
P = qmg
DWF_CALLS = [("direct", P.P_ALL, 0, 0), ("direct", P.P_HOPPING | P.P_ZERO, 0, 0), ("direct", P.P_EO | P.P_ZERO_E, 0, 0), ("direct", P.P_OE, 0, 0),
             ("inv5", P.P_CLOVER, 0, 0), ("inv5", P.P_CLOVER_O, 0, 0),
             ("hops", P.P_HOPPING, 0, 1), ("hops", P.P_OE | P.P_ZERO_O, 0, 1), ("hops", P.P_EO, 0, 0),
             ("schur", 0, 0, 0), ("schur", 0, 1, 3)]      # (entry, pieces, parity, Gamma5 flags)
MEAS_CALLS = [("wall_source", 0), ("wall_project", 0), ("wall_project", 1), ("slice_norms", 0)]
MEAS_BATCH = (3, 4, 6)     # test_gpu_dwf_meas.BATCHES[1]: (nsys, extra elements between 5-d systems, between 4-d systems)


class At:
    """a device address where the route modules expect a DeviceArray or an integer"""

    def __init__(self, ptr):
        self.ptr = int(ptr)

    def __int__(self):
        return self.ptr


@pytest.fixture(scope="module", autouse=True)
def _device():
    qmg.build()
    qmg.init(0)
    tr.set_knobs({})
    yield
    tr.set_knobs({})
    qmg.set_tuning("wilson_pair", 2)
    qmg.sync()


def on_device(images, launch):
    """upload the banded images, run launch({name: At}), download them: isolation.check_isolation's `execute`"""
    dev = {name: qmg.DeviceArray.from_host(im) for name, (im, _) in images.items()}
    at = {name: At(dev[name].ptr + off) for name, (_, off) in images.items()}
    scalars = launch(at)
    after = {name: d.to_host() for name, d in dev.items()}
    for d in dev.values():
        d.free()
    return after, scalars


def gaussian(n, seed, vdtype, data):
    if not data:
        return np.zeros(n, dtype=vdtype)
    return np.ascontiguousarray(cs.gaussian_cvec(n, seed), dtype=vdtype)


# ---------------------------------------------------------------- the stored-stencil table
def stencil_case(row, data=True):
    """{name: isolation.Operand} of a row of test_gpu_stencil_routes.ROUTES, with check_route's strides and seeds"""
    entry, storage, dims, nrhs, mask, pieces, flags = row[:7]
    vdtype = tr.STORAGE[storage][1]
    size = dims[0] * dims[1] * dims[2]
    stride = size + tr.PAD
    if entry in ("apply", "norm2"):
        assert mask == (1 << nrhs) - 1, "an entry without a mask serves every system"
    roles = iso.stencil_reads(entry, dims, nrhs, stride, mask, tr.PIECES[pieces], flags, "noclover" not in flags, "nohopping" not in flags)
    clean = {role: gaussian(nrhs * stride, seed, vdtype, data) for role, seed in (("rhs", 3), ("lhs", 4), ("other", 5), ("dotv", 6)) if role in roles}
    inplace = "inplace" in flags
    if inplace:
        clean["lhs"] = clean["rhs"]
    return iso.operands_of(roles, clean, [("lhs", "rhs")] if inplace else [])


def stencil_served(row):
    return row[8][0][0] not in (qmg.SF_UNSUPPORTED, qmg.SF_INVALID)


def run_stencil(row):
    entry, storage, dims, nrhs, mask, pieces, flags, knobs, plans = row
    assert [tr.instantiation(p) for p in tr.planned(row)] == plans
    mdtype, vdtype = tr.STORAGE[storage][:2]
    Lx, Ly, nc = dims
    stride = Lx * Ly * nc + tr.PAD
    clover, hopping = tr.operator(dims, mdtype)
    dcl = None if "noclover" in flags else tr.to_device(clover, mdtype)
    dhop = None if "nohopping" in flags else tr.to_device(hopping, mdtype)
    shifts = tr.SHIFTS if nc % 2 == 0 else tr.SHIFTS[:2] + (0.0,)
    desc = qmg.make_desc(Lx, Ly, nc, dcl, dhop, *shifts)
    act = tr.active(mask, nrhs)
    served = stencil_served(row)

    def launch(at):
        extra = {}
        if entry == "epi":
            extra.update(other_scale=0.75, acc_scale=-1.25)
            for role in ("other", "dotv"):
                if role in at:
                    extra[role] = at[role]
        slots = qmg.batch_mr_read_dots(nrhs) if "dotv" in extra else None
        try:
            tr.call(row, desc, at["lhs"], at.get("rhs", at["lhs"]), stride, extra)
        except qmg.QmgError:
            assert not served, "a served row was refused"
            return b""
        assert served, "a refused row was served"
        if slots is not None:      # the MR slots of the other systems: as the caller left them
            frozen = [k for k in range(nrhs) if k != act[0]]
            assert qmg.batch_mr_read_dots(nrhs)[frozen].tobytes() == slots[frozen].tobytes()
        if "norms" in extra:
            return np.asarray(extra["norms"])[act].tobytes()
        return np.asarray(extra["dots"]).tobytes() if "dots" in extra else b""

    return iso.check_isolation(stencil_case(row), lambda images: on_device(images, launch), served)


@pytest.mark.parametrize("row", tr.ROUTES, ids=tr.route_id)
def test_stencil_route_reads_nothing_it_must_not(row):
    try:
        tr.set_knobs(row[7])
        run_stencil(row)
    finally:
        tr.set_knobs({})


# ---------------------------------------------------------------- the Wilson table
def wilson_case(row, data=True):
    """({name: Operand}, {role: the role whose buffer it shares}, the roles the call passes) of a row of test_gpu_wilson_routes.ROUTES"""
    entry, storage, dims, nrhs, mask, pieces, flags = row[:7]
    fl = flags.split()
    vdtype = np.complex64 if storage == "c32" else np.complex128
    Lx, Ly = dims
    size = 2 * Lx * Ly
    stride, hstride = size + tw.PAD, 2 * Lx + tw.PAD
    roles = iso.wilson_reads(entry, dims, nrhs, stride, hstride, mask, tw.PIECES[pieces], flags)
    clean = {role: gaussian(nrhs * stride, seed, vdtype, data) for role, seed in (("rhs", 103), ("lhs", 104), ("other", 105), ("dotv", 106)) if role in roles}
    for role, seed in (("lo", 107), ("hi", 108)):
        if role in roles:
            clean[role] = gaussian(nrhs * hstride, seed, vdtype, data)
    alias, pairs = {}, []

    def join(a, b):
        """role b is the buffer of role a"""
        while a in alias:
            a = alias[a]
        clean[b], alias[b] = clean[a], a
        pairs.append((a, b))

    if "inplace" in fl:
        join("rhs", "lhs")
    if "aliaslhs" in fl:
        join("lhs", "other")
    if "dotsother" in fl:
        join("other", "dotv")
    if "dotsrhs" in fl:
        join("rhs", "dotv")
    return iso.operands_of(roles, clean, pairs), alias, set(roles)


def wilson_served(row):
    return row[8][0] in tw.SERVED


def run_wilson(row):
    entry, storage, dims, nrhs, mask, pieces, flags, pair, plan = row
    got_plan = tw.planned(row)
    assert tw.instantiation(got_plan) == plan
    f32 = storage == "c32"
    dtype, vdtype = (qmg.C32, np.complex64) if f32 else (qmg.C64, np.complex128)
    Lx, Ly = dims
    rows = tw.slab_of(flags)
    gLy, y0 = (Ly, 0) if rows is None else (2 * Ly, Ly)
    stride, hstride = 2 * Lx * Ly + tw.PAD, 2 * Lx + tw.PAD
    dg = qmg.DeviceArray.from_host(np.ascontiguousarray(tw.operator(Lx, gLy, f32)[0], dtype=vdtype))
    desc = qmg.make_desc(Lx, Ly, 2, None, None, *tw.SHIFTS)
    served = wilson_served(row)
    operands, alias, roles = wilson_case(row)
    act = tw.active(mask, nrhs)

    def launch(at):
        def find(role):
            if role not in roles:
                return None
            while role in alias:
                role = alias[role]
            return at[role]

        epi = qmg.make_epilogue(find("other"), tw.OTHER_SCALE, tw.ACC_SCALE, find("dotv")) if entry.endswith("_epi") else None
        slots = qmg.batch_mr_read_dots(nrhs)
        status = tw.call(row, dtype, desc, dg, gLy, y0, find("lhs"), find("rhs"), find("lo"), find("hi"), stride, hstride, epi)
        after = qmg.batch_mr_read_dots(nrhs)
        if not served:
            assert status == tw.STATUS[plan[0]] and after.tobytes() == slots.tobytes()
            return b""
        assert status == 0
        if got_plan[5] & qmg.WPF_DOTS:     # the MR slots of the other systems: as the caller left them
            frozen = [k for k in range(nrhs) if k != act[0]]
            assert after[frozen].tobytes() == slots[frozen].tobytes()
            return after[act[0]].tobytes()
        assert after.tobytes() == slots.tobytes()
        return b""

    return iso.check_isolation(operands, lambda images: on_device(images, launch), served)


@pytest.mark.parametrize("row", tw.ROUTES, ids=tw.route_id)
def test_wilson_route_reads_nothing_it_must_not(row):
    try:
        qmg.set_tuning("wilson_pair", row[7])
        run_wilson(row)
    finally:
        qmg.set_tuning("wilson_pair", 2)


# ---------------------------------------------------------------- the transfer table
def transfer_case(row, data=True):
    op, storage, fd, cd, nrhs, mask = row[:6]
    mis = len(row) > 7
    vdt = np.complex64 if storage == "c32" else np.complex128
    fsize, csize = fd[0] * fd[1] * fd[2], cd[0] * cd[1] * cd[2]
    fstride, cstride = fsize + tx.FPAD, csize + tx.CPAD
    roles = iso.transfer_reads(op, fsize, csize, nrhs, fstride, cstride, mask)
    clean = {"fine": gaussian(nrhs * fstride, 2, vdt, data), "coarse": gaussian(nrhs * cstride, 3, vdt, data)}
    return iso.operands_of(roles, clean, leads={"fine": 1 if mis and storage == "c32" else 0})


def transfer_served(row):
    return row[6] != [tx.REFUSED]


def run_transfer(row):
    op, storage, fd, cd, nrhs, mask, plans = row[:7]
    mis = len(row) > 7
    assert tx.planned(row) == plans
    nvec = cd[2]
    fsize, csize = fd[0] * fd[1] * fd[2], cd[0] * cd[1] * cd[2]
    nv = cs.gaussian_cvec(nvec * fsize, 1)
    dn = tx.Dev(nv, np.complex128 if storage == "c64" else np.complex64, 1 if mis and storage == "nv32" else 0)
    served = transfer_served(row)

    def launch(at):
        try:
            tx.call(row, dn, at["fine"], at["coarse"], fsize + tx.FPAD, csize + tx.CPAD)
        except qmg.QmgError:
            assert not served, "a served row was refused"
            return b""
        assert served, "a refused row was served"
        return b""

    return iso.check_isolation(transfer_case(row), lambda images: on_device(images, launch), served)


# The transfer table runs the one-system complex<double> restrict with one system only, so nothing is frozen beside it.  The plan takes the
# one-system kernels whenever ONE system is active, whatever nrhs: the table's (8, 8, 2) -> (2, 2, 8) shape again with a frozen neighbour, as its
# complex<float> rows have it (run_transfer asserts the plan) -- and the prolong likewise.
TRANSFER_ROWS = tx.ROUTES + [
    (tx.R, "c64", (8, 8, 2), (2, 2, 8), 2, 0b10, [tx.ONE_R(1)]),
    (tx.P, "c64", (8, 8, 2), (2, 2, 8), 2, 0b10, [tx.ONE_P(1)]),
]


@pytest.mark.parametrize("row", TRANSFER_ROWS, ids=tx.route_id)
def test_transfer_route_reads_nothing_it_must_not(row):
    run_transfer(row)


# ---------------------------------------------------------------- the masked batches of the domain-wall entries
def dwf_case(dims, Ls, f32, call, data=True):
    entry, pieces, parity, flags = call
    n = dims[0] * dims[1] * 2 * Ls
    nrhs, mask, stride = 3, 0b101, n + 4
    npt = np.complex64 if f32 else np.complex128
    roles = iso.dwf_reads(entry, n, nrhs, stride, mask, pieces, parity)
    vec = lambda seed: tde.cvec(nrhs * stride, seed).astype(npt) if data else np.zeros(nrhs * stride, dtype=npt)
    clean = {role: vec(seed) for role, seed in (("rhs", 3), ("lhs", 4), ("tmp", 5)) if role in roles}
    return iso.operands_of(roles, clean)


@pytest.mark.parametrize("f32", [False, True], ids=["c64", "c32"])
@pytest.mark.parametrize("call", DWF_CALLS, ids=lambda c: "%s-%x-p%d-g%d" % c)
@pytest.mark.parametrize("dims,Ls", DWF_CASES, ids=tde.IDS)
def test_dwf_batch_reads_nothing_it_must_not(dims, Ls, call, f32):
    entry, pieces, parity, flags = call
    n = dims[0] * dims[1] * 2 * Ls
    nrhs, mask, stride = 3, 0b101, n + 4
    dt, npt = tde.types(f32)
    dg = qmg.DeviceArray.from_host(tde.rounded(tde.gauge(*dims), f32).astype(npt))

    def launch(at):
        if entry == "direct":
            qmg.dwf_apply_direct(dt, qmg.make_desc(dims[0], dims[1], 2 * Ls, None, None, *tdw.SHIFTS), dg, Ls, tdw.M, at["lhs"], at["rhs"], pieces, tdw.W, nrhs, stride, mask)
        elif entry == "inv5":
            qmg.dwf_inv5(dt, tde.desc(dims, Ls), Ls, tde.M, at["lhs"], at["rhs"], pieces, tde.ALPHA, tde.W, nrhs, stride, mask)
        elif entry == "hops":
            qmg.dwf_hops_inv5(dt, tde.desc(dims, Ls), dg, Ls, tde.M, at["lhs"], at["rhs"], pieces, tde.ALPHA, flags, tde.W, nrhs, stride, mask)
        else:
            qmg.dwf_schur_apply(dt, tde.desc(dims, Ls), dg, Ls, tde.M, at["lhs"], at["rhs"], at["tmp"], parity, flags, tde.W, nrhs, stride, mask)
        return b""

    iso.check_isolation(dwf_case(dims, Ls, f32, call), lambda images: on_device(images, launch))


# ---------------------------------------------------------------- the batched dwf_meas entries
def meas_case(dims, Ls, f32, call, data=True):
    entry, which = call
    nsys, e5, e4 = MEAS_BATCH
    n5, n4 = dims[0] * dims[1] * 2 * Ls, dims[0] * dims[1] * 2
    npt = np.complex64 if f32 else np.complex128
    roles = iso.meas_reads(entry, n5, n4, nsys, n5 + e5, n4 + e4)
    sizes = {"psi5": nsys * (n5 + e5), "eta4": nsys * (n4 + e4), "q4": nsys * (n4 + e4)}
    clean = {role: (tde.cvec(sizes[role], seed).astype(npt) if data else np.zeros(sizes[role], dtype=npt)) for role, seed in (("psi5", 1), ("eta4", 2), ("q4", 3)) if role in roles}
    return iso.operands_of(roles, clean)


@pytest.mark.parametrize("f32", [False, True], ids=["c64", "c32"])
@pytest.mark.parametrize("call", MEAS_CALLS, ids=lambda c: "%s-%d" % c)
@pytest.mark.parametrize("dims,Ls", DWF_CASES, ids=tde.IDS)
def test_dwf_meas_batch_reads_no_gap(dims, Ls, call, f32):
    entry, which = call
    nsys, e5, e4 = MEAS_BATCH
    s5, s4 = dims[0] * dims[1] * 2 * Ls + e5, dims[0] * dims[1] * 2 + e4
    dt = qmg.C32 if f32 else qmg.C64
    served = not (entry == "wall_project" and which == 1 and Ls % 2)     # no midpoint between the walls at odd Ls

    def launch(at):
        if entry == "wall_source":
            qmg.dwf_wall_source(dt, dims, Ls, at["psi5"], at["eta4"], nsys, s5, s4)
        elif entry == "wall_project":
            assert qmg.dwf_wall_project_status(dt, dims, Ls, at["q4"], at["psi5"], which, nsys, s4, s5) == (0 if served else 3)
        else:
            return qmg.dwf_slice_norms(dt, dims, Ls, at["psi5"], nsys, s5).tobytes()
        return b""

    iso.check_isolation(meas_case(dims, Ls, f32, call), lambda images: on_device(images, launch), served)
