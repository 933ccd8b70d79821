"""CPU-side checks behind tests/test_gpu_singlet.py (no GPU: qmg_singlet_plan is host code, and the entry points refuse before any HIP call).

1. The twin's own identities (singlet_numpy): the dilution supports partition the lattice and sum to the noise; the exact Tr_y[gamma5 D^-1]
   of the dense Wilson operator is real; the diluted estimator is unbiased; `combine` against a direct double loop.
2. qmg_singlet_plan walked through the .so: the blocks cover every row and system once, no block is idle, the row cap is walked, every
   refusal is returned.
3. The symbols are declared, bound and exported, and `make wilson_singlet` builds.
"""
import ctypes as C
import importlib
import itertools
import os
import subprocess

import numpy as np
import pytest

import coordspace as cs
import singlet_numpy as sn

qmg = importlib.import_module("quantum-mg_amd")

LATTICES = [(2, 2), (4, 6), (130, 2), (16, 8)]
ROW_CAP = 65535
IDS = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.fixture(scope="module", autouse=True)
def _built():
    qmg.build()


def dilutions(Ly):
    return [(nt, spin, eo) for nt in sorted({1, 2, Ly}) for spin in (0, 1) for eo in (0, 1)]


@pytest.fixture(scope="module")
def dense8():
    """(Ux, Uy, D, D^-1) of the 8 x 8 end-to-end case of the GPU test: phases 0.5 uniform(-pi, pi), mass 0.2."""
    ph = 0.5 * np.random.default_rng(5).uniform(-np.pi, np.pi, 8 * 8 * 2)
    Ux, Uy = cs.phases_to_links(ph, 8, 8)
    D = sn.wilson_dense(Ux, Uy, 0.2)
    return Ux, Uy, D, np.linalg.inv(D)


# ---- 1. the twin
@pytest.mark.parametrize("dims", [(8, 8), (6, 4)], ids=IDS)
def test_supports_partition_and_sum_to_the_noise(dims):
    Lx, Ly = dims
    for nc, dil in itertools.product((1, 2, 4), dilutions(Ly)):
        n = Lx * Ly * nc
        cm = sn.class_map(Lx, Ly, nc, dil)
        nd = sn.n_classes(nc, dil)
        # every element in exactly one class, every class non-empty and of the same size
        assert cm.min() == 0 and cm.max() == nd - 1, (nc, dil)
        assert np.array_equal(np.bincount(cm, minlength=nd), np.full(nd, n // nd)), (nc, dil)
        eta = sn.noise_z4(77, n)
        assert np.array_equal(np.abs(eta), np.ones(n))
        parts = [sn.diluted(77, Lx, Ly, nc, dil, d) for d in range(nd)]
        assert np.array_equal(sum(parts), eta), (nc, dil)
        assert np.array_equal(sum((p != 0).astype(int) for p in parts), np.ones(n, dtype=int)), (nc, dil)
        for d in range(nd):
            assert sn.support_sizes(Lx, Ly, nc, dil, d).sum() == n // nd
            rows = np.nonzero(sn.support_sizes(Lx, Ly, nc, dil, d))[0]
            assert np.array_equal(rows % dil[0], np.full(rows.size, sn.class_row(d, nc, dil))), (nc, dil, d)


def test_hash_is_the_splitmix64_of_the_reference_vectors():
    """splitmix64's published first outputs from state 0 (the generator adds its increment before mixing, as this hash does)."""
    z, got = 0, []
    for _ in range(3):
        got.append(int(sn.splitmix64(np.array([z], dtype=np.uint64))[0]))
        z = (z + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    assert got == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]


def test_exact_gamma5_trace_is_real(dense8):
    Ux, Uy, D, Dinv = dense8
    tr, tr5 = sn.exact_traces(Dinv, 8, 8, 2)
    print("cond(D) = %.4f   |Im Tr_y g5 D^-1| max %.3e   norm %.6f" % (np.linalg.cond(D), np.abs(tr5.imag).max(), np.linalg.norm(tr5)))
    assert np.abs(tr5.imag).max() <= 1e-12 * np.linalg.norm(tr5)


@pytest.mark.parametrize("dil", [(1, 0, 0), (2, 1, 0), (8, 1, 1)], ids=IDS)
def test_estimator_is_unbiased(dense8, dil):
    """The mean of S(y), P(y) over 64 seeds (1 .. 64) within five standard errors of the dense traces, real and imaginary parts, every row.
    Measured worst deviations in sigmas over S, P and both parts: (1,0,0) 2.05; (2,1,0) 2.51; (8,1,1) 1.88 (real parts) -- at full dilution
    the imaginary parts vanish identically (spread and mean are both rounding, 1e-17), which is why the gate carries the rounding floor
    1e-12 |trace|."""
    Ux, Uy, D, Dinv = dense8
    tr, tr5 = sn.exact_traces(Dinv, 8, 8, 2)
    seeds = range(1, 65)
    ms = [sn.measure(D, s, 8, 8, 2, dil) for s in seeds]
    c = sn.combine(ms, 8, 8, 2, dil)
    for name, X, exact in (("S", c["S"], tr), ("P", c["P"], tr5)):
        floor = 1e-12 * np.linalg.norm(exact)
        for part in (np.real, np.imag):
            mean, se = part(X).mean(axis=0), part(X).std(axis=0, ddof=1) / np.sqrt(len(ms))
            dev = np.abs(mean - part(exact))
            print("%s %s %s worst %.2f sigma" % (dil, name, part.__name__, (dev / np.maximum(se, floor)).max()))
            assert np.all(dev <= 5 * se + floor), (dil, name, part.__name__)
    # and the estimate is an estimate: one noise alone misses the trace by more than rounding unless the dilution is complete
    assert abs(c["condensate"] - tr.real.sum() / 64) <= 5 * c["condensate_err"] + 1e-12


def test_combine_against_a_direct_double_loop():
    rng = np.random.default_rng(8)
    Lx, Ly, nc = 6, 4, 2
    for dil, nn in (((4, 1, 1), 3), ((2, 1, 0), 2), ((4, 0, 0), 1)):
        nd = sn.n_classes(nc, dil)
        noises = [{"S": rng.standard_normal((nd, Ly)) + 1j * rng.standard_normal((nd, Ly)),
                   "P": rng.standard_normal((nd, Ly)) + 1j * rng.standard_normal((nd, Ly)), "N": rng.random((nd, Ly))} for _ in range(nn)]
        c = sn.combine(noises, Lx, Ly, nc, dil, n_f=2)
        P = [[sum(m["P"][d][y] for d in range(nd)) for y in range(Ly)] for m in noises]
        S = [[sum(m["S"][d][y] for d in range(nd)) for y in range(Ly)] for m in noises]
        for a in range(nn):
            assert abs(c["q5"][a] - sum(P[a][y].real for y in range(Ly))) < 1e-13
            assert abs(c["condensate_per_noise"][a] - sum(S[a][y].real for y in range(Ly)) / (Lx * Ly)) < 1e-13
        if nn >= 2:
            for t in range(Ly):
                want = sum(P[a][y0].real * P[b][(y0 + t) % Ly].real for a in range(nn) for b in range(nn) if a != b for y0 in range(Ly)) / (nn * (nn - 1) * Ly)
                assert abs(c["Ddisc"][t] - want) < 1e-13
        else:
            assert "Ddisc" not in c and "Ceta" not in c
        if dil[0] == Ly:
            for t in range(Ly):
                want = sum(m["N"][d][(sn.class_row(d, nc, dil) + t) % Ly] for m in noises for d in range(nd)) / (nn * Ly)
                assert abs(c["Cpi"][t] - want) < 1e-13
                if nn >= 2:
                    assert abs(c["Ceta"][t] - (c["Cpi"][t] - 2 * c["Ddisc"][t])) < 1e-15
        else:
            assert "Cpi" not in c


# ---- 2. qmg_singlet_plan
def walk_plan(dims, nc, dil, first, nrhs, mask):
    Lx, Ly = dims
    rc, (fam, block, gx, gy, walk, lds, doubles, dgx, dgy, dwalk, nk, classes) = qmg.singlet_plan_status(dims, nc, dil, first, nrhs, mask)
    tag = (dims, nc, dil, first, nrhs, mask)
    active = [k for k in range(nrhs) if (mask >> k) & 1]
    assert rc == 0 and fam == qmg.SGF_ROWS and block == 256, tag
    assert classes == sn.n_classes(nc, dil), tag
    # the loops grid: one block column per active system, the rows once each, every block with a row, `walk` the most any block takes
    assert gx == dgy == nk == len(active), tag
    assert gy == min(Ly, ROW_CAP), tag
    seen = np.zeros(Ly, dtype=int)
    per_block = np.zeros(gy, dtype=int)
    for b in range(gy) if Ly <= 4096 else ():
        for y in range(b, Ly, gy):
            seen[y] += 1
            per_block[b] += 1
    if Ly > 4096:   # the same walk, vectorised
        y = np.arange(Ly)
        seen[:] = 1
        per_block = np.bincount(y % gy, minlength=gy)
    assert np.all(seen == 1) and per_block.min() >= 1 and per_block.max() == walk, tag
    assert doubles == 5 * Ly * len(active) and lds == 8 * (8 * 4 + 8), tag
    # the dilution grid: the lanes reach every element, no block is idle, and dwalk is the most a lane takes
    n = Lx * Ly * nc
    assert dgx <= 262144 and (dgx - 1) * block < n <= dgx * block * dwalk and n > dgx * block * (dwalk - 1), tag


def test_plan_covers_rows_and_systems_once():
    for dims, nc in itertools.product(LATTICES, (1, 2, 4)):
        for dil in dilutions(dims[1]):
            nd = sn.n_classes(nc, dil)
            for nrhs in (1, 3, 16):
                if nrhs > nd:
                    assert qmg.singlet_plan_status(dims, nc, dil, 0, nrhs)[0] == 1, (dims, nc, dil, nrhs)
                    continue
                for first in sorted({0, nd - nrhs}):
                    walk_plan(dims, nc, dil, first, nrhs, (1 << nrhs) - 1)
                if nrhs == 16:
                    walk_plan(dims, nc, dil, 0, nrhs, 0x8421)   # a sparse mask
    # bits of the mask above nrhs are not systems
    assert qmg.singlet_plan((16, 8), 2, (8, 1, 1), 0, 3, 0xFFFF)[10] == 3


def test_plan_walks_rows_beyond_the_grid_cap():
    # the smallest lattices whose rows exceed one grid dimension: one row more than the cap is odd, so Ly = 65536
    assert qmg.singlet_plan((2, ROW_CAP - 1), 1, (1, 0, 0))[3:5] == (ROW_CAP - 1, 1)
    for Ly in (65536, 65538, 2 * ROW_CAP, 2 * ROW_CAP + 2):
        walk_plan((2, Ly), 1, (1, 0, 0), 0, 1, 1)
        walk_plan((2, Ly), 2, (2, 1, 1), 3, 5, 0b10101)
    assert qmg.singlet_plan((2, 65536), 1, (1, 0, 0))[3:5] == (ROW_CAP, 2)
    assert qmg.singlet_plan((2, 2 * ROW_CAP + 2), 1, (1, 0, 0))[3:5] == (ROW_CAP, 3)
    # the tiny rows of Lx = 2 change nothing: a block of 256 lanes per (row, system)
    assert qmg.singlet_plan((2, 2), 1, (1, 0, 0))[:5] == (qmg.SGF_ROWS, 256, 1, 2, 1)
    # a vector beyond 2^18 blocks of elements: the dilution lanes walk
    assert qmg.singlet_plan((8192, 8192), 2, (1, 0, 0))[7:10] == (262144, 1, 2)


def test_plan_refusals_and_buffer_contract():
    ok, invalid = 0, 1
    good = dict(dims=(16, 8), nc=2, dil=(4, 1, 1), first_class=0, nrhs=16)
    assert qmg.singlet_plan_status(**good)[0] == ok
    bad = [dict(dims=(3, 4)), dict(dims=(4, 5)), dict(dims=(0, 2)), dict(dims=(2, 0)),       # an invalid lattice
           dict(nc=0), dict(nc=-1),
           dict(dil=(3, 1, 1)), dict(dil=(0, 1, 1)), dict(dil=(-1, 0, 0)), dict(dil=(16, 0, 0)),   # nt does not divide Ly
           dict(dil=(4, 2, 1)), dict(dil=(4, 1, -1)),
           dict(first_class=1), dict(first_class=-1), dict(dil=(1, 1, 1), nrhs=5),               # first_class + nrhs > D
           dict(nrhs=0), dict(nrhs=17), dict(nrhs=-1)]
    for change in bad:
        rc, plan = qmg.singlet_plan_status(**dict(good, **change))
        assert rc == invalid and plan[0] == qmg.SGF_INVALID, change
    # no active system: success with nothing launched
    rc, plan = qmg.singlet_plan_status(mask=0, **good)
    assert rc == ok and plan[0] == qmg.SGF_NONE and plan[2:5] == (0, 0, 0)
    lib = qmg.lib()
    out = (C.c_int * 16)(*([7] * 16))
    assert lib.qmg_singlet_plan(16, 8, 2, 4, 1, 1, 0, 16, C.c_uint(0xFFFF), out, 16) == ok
    assert list(out[12:]) == [-1] * 4 and list(out[:12]) == [1, 256, 16, 8, 1, 320, 640, 1, 16, 1, 16, 16]
    assert lib.qmg_singlet_plan(16, 8, 2, 4, 1, 1, 0, 16, C.c_uint(0xFFFF), out, 11) == invalid
    assert lib.qmg_singlet_plan(16, 8, 2, 4, 1, 1, 0, 16, C.c_uint(0xFFFF), None, 12) == invalid


def test_entries_refuse_before_any_launch():
    """Every refusal of the issue through the entry points themselves; none of these calls reaches HIP (there is no device here), so the
    vector pointer is never used: it only has to be non-null and aligned."""
    ok, invalid = 0, 1
    lib = qmg.lib()
    vec, host = C.c_void_p(0x10000), (C.c_double * (16 * 8 * 5))()

    def loops(dtype=qmg.C64, psi=vec, Lx=16, Ly=8, nc=2, nt=4, spin=1, eo=1, first=0, g5=0, nrhs=16, stride=256, mask=0xFFFF, dev=None, hst=host):
        return lib.qmg_loops_timeslice_batch(dtype, psi, Lx, Ly, nc, nt, spin, eo, first, C.c_ulonglong(1), g5, nrhs, C.c_size_t(stride), C.c_uint(mask), dev, hst, None)

    def dilute(dtype=qmg.C64, out=vec, Lx=16, Ly=8, nc=2, nt=4, spin=1, eo=1, first=0, nrhs=16, stride=256, mask=0xFFFF):
        return lib.qmg_noise_dilute_batch(dtype, out, Lx, Ly, nc, nt, spin, eo, first, C.c_ulonglong(1), nrhs, C.c_size_t(stride), C.c_uint(mask), None)

    for fn in (loops, dilute):
        for change in (dict(Lx=3), dict(Ly=5), dict(Ly=0), dict(nt=3), dict(nt=0), dict(first=1), dict(nrhs=0), dict(nrhs=17), dict(dtype=2), dict(dtype=-1),
                       dict(stride=255), dict(spin=2), dict(eo=2), dict(nc=0)):
            assert fn(**change) == invalid, (fn.__name__, change)
        assert fn(mask=0) == ok                                  # nothing active, nothing launched
    assert dilute(out=None) == invalid and dilute(out=C.c_void_p(0x10008)) == invalid
    assert loops(psi=None) == invalid and loops(psi=C.c_void_p(0x10008)) == invalid
    assert loops(hst=None) == invalid                            # both outputs NULL
    assert loops(nc=3, stride=16 * 8 * 3, nrhs=8, nt=1, eo=0) == invalid   # odd nc under the Wilson gamma5 (D = 3 < 8 too)
    assert loops(nc=3, stride=16 * 8 * 3, nrhs=3, nt=1, eo=0, g5=0) == invalid
    assert loops(nc=3, stride=16 * 8 * 3, nrhs=3, nt=1, eo=0, g5=1, mask=0) == ok   # the staggered sign takes any nc
    assert loops(g5=2) == invalid and loops(g5=-1) == invalid
    assert lib.qmg_noise_z4(None, C.c_size_t(4), C.c_ulonglong(1), None) == invalid
    assert lib.qmg_noise_z4(None, C.c_size_t(0), C.c_ulonglong(1), None) == ok


# ---- 3. the symbols and the driver
def test_symbols_are_declared_bound_and_exported():
    names = ["qmg_noise_z4", "qmg_noise_dilute_batch", "qmg_loops_timeslice_batch", "qmg_singlet_plan"]
    header = open(os.path.join(qmg.ROOT, "include", "qmg_hip.h")).read()
    for name in names:
        assert name in qmg.ABI_SYMBOLS and ("int %s(" % name) in header
        assert hasattr(qmg.lib(), name)


def test_the_driver_builds():
    drivers = os.path.join(qmg.HERE, "drivers")
    subprocess.check_call(["make", "-C", drivers, "wilson_singlet"], stdout=subprocess.DEVNULL)
    assert os.access(os.path.join(drivers, "wilson_singlet"), os.X_OK)
    assert "wilson_singlet" in open(os.path.join(drivers, "Makefile")).read().split("PROGS =")[1].split("\n")[0].split()
