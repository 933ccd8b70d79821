"""The ten single-vector element-wise entry points hold their documented operation order bit for bit.

The order, with z the vector an entry point writes and a, b its scalars:
  cmul(a, b) = (fma(a.x, b.x, -(a.y b.y)), fma(a.x, b.y, a.y b.x))
  cmac(r, a, b): r.x = fma(a.x, b.x, r.x); r.x = fma(-a.y, b.y, r.x); r.y = fma(a.x, b.y, r.y); r.y = fma(a.y, b.x, r.y)
  zero 0 | copy x | cax cmul(a, z) | caxy cmul(a, x) | caxpy r = z, cmac(r, a, x) | cxpy z + x | cxpay r = x, cmac(r, a, z)
  caxpby r = cmul(b, z), cmac(r, a, x) | cxpyz x + y | caxpbyz r = cmul(a, x), cmac(r, b, y)
The numpy side below is written from that table in float64, real and imaginary parts apart.  The inputs are reduce_order_numpy's: 25-bit
mantissas, exponents within +-30, so every product of two inputs is exact in a double and fma(p, q, c) is numpy's c + p * q -- one rounding
of the same exact sum, signed zeros included (a few elements are +0.0 and -0.0).  A swapped pointer or coefficient in an entry point
changes nearly every output.

Sizes: n in {1, 255, 256, 257, 1000} (below, at and above a block), and n = 100001 with "blas_nt_mb" at 1 (non-temporal reads) and at 0
(never).  Every in-place form: caxpbyz and cxpyz with z aliasing x and z aliasing y.  Each vector is followed by three guard elements that
must come back as they were, and every read-only operand must come back byte for byte.
"""
import importlib

import numpy as np
import pytest

import reduce_order_numpy as ro

qmg = importlib.import_module("quantum-mg_amd")

pytestmark = pytest.mark.gpu

GUARD = 3
NT_DEFAULT = 256      # blas_nt_mb


@pytest.fixture(scope="module", autouse=True)
def _device():
    qmg.build()
    qmg.init(0)
    yield
    qmg.sync()


# ---- the table, in float64 on (re, im) pairs
def cmul(a, b):
    return a[0] * b[0] + (-(a[1] * b[1])), a[0] * b[1] + a[1] * b[0]


def cmac(r, a, b):
    rx = r[0] + a[0] * b[0]
    rx = rx + (-a[1]) * b[1]
    ry = r[1] + a[0] * b[1]
    ry = ry + a[1] * b[0]
    return rx, ry


def cadd(a, b):
    return a[0] + b[0], a[1] + b[1]


TABLE = {
    "zero": lambda a, b, x, y, z: (np.zeros_like(z[0]), np.zeros_like(z[1])),
    "copy": lambda a, b, x, y, z: x,
    "cax": lambda a, b, x, y, z: cmul(a, z),
    "caxy": lambda a, b, x, y, z: cmul(a, x),
    "caxpy": lambda a, b, x, y, z: cmac(z, a, x),
    "cxpy": lambda a, b, x, y, z: cadd(z, x),
    "cxpay": lambda a, b, x, y, z: cmac(x, a, z),
    "caxpby": lambda a, b, x, y, z: cmac(cmul(b, z), a, x),
    "cxpyz": lambda a, b, x, y, z: cadd(x, y),
    "caxpbyz": lambda a, b, x, y, z: cmac(cmul(a, x), b, y),
}
# the entry point of each op on device vectors (x, y read, z written)
CALL = {
    "zero": lambda a, b, x, y, z, n: qmg.zero_vector(z, n),
    "copy": lambda a, b, x, y, z, n: qmg.copy_vector(z, x, n),
    "cax": lambda a, b, x, y, z, n: qmg.cax(a, z, n),
    "caxy": lambda a, b, x, y, z, n: qmg.caxy(a, x, z, n),
    "caxpy": lambda a, b, x, y, z, n: qmg.caxpy(a, x, z, n),
    "cxpy": lambda a, b, x, y, z, n: qmg.cxpy(x, z, n),
    "cxpay": lambda a, b, x, y, z, n: qmg.cxpay(x, a, z, n),
    "caxpby": lambda a, b, x, y, z, n: qmg.caxpby(a, x, b, z, n),
    "cxpyz": lambda a, b, x, y, z, n: qmg.cxpyz(x, y, z, n),
    "caxpbyz": lambda a, b, x, y, z, n: qmg.caxpbyz(a, x, b, y, z, n),
}
OPS = tuple(TABLE)
ALIASES = (("caxpbyz", "x"), ("caxpbyz", "y"), ("cxpyz", "x"), ("cxpyz", "y"))     # (op, the operand z aliases)


def parts(v):
    return np.ascontiguousarray(v.real), np.ascontiguousarray(v.imag)


def same_bits(got, want):
    return np.array_equal(np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(want).view(np.uint64))


def inputs(n, seed):
    """x, y, z of n + GUARD elements and the scalars a, b; signed zeros in a few places"""
    rng = np.random.default_rng(seed)
    (x, y, z), _ = ro.cvalues(rng, (3, n + GUARD), 25)
    (a, b), _ = ro.cvalues(rng, (2,), 25)
    for v, at, val in ((x, 0, complex(0.0, -0.0)), (y, n // 2, complex(-0.0, 0.0)), (z, n - 1, complex(-0.0, -0.0)), (x, n // 3, complex(0.0, 0.0)),
                       (z, n // 3, complex(-0.0, 0.0))):
        if n > 4:
            v[at] = val
    return x, y, z, complex(a), complex(b)


def check(op, n, seed, alias=None):
    x, y, z, a, b = inputs(n, seed)
    if alias == "x":
        x = z
    if alias == "y":
        y = z
    host = {"x": x, "y": y, "z": z}
    dev = {k: qmg.DeviceArray.from_host(v) for k, v in host.items() if k != alias}
    if alias:
        dev[alias] = dev["z"]
    CALL[op](a, b, dev["x"], dev["y"], dev["z"], n)
    got = {k: d.to_host() for k, d in dev.items()}
    for d in set(dev.values()):
        d.free()
    wx, wy = TABLE[op](parts(np.complex128(a)), parts(np.complex128(b)), parts(x[:n]), parts(y[:n]), parts(z[:n]))
    gx, gy = parts(got["z"][:n])
    assert same_bits(gx, wx) and same_bits(gy, wy), (op, n, alias, int(np.sum(gx.view(np.uint64) != np.asarray(wx).view(np.uint64))))
    assert got["z"][n:].tobytes() == z[n:].tobytes(), (op, n, "written past n")
    for k in ("x", "y"):
        if k != alias:
            assert got[k].tobytes() == host[k].tobytes(), (op, n, "read-only operand %s was written" % k)


@pytest.mark.parametrize("op", OPS)
def test_single_vector_op_bits(op):
    for n in (1, 255, 256, 257, 1000):
        check(op, n, 31000 + 17 * OPS.index(op) + n)


@pytest.mark.parametrize("op,alias", ALIASES, ids=["%s-z_is_%s" % oa for oa in ALIASES])
def test_single_vector_op_in_place_bits(op, alias):
    for n in (1, 255, 256, 257, 1000):
        check(op, n, 32000 + n, alias)


@pytest.mark.parametrize("nt_mb", (1, 0))
@pytest.mark.parametrize("op", OPS)
def test_single_vector_op_bits_past_and_below_the_non_temporal_threshold(op, nt_mb):
    qmg.set_tuning("blas_nt_mb", nt_mb)
    try:
        check(op, 100001, 33000 + OPS.index(op))
        for o, alias in ALIASES:
            if o == op:
                check(op, 100001, 34000 + OPS.index(op), alias)
    finally:
        qmg.set_tuning("blas_nt_mb", NT_DEFAULT)
