"""Time per call of the single-vector BLAS-1 and reduction entry points of the C ABI, for an A/B between two builds of the library.

    python tools/bench_blas_single.py [--lib other/libqmg_hip.so] [--batch] > run.json

The ten element-wise entry points and the four reductions (norm2sq, dot, diffnorm2sq, multidot of 8; results left on the device, so nothing
waits inside the timed loop) at n = 128*128*24 (a coarse level) and n = 2*4096*4096 (512 MiB per vector, above "blas_nt_mb"), HIP events
around `reps` back-to-back calls.  --batch adds qmg_batch_blas_t on 8 systems of n = 2*2048*2048 for COPY, CAXPY and CAXPBYZ.
--lib loads another build of the library (the parent commit's, say) in place of the tree's own; run the two alternately, a few times each,
and compare a route's mean against the other build's min-to-max spread (profiles/blas_one_engine.txt).
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
qmg = importlib.import_module("quantum-mg_amd")

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None)
ap.add_argument("--batch", action="store_true")
args = ap.parse_args()
if args.lib:
    qmg.SO_PATH = os.path.abspath(args.lib)
qmg.init(0)
L = qmg.lib()


def timeit(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    qmg.sync()
    t = qmg.Timer()
    t.start()
    for _ in range(reps):
        fn()
    return 1e3 * t.stop_ms() / reps     # microseconds per call


def gauss(n, seed):
    d = qmg.DeviceArray(n)
    qmg.gaussian(d, n, seed)
    return d


rows = {}
for n, reps in ((128 * 128 * 24, 200), (2 * 4096 * 4096, 20)):
    x, y, z = gauss(n, 1), gauss(n, 2), gauss(n, 3)
    vs = [gauss(n, 10 + j) for j in range(8)]
    res = qmg.DeviceArray.zeros(16)
    pr = C.cast(C.c_void_p(res.ptr), C.POINTER(C.c_double))
    px, py, pz, nn = C.c_void_p(x.ptr), C.c_void_p(y.ptr), C.c_void_p(z.ptr), C.c_size_t(n)
    ptrs = (C.c_void_p * 8)(*[v.ptr for v in vs])
    a, b = 0.3 - 0.1j, 1.0 + 0.0j      # (|a| < 1, b = 1 where z feeds itself: the values stay bounded over the repetitions)
    calls = {
        "zero_vector": lambda: qmg.zero_vector(z, n), "copy_vector": lambda: qmg.copy_vector(z, x, n), "cax": lambda: qmg.cax(a, z, n),
        "caxy": lambda: qmg.caxy(a, x, z, n), "caxpy": lambda: qmg.caxpy(1e-3 * a, x, z, n), "cxpy": lambda: qmg.cxpy(x, z, n),
        "cxpay": lambda: qmg.cxpay(x, a, z, n), "caxpby": lambda: qmg.caxpby(a, x, a, z, n), "cxpyz": lambda: qmg.cxpyz(x, y, z, n),
        "caxpbyz": lambda: qmg.caxpbyz(a, x, b, y, z, n), "caxpbyz (z = y)": lambda: qmg.caxpbyz(1e-3 * a, x, b, z, z, n),
        "norm2sq": lambda: L.qmg_norm2sq(px, nn, pr, None, None), "dot": lambda: L.qmg_dot(px, py, nn, pr, None, None),
        "diffnorm2sq": lambda: L.qmg_diffnorm2sq(px, py, nn, pr, None, None), "multidot 8": lambda: L.qmg_multidot(ptrs, 8, py, nn, pr, None, None),
    }
    for name, fn in calls.items():
        rows["%s n=%d" % (name, n)] = timeit(fn, reps)
    for v in [x, y, z, res] + vs:
        v.free()

if args.batch:
    n, k = 2 * 2048 * 2048, 8
    x, y, z = gauss(k * n, 4), gauss(k * n, 5), gauss(k * n, 6)
    for name, op, kw in (("COPY", qmg.BOP_COPY, dict(x=x)), ("CAXPY", qmg.BOP_CAXPY, dict(a=1e-3, x=x)), ("CAXPBYZ", qmg.BOP_CAXPBYZ, dict(a=0.3, b=1.0, x=x, y=y))):
        rows["batch %s 8 x n=%d" % (name, n)] = timeit(lambda: qmg.batch_blas_t(qmg.C64, op, z, n, k, n, 0xFF, **kw), 20)

print(json.dumps({"lib": qmg.SO_PATH, "us_per_call": rows}))
