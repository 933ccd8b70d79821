"""Kernel C at nc = 24 with 8 systems (MODE 1, the packed last row tile) and the batched multi-dot at the K-cycle's coarsest shape, timed
with HIP events for an A/B of two builds in one GPU visit (profiles/kernelc_pack_multidot.txt).

    python tools/pack_multidot_bench.py [--package-root DIR] [--reps 5] [--launches 200] [--tag new]

--package-root: the directory that holds the quantum-mg_amd package to measure (default: this checkout); a second checkout with its own
libqmg_hip.so is measured by pointing at it.  Run the two builds alternately, several processes each, and compare the RANGES: a kernel counts
as faster only if its slowest new repetition beats the fastest old one.  One line per repetition:
    <tag> <kernel> rep <i> <us per launch>
Kernel C: nc = 24 on 512^2 and 128^2 and the one-site nc = 8 form on 1022 x 1024; complex<float> matrices with fp64 vectors (mat32), all complex<float> (fp32), and all fp64 (fp64).
Multi-dot: qmg_batch_multidot_t with 8, 4 and 2 vector sets on 8 systems of 393216 elements (128^2 sites of nc = 24: the coarsest level of the
2048^2 three-level K-cycle), complex<double> and complex<float>; the time is the whole call, the host's pick-up of the results included."""
import argparse
import importlib
import os
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--launches", type=int, default=200)
ap.add_argument("--tag", default="build")
ap.add_argument("--only", default="", help="comma-separated fragments of kernel names to run")
args = ap.parse_args()
sys.path.insert(0, args.package_root)
qmg = importlib.import_module("quantum-mg_amd")
qmg.init(0)
timer = qmg.Timer()


def gauss(n, seed, dtype):
    d = qmg.DeviceArray(n)
    qmg.gaussian(d, n, seed)
    if dtype == qmg.C32:
        f = qmg.DeviceArray(n, np.complex64)
        qmg.convert(f, qmg.C32, d, qmg.C64, n)
        d.free()
        return f
    return d


def measure(name, fn):
    if args.only and not any(frag in name for frag in args.only.split(",")):
        return
    for _ in range(10):
        fn()
    qmg.sync()
    for rep in range(args.reps):
        timer.start()
        for _ in range(args.launches):
            fn()
        print("%s %s rep %d %.3f" % (args.tag, name, rep, 1e3 * timer.stop_ms() / args.launches), flush=True)


K = 8
for Lx, Ly, NC in ((512, 512, 24), (128, 128, 24), (1022, 1024, 8)):   # (an odd half-row: the one-site nc = 8 form, not the two-site one)
    vol = Lx * Ly
    for tag, mdt, vdt in (("mat32", qmg.C32, qmg.C64), ("fp32", qmg.C32, qmg.C32), ("fp64", qmg.C64, qmg.C64)):
        cl, ho = gauss(vol * NC * NC, 1, mdt), gauss(4 * vol * NC * NC, 2, mdt)
        d = qmg.make_desc(Lx, Ly, NC, cl, ho, 0.1)
        x, y = gauss(K * vol * NC, 3, vdt), gauss(K * vol * NC, 4, vdt)
        if tag == "mat32":
            fn = lambda: qmg.stencil_apply_mat32(d, y, x, qmg.P_ALL | qmg.P_ZERO, nrhs=K, vec_stride=vol * NC, mask=(1 << K) - 1)
        else:
            fn = lambda: qmg.stencil_apply_t(vdt, d, y, x, qmg.P_ALL | qmg.P_ZERO, nrhs=K, vec_stride=vol * NC, mask=(1 << K) - 1)
        measure("kernelC_nc%d_k8_%d_%s" % (NC, Lx, tag), fn)
        for a in (cl, ho, x, y):
            a.free()

N = 393216
for tag, dt in (("f64", qmg.C64), ("f32", qmg.C32)):
    xs = [gauss(K * N, 10 + j, dt) for j in range(8)]
    yv = gauss(K * N, 9, dt)
    for nj in (8, 4, 2):
        measure("bmultidot_nj%d_%s" % (nj, tag), lambda: qmg.batch_multidot_t(dt, xs[:nj], yv, N, K, N, (1 << K) - 1))
    for a in xs + [yv]:
        a.free()
