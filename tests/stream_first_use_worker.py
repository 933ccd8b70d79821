"""Worker for tests/test_gpu_streams.py::test_first_use_on_a_created_stream: one leg per per-thread workspace of the library.

    python stream_first_use_worker.py LEG

The leg's entry point is the FIRST compute call of this process -- the call that creates the calling thread's workspace -- and it runs on a
created (non-blocking) stream behind a gate (tests/stream_gate.py), with the inputs uploaded on the null stream and synchronised before.
Then the device is synchronised and the call is repeated on the null stream.  Printed: `gate closed` (the gate as found immediately before
the call), `stream <hex>` and `null <hex>` (the bytes of the two results; the parent wants them equal) and `twin ok` (both results against
the numpy twin of the entry point at the tolerance of its own test).  Leg `thread` makes the call the first reduction of a second host
thread, on a stream of its own, while the main thread waits: the emulated-rank situation of drivers/driver_common.hpp.
"""
import importlib
import os
import sys
import threading

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
qmg = importlib.import_module("quantum-mg_amd")
import batch_numpy as bn
import coordspace as cs
import dwf_meas_numpy as dm
import flow_numpy as fn
import singlet_numpy as sgl
import stencil_numpy as sn
import stream_gate as sg
import u1_numpy as un

GATE_COPIES = 64
TOL_REDUCE = 1e-12     # tests/test_gpu_batch_routes.py
D = qmg.DeviceArray.from_host


def cv(n, seed):
    return cs.gaussian_cvec(n, seed)


def leg_norm2sq():
    n = 4099
    x = cv(n, 1)
    dx = D(x)
    want = bn.norm2(x)
    return (lambda st: np.asarray(qmg.norm2sq(dx, n, stream=st))), (lambda got: abs(got - want) <= TOL_REDUCE * want)


def leg_batch_reduce():
    n, stride, nrhs, mask = 4099, 4104, 3, 0b101
    x, y = cv(stride * nrhs, 1), cv(stride * nrhs, 2)
    dx, dy = D(x), D(y)

    def twin(got):
        for i, k in enumerate((0, 2)):
            want, scale = bn.reduce(bn.DOT, x[k * stride:k * stride + n], y[k * stride:k * stride + n])
            if not abs(got[i] - complex(want)) <= TOL_REDUCE * scale:
                return False
        return True
    return (lambda st: qmg.batch_reduce_t(qmg.C64, qmg.BRED_DOT, dx, dy, n, nrhs, stride, mask, stream=st)[[0, 2]]), twin


def leg_mr_dots():
    n, stride, nrhs, mask = 4099, 4104, 3, 0b101
    r, p = cv(stride * nrhs, 1), cv(stride * nrhs, 2)
    dr, dp = D(r), D(p)

    def call(st):
        qmg.batch_mr_dots(qmg.C64, dr, dp, n, nrhs, stride, mask, stream=st)
        return qmg.batch_mr_read_dots(nrhs, stream=st)[[0, 2], :3]

    def twin(got):
        for i, k in enumerate((0, 2)):
            pr, pp, s_pr, s_pp = bn.mr_dots(r[k * stride:k * stride + n], p[k * stride:k * stride + n])
            if not (abs(complex(got[i, 0], got[i, 1]) - complex(pr)) <= TOL_REDUCE * s_pr and abs(got[i, 2] - pp) <= TOL_REDUCE * s_pp):
                return False
        return True
    return call, twin


def leg_apply_norm2():
    Lx, Ly, nc, nrhs = 12, 6, 2, 2
    vol = Lx * Ly * nc
    gd = qmg.make_desc(Lx, Ly, nc, D(cv(Lx * Ly * nc * nc, 1)), D(cv(4 * Lx * Ly * nc * nc, 2)), 0.1)
    rhs, lhs = D(cv(vol * nrhs, 3)), qmg.DeviceArray.zeros(vol * nrhs)

    def twin(got):     # tests/test_gpu_apply_norm.py: the norms of the vectors the apply left, to 1e-13
        out = lhs.to_host()
        return all(abs(got[k] - float(np.vdot(out[k * vol:(k + 1) * vol], out[k * vol:(k + 1) * vol]).real)) <= 1e-13 * got[k] for k in range(nrhs))
    return (lambda st: qmg.stencil_apply_norm2(gd, lhs, rhs, qmg.P_ALL | qmg.P_ZERO, nrhs, vol, stream=st)), twin


def leg_basis_dot():
    n, nv, nrhs, mask = 1000, 5, 3, 0b101
    ldv, stride = n + 3, n + 5
    V, B = cv(nv * ldv, 1), cv(nrhs * stride, 2)
    dV, dB = D(V), D(B)
    Vm, Bm = V.reshape(nv, ldv)[:, :n], B.reshape(nrhs, stride)[:, :n]
    want = (Vm.conj() @ Bm.T).T

    def twin(got):     # tests/test_gpu_deflation.py
        return all(np.linalg.norm(got[i] - want[k]) <= 1e-13 * np.linalg.norm(Vm, 2) * np.linalg.norm(Bm[k]) for i, k in enumerate((0, 2)))
    return (lambda st: qmg.basis_dot_t(qmg.C64, dV, nv, ldv, dB, n, nrhs, stride, mask, stream=st)[[0, 2]]), twin


def _links(Lx, Ly, seed):
    th = np.random.default_rng(seed).uniform(-3, 3, (2, Lx, Ly))
    Ux, Uy = np.exp(1j * th[0]), np.exp(1j * th[1])
    return Ux, Uy, D(cs.links_to_eo_gauge(Ux, Uy, Lx, Ly))


def leg_plaquette():
    Lx, Ly = 12, 6
    Ux, Uy, dg = _links(Lx, Ly, 1)
    want = un.plaquette(Ux, Uy)
    return (lambda st: np.asarray(qmg.u1_plaquette(dg, Lx, Ly, stream=st), dtype=np.complex128)), \
           (lambda got: abs(got[0] - want[0]) < 1e-13 and abs(got[1].real - want[1]) < 1e-9)     # tests/test_gpu_u1_tools.py


def leg_wilson_loops():
    Lx, Ly = 12, 6
    Ux, Uy, dg = _links(Lx, Ly, 1)
    want = fn.wilson_loops(Ux, Uy, 3, 2)
    return (lambda st: qmg.u1_wilson_loops(dg, Lx, Ly, 3, 2, stream=st)), (lambda got: np.abs(got - want).max() <= 1e-12)     # tests/test_gpu_flow.py


def leg_slice_norms():
    Lx, Ly, Ls = 12, 6, 4
    x = cv(Lx * Ly * 2 * Ls, 1)
    dx = D(x)
    want = dm.slice_norms(x, Lx, Ly, Ls)
    bound = sn.elementwise_bound(want, Lx + 2)     # tests/test_gpu_dwf_meas.py
    return (lambda st: qmg.dwf_slice_norms(qmg.C64, (Lx, Ly), Ls, dx, stream=st)), (lambda got: bool(np.all(np.abs(got[0].astype(np.longdouble) - want) <= bound)))


def leg_loops():
    Lx, Ly, nc, dil, seed = 12, 6, 2, (2, 1, 1), 5
    x = cv(Lx * Ly * nc, 1)
    dx = D(x)
    want = sgl.loops(x, seed, Lx, Ly, nc, dil, 3, 0)
    gate = 1e-12 * sgl.row_abs_sum(x, Lx, Ly, nc)     # tests/test_gpu_singlet.py
    return (lambda st: qmg.loops_timeslice_batch(qmg.C64, dx, (Lx, Ly), nc, dil, 3, seed, 0, stream=st)), (lambda got: bool(np.all(np.abs(got[0] - want) <= gate[:, None])))


LEGS = {"norm2sq": leg_norm2sq, "batch_reduce": leg_batch_reduce, "mr_dots": leg_mr_dots, "apply_norm2": leg_apply_norm2, "basis_dot": leg_basis_dot,
        "plaquette": leg_plaquette, "wilson_loops": leg_wilson_loops, "slice_norms": leg_slice_norms, "loops": leg_loops, "thread": leg_norm2sq}


def first_use(call, twin):
    st = qmg.stream_create()
    gate = sg.Gate(st, GATE_COPIES)
    print("gate %s" % ("closed" if gate.closed() else "open"))
    on_stream = np.ascontiguousarray(call(st))
    qmg.sync(st)
    qmg.sync()
    on_null = np.ascontiguousarray(call(None))
    qmg.sync()
    print("stream %s" % on_stream.tobytes().hex())
    print("null %s" % on_null.tobytes().hex())
    print("twin %s" % ("ok" if twin(on_stream) and twin(on_null) else "FAIL"))
    qmg.stream_destroy(st)


def main():
    leg = sys.argv[1]
    qmg.init(0)
    call, twin = LEGS[leg]()     # uploads on the null stream
    qmg.sync()
    if leg == "thread":
        failed = []

        def rank():
            try:
                qmg.init(0)
                first_use(call, twin)
            except BaseException as e:     # noqa: a failure in the thread must fail the process
                failed.append(e)
        t = threading.Thread(target=rank)
        t.start()
        t.join()
        if failed:
            raise failed[0]
    else:
        first_use(call, twin)
    sys.stdout.flush()


if __name__ == "__main__":
    main()
