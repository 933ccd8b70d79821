"""quantum-mg_amd -- MI355X-native multigrid hot path behind the quantum-mg operator API.

The product is `libqmg_hip.so` (hand-written HIP kernels for gfx950 + a C-ABI, include/qmg_hip.h)
and the C++ facade in `include/qmg/` that mirrors the reference's Stencil2D / TransferMG /
StatefulMultigridMG classes.  This Python module is only the ctypes binding used by tests/,
bench.py and __graft_entry__.py to drive the C-ABI; it holds no compute and has NO CPU
fallback: if the shared library is missing, importing `lib()` raises.

(The directory name contains a hyphen, so import it with
 `importlib.import_module("quantum-mg_amd")`.)
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO_PATH = os.path.join(HERE, "libqmg_hip.so")

# ---- enums (include/qmg_hip.h) ----
P_CLOVER_E, P_CLOVER_O = 1 << 0, 1 << 1
P_EO_XP1, P_OE_XP1 = 1 << 2, 1 << 6
P_SHIFT_E, P_SHIFT_O = 1 << 10, 1 << 11
P_ZERO_E, P_ZERO_O = 1 << 12, 1 << 13
P_CLOVER, P_EO, P_OE, P_HOPPING = 3, 0xF << 2, 0xF << 6, 0xFF << 2
P_SHIFT, P_ZERO, P_ALL = 3 << 10, 3 << 12, 0xFFF
CSHIFT_FROM_0, CSHIFT_XP1, CSHIFT_YP1, CSHIFT_XM1, CSHIFT_YM1 = 1, 2, 3, 4, 5
EO_FROM_EVEN, EO_FROM_ODD, EO_FROM_EVENODD = 1, 2, 3

# every symbol include/qmg_hip.h declares (checked by tests/test_abi_symbols.py against the header text)
ABI_SYMBOLS = [
    "qmg_init", "qmg_device_count", "qmg_status_string", "qmg_last_hip_error", "qmg_version",
    "qmg_malloc", "qmg_free", "qmg_poison_scratch", "qmg_shutdown", "qmg_mem_info", "qmg_memcpy_h2d", "qmg_memcpy_d2h", "qmg_memcpy_d2d", "qmg_memset_zero",
    "qmg_stream_create", "qmg_stream_destroy", "qmg_stream_sync",
    "qmg_event_create", "qmg_event_destroy", "qmg_event_record", "qmg_event_elapsed_ms", "qmg_stream_wait_event",
    "qmg_cshift", "qmg_stencil_apply", "qmg_stencil_apply_batch", "qmg_stencil_apply_mat32", "qmg_c64_to_c32", "qmg_wilson_fill", "qmg_staggered_fill", "qmg_laplace_fill",
    "qmg_build_dagger", "qmg_build_rbjacobi", "qmg_cmat_conjtrans",
    "qmg_zero_vector", "qmg_copy_vector", "qmg_cax", "qmg_caxy", "qmg_caxpy", "qmg_cxpy", "qmg_cxpay",
    "qmg_caxpby", "qmg_cxpyz", "qmg_caxpbyz", "qmg_multi_caxpy", "qmg_caxy_pattern", "qmg_gaussian",
    "qmg_norm2sq", "qmg_dot", "qmg_diffnorm2sq", "qmg_norminf", "qmg_multidot",
    "qmg_norm2sq_cv_timeslice", "qmg_dot_cv_timeslice", "qmg_redot_cv_timeslice", "qmg_gaussian_wall_source",
    "qmg_prolong", "qmg_restrict", "qmg_block_orthonormalize", "qmg_block_orthonormalize_n", "qmg_block_bi_orthonormalize", "qmg_coarse_build", "qmg_set_tuning",
    "qmg_batch_blas", "qmg_batch_multi_caxpy", "qmg_batch_reduce", "qmg_batch_multidot", "qmg_prolong_batch", "qmg_restrict_batch",
    "qmg_comm_get_unique_id", "qmg_comm_init", "qmg_comm_init_env", "qmg_comm_rendezvous", "qmg_comm_all_ok", "qmg_comm_world", "qmg_allreduce_sum_f64", "qmg_comm_finalize",
    "qmg_convert", "qmg_stencil_apply_t", "qmg_batch_blas_t", "qmg_batch_multi_caxpy_t", "qmg_batch_gcr_update_t", "qmg_batch_cgm_update_t", "qmg_prolong_batch_nv32", "qmg_restrict_batch_nv32", "qmg_batch_reduce_t", "qmg_batch_multidot_t",
    "qmg_prolong_batch_t", "qmg_restrict_batch_t", "qmg_transfer_plan", "qmg_stencil_plan",
    "qmg_convert_to_c16", "qmg_convert_from_c16", "qmg_stencil_apply_h16", "qmg_stencil_apply_mat16_t", "qmg_stencil_apply_norm2",
    "qmg_wilson_apply_direct", "qmg_wilson_hops_direct", "qmg_halo_exchange", "qmg_halo_exchange_parity", "qmg_stencil_apply_slab", "qmg_wilson_fill_slab", "qmg_comm_set_distributed_reductions", "qmg_coarse_build_slab", "qmg_gaussian_slab", "qmg_rb_hopping_slab", "qmg_build_dagger_slab", "qmg_staggered_fill_slab", "qmg_laplace_fill_slab", "qmg_comm_emulate_begin", "qmg_comm_emulate_attach", "qmg_comm_emulate_end",
    "qmg_stencil_apply_epi_t", "qmg_wilson_apply_direct_epi", "qmg_wilson_hops_direct_epi", "qmg_batch_mr_dots_t", "qmg_batch_mr_update_t", "qmg_batch_mr_read_dots",
    "qmg_basis_dot_t", "qmg_basis_update_t", "qmg_batch_deflate_t",
    "qmg_u1_heatbath_noncompact", "qmg_u1_phase_to_gauge", "qmg_u1_gauge_to_phase", "qmg_u1_plaquette", "qmg_u1_noncompact_action",
    "qmg_u1_hot_gauge", "qmg_u1_gauss_gauge", "qmg_u1_random_trans", "qmg_u1_gauge_transform", "qmg_u1_ape_smear", "qmg_u1_instanton", "qmg_u1_noncompact_instanton",
    "qmg_hmc_momentum_update", "qmg_hmc_momentum_update_poles", "qmg_hmc_momentum_update_staggered", "qmg_hmc_link_update", "qmg_hmc_momentum_refresh", "qmg_hmc_stream_seed",
    "qmg_hmc_momentum_update_dwf", "qmg_hmc_dwf_plan", "qmg_hmc_gauge_step",
    "qmg_u1_stout_smear", "qmg_hmc_fermion_force", "qmg_u1_stout_force_level", "qmg_hmc_momentum_update_stout",
    "qmg_u1_flow_stage", "qmg_u1_flow", "qmg_u1_wilson_loops", "qmg_u1_polyakov",
    "qmg_dwf_fill", "qmg_dwf_apply_direct", "qmg_dwf_plan", "qmg_batch_plan", "qmg_wilson_plan",
    "qmg_dwf_inv5", "qmg_dwf_hops_inv5", "qmg_dwf_schur_apply", "qmg_dwf_eo_plan",
    "qmg_dwf_wall_source", "qmg_dwf_wall_project", "qmg_dwf_slice_norms", "qmg_dwf_meas_plan",
    "qmg_mobius_fill", "qmg_mobius_apply_direct", "qmg_mobius_plan",
    "qmg_mobius_inv5", "qmg_mobius_hops_inv5", "qmg_mobius_schur_apply", "qmg_mobius_eo_plan",
    "qmg_setup_plan",
    "qmg_noise_z4", "qmg_noise_dilute_batch", "qmg_loops_timeslice_batch", "qmg_singlet_plan",
]


class StencilDesc(C.Structure):
    _fields_ = [("Lx", C.c_int), ("Ly", C.c_int), ("nc", C.c_int),
                ("clover", C.c_void_p), ("hopping", C.c_void_p),
                ("shift", C.c_double * 2), ("eo_shift", C.c_double * 2), ("dof_shift", C.c_double * 2)]


class QmgError(RuntimeError):
    pass


def build(force=False):
    """Compile libqmg_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-C", HERE, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", HERE, "-j4", "libqmg_hip.so"], stdout=subprocess.DEVNULL)
    return SO_PATH


_lib = None


def lib():
    """The loaded C-ABI library.  Raises if it has not been built: there is no fallback path."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise QmgError("libqmg_hip.so not built (%s); run __graft_entry__.build() -- there is no CPU fallback" % SO_PATH)
        _lib = C.CDLL(SO_PATH)
        _lib.qmg_status_string.restype = C.c_char_p
        _lib.qmg_last_hip_error.restype = C.c_char_p
        _lib.qmg_version.restype = C.c_char_p
    return _lib


def check(status, what=""):
    if status != 0:
        L = lib()
        raise QmgError("%s failed: %s [%s]" % (what or "qmg call", L.qmg_status_string(status).decode(), L.qmg_last_hip_error().decode()))


def init(device=0):
    check(lib().qmg_init(device), "qmg_init")


def device_count():
    n = C.c_int(0)
    lib().qmg_device_count(C.byref(n))
    return n.value


def sync(stream=None):
    check(lib().qmg_stream_sync(C.c_void_p(stream)), "qmg_stream_sync")


def stream_create():
    """A non-default HIP stream as the raw handle every `stream=` argument takes."""
    st = C.c_void_p()
    check(lib().qmg_stream_create(C.byref(st)), "qmg_stream_create")
    return st.value


def stream_destroy(stream):
    check(lib().qmg_stream_destroy(C.c_void_p(stream)), "qmg_stream_destroy")


class DeviceArray:
    """A complex128 (or raw bytes) array in HBM owned through qmg_malloc / qmg_free."""

    def __init__(self, n, dtype=np.complex128):
        self.n = int(n)
        self.dtype = np.dtype(dtype)
        self.nbytes = self.n * self.dtype.itemsize
        p = C.c_void_p()
        check(lib().qmg_malloc(C.byref(p), C.c_size_t(self.nbytes)), "qmg_malloc")
        self.ptr = p.value or 0

    @classmethod
    def from_host(cls, a):
        a = np.ascontiguousarray(a)
        d = cls(a.size, a.dtype)
        check(lib().qmg_memcpy_h2d(C.c_void_p(d.ptr), a.ctypes.data_as(C.c_void_p), C.c_size_t(d.nbytes), None), "h2d")
        return d

    @classmethod
    def zeros(cls, n, dtype=np.complex128):
        d = cls(n, dtype)
        check(lib().qmg_memset_zero(C.c_void_p(d.ptr), C.c_size_t(d.nbytes), None), "memset")
        return d

    def to_host(self):
        out = np.empty(self.n, dtype=self.dtype)
        sync()
        check(lib().qmg_memcpy_d2h(out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr), C.c_size_t(self.nbytes), None), "d2h")
        return out

    def read(self, first, count):
        """`count` elements starting at element `first`, copied to the host (spot checks on arrays too large to download)."""
        out = np.empty(int(count), dtype=self.dtype)
        sync()
        check(lib().qmg_memcpy_d2h(out.ctypes.data_as(C.c_void_p), C.c_void_p(self.offset(first)), C.c_size_t(out.nbytes), None), "d2h")
        return out

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=self.dtype)
        assert a.size == self.n
        check(lib().qmg_memcpy_h2d(C.c_void_p(self.ptr), a.ctypes.data_as(C.c_void_p), C.c_size_t(self.nbytes), None), "h2d")

    def offset(self, elems):
        return self.ptr + int(elems) * self.dtype.itemsize

    def free(self):
        if self.ptr:
            lib().qmg_free(C.c_void_p(self.ptr))
            self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _checked(status_fn, what):
    """The raising form of a wrapper that returns its status: same parameters (stream= among them)."""
    @functools.wraps(status_fn)
    def call(*args, **kw):
        check(status_fn(*args, **kw), what)
    call.__name__ = call.__qualname__ = status_fn.__name__[:-len("_status")]
    return call


def memcpy_h2d(dst_dev, src_host, nbytes=None, stream=None):
    """src_host: a contiguous numpy array; synchronous when stream is None"""
    check(lib().qmg_memcpy_h2d(_vp(dst_dev), src_host.ctypes.data_as(C.c_void_p), C.c_size_t(src_host.nbytes if nbytes is None else nbytes), C.c_void_p(stream)), "qmg_memcpy_h2d")


def memcpy_d2h(dst_host, src_dev, nbytes=None, stream=None):
    check(lib().qmg_memcpy_d2h(dst_host.ctypes.data_as(C.c_void_p), _vp(src_dev), C.c_size_t(dst_host.nbytes if nbytes is None else nbytes), C.c_void_p(stream)), "qmg_memcpy_d2h")


def memcpy_d2d(dst_dev, src_dev, nbytes, stream=None):
    check(lib().qmg_memcpy_d2d(_vp(dst_dev), _vp(src_dev), C.c_size_t(nbytes), C.c_void_p(stream)), "qmg_memcpy_d2d")


def memset_zero(dev, nbytes, stream=None):
    check(lib().qmg_memset_zero(_vp(dev), C.c_size_t(nbytes), C.c_void_p(stream)), "qmg_memset_zero")


def poison_scratch(dev, nbytes, stream=None):
    check(lib().qmg_poison_scratch(_vp(dev), C.c_size_t(nbytes), C.c_void_p(stream)), "qmg_poison_scratch")


def event_create():
    ev = C.c_void_p()
    check(lib().qmg_event_create(C.byref(ev)), "qmg_event_create")
    return ev.value


def event_destroy(ev):
    check(lib().qmg_event_destroy(C.c_void_p(ev)), "qmg_event_destroy")


def event_record(ev, stream=None):
    check(lib().qmg_event_record(C.c_void_p(ev), C.c_void_p(stream)), "qmg_event_record")


def event_elapsed_ms(ev_start, ev_stop):
    ms = C.c_float()
    check(lib().qmg_event_elapsed_ms(C.c_void_p(ev_start), C.c_void_p(ev_stop), C.byref(ms)), "qmg_event_elapsed_ms")
    return ms.value


def allreduce_sum_f64(buf_dev, n, stream=None):
    check(lib().qmg_allreduce_sum_f64(C.cast(_vp(buf_dev), C.POINTER(C.c_double)), C.c_size_t(n), C.c_void_p(stream)), "qmg_allreduce_sum_f64")


def _vp(x):
    if x is None:
        return C.c_void_p(None)
    if isinstance(x, DeviceArray):
        return C.c_void_p(x.ptr)
    return C.c_void_p(int(x))


def make_desc(Lx, Ly, nc, clover, hopping, shift=0.0, eo_shift=0.0, dof_shift=0.0):
    d = StencilDesc()
    d.Lx, d.Ly, d.nc = Lx, Ly, nc
    d.clover = None if clover is None else (clover.ptr if isinstance(clover, DeviceArray) else int(clover))
    d.hopping = None if hopping is None else (hopping.ptr if isinstance(hopping, DeviceArray) else int(hopping))
    for name, v in (("shift", shift), ("eo_shift", eo_shift), ("dof_shift", dof_shift)):
        v = complex(v)
        getattr(d, name)[0], getattr(d, name)[1] = v.real, v.imag
    d._keep = (clover, hopping)
    return d


def stencil_apply(desc, lhs, rhs, pieces=P_ALL | P_ZERO, nrhs=1, vec_stride=0, stream=None):
    check(lib().qmg_stencil_apply(C.byref(desc), _vp(lhs), _vp(rhs), C.c_uint(pieces), C.c_int(nrhs),
                                  C.c_size_t(vec_stride), C.c_void_p(stream)), "qmg_stencil_apply")


def stencil_apply_norm2(desc, lhs, rhs, pieces=P_ALL | P_ZERO, nrhs=1, vec_stride=0, norms_dev=None, stream=None):
    """The apply and |lhs_k|^2 of its results in one pass.  With norms_dev (a device pointer to nrhs doubles) nothing
    synchronises and None is returned; otherwise the norms come back as a numpy array."""
    out = None if norms_dev is not None else np.full(nrhs, np.nan)
    check(lib().qmg_stencil_apply_norm2(C.byref(desc), _vp(lhs), _vp(rhs), C.c_uint(pieces), C.c_int(nrhs), C.c_size_t(vec_stride),
                                        C.c_void_p(norms_dev), None if out is None else out.ctypes.data_as(C.POINTER(C.c_double)),
                                        C.c_void_p(stream)), "qmg_stencil_apply_norm2")
    return out


def cshift(lhs, rhs, cdir, eo, dof, Lx, Ly, stream=None):
    check(lib().qmg_cshift(_vp(lhs), _vp(rhs), cdir, eo, dof, Lx, Ly, C.c_void_p(stream)), "qmg_cshift")


def wilson_fill(clover, hopping, gauge, Lx, Ly, w=1.0, stream=None):
    check(lib().qmg_wilson_fill(_vp(clover), _vp(hopping), _vp(gauge), Lx, Ly, C.c_double(w), C.c_void_p(stream)), "qmg_wilson_fill")


def staggered_fill(hopping, gauge, Lx, Ly, stream=None):
    check(lib().qmg_staggered_fill(_vp(hopping), _vp(gauge), Lx, Ly, C.c_void_p(stream)), "qmg_staggered_fill")


def laplace_fill(clover, hopping, gauge, Lx, Ly, stream=None):
    check(lib().qmg_laplace_fill(_vp(clover), _vp(hopping), _vp(gauge), Lx, Ly, C.c_void_p(stream)), "qmg_laplace_fill")


def build_dagger(dclover, dhopping, clover, hopping, Lx, Ly, nc, stream=None):
    check(lib().qmg_build_dagger(_vp(dclover), _vp(dhopping), _vp(clover), _vp(hopping), Lx, Ly, nc, C.c_void_p(stream)), "qmg_build_dagger")


def staggered_fill_slab(hopping, gauge_global, Lx, Ly_global, y0, Ly_local, stream=None):
    check(lib().qmg_staggered_fill_slab(_vp(hopping), _vp(gauge_global), Lx, Ly_global, y0, Ly_local, C.c_void_p(stream)), "qmg_staggered_fill_slab")


def laplace_fill_slab(clover, hopping, gauge_global, Lx, Ly_global, y0, Ly_local, stream=None):
    check(lib().qmg_laplace_fill_slab(_vp(clover), _vp(hopping), _vp(gauge_global), Lx, Ly_global, y0, Ly_local, C.c_void_p(stream)), "qmg_laplace_fill_slab")


def build_dagger_slab(dclover, dhopping, clover, hopping, Lx, Ly, nc, ym_halo_hi, yp_halo_lo, stream=None):
    check(lib().qmg_build_dagger_slab(_vp(dclover), _vp(dhopping), _vp(clover), _vp(hopping), Lx, Ly, nc, _vp(ym_halo_hi), _vp(yp_halo_lo), C.c_void_p(stream)),
          "qmg_build_dagger_slab")


def build_rbjacobi(cinv, rclover, rhopping, desc, stream=None):
    check(lib().qmg_build_rbjacobi(_vp(cinv), _vp(rclover), _vp(rhopping), C.byref(desc), C.c_void_p(stream)), "qmg_build_rbjacobi")


def cmat_conjtrans(out, inp, nsite, nc, stream=None):
    """out[i] = in[i]^dagger for nsite row-major nc x nc blocks (cMATcopy_conjtrans_square; stencil_2d.h:2012-2020: cinv of the rbj-dagger stencil)."""
    check(lib().qmg_cmat_conjtrans(_vp(out), _vp(inp), C.c_size_t(nsite), nc, C.c_void_p(stream)), "qmg_cmat_conjtrans")


def _scalar(a):
    a = complex(a)
    return C.c_double(a.real), C.c_double(a.imag)


def zero_vector(x, n, stream=None):
    check(lib().qmg_zero_vector(_vp(x), C.c_size_t(n), C.c_void_p(stream)))


def copy_vector(dst, src, n, stream=None):
    check(lib().qmg_copy_vector(_vp(dst), _vp(src), C.c_size_t(n), C.c_void_p(stream)))


def cax(a, x, n, stream=None):
    check(lib().qmg_cax(*_scalar(a), _vp(x), C.c_size_t(n), C.c_void_p(stream)))


def caxy(a, x, y, n, stream=None):
    check(lib().qmg_caxy(*_scalar(a), _vp(x), _vp(y), C.c_size_t(n), C.c_void_p(stream)))


def caxpy(a, x, y, n, stream=None):
    check(lib().qmg_caxpy(*_scalar(a), _vp(x), _vp(y), C.c_size_t(n), C.c_void_p(stream)))


def cxpy(x, y, n, stream=None):
    check(lib().qmg_cxpy(_vp(x), _vp(y), C.c_size_t(n), C.c_void_p(stream)))


def cxpay(x, a, y, n, stream=None):
    check(lib().qmg_cxpay(_vp(x), *_scalar(a), _vp(y), C.c_size_t(n), C.c_void_p(stream)))


def caxpby(a, x, b, y, n, stream=None):
    check(lib().qmg_caxpby(*_scalar(a), _vp(x), *_scalar(b), _vp(y), C.c_size_t(n), C.c_void_p(stream)))


def cxpyz(x, y, z, n, stream=None):
    check(lib().qmg_cxpyz(_vp(x), _vp(y), _vp(z), C.c_size_t(n), C.c_void_p(stream)))


def caxpbyz(a, x, b, y, z, n, stream=None):
    check(lib().qmg_caxpbyz(*_scalar(a), _vp(x), *_scalar(b), _vp(y), _vp(z), C.c_size_t(n), C.c_void_p(stream)))


def multi_caxpy(coeffs, xs, y, n, stream=None):
    k = len(xs)
    cf = (C.c_double * (2 * k))(*[v for a in coeffs for v in (complex(a).real, complex(a).imag)])
    ptrs = (C.c_void_p * k)(*[(x.ptr if isinstance(x, DeviceArray) else int(x)) for x in xs])
    check(lib().qmg_multi_caxpy(cf, ptrs, k, _vp(y), C.c_size_t(n), C.c_void_p(stream)), "qmg_multi_caxpy")


def caxy_pattern(scale, shuffle, x, y, nsite, stream=None):
    nc = len(scale)
    sc = (C.c_double * nc)(*scale)
    sh = (C.c_int * nc)(*shuffle)
    check(lib().qmg_caxy_pattern(sc, sh, nc, _vp(x), _vp(y), C.c_size_t(nsite), C.c_void_p(stream)))


def gaussian(x, n, seed, stream=None):
    check(lib().qmg_gaussian(_vp(x), C.c_size_t(n), C.c_ulonglong(seed), C.c_void_p(stream)))


def norm2sq(x, n, stream=None):
    out = C.c_double()
    check(lib().qmg_norm2sq(_vp(x), C.c_size_t(n), None, C.byref(out), C.c_void_p(stream)))
    return out.value


def dot(x, y, n, stream=None):
    out = (C.c_double * 2)()
    check(lib().qmg_dot(_vp(x), _vp(y), C.c_size_t(n), None, out, C.c_void_p(stream)))
    return complex(out[0], out[1])


def diffnorm2sq(x, y, n, stream=None):
    out = C.c_double()
    check(lib().qmg_diffnorm2sq(_vp(x), _vp(y), C.c_size_t(n), None, C.byref(out), C.c_void_p(stream)))
    return out.value


def norminf(x, n, stream=None):
    out = C.c_double()
    check(lib().qmg_norminf(_vp(x), C.c_size_t(n), None, C.byref(out), C.c_void_p(stream)))
    return out.value


def multidot(xs, y, n, stream=None):
    k = len(xs)
    ptrs = (C.c_void_p * k)(*[(x.ptr if isinstance(x, DeviceArray) else int(x)) for x in xs])
    out = (C.c_double * (2 * k))()
    check(lib().qmg_multidot(ptrs, k, _vp(y), C.c_size_t(n), None, out, C.c_void_p(stream)))
    return np.array([complex(out[2 * i], out[2 * i + 1]) for i in range(k)])


def norm2sq_cv_timeslice(cv, Lx, Ly, nc, stream=None):
    out = np.zeros(Ly)
    check(lib().qmg_norm2sq_cv_timeslice(_vp(cv), Lx, Ly, nc, None, out.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(stream)))
    return out


def dot_cv_timeslice(a, b, Lx, Ly, nc, stream=None):
    out = np.zeros(2 * Ly)
    check(lib().qmg_dot_cv_timeslice(_vp(a), _vp(b), Lx, Ly, nc, None, out.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(stream)))
    return out[0::2] + 1j * out[1::2]


def redot_cv_timeslice(a, b, Lx, Ly, nc, stream=None):
    out = np.zeros(Ly)
    check(lib().qmg_redot_cv_timeslice(_vp(a), _vp(b), Lx, Ly, nc, None, out.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(stream)))
    return out


def gaussian_wall_source(cv, Lx, Ly, nc, timeslice, color, seed, deviation=1.0, mean=0.0, stream=None):
    """reductions/reductions.h:90-162; returns the status instead of raising for an out-of-range timeslice / color (the reference prints and returns)."""
    return lib().qmg_gaussian_wall_source(_vp(cv), Lx, Ly, nc, timeslice, color, C.c_ulonglong(seed), C.c_double(deviation), C.c_double(mean), C.c_void_p(stream))


def prolong(nullvecs, nvec, coarse, fine, fdims, cdims, stream=None):
    check(lib().qmg_prolong(_vp(nullvecs), nvec, _vp(coarse), _vp(fine), *fdims, *cdims, C.c_void_p(stream)), "qmg_prolong")


def restrict(nullvecs, nvec, fine, coarse, fdims, cdims, stream=None):
    check(lib().qmg_restrict(_vp(nullvecs), nvec, _vp(fine), _vp(coarse), *fdims, *cdims, C.c_void_p(stream)), "qmg_restrict")


def block_orthonormalize(nullvecs, nvec, fdims, cLx, cLy, cholesky=None, stream=None):
    check(lib().qmg_block_orthonormalize(_vp(nullvecs), nvec, *fdims, cLx, cLy, _vp(cholesky), C.c_void_p(stream)), "qmg_block_orthonormalize")


def block_orthonormalize_n(nullvecs, nvec, fdims, cLx, cLy, cholesky=None, passes=2, stream=None):
    """`passes` (1 or 2) passes in one call, the factor saved in the first (qmg_block_orthonormalize_n)"""
    check(lib().qmg_block_orthonormalize_n(_vp(nullvecs), nvec, *fdims, cLx, cLy, _vp(cholesky), passes, C.c_void_p(stream)), "qmg_block_orthonormalize_n")


def block_bi_orthonormalize(pvecs, rvecs, nvec, fdims, cLx, cLy, block_L=None, block_U=None, stream=None):
    check(lib().qmg_block_bi_orthonormalize(_vp(pvecs), _vp(rvecs), nvec, *fdims, cLx, cLy, _vp(block_L), _vp(block_U), C.c_void_p(stream)), "qmg_block_bi_orthonormalize")


def coarse_build(cclover, chopping, fdesc, nullvecs, cdims, restrict_vecs=None, stream=None):
    check(lib().qmg_coarse_build(_vp(cclover), _vp(chopping), C.byref(fdesc), _vp(nullvecs), _vp(restrict_vecs), *cdims, C.c_void_p(stream)), "qmg_coarse_build")


def coarse_build_slab(cclover, chopping, fdesc, nullvecs, cdims, halo_lo, halo_hi, halo_stride, restrict_vecs=None, stream=None):
    check(lib().qmg_coarse_build_slab(_vp(cclover), _vp(chopping), C.byref(fdesc), _vp(nullvecs), _vp(restrict_vecs), *cdims, _vp(halo_lo), _vp(halo_hi),
                                      C.c_size_t(halo_stride), C.c_void_p(stream)), "qmg_coarse_build_slab")


# the `op` argument, the families and the flags of qmg_setup_plan (include/qmg_hip.h)
SETUP_OP_ORTHO, SETUP_OP_GALERKIN, SETUP_OP_CINV = range(3)
SUF_UNSUPPORTED, SUF_ORTHO_LDS, SUF_ORTHO_PASSES, SUF_INVALID, SUF_GALERKIN, SUF_GALERKIN_PROBES, SUF_CINV = range(7)
SUP_LDS_OPTIN, SUP_IDLE_GROUP, SUP_STRIDED = 1, 2, 4
SETUP_PLAN_INTS = 8


def setup_plan(op, fdims, cdims=(0, 0), ncv=0, a=0, b=0):
    """What the setup entry points do with a request (qmg_setup_plan; host only): (family, tpb, groups, workgroups, lds, flags, outs, threads).
    ORTHO: fdims -> cdims, ncv = nvec, a = passes; GALERKIN: ncv = cnc, a = slab; CINV: fdims = (Lx, Ly, nc), a = clover present, b = any shift."""
    out = (C.c_int * SETUP_PLAN_INTS)()
    check(lib().qmg_setup_plan(op, fdims[0], fdims[1], fdims[2], cdims[0], cdims[1], ncv, int(a), int(b), out, SETUP_PLAN_INTS), "qmg_setup_plan")
    return tuple(out)


class ApplyEpilogue(C.Structure):
    _fields_ = [("other", C.c_void_p), ("other_scale", C.c_double), ("acc_scale", C.c_double), ("dotv", C.c_void_p)]


def make_epilogue(other=None, other_scale=1.0, acc_scale=-1.0, dotv=None):
    e = ApplyEpilogue()
    e.other = None if other is None else (other.ptr if isinstance(other, DeviceArray) else int(other))
    e.other_scale, e.acc_scale = other_scale, acc_scale
    e.dotv = None if dotv is None else (dotv.ptr if isinstance(dotv, DeviceArray) else int(dotv))
    return e


def stencil_apply_epi(dtype, mat32, desc, lhs, rhs, pieces, epi, vec_stride=0, system=0, stream=None):
    """status (0 = done, 3 = this operator is not served with an epilogue) of qmg_stencil_apply_epi_t"""
    return lib().qmg_stencil_apply_epi_t(dtype, int(mat32), C.byref(desc), _vp(lhs), _vp(rhs), C.c_uint(pieces), C.c_size_t(vec_stride), system, C.byref(epi), C.c_void_p(stream))


def wilson_apply_direct_epi(dtype, desc, gauge, lhs, rhs, pieces, epi, nrhs=1, vec_stride=0, mask=1, wilson_coeff=1.0, stream=None):
    return lib().qmg_wilson_apply_direct_epi(dtype, C.byref(desc), _vp(gauge), desc.Ly, 0, C.c_double(wilson_coeff), _vp(lhs), _vp(rhs), None, None, C.c_uint(pieces), nrhs,
                                             C.c_size_t(vec_stride), C.c_size_t(0), C.c_uint(mask), C.byref(epi), C.c_void_p(stream))


def wilson_hops_direct_epi(dtype, desc, gauge, hop_scale, lhs, rhs, pieces, epi, nrhs=1, vec_stride=0, mask=1, wilson_coeff=1.0, stream=None):
    return lib().qmg_wilson_hops_direct_epi(dtype, C.byref(desc), _vp(gauge), desc.Ly, 0, C.c_double(wilson_coeff), C.c_double(hop_scale), _vp(lhs), _vp(rhs), None, None,
                                            C.c_uint(pieces), nrhs, C.c_size_t(vec_stride), C.c_size_t(0), C.c_uint(mask), C.byref(epi), C.c_void_p(stream))


def batch_mr_dots(dtype, r, p, n, nrhs, stride, mask, stream=None):
    check(lib().qmg_batch_mr_dots_t(dtype, _vp(r), _vp(p), C.c_size_t(n), nrhs, C.c_size_t(stride), C.c_uint(mask), C.c_void_p(stream)), "qmg_batch_mr_dots_t")


def batch_mr_update(dtype, omega, x, r_in, r_out, p, x_set, n, nrhs, stride, mask, stream=None):
    check(lib().qmg_batch_mr_update_t(dtype, C.c_double(omega), _vp(x), _vp(r_in), _vp(r_out), _vp(p), int(x_set), C.c_size_t(n), nrhs, C.c_size_t(stride), C.c_uint(mask), C.c_void_p(stream)),
          "qmg_batch_mr_update_t")


def batch_mr_read_dots(nrhs, stream=None):
    out = (C.c_double * (4 * nrhs))()
    check(lib().qmg_batch_mr_read_dots(out, nrhs, C.c_void_p(stream)), "qmg_batch_mr_read_dots")
    return np.array(out).reshape(nrhs, 4)


def gaussian_slab(x, Lx, Ly_global, y0, Ly_local, nc, seed, stream=None):
    check(lib().qmg_gaussian_slab(_vp(x), Lx, Ly_global, y0, Ly_local, nc, C.c_ulonglong(seed), C.c_void_p(stream)), "qmg_gaussian_slab")


# ---------------- lock-step batches (qmg_batch.hip) ----------------
BOP_ZERO, BOP_COPY, BOP_CAX, BOP_CAXPY, BOP_CXPY, BOP_CAXPBYZ, BOP_CAXY, BOP_CXPAY, BOP_CAXPBY, BOP_CXPYZ = range(10)
BRED_NORM2, BRED_DOT, BRED_DIFFNORM2 = range(3)


def _coef(a, nrhs):
    if a is None:
        return None
    v = np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.complex128), (nrhs,))).view(np.float64)
    return v.ctypes.data_as(C.POINTER(C.c_double)), v


def stencil_apply_batch(desc, lhs, rhs, pieces, nrhs, vec_stride, mask, stream=None):
    check(lib().qmg_stencil_apply_batch(C.byref(desc), _vp(lhs), _vp(rhs), C.c_uint(pieces), nrhs, C.c_size_t(vec_stride), C.c_uint(mask), C.c_void_p(stream)),
          "qmg_stencil_apply_batch")


def stencil_apply_mat32(desc, lhs, rhs, pieces, nrhs, vec_stride, mask, stream=None):
    check(lib().qmg_stencil_apply_mat32(C.byref(desc), _vp(lhs), _vp(rhs), C.c_uint(pieces), nrhs, C.c_size_t(vec_stride), C.c_uint(mask), C.c_void_p(stream)),
          "qmg_stencil_apply_mat32")


def stencil_apply_mat16(vec_dtype, desc, lhs, rhs, pieces, nrhs=1, vec_stride=0, mask=1, stream=None):
    """status of qmg_stencil_apply_mat16_t: complex<half> matrices (convert_to_c16), vectors of vec_dtype"""
    return lib().qmg_stencil_apply_mat16_t(vec_dtype, C.byref(desc), _vp(lhs), _vp(rhs), C.c_uint(pieces), nrhs, C.c_size_t(vec_stride), C.c_uint(mask), C.c_void_p(stream))


def convert_from_c16(dst, dst_dtype, src, n, stream=None):
    check(lib().qmg_convert_from_c16(_vp(dst), dst_dtype, _vp(src), C.c_size_t(n), C.c_void_p(stream)), "qmg_convert_from_c16")


def c64_to_c32(dst, src, n, stream=None):
    check(lib().qmg_c64_to_c32(_vp(dst), _vp(src), C.c_size_t(n), C.c_void_p(stream)), "qmg_c64_to_c32")


def batch_blas(op, z, n, nrhs, stride, mask, a=None, b=None, x=None, y=None, stream=None):
    ca, cb = _coef(a, nrhs), _coef(b, nrhs)
    check(lib().qmg_batch_blas(op, ca[0] if ca else None, cb[0] if cb else None, _vp(x), _vp(y), _vp(z), C.c_size_t(n), nrhs, C.c_size_t(stride),
                               C.c_uint(mask), C.c_void_p(stream)), "qmg_batch_blas")


def batch_multi_caxpy(coeffs, xs, y, n, nrhs, stride, mask, stream=None):
    nj = len(xs)
    cf = np.ascontiguousarray(np.asarray(coeffs, dtype=np.complex128).reshape(nj, nrhs)).view(np.float64)
    ptrs = (C.c_void_p * nj)(*[x.ptr for x in xs])
    check(lib().qmg_batch_multi_caxpy(cf.ctypes.data_as(C.POINTER(C.c_double)), ptrs, nj, _vp(y), C.c_size_t(n), nrhs, C.c_size_t(stride), C.c_uint(mask), C.c_void_p(stream)),
          "qmg_batch_multi_caxpy")


def batch_reduce(op, x, y, n, nrhs, stride, mask, stream=None):
    out = np.full(2 * nrhs, np.nan)
    check(lib().qmg_batch_reduce(op, _vp(x), _vp(y), C.c_size_t(n), nrhs, C.c_size_t(stride), C.c_uint(mask), out.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(stream)),
          "qmg_batch_reduce")
    return out[0::2] + 1j * out[1::2]


def batch_multidot(xs, y, n, nrhs, stride, mask, stream=None):
    nj = len(xs)
    ptrs = (C.c_void_p * nj)(*[x.ptr for x in xs])
    out = np.full(2 * nrhs * nj, np.nan)
    check(lib().qmg_batch_multidot(ptrs, nj, _vp(y), C.c_size_t(n), nrhs, C.c_size_t(stride), C.c_uint(mask), out.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(stream)),
          "qmg_batch_multidot")
    return (out[0::2] + 1j * out[1::2]).reshape(nrhs, nj)


def prolong_batch(nullvecs, nvec, coarse, fine, fdims, cdims, nrhs, cstride, fstride, mask, stream=None):
    check(lib().qmg_prolong_batch(_vp(nullvecs), nvec, _vp(coarse), _vp(fine), *fdims, *cdims, nrhs, C.c_size_t(cstride), C.c_size_t(fstride), C.c_uint(mask), C.c_void_p(stream)),
          "qmg_prolong_batch")


def restrict_batch(nullvecs, nvec, fine, coarse, fdims, cdims, nrhs, fstride, cstride, mask, stream=None):
    check(lib().qmg_restrict_batch(_vp(nullvecs), nvec, _vp(fine), _vp(coarse), *fdims, *cdims, nrhs, C.c_size_t(fstride), C.c_size_t(cstride), C.c_uint(mask), C.c_void_p(stream)),
          "qmg_restrict_batch")


# ---------------- either storage precision (`_t` entry points; dtype = C64 | C32) ----------------
C64, C32 = 0, 1
NP_DTYPE = {C64: np.complex128, C32: np.complex64}


def convert(dst, dst_dtype, src, src_dtype, n, stream=None):
    check(lib().qmg_convert(_vp(dst), dst_dtype, _vp(src), src_dtype, C.c_size_t(n), C.c_void_p(stream)), "qmg_convert")


def stencil_apply_t(dtype, desc, lhs, rhs, pieces, nrhs=1, vec_stride=0, mask=1, stream=None):
    check(lib().qmg_stencil_apply_t(dtype, C.byref(desc), _vp(lhs), _vp(rhs), C.c_uint(pieces), nrhs, C.c_size_t(vec_stride), C.c_uint(mask), C.c_void_p(stream)),
          "qmg_stencil_apply_t")


def batch_blas_t(dtype, op, z, n, nrhs, stride, mask, a=None, b=None, x=None, y=None, stream=None):
    ca, cb = _coef(a, nrhs), _coef(b, nrhs)
    check(lib().qmg_batch_blas_t(dtype, op, ca[0] if ca else None, cb[0] if cb else None, _vp(x), _vp(y), _vp(z), C.c_size_t(n), nrhs, C.c_size_t(stride),
                                 C.c_uint(mask), C.c_void_p(stream)), "qmg_batch_blas_t")


def batch_multi_caxpy_t(dtype, coeffs, xs, y, n, nrhs, stride, mask, stream=None):
    nj = len(xs)
    cf = np.ascontiguousarray(np.asarray(coeffs, dtype=np.complex128).reshape(nj, nrhs)).view(np.float64)
    ptrs = (C.c_void_p * nj)(*[x.ptr for x in xs])
    check(lib().qmg_batch_multi_caxpy_t(dtype, cf.ctypes.data_as(C.POINTER(C.c_double)), ptrs, nj, _vp(y), C.c_size_t(n), nrhs, C.c_size_t(stride), C.c_uint(mask), C.c_void_p(stream)),
          "qmg_batch_multi_caxpy_t")


def batch_gcr_update_t(dtype, coeffs, ws, w, a, r, z_next, n, nrhs, stride, mask, stream=None):
    """w += sum_j c_j ws_j ; r += a w ; z_next = r (optional) in one pass (qmg_batch_gcr_update_t)"""
    nj = len(ws)
    cf = np.ascontiguousarray(np.asarray(coeffs, dtype=np.complex128).reshape(max(nj, 1), nrhs)).view(np.float64) if nj else None
    ptrs = (C.c_void_p * max(nj, 1))(*[x.ptr for x in ws]) if nj else None
    av = np.ascontiguousarray(np.asarray(a, dtype=np.complex128).reshape(nrhs)).view(np.float64)
    check(lib().qmg_batch_gcr_update_t(dtype, cf.ctypes.data_as(C.POINTER(C.c_double)) if nj else None, ptrs, nj, _vp(w), av.ctypes.data_as(C.POINTER(C.c_double)), _vp(r),
                                       _vp(z_next), C.c_size_t(n), nrhs, C.c_size_t(stride), C.c_uint(mask), C.c_void_p(stream)), "qmg_batch_gcr_update_t")


def batch_cgm_update_status(dtype, xs, ps, a, z, c, shift_masks, r, n, nrhs, stride, mask, ns=None, stream=None):
    """qmg_batch_cgm_update_t's status code (xs / ps / a / z / c / shift_masks may be None: the argument checks are part of the ABI)"""
    ns = len(xs) if ns is None else ns

    def table(v):
        return (C.c_void_p * max(len(v), 1))(*[_vp(x).value for x in v]) if v is not None else None

    def reals(v):
        return np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1)) if v is not None else None

    av, zv, cv = reals(a), reals(z), reals(c)
    dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double)) if v is not None else None
    sm = (C.c_uint * max(len(shift_masks), 1))(*shift_masks) if shift_masks is not None else None
    return lib().qmg_batch_cgm_update_t(dtype, table(xs), table(ps), ns, dp(av), dp(zv), dp(cv), sm, _vp(r), C.c_size_t(n), nrhs, C.c_size_t(stride), C.c_uint(mask), C.c_void_p(stream))


def batch_cgm_update_t(dtype, xs, ps, a, z, c, shift_masks, r, n, nrhs, stride, mask, stream=None):
    """x[s] += a[s] p[s] ; p[s] = z[s] r + c[s] p[s] for the systems of mask & shift_masks[s], every shift in one pass (qmg_batch_cgm_update_t);
    a, z, c: real, shape (ns, nrhs)"""
    check(batch_cgm_update_status(dtype, xs, ps, a, z, c, shift_masks, r, n, nrhs, stride, mask, stream=stream), "qmg_batch_cgm_update_t")


def batch_reduce_t(dtype, op, x, y, n, nrhs, stride, mask, stream=None):
    out = np.full(2 * nrhs, np.nan)
    check(lib().qmg_batch_reduce_t(dtype, op, _vp(x), _vp(y), C.c_size_t(n), nrhs, C.c_size_t(stride), C.c_uint(mask), out.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(stream)),
          "qmg_batch_reduce_t")
    return out[0::2] + 1j * out[1::2]


def batch_multidot_t(dtype, xs, y, n, nrhs, stride, mask, stream=None):
    nj = len(xs)
    ptrs = (C.c_void_p * nj)(*[x.ptr for x in xs])
    out = np.full(2 * nrhs * nj, np.nan)
    check(lib().qmg_batch_multidot_t(dtype, ptrs, nj, _vp(y), C.c_size_t(n), nrhs, C.c_size_t(stride), C.c_uint(mask), out.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(stream)),
          "qmg_batch_multidot_t")
    return (out[0::2] + 1j * out[1::2]).reshape(nrhs, nj)


def basis_dot_t(dtype, V, nv, ldv, B, n, nrhs, stride, mask, out_dev=None, stream=None):
    """C[k][j] = <v_j, b_k> for one basis V shared by the batch (qmg_basis_dot_t); (nrhs, nv) complex array, NaN for inactive systems.
    out_dev: a DeviceArray of nrhs * nv complex128 to receive them on the device instead (returns None)."""
    if out_dev is not None:
        check(lib().qmg_basis_dot_t(dtype, _vp(V), nv, C.c_size_t(ldv), _vp(B), C.c_size_t(n), nrhs, C.c_size_t(stride), C.c_uint(mask),
                                    C.cast(C.c_void_p(out_dev.ptr), C.POINTER(C.c_double)), 1, C.c_void_p(stream)), "qmg_basis_dot_t")
        return None
    out = np.full(2 * nrhs * nv, np.nan)
    check(lib().qmg_basis_dot_t(dtype, _vp(V), nv, C.c_size_t(ldv), _vp(B), C.c_size_t(n), nrhs, C.c_size_t(stride), C.c_uint(mask),
                                out.ctypes.data_as(C.POINTER(C.c_double)), 0, C.c_void_p(stream)), "qmg_basis_dot_t")
    return (out[0::2] + 1j * out[1::2]).reshape(nrhs, nv)


def basis_update_t(dtype, coeffs, V, nv, ldv, B, n, nrhs, stride, mask, stream=None):
    """b_k += sum_j C[k][j] v_j (qmg_basis_update_t); coeffs: (nrhs, nv) complex on the host, or a DeviceArray of them"""
    if isinstance(coeffs, DeviceArray):
        cp, dev = C.cast(C.c_void_p(coeffs.ptr), C.POINTER(C.c_double)), 1
    else:
        cf = np.ascontiguousarray(np.asarray(coeffs, dtype=np.complex128).reshape(nrhs, nv)).view(np.float64)
        cp, dev = cf.ctypes.data_as(C.POINTER(C.c_double)), 0
    check(lib().qmg_basis_update_t(dtype, cp, dev, _vp(V), nv, C.c_size_t(ldv), _vp(B), C.c_size_t(n), nrhs, C.c_size_t(stride), C.c_uint(mask), C.c_void_p(stream)),
          "qmg_basis_update_t")


def batch_deflate_t(dtype, V, nv, ldv, inv_lambda_dev, B, E, n, nrhs, stride, mask, stream=None):
    """e_k = sum_j v_j <v_j, b_k> inv_lambda[j] (qmg_batch_deflate_t); inv_lambda_dev: a DeviceArray of nv float64"""
    check(lib().qmg_batch_deflate_t(dtype, _vp(V), nv, C.c_size_t(ldv), C.cast(C.c_void_p(inv_lambda_dev.ptr), C.POINTER(C.c_double)), _vp(B), _vp(E),
                                    C.c_size_t(n), nrhs, C.c_size_t(stride), C.c_uint(mask), C.c_void_p(stream)), "qmg_batch_deflate_t")


def prolong_batch_t(dtype, nullvecs, nvec, coarse, fine, fdims, cdims, nrhs, cstride, fstride, mask, stream=None):
    check(lib().qmg_prolong_batch_t(dtype, _vp(nullvecs), nvec, _vp(coarse), _vp(fine), *fdims, *cdims, nrhs, C.c_size_t(cstride), C.c_size_t(fstride), C.c_uint(mask), C.c_void_p(stream)),
          "qmg_prolong_batch_t")


def restrict_batch_t(dtype, nullvecs, nvec, fine, coarse, fdims, cdims, nrhs, fstride, cstride, mask, stream=None):
    check(lib().qmg_restrict_batch_t(dtype, _vp(nullvecs), nvec, _vp(fine), _vp(coarse), *fdims, *cdims, nrhs, C.c_size_t(fstride), C.c_size_t(cstride), C.c_uint(mask), C.c_void_p(stream)),
          "qmg_restrict_batch_t")


XFER_RESTRICT, XFER_PROLONG = 0, 1
# kernel families of qmg_transfer_plan (include/qmg_hip.h)
XF_UNSUPPORTED, XF_RESTRICT, XF_RESTRICT_GENERIC, XF_PROLONG, XF_BRESTRICT_MFMA, XF_BRESTRICT_SMALL, XF_BRESTRICT_TILE, XF_BPROLONG_TILE = range(8)
XF_RESTRICT_NV32, XF_PROLONG_NV32 = 8, 9


def transfer_plan(op, dtype, null32, nvec, fdims, cdims, n_active, aligned16=True):
    """The kernel plan of a restrict / prolong request (qmg_transfer_plan; host only): a list with one tuple
    (family, KB, NV, MT, CR, nchunk, small, W) per pass of up to 8 systems."""
    out = (C.c_int * 16)()
    check(lib().qmg_transfer_plan(op, dtype, int(null32), nvec, *fdims, *cdims, n_active, int(aligned16), out, 16), "qmg_transfer_plan")
    return [tuple(out[8 * p:8 * p + 8]) for p in range(2) if out[8 * p] >= 0]


# entry points, kernel families, storage bits and flags of qmg_stencil_plan (include/qmg_hip.h)
SE_APPLY, SE_MASKED, SE_H16, SE_NORM2, SE_EPI, SE_SLAB = range(6)
SF_UNSUPPORTED, SF_ELEM, SF_PAIR, SF_SITE, SF_GEN, SF_GEN32, SF_MFMA, SF_VOLUME1, SF_NOTHING, SF_INVALID = range(10)
SST_M32, SST_V32, SST_M16 = 1, 2, 4
SPF_EPI, SPF_DOTS, SPF_NORM, SPF_PF, SPF_ZERO, SPF_BATCH, SPF_VL, SPF_PAIR, SPF_SHIFT = 1, 2, 4, 8, 16, 32, 64, 128, 256
STENCIL_PLAN_INTS = 12


def stencil_plan(entry, mat, vec32, dims, pieces, n_active, holes=False, inplace=False, clover=True, hopping=True, epilogue=0, slab_rows=0, max_passes=4):
    """The kernel plan of a stencil apply at the current tuning knobs (qmg_stencil_plan; host only): a list with one tuple
    (family, storage, NC, P, K, flags, S, H, smem, gx, gy, nk) per pass."""
    n = STENCIL_PLAN_INTS * max_passes
    out = (C.c_int * n)()
    check(lib().qmg_stencil_plan(entry, mat, int(vec32), *dims, C.c_uint(pieces), n_active, int(holes), int(inplace), int(clover), int(hopping), epilogue, slab_rows,
                                 out, n), "qmg_stencil_plan")
    return [tuple(out[STENCIL_PLAN_INTS * p:STENCIL_PLAN_INTS * (p + 1)]) for p in range(max_passes) if out[STENCIL_PLAN_INTS * p] >= 0]


# entry points, kernel families and variant bits of qmg_batch_plan (include/qmg_hip.h)
BE_BLAS, BE_MULTI_CAXPY, BE_GCR_UPDATE, BE_CGM_UPDATE, BE_REDUCE, BE_MULTIDOT, BE_MR_DOTS, BE_MR_UPDATE = range(8)
BF_NOTHING, BF_BLAS, BF_MAXPY_SMALL, BF_MAXPY_LONG, BF_MAXPY_SINGLE, BF_GCR, BF_CGM, BF_REDUCE, BF_MULTIDOT, BF_MR_DOTS, BF_MR_UPDATE = range(11)
BPV_XSET, BPV_ROUT, BPV_ZNEXT = 1, 2, 1
BATCH_PLAN_INTS = 5
BATCH_LONG_BYTES = 16 << 20   # BATCH_LONG_BYTES of csrc/qmg_batch_plan.h: a vector of this many bytes per system is a long vector


def batch_plan(entry, dtype, n, stride, nrhs, mask, op=0, nj=0, shift_masks=None, flags=0, aligned16=True, max_passes=8):
    """The kernel plan of a batch vector call at the current blas_nt_mb (qmg_batch_plan; host only): a list with one tuple
    (family, W, nt, J, variant) per pass, in launch order."""
    out = (C.c_int * (BATCH_PLAN_INTS * max_passes))()
    sm = (C.c_uint * max(len(shift_masks), 1))(*shift_masks) if shift_masks is not None else None
    check(lib().qmg_batch_plan(entry, dtype, op, C.c_size_t(n), C.c_size_t(stride), nrhs, C.c_uint(mask), nj, sm, flags, int(aligned16), out, max_passes),
          "qmg_batch_plan")
    return [tuple(out[BATCH_PLAN_INTS * p:BATCH_PLAN_INTS * (p + 1)]) for p in range(max_passes) if out[BATCH_PLAN_INTS * p] >= 0]


def prolong_batch_nv32(null32, nvec, coarse, fine, fdims, cdims, nrhs, cstride, fstride, mask, stream=None):
    """complex<double> vectors, complex<float> null vectors (qmg_prolong_batch_nv32)"""
    check(lib().qmg_prolong_batch_nv32(_vp(null32), nvec, _vp(coarse), _vp(fine), *fdims, *cdims, nrhs, C.c_size_t(cstride), C.c_size_t(fstride), C.c_uint(mask), C.c_void_p(stream)),
          "qmg_prolong_batch_nv32")


def restrict_batch_nv32(null32, nvec, fine, coarse, fdims, cdims, nrhs, fstride, cstride, mask, stream=None):
    check(lib().qmg_restrict_batch_nv32(_vp(null32), nvec, _vp(fine), _vp(coarse), *fdims, *cdims, nrhs, C.c_size_t(fstride), C.c_size_t(cstride), C.c_uint(mask), C.c_void_p(stream)),
          "qmg_restrict_batch_nv32")


def convert_to_c16(dst, src, src_dtype, n, stream=None):
    check(lib().qmg_convert_to_c16(_vp(dst), _vp(src), src_dtype, C.c_size_t(n), C.c_void_p(stream)), "qmg_convert_to_c16")


def stencil_apply_h16(desc, lhs, rhs, pieces, nrhs=1, vec_stride=0, mask=1, stream=None):
    check(lib().qmg_stencil_apply_h16(C.byref(desc), _vp(lhs), _vp(rhs), C.c_uint(pieces), nrhs, C.c_size_t(vec_stride), C.c_uint(mask), C.c_void_p(stream)),
          "qmg_stencil_apply_h16")


def comm_init_env(world, rank):
    check(lib().qmg_comm_init_env(world, rank), "qmg_comm_init_env")


SLAB_H16 = 0x100
SLAB_M32 = 0x200   # nc != 2: complex<float> matrices whatever the vectors' type
SLAB_M16 = 0x400   # nc != 2, a multiple of 4: complex<half> matrices


def halo_exchange(dtype, vec, Lx, Ly_local, nc, halo_lo, halo_hi, nrhs=1, vec_stride=0, halo_stride=0, stream=None):
    check(lib().qmg_halo_exchange(dtype, _vp(vec), Lx, Ly_local, nc, _vp(halo_lo), _vp(halo_hi), nrhs, C.c_size_t(vec_stride), C.c_size_t(halo_stride), C.c_void_p(stream)),
          "qmg_halo_exchange")


def halo_exchange_parity(dtype, vec, Lx, Ly_local, nc, halo_lo, halo_hi, parities, nrhs=1, vec_stride=0, halo_stride=0, stream=None):
    check(lib().qmg_halo_exchange_parity(dtype, _vp(vec), Lx, Ly_local, nc, _vp(halo_lo), _vp(halo_hi), nrhs, C.c_size_t(vec_stride), C.c_size_t(halo_stride),
                                         C.c_uint(parities), C.c_void_p(stream)), "qmg_halo_exchange_parity")


def rb_hopping_slab(rb_hopping, desc, cinv, cinv_halo_lo, cinv_halo_hi, stream=None):
    check(lib().qmg_rb_hopping_slab(_vp(rb_hopping), C.byref(desc), _vp(cinv), _vp(cinv_halo_lo), _vp(cinv_halo_hi), C.c_void_p(stream)), "qmg_rb_hopping_slab")


def stencil_apply_slab(storage, desc, lhs, rhs, halo_lo, halo_hi, pieces, nrhs=1, vec_stride=0, halo_stride=0, mask=1, rows=0, stream=None):
    check(lib().qmg_stencil_apply_slab(storage, C.byref(desc), _vp(lhs), _vp(rhs), _vp(halo_lo), _vp(halo_hi), C.c_uint(pieces), nrhs, C.c_size_t(vec_stride),
                                       C.c_size_t(halo_stride), C.c_uint(mask), rows, C.c_void_p(stream)), "qmg_stencil_apply_slab")


def wilson_fill_slab(clover, hopping, gauge_global, Lx, Ly_global, y0, Ly_local, w=1.0, stream=None):
    check(lib().qmg_wilson_fill_slab(_vp(clover), _vp(hopping), _vp(gauge_global), Lx, Ly_global, y0, Ly_local, C.c_double(w), C.c_void_p(stream)), "qmg_wilson_fill_slab")


def wilson_apply_direct(dtype, desc, gauge, lhs, rhs, pieces, w=1.0, nrhs=1, vec_stride=0, mask=1, gauge_Ly=None, y0=0, halo_lo=None, halo_hi=None,
                        halo_stride=0, rows=0, stream=None):
    check(lib().qmg_wilson_apply_direct(dtype, C.byref(desc), _vp(gauge), desc.Ly if gauge_Ly is None else gauge_Ly, y0, C.c_double(w), _vp(lhs), _vp(rhs),
                                        _vp(halo_lo), _vp(halo_hi), C.c_uint(pieces), nrhs, C.c_size_t(vec_stride), C.c_size_t(halo_stride), C.c_uint(mask), rows,
                                        C.c_void_p(stream)), "qmg_wilson_apply_direct")


def wilson_hops_direct(dtype, desc, gauge, lhs, rhs, pieces, w, hop_scale, nrhs=1, vec_stride=0, mask=1, gauge_Ly=None, y0=0, halo_lo=None, halo_hi=None,
                       halo_stride=0, rows=0, stream=None):
    check(lib().qmg_wilson_hops_direct(dtype, C.byref(desc), _vp(gauge), desc.Ly if gauge_Ly is None else gauge_Ly, y0, C.c_double(w), C.c_double(hop_scale),
                                       _vp(lhs), _vp(rhs), _vp(halo_lo), _vp(halo_hi), C.c_uint(pieces), nrhs, C.c_size_t(vec_stride), C.c_size_t(halo_stride),
                                       C.c_uint(mask), rows, C.c_void_p(stream)), "qmg_wilson_hops_direct")


# families, flags and the epilogue description of qmg_wilson_plan (include/qmg_hip.h)
WF_UNSUPPORTED, WF_DIRECT, WF_NOTHING, WF_INVALID, WF_PAIR, WF_PAIR2 = range(6)
WPF_ZERO, WPF_BATCH, WPF_F32, WPF_DOTS = 1, 2, 4, 8
WPE_ON, WPE_OTHER, WPE_DOTV, WPE_DOTV_IS_OTHER, WPE_DOTV_IS_RHS, WPE_ALIASES_LHS = 1, 2, 4, 8, 16, 32
WILSON_PLAN_INTS = 16


def wilson_plan(dtype, dims, pieces, n_active=1, inplace=False, scaled=False, epi=0, gauge_Ly=None, y0=0, halos=False, rows=0, nc=2, layout_ok=True):
    """What the Wilson applies from the links do with a request at the current "wilson_pair" (qmg_wilson_plan; host only): (family, lps, block,
    gx, gy, flags, shape, emode, nk, y_first, y_count, boundary_only, npart, status, par_first, par_count)."""
    out = (C.c_int * WILSON_PLAN_INTS)()
    check(lib().qmg_wilson_plan(dtype, dims[0], dims[1], nc, dims[1] if gauge_Ly is None else gauge_Ly, y0, int(halos), int(layout_ok), int(scaled), C.c_uint(pieces),
                                n_active, int(inplace), rows, C.c_uint(epi), out, WILSON_PLAN_INTS), "qmg_wilson_plan")
    return tuple(out)


def dwf_fill(clover, hopping, gauge, Lx, Ly, Ls, mass=0.0, w=1.0, stream=None):
    """The stored nc = 2 Ls clover / hopping fields of the Shamir domain-wall operator (qmg_dwf_fill)."""
    mass = complex(mass)
    check(lib().qmg_dwf_fill(_vp(clover), _vp(hopping), _vp(gauge), Lx, Ly, Ls, C.c_double(mass.real), C.c_double(mass.imag), C.c_double(w), C.c_void_p(stream)),
          "qmg_dwf_fill")


def dwf_apply_direct_status(dtype, desc, gauge, Ls, mass, lhs, rhs, pieces, w=1.0, nrhs=1, vec_stride=0, mask=1, stream=None):
    """qmg_dwf_apply_direct's status, unchecked (the refusals are part of its contract)."""
    mass = complex(mass)
    return lib().qmg_dwf_apply_direct(dtype, C.byref(desc), _vp(gauge), Ls, C.c_double(mass.real), C.c_double(mass.imag), C.c_double(w), _vp(lhs), _vp(rhs),
                                      C.c_uint(pieces), nrhs, C.c_size_t(vec_stride), C.c_uint(mask), C.c_void_p(stream))


def dwf_apply_direct(dtype, desc, gauge, Ls, mass, lhs, rhs, pieces, w=1.0, nrhs=1, vec_stride=0, mask=1, stream=None):
    check(dwf_apply_direct_status(dtype, desc, gauge, Ls, mass, lhs, rhs, pieces, w, nrhs, vec_stride, mask, stream), "qmg_dwf_apply_direct")


# families and flags of qmg_dwf_plan (include/qmg_hip.h)
DF_UNSUPPORTED, DF_DIRECT, DF_NOTHING, DF_INVALID, DF_PAIR = range(5)
DPF_ZERO, DPF_BATCH, DPF_F32 = 1, 2, 4
DWF_PLAN_INTS = 8


def dwf_plan(dtype, dims, Ls, pieces, n_active=1, inplace=False):
    """What qmg_dwf_apply_direct does with a request (qmg_dwf_plan; host only): (family, lps, block, gx, gy, flags, shape, nk)."""
    out = (C.c_int * DWF_PLAN_INTS)()
    check(lib().qmg_dwf_plan(dtype, dims[0], dims[1], Ls, C.c_uint(pieces), n_active, int(inplace), out, DWF_PLAN_INTS), "qmg_dwf_plan")
    return tuple(out)


# ---- the even-odd Schur complement of the domain-wall operator from the links (csrc/qmg_dwf_eo.hip)
DWF_G5_IN, DWF_G5_OUT = 1, 2
# the `kernel` argument and the families of qmg_dwf_eo_plan (include/qmg_hip.h)
DEK_INV5, DEK_HOPS_INV5, DEK_SCHUR2 = range(3)
DEF_UNSUPPORTED, DEF_HOPS_INV5, DEF_NOTHING, DEF_INVALID, DEF_INV5, DEF_SCHUR2 = range(6)
DWF_EO_PLAN_INTS = 8


def dwf_inv5_status(dtype, desc, Ls, mass, lhs, rhs, pieces, alpha=1.0, w=1.0, nrhs=1, vec_stride=0, mask=1, stream=None):
    """qmg_dwf_inv5's status, unchecked: lhs_p = alpha A_p^-1 rhs_p on the parities P_CLOVER_E / P_CLOVER_O name."""
    mass, alpha = complex(mass), complex(alpha)
    return lib().qmg_dwf_inv5(dtype, C.byref(desc), Ls, C.c_double(mass.real), C.c_double(mass.imag), C.c_double(w), _vp(lhs), _vp(rhs), C.c_uint(pieces),
                              C.c_double(alpha.real), C.c_double(alpha.imag), nrhs, C.c_size_t(vec_stride), C.c_uint(mask), C.c_void_p(stream))


dwf_inv5 = _checked(dwf_inv5_status, "qmg_dwf_inv5")


def dwf_hops_inv5_status(dtype, desc, gauge, Ls, mass, lhs, rhs, pieces, alpha=1.0, flags=0, w=1.0, nrhs=1, vec_stride=0, mask=1, stream=None):
    """qmg_dwf_hops_inv5's status, unchecked: lhs_p (+)= alpha A_p^-1 H_{p,1-p} [Gamma5] rhs_{1-p}."""
    mass, alpha = complex(mass), complex(alpha)
    return lib().qmg_dwf_hops_inv5(dtype, C.byref(desc), _vp(gauge), Ls, C.c_double(mass.real), C.c_double(mass.imag), C.c_double(w), _vp(lhs), _vp(rhs),
                                   C.c_uint(pieces), C.c_double(alpha.real), C.c_double(alpha.imag), C.c_uint(flags), nrhs, C.c_size_t(vec_stride), C.c_uint(mask),
                                   C.c_void_p(stream))


dwf_hops_inv5 = _checked(dwf_hops_inv5_status, "qmg_dwf_hops_inv5")


def dwf_schur_apply_status(dtype, desc, gauge, Ls, mass, lhs, rhs, tmp, parity=0, flags=0, w=1.0, nrhs=1, vec_stride=0, mask=1, stream=None):
    """qmg_dwf_schur_apply's status, unchecked: lhs_p = Gamma5^out M_p Gamma5^in rhs_p, two launches."""
    mass = complex(mass)
    return lib().qmg_dwf_schur_apply(dtype, C.byref(desc), _vp(gauge), Ls, C.c_double(mass.real), C.c_double(mass.imag), C.c_double(w), _vp(lhs), _vp(rhs), _vp(tmp),
                                     parity, C.c_uint(flags), nrhs, C.c_size_t(vec_stride), C.c_uint(mask), C.c_void_p(stream))


dwf_schur_apply = _checked(dwf_schur_apply_status, "qmg_dwf_schur_apply")


def dwf_eo_plan(dtype, dims, Ls, kernel, pieces, n_active=1, inplace=False):
    """What the even-odd entries launch (qmg_dwf_eo_plan; host only): (family, lps, block, gx, gy, flags, lds, nk)."""
    out = (C.c_int * DWF_EO_PLAN_INTS)()
    check(lib().qmg_dwf_eo_plan(dtype, dims[0], dims[1], Ls, kernel, C.c_uint(pieces), n_active, int(inplace), out, DWF_EO_PLAN_INTS), "qmg_dwf_eo_plan")
    return tuple(out)


# ---- the Moebius domain-wall operator from the links (csrc/qmg_mobius.hip)
# the `op` argument and the families of qmg_mobius_plan (include/qmg_hip.h)
MOP_D, MOP_DAGGER = 0, 1
MF_UNSUPPORTED, MF_LOAD, MF_NOTHING, MF_INVALID, MF_RESULT = range(5)
MOBIUS_PLAN_INTS = 8


def mobius_fill(clover, hopping, gauge, Lx, Ly, Ls, mass=0.0, w=1.0, M5=-1.0, b5=1.0, c5=0.0, stream=None):
    """The stored nc = 2 Ls fields of the Moebius operator D = A + H B (qmg_mobius_fill): clover = A, hopping = H B."""
    mass = complex(mass)
    check(lib().qmg_mobius_fill(_vp(clover), _vp(hopping), _vp(gauge), Lx, Ly, Ls, C.c_double(mass.real), C.c_double(mass.imag), C.c_double(w), C.c_double(M5),
                                C.c_double(b5), C.c_double(c5), C.c_void_p(stream)), "qmg_mobius_fill")


def mobius_apply_direct_status(dtype, desc, gauge, Ls, mass, lhs, rhs, pieces, w=1.0, M5=-1.0, b5=1.0, c5=0.0, op=0, nrhs=1, vec_stride=0, mask=1, stream=None):
    """qmg_mobius_apply_direct's status, unchecked: lhs (+)= D rhs (op 0) or D^dagger rhs (op 1) from the links."""
    mass = complex(mass)
    return lib().qmg_mobius_apply_direct(dtype, C.byref(desc), _vp(gauge), Ls, C.c_double(mass.real), C.c_double(mass.imag), C.c_double(w), C.c_double(M5),
                                         C.c_double(b5), C.c_double(c5), int(op), _vp(lhs), _vp(rhs), C.c_uint(pieces), nrhs, C.c_size_t(vec_stride), C.c_uint(mask),
                                         C.c_void_p(stream))


mobius_apply_direct = _checked(mobius_apply_direct_status, "qmg_mobius_apply_direct")


def mobius_plan(dtype, dims, Ls, op, pieces, n_active=1, inplace=False):
    """What qmg_mobius_apply_direct launches (qmg_mobius_plan; host only): (family, lps, block, gx, gy, flags, lds, nk)."""
    out = (C.c_int * MOBIUS_PLAN_INTS)()
    check(lib().qmg_mobius_plan(dtype, dims[0], dims[1], Ls, int(op), C.c_uint(pieces), n_active, int(inplace), out, MOBIUS_PLAN_INTS), "qmg_mobius_plan")
    return tuple(out)


# ---- the even-odd Schur complement of the Moebius operator and its dagger from the links (csrc/qmg_mobius_eo.hip)
# the `kernel`, `table` and `source` arguments and the families of qmg_mobius_eo_plan (include/qmg_hip.h)
MEK_INV5, MEK_HOPS_INV5, MEK_SCHUR2, MEK_SCHUR2_DAGGER = range(4)
MOBIUS_S_ONE, MOBIUS_S_AINV, MOBIUS_S_AINV_B = range(3)
MOBIUS_R_ONE, MOBIUS_R_B = range(2)
MEF_UNSUPPORTED, MEF_HOPS_MIX, MEF_NOTHING, MEF_INVALID, MEF_MIX, MEF_SCHUR2, MEF_SCHUR2_DAGGER = range(7)
MEPF_RMIX = 8
MOBIUS_EO_PLAN_INTS = 8


def mobius_inv5_status(dtype, desc, Ls, mass, lhs, rhs, pieces, table=MOBIUS_S_AINV, scale=1.0, w=1.0, M5=-1.0, b5=1.0, c5=0.0, nrhs=1, vec_stride=0, mask=1,
                       stream=None):
    """qmg_mobius_inv5's status, unchecked: lhs_p = scale S rhs_p on the parities P_CLOVER_E / P_CLOVER_O name; S = A^-1 or A^-1 B."""
    mass, scale = complex(mass), complex(scale)
    return lib().qmg_mobius_inv5(dtype, C.byref(desc), Ls, C.c_double(mass.real), C.c_double(mass.imag), C.c_double(w), C.c_double(M5), C.c_double(b5),
                                 C.c_double(c5), _vp(lhs), _vp(rhs), C.c_uint(pieces), int(table), C.c_double(scale.real), C.c_double(scale.imag), nrhs,
                                 C.c_size_t(vec_stride), C.c_uint(mask), C.c_void_p(stream))


mobius_inv5 = _checked(mobius_inv5_status, "qmg_mobius_inv5")


def mobius_hops_inv5_status(dtype, desc, gauge, Ls, mass, lhs, rhs, pieces, table=MOBIUS_S_AINV, source=MOBIUS_R_B, scale=1.0, flags=0, w=1.0, M5=-1.0, b5=1.0,
                            c5=0.0, nrhs=1, vec_stride=0, mask=1, stream=None):
    """qmg_mobius_hops_inv5's status, unchecked: lhs_p (+)= scale S H_{p,1-p} (R [Gamma5] rhs_{1-p})."""
    mass, scale = complex(mass), complex(scale)
    return lib().qmg_mobius_hops_inv5(dtype, C.byref(desc), _vp(gauge), Ls, C.c_double(mass.real), C.c_double(mass.imag), C.c_double(w), C.c_double(M5),
                                      C.c_double(b5), C.c_double(c5), _vp(lhs), _vp(rhs), C.c_uint(pieces), int(table), int(source), C.c_double(scale.real),
                                      C.c_double(scale.imag), C.c_uint(flags), nrhs, C.c_size_t(vec_stride), C.c_uint(mask), C.c_void_p(stream))


mobius_hops_inv5 = _checked(mobius_hops_inv5_status, "qmg_mobius_hops_inv5")


def mobius_schur_apply_status(dtype, desc, gauge, Ls, mass, lhs, rhs, tmp, parity=0, op=0, w=1.0, M5=-1.0, b5=1.0, c5=0.0, nrhs=1, vec_stride=0, mask=1,
                              stream=None):
    """qmg_mobius_schur_apply's status, unchecked: lhs_p = M_p rhs_p (op 0) or M_p^dagger rhs_p (op 1), two launches."""
    mass = complex(mass)
    return lib().qmg_mobius_schur_apply(dtype, C.byref(desc), _vp(gauge), Ls, C.c_double(mass.real), C.c_double(mass.imag), C.c_double(w), C.c_double(M5),
                                        C.c_double(b5), C.c_double(c5), _vp(lhs), _vp(rhs), _vp(tmp), int(parity), int(op), nrhs, C.c_size_t(vec_stride),
                                        C.c_uint(mask), C.c_void_p(stream))


mobius_schur_apply = _checked(mobius_schur_apply_status, "qmg_mobius_schur_apply")


def mobius_eo_plan(dtype, dims, Ls, kernel, pieces, table=MOBIUS_S_AINV, source=MOBIUS_R_ONE, n_active=1, inplace=False):
    """What the even-odd Moebius entries launch (qmg_mobius_eo_plan; host only): (family, lps, block, gx, gy, flags, lds, nk)."""
    out = (C.c_int * MOBIUS_EO_PLAN_INTS)()
    check(lib().qmg_mobius_eo_plan(dtype, dims[0], dims[1], Ls, int(kernel), C.c_uint(pieces), int(table), int(source), n_active, int(inplace), out,
                                   MOBIUS_EO_PLAN_INTS), "qmg_mobius_eo_plan")
    return tuple(out)


# ---- domain-wall measurements: wall source, wall / midpoint projection, slice norms (csrc/qmg_dwf_meas.hip)
# the `kernel` argument and the families of qmg_dwf_meas_plan (include/qmg_hip.h)
DMK_SOURCE, DMK_PROJECT_WALL, DMK_PROJECT_MID, DMK_NORMS = range(4)
DMF_UNSUPPORTED, DMF_SOURCE, DMF_PROJECT, DMF_INVALID, DMF_NORMS = range(5)
DWF_MEAS_PLAN_INTS = 8


def dwf_wall_source_status(dtype, dims, Ls, psi5, eta4, nsys=1, stride5=0, stride4=0, stream=None):
    """qmg_dwf_wall_source's status, unchecked: psi5(x; 0, 0) = eta4(x, 0), psi5(x; Ls-1, 1) = eta4(x, 1), zero elsewhere."""
    return lib().qmg_dwf_wall_source(dtype, dims[0], dims[1], Ls, _vp(psi5), _vp(eta4), nsys, C.c_size_t(stride5), C.c_size_t(stride4), C.c_void_p(stream))


dwf_wall_source = _checked(dwf_wall_source_status, "qmg_dwf_wall_source")


def dwf_wall_project_status(dtype, dims, Ls, q4, psi5, which=0, nsys=1, stride4=0, stride5=0, stream=None):
    """qmg_dwf_wall_project's status, unchecked: which = 0 the walls (Ls-1, 0), (0, 1); 1 the midpoint (Ls/2-1, 0), (Ls/2, 1)."""
    return lib().qmg_dwf_wall_project(dtype, dims[0], dims[1], Ls, _vp(q4), _vp(psi5), which, nsys, C.c_size_t(stride4), C.c_size_t(stride5), C.c_void_p(stream))


dwf_wall_project = _checked(dwf_wall_project_status, "qmg_dwf_wall_project")


def dwf_slice_norms_status(dtype, dims, Ls, psi5, nsys=1, stride5=0, out_dev=None, out_host=None, stream=None):
    """qmg_dwf_slice_norms's status, unchecked; out_host: a float64 array of nsys * Ly * 2 Ls numbers or None."""
    host = None if out_host is None else out_host.ctypes.data_as(C.POINTER(C.c_double))
    return lib().qmg_dwf_slice_norms(dtype, dims[0], dims[1], Ls, _vp(psi5), nsys, C.c_size_t(stride5), C.cast(_vp(out_dev), C.POINTER(C.c_double)), host,
                                     C.c_void_p(stream))


def dwf_slice_norms(dtype, dims, Ls, psi5, nsys=1, stride5=0, out_dev=None, stream=None):
    """N[sys, y, s, sigma] = sum_x |psi5(x, y; s, sigma)|^2 on the host (and in out_dev where given)."""
    out = np.empty((nsys, dims[1], Ls, 2), dtype=np.float64)
    check(dwf_slice_norms_status(dtype, dims, Ls, psi5, nsys, stride5, out_dev, out, stream), "qmg_dwf_slice_norms")
    return out


def dwf_meas_plan(dtype, dims, Ls, kernel, nsys=1):
    """What the measurement entries launch (qmg_dwf_meas_plan; host only): (family, lps, block, gx, gy, pbr, lds, nk)."""
    out = (C.c_int * DWF_MEAS_PLAN_INTS)()
    check(lib().qmg_dwf_meas_plan(dtype, dims[0], dims[1], Ls, kernel, nsys, out, DWF_MEAS_PLAN_INTS), "qmg_dwf_meas_plan")
    return tuple(out)


# ---- flavour-singlet loops from diluted Z4 noise (csrc/qmg_singlet.hip)
# the families of qmg_singlet_plan (include/qmg_hip.h); `dil` below is the dilution (nt, spin, eo)
SGF_INVALID, SGF_ROWS, SGF_NONE = range(3)
SINGLET_PLAN_INTS = 12


def noise_z4(eta, n, seed, stream=None):
    check(lib().qmg_noise_z4(_vp(eta), C.c_size_t(n), C.c_ulonglong(seed), C.c_void_p(stream)), "qmg_noise_z4")


def noise_dilute_batch_status(dtype, out, dims, nc, dil, first_class, seed, nrhs=1, stride=0, mask=None, stream=None):
    """qmg_noise_dilute_batch's status, unchecked: system k of the batch becomes the diluted source of class first_class + k."""
    mask = (1 << min(max(nrhs, 0), 32)) - 1 if mask is None else mask
    return lib().qmg_noise_dilute_batch(dtype, _vp(out), dims[0], dims[1], nc, dil[0], dil[1], dil[2], first_class, C.c_ulonglong(seed), nrhs,
                                        C.c_size_t(stride), C.c_uint(mask), C.c_void_p(stream))


noise_dilute_batch = _checked(noise_dilute_batch_status, "qmg_noise_dilute_batch")


def loops_timeslice_batch_status(dtype, psi, dims, nc, dil, first_class, seed, g5_mode, nrhs=1, stride=0, mask=None, out_dev=None, out_host=None, stream=None):
    """qmg_loops_timeslice_batch's status, unchecked; out_host: a float64 array of nrhs * Ly * 5 numbers or None."""
    mask = (1 << min(max(nrhs, 0), 32)) - 1 if mask is None else mask
    host = None if out_host is None else out_host.ctypes.data_as(C.POINTER(C.c_double))
    return lib().qmg_loops_timeslice_batch(dtype, _vp(psi), dims[0], dims[1], nc, dil[0], dil[1], dil[2], first_class, C.c_ulonglong(seed), g5_mode, nrhs,
                                           C.c_size_t(stride), C.c_uint(mask), C.cast(_vp(out_dev), C.POINTER(C.c_double)), host, C.c_void_p(stream))


def loops_timeslice_batch(dtype, psi, dims, nc, dil, first_class, seed, g5_mode, nrhs=1, stride=0, mask=None, out_dev=None, fill=0.0, stream=None):
    """out[k, y] = (Re S, Im S, Re P, Im P, N) of system k on the host (and in out_dev where given); entries of frozen systems keep `fill`."""
    out = np.full((nrhs, dims[1], 5), fill, dtype=np.float64)
    check(loops_timeslice_batch_status(dtype, psi, dims, nc, dil, first_class, seed, g5_mode, nrhs, stride, mask, out_dev, out, stream), "qmg_loops_timeslice_batch")
    return out


def singlet_plan_status(dims, nc, dil, first_class=0, nrhs=1, mask=None):
    """(status, (family, block, gx, gy, walk, lds, doubles, dgx, dgy, dwalk, nk, classes)) of qmg_singlet_plan; host only."""
    mask = (1 << min(max(nrhs, 0), 32)) - 1 if mask is None else mask
    out = (C.c_int * SINGLET_PLAN_INTS)()
    rc = lib().qmg_singlet_plan(dims[0], dims[1], nc, dil[0], dil[1], dil[2], first_class, nrhs, C.c_uint(mask), out, SINGLET_PLAN_INTS)
    return rc, tuple(out)


def singlet_plan(*args, **kw):
    rc, plan = singlet_plan_status(*args, **kw)
    check(rc, "qmg_singlet_plan")
    return plan


def comm_set_distributed_reductions(on):
    check(lib().qmg_comm_set_distributed_reductions(1 if on else 0), "qmg_comm_set_distributed_reductions")


def comm_all_ok(ok):
    out = C.c_int(0)
    check(lib().qmg_comm_all_ok(1 if ok else 0, C.byref(out)), "qmg_comm_all_ok")
    return bool(out.value)


def u1_heatbath_noncompact(phase, Lx, Ly, beta, n_update, seed, first_sweep=0, stream=None):
    check(lib().qmg_u1_heatbath_noncompact(_vp(phase), Lx, Ly, C.c_double(beta), n_update, C.c_ulonglong(seed), C.c_ulonglong(first_sweep), C.c_void_p(stream)), "qmg_u1_heatbath_noncompact")


def u1_phase_to_gauge(gauge, phase, n, stream=None):
    check(lib().qmg_u1_phase_to_gauge(_vp(gauge), _vp(phase), C.c_size_t(n), C.c_void_p(stream)), "qmg_u1_phase_to_gauge")


def u1_gauge_to_phase(phase, gauge, n, stream=None):
    check(lib().qmg_u1_gauge_to_phase(_vp(phase), _vp(gauge), C.c_size_t(n), C.c_void_p(stream)), "qmg_u1_gauge_to_phase")


def u1_plaquette(gauge, Lx, Ly, stream=None):
    """(average plaquette, topological charge)"""
    out = (C.c_double * 3)()
    check(lib().qmg_u1_plaquette(_vp(gauge), Lx, Ly, out, C.c_void_p(stream)), "qmg_u1_plaquette")
    return complex(out[0], out[1]), out[2]


def u1_noncompact_action(phase, Lx, Ly, beta, stream=None):
    out = C.c_double()
    check(lib().qmg_u1_noncompact_action(_vp(phase), Lx, Ly, C.c_double(beta), C.byref(out), C.c_void_p(stream)), "qmg_u1_noncompact_action")
    return out.value


def u1_hot_gauge(gauge, Lx, Ly, seed, stream=None):
    check(lib().qmg_u1_hot_gauge(_vp(gauge), Lx, Ly, C.c_ulonglong(seed), C.c_void_p(stream)), "qmg_u1_hot_gauge")


def u1_gauss_gauge(gauge, Lx, Ly, beta, seed, stream=None):
    check(lib().qmg_u1_gauss_gauge(_vp(gauge), Lx, Ly, C.c_double(beta), C.c_ulonglong(seed), C.c_void_p(stream)), "qmg_u1_gauss_gauge")


def u1_random_trans(trans, Lx, Ly, seed, stream=None):
    check(lib().qmg_u1_random_trans(_vp(trans), Lx, Ly, C.c_ulonglong(seed), C.c_void_p(stream)), "qmg_u1_random_trans")


def u1_gauge_transform(gauge, trans, Lx, Ly, stream=None):
    check(lib().qmg_u1_gauge_transform(_vp(gauge), _vp(trans), Lx, Ly, C.c_void_p(stream)), "qmg_u1_gauge_transform")


def u1_ape_smear(smeared, gauge, Lx, Ly, alpha, n_iter, stream=None):
    check(lib().qmg_u1_ape_smear(_vp(smeared), _vp(gauge), Lx, Ly, C.c_double(alpha), n_iter, C.c_void_p(stream)), "qmg_u1_ape_smear")


def u1_instanton(gauge, Lx, Ly, Q, x0, y0, stream=None):
    check(lib().qmg_u1_instanton(_vp(gauge), Lx, Ly, C.c_double(Q), x0, y0, C.c_void_p(stream)), "qmg_u1_instanton")


def u1_noncompact_instanton(phase, Lx, Ly, Q, stream=None):
    check(lib().qmg_u1_noncompact_instanton(_vp(phase), Lx, Ly, C.c_double(Q), C.c_void_p(stream)), "qmg_u1_noncompact_instanton")


HMC_GAUGE_ONLY = 1   # flags of hmc_momentum_update


def hmc_momentum_update(pi, gauge, X, Y, Lx, Ly, beta, dt, flags=0, stream=None):
    """pi -= dt (gauge force + two-flavour Wilson force); flags = HMC_GAUGE_ONLY drops the fermions (X, Y may be None)"""
    check(lib().qmg_hmc_momentum_update(_vp(pi), _vp(gauge), _vp(X), _vp(Y), Lx, Ly, C.c_double(beta), C.c_double(dt), C.c_uint(flags), C.c_void_p(stream)),
          "qmg_hmc_momentum_update")


def hmc_momentum_update_poles(pi, gauge, X, Y, weights, Lx, Ly, beta, dt, flags=0, stream=None, n_poles=None):
    """pi -= dt (gauge force + sum_j weights[j] Ff(X[j], Y[j])) in one pass; X, Y: sequences of device spinors, weights: floats (None: null)"""
    n = n_poles if n_poles is not None else (len(weights) if weights is not None else 0)
    xs = (C.c_void_p * max(len(X), 1))(*[_vp(x).value for x in X]) if X is not None else None
    ys = (C.c_void_p * max(len(Y), 1))(*[_vp(y).value for y in Y]) if Y is not None else None
    ws = (C.c_double * max(len(weights), 1))(*[float(w) for w in weights]) if weights is not None else None
    check(lib().qmg_hmc_momentum_update_poles(_vp(pi), _vp(gauge), xs, ys, ws, n, Lx, Ly, C.c_double(beta), C.c_double(dt), C.c_uint(flags), C.c_void_p(stream)),
          "qmg_hmc_momentum_update_poles")


def hmc_momentum_update_staggered(pi, gauge, W, weights, Lx, Ly, beta, dt, flags=0, stream=None, n_poles=None):
    """pi -= dt (gauge force + sum_j weights[j] Fs(W[j])), Fs the staggered force; W: a sequence of device nc = 1 vectors, weights: floats (None: null)"""
    n = n_poles if n_poles is not None else (len(weights) if weights is not None else 0)
    ws_ = (C.c_void_p * max(len(W), 1))(*[_vp(w).value for w in W]) if W is not None else None
    ws = (C.c_double * max(len(weights), 1))(*[float(w) for w in weights]) if weights is not None else None
    check(lib().qmg_hmc_momentum_update_staggered(_vp(pi), _vp(gauge), ws_, ws, n, Lx, Ly, C.c_double(beta), C.c_double(dt), C.c_uint(flags), C.c_void_p(stream)),
          "qmg_hmc_momentum_update_staggered")


HMC_DWF_G5_Y = 2   # flag of hmc_momentum_update_dwf: every Y[j] is read as Gamma5 Y[j]
# the families of qmg_hmc_dwf_plan (include/qmg_hip.h)
HDF_UNSUPPORTED, HDF_FUSED, HDF_GAUGE, HDF_INVALID = range(4)
HMC_DWF_PLAN_INTS = 8


def hmc_momentum_update_dwf_status(pi, gauge, X, Y, weights, Ls, Lx, Ly, beta, dt, flags=0, stream=None, n_pairs=None):
    """qmg_hmc_momentum_update_dwf's status, unchecked."""
    n = n_pairs if n_pairs is not None else (len(weights) if weights is not None else 0)
    xs = (C.c_void_p * max(len(X), 1))(*[_vp(x).value for x in X]) if X is not None else None
    ys = (C.c_void_p * max(len(Y), 1))(*[_vp(y).value for y in Y]) if Y is not None else None
    ws = (C.c_double * max(len(weights), 1))(*[float(w) for w in weights]) if weights is not None else None
    return lib().qmg_hmc_momentum_update_dwf(_vp(pi), _vp(gauge), xs, ys, ws, n, Ls, Lx, Ly, C.c_double(beta), C.c_double(dt), C.c_uint(flags), C.c_void_p(stream))


# pi -= dt (gauge force + sum_j weights[j] sum_s Ff(X[j](.; s), Y[j](.; s))) in one pass; X, Y: sequences of device nc = 2 Ls vectors
hmc_momentum_update_dwf = _checked(hmc_momentum_update_dwf_status, "qmg_hmc_momentum_update_dwf")


def hmc_dwf_plan_status(dims, Ls, n_pairs, flags=0):
    """(status, plan) of qmg_hmc_dwf_plan (host only): plan = (family, lps, block, gx, gy, lds, launches, pairs per launch)."""
    out = (C.c_int * HMC_DWF_PLAN_INTS)()
    rc = lib().qmg_hmc_dwf_plan(dims[0], dims[1], Ls, n_pairs, C.c_uint(flags), out, HMC_DWF_PLAN_INTS)
    return rc, tuple(out)


def hmc_dwf_plan(dims, Ls, n_pairs, flags=0):
    rc, plan = hmc_dwf_plan_status(dims, Ls, n_pairs, flags)
    check(rc, "qmg_hmc_dwf_plan")
    return plan


def hmc_link_update(theta, gauge, pi, n, dt, stream=None):
    """theta += dt pi ; gauge = exp(i theta)"""
    check(lib().qmg_hmc_link_update(_vp(theta), _vp(gauge), _vp(pi), C.c_size_t(n), C.c_double(dt), C.c_void_p(stream)), "qmg_hmc_link_update")


def hmc_gauge_step(theta, gauge_out, gauge_in, pi, Lx, Ly, beta, dt_kick, dt_drift, stream=None):
    """pi -= dt_kick (gauge force on gauge_in) ; theta += dt_drift pi ; gauge_out = exp(i theta), one launch; gauge_out is not gauge_in"""
    check(lib().qmg_hmc_gauge_step(_vp(theta), _vp(gauge_out), _vp(gauge_in), _vp(pi), Lx, Ly, C.c_double(beta), C.c_double(dt_kick), C.c_double(dt_drift),
                                   C.c_void_p(stream)), "qmg_hmc_gauge_step")


def hmc_momentum_refresh(pi, n, seed, trajectory, stream=None):
    check(lib().qmg_hmc_momentum_refresh(_vp(pi), C.c_size_t(n), C.c_ulonglong(seed), C.c_ulonglong(trajectory), C.c_void_p(stream)), "qmg_hmc_momentum_refresh")


def hmc_stream_seed(seed, trajectory, field):
    f = lib().qmg_hmc_stream_seed
    f.restype = C.c_ulonglong
    return f(C.c_ulonglong(seed), C.c_ulonglong(trajectory), field)


def u1_stout_smear(levels, gauge, Lx, Ly, rho, n_levels, stream=None):
    """levels[k] = stout level k + 1 of `gauge` (n_levels fields of 2 Lx Ly links, back to back); level 0 is `gauge`, which is not copied"""
    check(lib().qmg_u1_stout_smear(_vp(levels), _vp(gauge), Lx, Ly, C.c_double(rho), n_levels, C.c_void_p(stream)), "qmg_u1_stout_smear")


def hmc_fermion_force(F, gauge, X, Y, weights, Lx, Ly, stream=None, n_poles=None):
    """F = sum_j weights[j] Ff(X[j], Y[j]) on the links `gauge`, written to the link field F; the pole lists of hmc_momentum_update_poles"""
    n = n_poles if n_poles is not None else (len(weights) if weights is not None else 0)
    xs = (C.c_void_p * max(len(X), 1))(*[_vp(x).value for x in X]) if X is not None else None
    ys = (C.c_void_p * max(len(Y), 1))(*[_vp(y).value for y in Y]) if Y is not None else None
    ws = (C.c_double * max(len(weights), 1))(*[float(w) for w in weights]) if weights is not None else None
    check(lib().qmg_hmc_fermion_force(_vp(F), _vp(gauge), xs, ys, ws, n, Lx, Ly, C.c_void_p(stream)), "qmg_hmc_fermion_force")


def u1_stout_force_level(F_out, F_in, gauge_k, Lx, Ly, rho, stream=None):
    """F_out = J_k F_in = F_in - rho C^T [cos P . (C F_in)] on the links of level k; F_out is not F_in"""
    check(lib().qmg_u1_stout_force_level(_vp(F_out), _vp(F_in), _vp(gauge_k), Lx, Ly, C.c_double(rho), C.c_void_p(stream)), "qmg_u1_stout_force_level")


def hmc_momentum_update_stout(pi, gauge, F_in, Lx, Ly, beta, rho, dt, stream=None):
    """pi -= dt (gauge force + J_0 F_in) in one pass over the thin links"""
    check(lib().qmg_hmc_momentum_update_stout(_vp(pi), _vp(gauge), _vp(F_in), Lx, Ly, C.c_double(beta), C.c_double(rho), C.c_double(dt), C.c_void_p(stream)),
          "qmg_hmc_momentum_update_stout")


def u1_flow_stage(theta, acc, gauge_out, gauge_in, Lx, Ly, eps, stage, stream=None):
    """one Runge-Kutta stage (1, 2, 3) of the Wilson flow: acc and theta in place, gauge_out = exp(i theta); neighbours from gauge_in"""
    check(lib().qmg_u1_flow_stage(_vp(theta), _vp(acc), _vp(gauge_out), _vp(gauge_in), Lx, Ly, C.c_double(eps), stage, C.c_void_p(stream)), "qmg_u1_flow_stage")


def u1_flow(theta, gauge, Lx, Ly, eps, n_steps, stream=None):
    """n_steps third-order Runge-Kutta steps of the Wilson flow; gauge = exp(i theta) on entry and on return"""
    check(lib().qmg_u1_flow(_vp(theta), _vp(gauge), Lx, Ly, C.c_double(eps), n_steps, C.c_void_p(stream)), "qmg_u1_flow")


def u1_wilson_loops(gauge, Lx, Ly, r_max, t_max, stream=None):
    """W[R - 1, T - 1]: the lattice average of the R x T Wilson loop, a complex (r_max, t_max) array"""
    out = np.full(2 * r_max * t_max, np.nan)
    check(lib().qmg_u1_wilson_loops(_vp(gauge), Lx, Ly, r_max, t_max, out.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(stream)), "qmg_u1_wilson_loops")
    return (out[0::2] + 1j * out[1::2]).reshape(r_max, t_max)


def u1_polyakov(gauge, Lx, Ly, stream=None):
    """(Polyakov loop in x averaged over y, Polyakov loop in y averaged over x)"""
    out = (C.c_double * 4)()
    check(lib().qmg_u1_polyakov(_vp(gauge), Lx, Ly, out, C.c_void_p(stream)), "qmg_u1_polyakov")
    return complex(out[0], out[1]), complex(out[2], out[3])


def set_tuning(key, value):
    check(lib().qmg_set_tuning(key.encode(), int(value)), "qmg_set_tuning")


class Timer:
    """HIP-event timing on the stream the kernels are launched on (NULL stream by default)."""

    def __init__(self):
        self.a, self.b = C.c_void_p(), C.c_void_p()
        check(lib().qmg_event_create(C.byref(self.a)))
        check(lib().qmg_event_create(C.byref(self.b)))

    def start(self, stream=None):
        check(lib().qmg_event_record(self.a, C.c_void_p(stream)))

    def stop_ms(self, stream=None):
        check(lib().qmg_event_record(self.b, C.c_void_p(stream)))
        ms = C.c_float()
        check(lib().qmg_event_elapsed_ms(self.a, self.b, C.byref(ms)))
        return ms.value
