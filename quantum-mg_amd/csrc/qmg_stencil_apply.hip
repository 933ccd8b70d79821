// qmg_stencil_apply.hip -- the host surface of the stencil apply: the C entry points, the dispatcher that routes a request to one kernel
// family (qmg_stencil.hip: A / A2; qmg_stencil_gen.hip: B; qmg_stencil_gen32.hip: B32; qmg_stencil_mfma.hip: C; qmg_site.hip: S) and the 1 x 1 lattice.

#include "qmg_stencil_common.h"

namespace qmg {
int g_stencil_site = 3;    // tuning knob: nc 2 through the site kernel (qmg_site.hip): bit 0 fp64 where it is faster, bit 1 fp32, bit 2 fp64 always
int g_stencil_pair = 2;    // tuning knob: 0 = one site per lane group (kernel A), 2 = fp64 paired parities x 2 rows where Ly is even (kernel A2)
}  // namespace qmg

using namespace qmg;

// The 1 x 1 lattice (lattice.h:77,201; stencil_2d.h:870-888, "this corner case is annoying").  Every half-volume loop of the reference runs
// volume / 2 = 0 times there -- the clover sweeps, the cshifts and the hopping cMATxpy's touch nothing -- so apply_M is its shift term alone:
// the one site counts as even, lhs[c] += (shift + eo_shift +- dof_shift) rhs[c] (dof_shift only for even nc, + on the first half).
// The zero pieces clear the site.  One tiny launch; plain applies only.
template <typename T>
__global__ void k_stencil_volume1(void* lhs_, const void* rhs_, int nc, int nrhs, long stride, const unsigned char* ridx_dev_unused, StencilArgs a, int zero, int shift_on) {
  typedef typename CStore<T>::type ct;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nc * nrhs) return;
  const int k = i / nc, c = i - k * nc;
  const long o = (long)system_index(a, k) * stride + c;
  ct* lhs = reinterpret_cast<ct*>(lhs_);
  const ct* rhs = reinterpret_cast<const ct*>(rhs_);
  cplx v = cmake(0.0, 0.0);
  if (!zero) { const ct l = lhs[o]; v = cmake((double)l.x, (double)l.y); }
  if (shift_on) {
    const double dg = (nc % 2 == 0) ? ((c < nc / 2) ? 1.0 : -1.0) : 0.0;
    const cplx sh = cmake(a.shift[0] + a.eo_shift[0] + dg * a.dof_shift[0], a.shift[1] + a.eo_shift[1] + dg * a.dof_shift[1]);
    const ct r = rhs[o];
    cmac(v, sh, cmake((double)r.x, (double)r.y));
  }
  ct w; w.x = (T)v.x; w.y = (T)v.y;
  lhs[o] = w;
}

// what every route copies from the request: the systems of the launch and the operator's shifts
static void fill_systems_and_shifts(StencilArgs& a, const StencilRequest& q) {
  a.use_idx = q.ridx ? 1 : 0;
  for (int k = 0; k < 16; k++) a.ridx[k] = q.ridx ? q.ridx[k < q.nrhs ? k : 0] : (unsigned char)k;
  for (int i = 0; i < 2; i++) { a.shift[i] = q.d->shift[i]; a.eo_shift[i] = q.d->eo_shift[i]; a.dof_shift[i] = q.d->dof_shift[i]; }
}

static int stencil_apply_volume1(const StencilRequest& q) {
  const qmg_stencil_desc* d = q.d;
  if (d->nc < 1 || q.nrhs > 16 || (q.nrhs > 1 && q.vec_stride < (size_t)d->nc)) return QMG_ERR_INVALID;
  StencilArgs a;
  memset(&a, 0, sizeof(a));
  fill_systems_and_shifts(a, q);
  const int zero = (q.pieces & (QMG_P_ZERO_E | QMG_P_ZERO_O)) ? 1 : 0, shift_on = (q.pieces & QMG_P_SHIFT_E) ? 1 : 0;
  if (!zero && !shift_on) return QMG_SUCCESS;
  const int n = d->nc * q.nrhs;
  if (q.vec32) k_stencil_volume1<float><<<(n + 63) / 64, 64, 0, as_stream(q.stream)>>>(q.lhs, q.rhs, d->nc, q.nrhs, (long)q.vec_stride, nullptr, a, zero, shift_on);
  else k_stencil_volume1<double><<<(n + 63) / 64, 64, 0, as_stream(q.stream)>>>(q.lhs, q.rhs, d->nc, q.nrhs, (long)q.vec_stride, nullptr, a, zero, shift_on);
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

// The dispatcher: validation, then the kernel families in route order -- the first one that serves the request takes it.
int qmg::stencil_apply(const StencilRequest& q) {
  const qmg_stencil_desc* d = q.d;
  const bool mat32 = q.mat != MatStorage::fp64, mat16 = q.mat == MatStorage::fp16, vec32 = q.vec32;   // (mat32: narrow-stored matrices, either width)
  const SlabHalo* slab = q.slab;
  const int nrhs = q.nrhs;
  if (!d || !q.lhs || !q.rhs || nrhs < 1) return QMG_ERR_INVALID;
  if (d->Lx == 1 && d->Ly == 1) {
    if (slab || q.norms_dev || q.epi) return QMG_ERR_UNSUPPORTED;
    return stencil_apply_volume1(q);
  }
  if (!valid_lattice(d->Lx, d->Ly) || d->nc < 1) return QMG_ERR_INVALID;
  const int nc = d->nc;
  if (nrhs > 1 && q.vec_stride < (size_t)d->Lx * d->Ly * nc) return QMG_ERR_INVALID;

  if (vec32 && !mat32) return QMG_ERR_UNSUPPORTED;   // fp32 vectors come with fp32 matrices (qmg_stencil_apply_t)
  // nc = 2 in one storage precision: the site kernel (kernel S, qmg_site.hip)
  const bool one_precision = !mat16 && mat32 == vec32;
  if (slab && nc == 2 && !one_precision) return QMG_ERR_UNSUPPORTED;   // slabs at nc = 2: kernel S, matrices and vectors in ONE precision (or its own 16-bit form)
  if (q.epi && (q.norms_dev || nrhs != 1)) return QMG_ERR_UNSUPPORTED;   // the epilogue is served for ONE system per launch, by kernels B / B32
  hipStream_t st = as_stream(q.stream);
  if (nc == 2 && one_precision && nrhs <= 16 && !q.norms_dev && !q.epi && (slab || (vec32 ? (g_stencil_site & 2) : (g_stencil_site & 5)))) {
    const int rc = site_kernel_apply(vec32 ? 1 : 2, d, q.lhs, q.rhs, q.pieces, nrhs, (long)q.vec_stride, q.ridx, st, !slab && !(g_stencil_site & 4), slab);
    if (rc != SITE_DECLINED) return rc;
  }

  StencilArgs a;
  a.clover = (const cplx*)d->clover;
  a.hopping = (const cplx*)d->hopping;
  a.lhs = q.lhs;
  a.rhs = q.rhs;
  a.vec32 = vec32;
  a.hr = d->Lx / 2;
  a.Ly = d->Ly;
  a.half_vol = (long)a.hr * d->Ly;
  a.size_cm = 2 * a.half_vol * nc * nc;
  a.pieces = q.pieces;
  a.nrhs = nrhs;
  a.vec_stride = (long)q.vec_stride;
  a.mat32 = mat32;
  a.mat16 = mat16;
  a.halo_lo = slab ? slab->lo : nullptr;
  a.halo_hi = slab ? slab->hi : nullptr;
  a.halo_stride = slab ? slab->stride : 0;
  a.norm_part = nullptr;
  a.epi = no_epilogue();
  fill_systems_and_shifts(a, q);

  // which parity halves have any work
  const unsigned even_bits = QMG_P_CLOVER_E | QMG_P_EO | QMG_P_SHIFT_E | QMG_P_ZERO_E;
  const unsigned odd_bits = QMG_P_CLOVER_O | QMG_P_OE | QMG_P_SHIFT_O | QMG_P_ZERO_O;
  const bool ev = q.pieces & even_bits, od = q.pieces & odd_bits;
  if (!ev && !od) return QMG_SUCCESS;
  a.par_first = ev ? 0 : 1;
  a.par_count = (ev && od) ? 2 : 1;
  a.nrows = d->Ly * a.par_count;
  const bool fine = nc == 1 || nc == 2 || nc == 4;   // kernels A / A2

  if (q.norms_dev) {
    // apply + |lhs_k|^2 in one pass: kernel A2 in fp64, nc = 1 or 2, every site written
    if (vec32 || mat32 || slab || q.ridx || !(nc == 1 || nc == 2) || a.par_count != 2 || q.lhs == q.rhs || nrhs > 16) return QMG_ERR_UNSUPPORTED;
    return launch_stencil_norm(a, nc, q.norms_dev, st);
  }

  if (q.epi) {
    // out = other_scale other + acc_scale acc and the MR dots, in kernels B / B32 (any nc the generic kernels serve); the processed
    // parities must be overwritten (an accumulate into lhs and an `other` term at once has no single meaning)
    if (fine) return QMG_ERR_UNSUPPORTED;   // kernels A / S / W: qmg_wilson_*_direct has its own epilogue, the rest falls back
    if ((ev && !(q.pieces & QMG_P_ZERO_E)) || (od && !(q.pieces & QMG_P_ZERO_O))) return QMG_ERR_INVALID;
    if (q.lhs == q.rhs || q.epi->other == q.lhs || q.epi->dotv == q.lhs) return QMG_ERR_INVALID;
    a.epi.on = 1;
    a.epi.other = q.epi->other; a.epi.other_scale = q.epi->other_scale; a.epi.acc_scale = q.epi->acc_scale;
    a.epi.dotv = q.epi->dotv;
    // partials: one per wavefront of the launch; the launchers of kernels B / B32 fix the grid and ask for them
  }

  // fp32: the one-site-per-lane-group kernel is the faster one (4096^2 Wilson: 0.573 ms against 0.592 ms for the paired
  // kernel, profiles/r02_kernel_rooflines.json: half the bytes per site leave the paired kernel's longer dependent chain
  // exposed), so the paired kernel serves fp64 only
  if (fine && a.par_count == 2 && g_stencil_pair && !vec32 && q.lhs != q.rhs && !slab) return launch_stencil_pair(a, nc, st);

  if (fine && !slab) return launch_stencil_elem(a, nc, st);

  // several right-hand sides against one matrix read: kernel C (f64 MFMA) from 4 systems up -- measured 512^2 nc = 24, 8 rhs:
  // 2.84 ms against 4.84 ms for the vector-FMA kernel B, which tops out near 10 TFLOP/s on LDS traffic; with 2-3 systems
  // kernel B's shared tile wins (nc = 8, 1024^2, 3 rhs: 1.06 vs 1.39 ms) and it serves every other nc
  // (nc <= 16: kernel B with one 4-accumulator pass still wins at exactly 4 systems -- nc = 8, 1024^2: 1.21 vs 1.52 ms;
  //  nc = 16, 512^2: 0.98 vs 1.08 ms -- so there the matrix cores take over from 5)
  if (nrhs >= (nc <= 16 ? 5 : 4) && g_stencil_mfma && (nc == 8 || nc == 12 || nc == 16 || nc == 24 || nc == 32)) return launch_stencil_mfma(a, nc, !slab, st);

  if (nc > BLOCK) return QMG_ERR_UNSUPPORTED;
  if (mat32 && !(nc & 1) && !(slab && nc <= 4)) {   // (a slab's fp32 applies at nc = 4 keep kernel B's widening loads)
    const int rc = launch_stencil_gen32(a, nc, st);
    if (rc != ROUTE_DECLINED) return rc;
  }
  if (mat16) return QMG_ERR_UNSUPPORTED;   // complex<half> matrices are served by kernels B32 / C only (nc a multiple of 4)
  return launch_stencil_gen(a, nc, st);
}

// Generic-nc slab apply (csrc/qmg_site.hip holds the C entry qmg_stencil_apply_slab and serves nc = 2 itself): kernels B / B32 / C with the
// right-hand side's rows -1 / Ly from the halo buffers.  mat32: 0 fp64 matrices, 1 complex<float>, 2 complex<half>; vec32: complex<float> vectors.
static MatStorage storage_of(int mat32) { return mat32 == 2 ? MatStorage::fp16 : mat32 ? MatStorage::fp32 : MatStorage::fp64; }
int qmg::generic_slab_apply(const qmg_stencil_desc* d, void* lhs, const void* rhs, unsigned pieces, int n, long vec_stride, const unsigned char* ridx,
                            hipStream_t st, const SlabHalo* slab, int mat32, int vec32) {
  StencilRequest q = {d, lhs, rhs, pieces, n, (size_t)vec_stride, ridx, (void*)st, storage_of(mat32), vec32 != 0, slab};
  return stencil_apply(q);
}

// A masked batch (only the right-hand sides whose bit is set in `mask` are read or written; at most 16 per call) in q's storage:
// an empty mask is a success with nothing launched, a full mask runs without an index table (the kernels' direct path).
static int stencil_apply_masked(StencilRequest q, unsigned mask) {
  if (q.nrhs < 1 || q.nrhs > 16) return QMG_ERR_INVALID;
  const BatchIdx b = expand_mask(mask, q.nrhs);
  if (b.n == 0) return QMG_SUCCESS;
  if (b.n < q.nrhs) { q.ridx = b.id; q.nrhs = b.n; }
  return stencil_apply(q);
}

extern "C" int qmg_stencil_apply(const qmg_stencil_desc* d, void* lhs, const void* rhs, unsigned pieces,
                                 int nrhs, size_t vec_stride, void* stream) {
  StencilRequest q = {d, lhs, rhs, pieces, nrhs, vec_stride, nullptr, stream};
  return stencil_apply(q);
}

// Masked batch: only the right-hand sides whose bit is set in `mask` are read or written (a lock-step batched solver
// freezes the systems that have converged).  At most 16 right-hand sides per call.
extern "C" int qmg_stencil_apply_batch(const qmg_stencil_desc* d, void* lhs, const void* rhs, unsigned pieces,
                                       int nrhs, size_t vec_stride, unsigned mask, void* stream) {
  return stencil_apply_masked({d, lhs, rhs, pieces, nrhs, vec_stride, nullptr, stream}, mask);
}

// Matrices stored as complex<float> (d->clover / d->hopping point to float pairs), everything else fp64: vectors, shifts,
// accumulation.  Halves the matrix stream of the HBM-bound coarse applies.  An OPT-IN storage format for operators that
// only precondition (the K-cycle inside a flexible fp64 outer solver); nc = 1, 2, 4 are not served.
extern "C" int qmg_stencil_apply_mat32(const qmg_stencil_desc* d, void* lhs, const void* rhs, unsigned pieces,
                                       int nrhs, size_t vec_stride, unsigned mask, void* stream) {
  if (!d || d->nc == 1 || d->nc == 2 || d->nc == 4) return QMG_ERR_UNSUPPORTED;
  return stencil_apply_masked({d, lhs, rhs, pieces, nrhs, vec_stride, nullptr, stream, MatStorage::fp32}, mask);
}

// Matrices stored as complex<half> (d->clover / d->hopping point to __half2 pairs: qmg_convert_to_c16), vectors complex<double> (QMG_C64) or
// complex<float> (QMG_C32), accumulation fp64.  A quarter of the fp64 matrix stream.  For operators that only PRECONDITION; nc a multiple of 4
// (the Galerkin operators: 8, 12, 16, 24, 32); QMG_ERR_UNSUPPORTED otherwise.  The values must be inside half range (|x| < 65504; magnitudes
// below 6e-8 flush to zero): the caller checks that when it converts.
extern "C" int qmg_stencil_apply_mat16_t(int vec_dtype, const qmg_stencil_desc* d, void* lhs, const void* rhs, unsigned pieces,
                                         int nrhs, size_t vec_stride, unsigned mask, void* stream) {
  if (vec_dtype != QMG_C64 && vec_dtype != QMG_C32) return QMG_ERR_INVALID;
  if (!d || (d->nc & 3) || d->nc == 4) return QMG_ERR_UNSUPPORTED;
  return stencil_apply_masked({d, lhs, rhs, pieces, nrhs, vec_stride, nullptr, stream, MatStorage::fp16, vec_dtype == QMG_C32}, mask);
}

// Either storage precision, masked batch semantics.  QMG_C64: qmg_stencil_apply_batch.  QMG_C32: matrices AND vectors are
// complex<float>; nc in {1,2,4} run kernel A in fp32 arithmetic, every other nc the fp32-tile kernels B32 / B / C with
// fp32 vector loads and stores around their fp64 accumulation.
extern "C" int qmg_stencil_apply_t(int dtype, const qmg_stencil_desc* d, void* lhs, const void* rhs, unsigned pieces,
                                   int nrhs, size_t vec_stride, unsigned mask, void* stream) {
  if (dtype == QMG_C64) return qmg_stencil_apply_batch(d, lhs, rhs, pieces, nrhs, vec_stride, mask, stream);
  if (dtype != QMG_C32) return QMG_ERR_INVALID;
  return stencil_apply_masked({d, lhs, rhs, pieces, nrhs, vec_stride, nullptr, stream, MatStorage::fp32, true}, mask);
}

// lhs_k (+)= pieces(M) rhs_k and norms[k] = |lhs_k|^2 from the same pass (the vector is not read again): fp64, nc = 1 or 2,
// both parities written, lhs != rhs, nrhs <= 16 (QMG_ERR_UNSUPPORTED otherwise; also under distributed reductions, where the
// caller sums the norms itself).  norms_dev: nrhs doubles in device memory, or NULL; norms_host: nrhs doubles, or NULL
// (synchronises the stream).  The bytes of lhs are those qmg_stencil_apply writes.
extern "C" int qmg_stencil_apply_norm2(const qmg_stencil_desc* d, void* lhs, const void* rhs, unsigned pieces, int nrhs, size_t vec_stride,
                                       double* norms_dev, double* norms_host, void* stream) {
  if (!norms_dev && !norms_host) return QMG_ERR_INVALID;
  if (nrhs < 1 || nrhs > 16) return QMG_ERR_INVALID;
  if (dist_reductions_on()) return QMG_ERR_UNSUPPORTED;
  if (!(pieces & (QMG_P_CLOVER_E | QMG_P_EO | QMG_P_SHIFT_E | QMG_P_ZERO_E)) || !(pieces & (QMG_P_CLOVER_O | QMG_P_OE | QMG_P_SHIFT_O | QMG_P_ZERO_O)))
    return QMG_ERR_UNSUPPORTED;   // a parity left untouched: its part of |lhs|^2 is not seen by the kernel
  double* res = norms_dev;
  if (!res) { if (const int rc = norm_result_slot(&res)) return rc; }
  StencilRequest q = {d, lhs, rhs, pieces, nrhs, vec_stride, nullptr, stream};
  q.norms_dev = res;
  if (const int rc = stencil_apply(q)) return rc;
  if (norms_host) {
    QMG_HIP_CHECK(hipMemcpyAsync(norms_host, res, sizeof(double) * nrhs, hipMemcpyDeviceToHost, as_stream(stream)));
    QMG_HIP_CHECK(hipStreamSynchronize(as_stream(stream)));
  }
  return QMG_SUCCESS;
}

// One system with an epilogue on the finished site values (include/qmg_hip.h: qmg_apply_epilogue).  dtype QMG_C64: fp64 matrices and
// vectors; mat32 == 1: complex<float> matrices (d->clover / d->hopping point to float pairs), mat32 == 2: complex<half> matrices, with fp64 vectors;
// QMG_C32: fp32 vectors with either.
// QMG_ERR_UNSUPPORTED where the dispatch lands on a kernel without the epilogue (nc = 1, 2, 4; batches): the caller runs the
// separate passes instead.
extern "C" int qmg_stencil_apply_epi_t(int dtype, int mat32, const qmg_stencil_desc* d, void* lhs, const void* rhs, unsigned pieces, size_t vec_stride, int system,
                                       const qmg_apply_epilogue* epi, void* stream) {
  if (!epi || (dtype != QMG_C64 && dtype != QMG_C32) || system < 0 || system > 15) return QMG_ERR_INVALID;
  if (dtype == QMG_C32 && !mat32) return QMG_ERR_INVALID;
  if (mat32 && d && (d->nc == 1 || d->nc == 2 || d->nc == 4)) return QMG_ERR_UNSUPPORTED;
  unsigned char ridx[16];
  for (int k = 0; k < 16; k++) ridx[k] = (unsigned char)system;
  StencilRequest q = {d, lhs, rhs, pieces, 1, vec_stride, system ? ridx : nullptr, stream, storage_of(mat32), dtype == QMG_C32};
  q.epi = epi;
  return stencil_apply(q);
}
