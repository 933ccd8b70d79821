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

static int stencil_apply_volume1(const StencilRequest& q, const StencilPlan& pl) {
  const qmg_stencil_desc* d = q.d;
  StencilArgs a;
  memset(&a, 0, sizeof(a));
  fill_systems_and_shifts(a, q);
  const int zero = (pl.flags & SPF_ZERO) ? 1 : 0, shift_on = (pl.flags & SPF_SHIFT) ? 1 : 0;
  if (pl.storage & SST_V32) k_stencil_volume1<float><<<pl.gx, 64, 0, as_stream(q.stream)>>>(q.lhs, q.rhs, d->nc, q.nrhs, (long)q.vec_stride, nullptr, a, zero, shift_on);
  else k_stencil_volume1<double><<<pl.gx, 64, 0, as_stream(q.stream)>>>(q.lhs, q.rhs, d->nc, q.nrhs, (long)q.vec_stride, nullptr, a, zero, shift_on);
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

// what stencil_plan reads of a request, with the knobs as they stand
StencilPlanRequest qmg::plan_request(const qmg_stencil_desc* d, unsigned pieces, int nrhs, bool holes, bool inplace, int mat, bool vec32, const SlabHalo* slab) {
  StencilPlanRequest r = {};
  r.mat = mat; r.vec32 = vec32;
  r.Lx = d->Lx; r.Ly = d->Ly; r.nc = d->nc;
  r.pieces = pieces;
  r.nrhs = nrhs; r.holes = holes; r.inplace = inplace;
  r.clover = d->clover != nullptr; r.hopping = d->hopping != nullptr;
  r.slab = slab != nullptr; r.rows = slab ? slab->rows : 0;
  r.k_site = g_stencil_site; r.k_pair = g_stencil_pair; r.k_mfma = g_stencil_mfma; r.k_prefetch = g_pair_prefetch;
  return r;
}

// The dispatcher: the request's own validation, then the plan (qmg_stencil_plan.h: the kernel families in route order -- the first one that serves
// the request takes it) and the launch function of the plan's family.
int qmg::stencil_apply(const StencilRequest& q) {
  const qmg_stencil_desc* d = q.d;
  const bool mat32 = q.mat != MatStorage::fp64, mat16 = q.mat == MatStorage::fp16, vec32 = q.vec32;   // (mat32: narrow-stored matrices, either width)
  const SlabHalo* slab = q.slab;
  const int nrhs = q.nrhs;
  if (!d || !q.lhs || !q.rhs || nrhs < 1) return QMG_ERR_INVALID;
  StencilPlanRequest r = plan_request(d, q.pieces, nrhs, q.ridx != nullptr, q.lhs == q.rhs, mat16 ? 2 : mat32 ? 1 : 0, vec32, slab);
  r.norm = q.norms_dev != nullptr;
  r.epi = q.epi ? (q.epi->dotv ? 2 : 1) : 0;
  const StencilPlan pl = stencil_plan(r);
  if (pl.status == QMG_ERR_INVALID) return QMG_ERR_INVALID;
  const bool volume1 = d->Lx == 1 && d->Ly == 1;
  if (volume1 && pl.status) return pl.status;
  if (nrhs > 1 && q.vec_stride < (volume1 ? (size_t)d->nc : (size_t)d->Lx * d->Ly * d->nc)) return QMG_ERR_INVALID;
  if (pl.status) return pl.status;
  if (q.epi && (q.epi->other == q.lhs || q.epi->dotv == q.lhs)) return QMG_ERR_INVALID;
  if (pl.family == SF_NOTHING) return QMG_SUCCESS;
  if (pl.family == SF_VOLUME1) return stencil_apply_volume1(q, pl);
  hipStream_t st = as_stream(q.stream);
  if (pl.family == SF_SITE) return launch_stencil_site(pl, d, q.lhs, q.rhs, q.pieces, nrhs, (long)q.vec_stride, q.ridx, st, slab);
  const int nc = d->nc;

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
  a.par_first = ev ? 0 : 1;
  a.par_count = (ev && od) ? 2 : 1;
  a.nrows = d->Ly * a.par_count;

  if (q.epi) {
    // out = other_scale other + acc_scale acc and the MR dots, in kernels B / B32
    a.epi.on = 1;
    a.epi.other = q.epi->other; a.epi.other_scale = q.epi->other_scale; a.epi.acc_scale = q.epi->acc_scale;
    a.epi.dotv = q.epi->dotv;
    // partials: one per wavefront of the launch; the launchers of kernels B / B32 ask for them
  }

  switch (pl.family) {
    case SF_PAIR: return (pl.flags & SPF_NORM) ? launch_stencil_norm(a, pl, q.norms_dev, st) : launch_stencil_pair(a, pl, st);
    case SF_ELEM: return launch_stencil_elem(a, pl, st);
    case SF_GEN32: return launch_stencil_gen32(a, nc, pl, st);
    case SF_GEN: return launch_stencil_gen(a, nc, pl, st);
    case SF_MFMA:
      // up to 16 right-hand sides per pass share one read of the matrices; the plan of each further pass from the same request
      for (int k0 = 0;;) {
        const StencilPlan pass = k0 ? stencil_plan(r, k0) : pl;
        if (pass.family != SF_MFMA) return pass.status ? pass.status : QMG_ERR_INVALID;
        if (const int rc = launch_stencil_mfma(a, pass, k0, st)) return rc;
        k0 += pass.nk;
        if (k0 >= nrhs) return QMG_SUCCESS;
      }
    default: return QMG_ERR_INVALID;
  }
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
  if (q.d && !entry_rules::narrow_storage_served(q.mat == MatStorage::fp16 ? 2 : q.mat == MatStorage::fp32 ? 1 : 0, q.vec32, q.d->nc)) return QMG_ERR_UNSUPPORTED;
  if (!entry_rules::batch_size_ok(q.nrhs)) return QMG_ERR_INVALID;
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
  if (!d) return QMG_ERR_UNSUPPORTED;
  return stencil_apply_masked({d, lhs, rhs, pieces, nrhs, vec_stride, nullptr, stream, MatStorage::fp32}, mask);   // (nc = 1, 2, 4: refused there)
}

// Matrices stored as complex<half> (d->clover / d->hopping point to __half2 pairs: qmg_convert_to_c16), vectors complex<double> (QMG_C64) or
// complex<float> (QMG_C32), accumulation fp64.  A quarter of the fp64 matrix stream.  For operators that only PRECONDITION; nc a multiple of 4
// (the Galerkin operators: 8, 12, 16, 24, 32); QMG_ERR_UNSUPPORTED otherwise.  The values must be inside half range (|x| < 65504; magnitudes
// below 6e-8 flush to zero): the caller checks that when it converts.
extern "C" int qmg_stencil_apply_mat16_t(int vec_dtype, const qmg_stencil_desc* d, void* lhs, const void* rhs, unsigned pieces,
                                         int nrhs, size_t vec_stride, unsigned mask, void* stream) {
  if (vec_dtype != QMG_C64 && vec_dtype != QMG_C32) return QMG_ERR_INVALID;
  if (!d) return QMG_ERR_UNSUPPORTED;
  return stencil_apply_masked({d, lhs, rhs, pieces, nrhs, vec_stride, nullptr, stream, MatStorage::fp16, vec_dtype == QMG_C32}, mask);   // (nc: refused there)
}

// Either storage precision, masked batch semantics.  QMG_C64: qmg_stencil_apply_batch.  QMG_C32: matrices AND vectors are
// complex<float>; nc in {1,2,4} run kernel A in fp32 arithmetic, every other nc the fp32-tile kernels B32 / B with
// fp32 vector loads and stores around their fp64 accumulation, or kernel C on the f32 matrix cores (fp32 accumulators).
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
  if (!entry_rules::batch_size_ok(nrhs)) return QMG_ERR_INVALID;
  if (dist_reductions_on()) return QMG_ERR_UNSUPPORTED;
  if (!entry_rules::both_parities(pieces)) return QMG_ERR_UNSUPPORTED;   // a parity left untouched: its part of |lhs|^2 is not seen by the kernel
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
  if (!entry_rules::epilogue_storage_valid(mat32, dtype == QMG_C32)) return QMG_ERR_INVALID;
  if (d && !entry_rules::epilogue_storage_served(mat32, d->nc)) return QMG_ERR_UNSUPPORTED;
  unsigned char ridx[16];
  for (int k = 0; k < 16; k++) ridx[k] = (unsigned char)system;
  StencilRequest q = {d, lhs, rhs, pieces, 1, vec_stride, system ? ridx : nullptr, stream, storage_of(mat32), dtype == QMG_C32};
  q.epi = epi;
  return stencil_apply(q);
}

// Which kernel serves a stencil apply (include/qmg_hip.h): the entry's own checks, then the answer of stencil_plan -- the function the launches
// above switch on -- for every pass.  Host only: no HIP call.
extern "C" int qmg_stencil_plan(int entry, int mat, int vec32, int Lx, int Ly, int nc, unsigned pieces, int n_active, int holes, int inplace,
                                int has_clover, int has_hopping, int epilogue, int slab_rows, int* plan_out, int plan_len) {
  if (!plan_out || plan_len < STENCIL_PLAN_INTS || entry < QMG_SE_APPLY || entry > QMG_SE_SLAB || mat < 0 || mat > 2 || n_active < 1) return QMG_ERR_INVALID;
  if ((epilogue != 0) != (entry == QMG_SE_EPI) || epilogue < 0 || epilogue > 2 || (slab_rows != 0 && entry != QMG_SE_SLAB)) return QMG_ERR_INVALID;
  if (mat == 0 && vec32) return QMG_ERR_INVALID;   // no entry point takes complex<float> vectors with complex<double> matrices
  using namespace entry_rules;
  int status = QMG_SUCCESS, site_entry = 0;   // the entry's own refusal, if any
  SlabHalo halo = {nullptr, nullptr, 0, slab_rows};
  switch (entry) {
    case QMG_SE_APPLY:   // qmg_stencil_apply: fp64, no mask, any number of systems
      if (mat || holes) return QMG_ERR_INVALID;
      break;
    case QMG_SE_MASKED:  // qmg_stencil_apply_batch / _t / _mat32 / _mat16_t, by mat and vec32
      if (!narrow_storage_served(mat, vec32, nc)) status = QMG_ERR_UNSUPPORTED;
      else if (!batch_size_ok(n_active)) return QMG_ERR_INVALID;
      break;
    case QMG_SE_H16:     // qmg_stencil_apply_h16
      if (mat != 2 || !vec32 || !batch_size_ok(n_active)) return QMG_ERR_INVALID;
      site_entry = 1;
      break;
    case QMG_SE_NORM2:   // qmg_stencil_apply_norm2
      if (mat || holes || !batch_size_ok(n_active)) return QMG_ERR_INVALID;
      if (!both_parities(pieces)) status = QMG_ERR_UNSUPPORTED;
      break;
    case QMG_SE_EPI:     // qmg_stencil_apply_epi_t: one system (holes: it is not system 0)
      if (n_active != 1 || !epilogue_storage_valid(mat, vec32)) return QMG_ERR_INVALID;
      if (!epilogue_storage_served(mat, nc)) status = QMG_ERR_UNSUPPORTED;
      break;
    default:             // qmg_stencil_apply_slab
      if (!batch_size_ok(n_active) || slab_rows < 0 || slab_rows > 2) return QMG_ERR_INVALID;
      if (inplace && !slab_inplace_ok(pieces)) return QMG_ERR_INVALID;
      if (!valid_lattice(Lx, Ly)) return QMG_ERR_INVALID;
      if (nc == 2) {
        if (mat != 0 && !vec32) return QMG_ERR_INVALID;   // narrow matrices under fp64 vectors are not a storage of kernel S
        site_entry = 1;
      } else if (!slab_generic_served(mat, mat == 2 || (mat == 1 && !vec32), nc, slab_rows)) status = QMG_ERR_UNSUPPORTED;
      break;
  }
  for (int i = 0; i < plan_len; i++) plan_out[i] = -1;
  static const char present = 0;   // a field that is there: stencil_plan reads the pointers' presence only
  const qmg_stencil_desc d = {Lx, Ly, nc, has_clover ? &present : nullptr, has_hopping ? &present : nullptr, {0, 0}, {0, 0}, {0, 0}};
  StencilPlanRequest r = plan_request(&d, pieces, n_active, holes != 0, inplace != 0, mat, vec32 != 0, entry == QMG_SE_SLAB ? &halo : nullptr);
  r.site_entry = site_entry;
  r.norm = entry == QMG_SE_NORM2;
  r.epi = epilogue;
  int at = 0;
  for (int k0 = 0; k0 < n_active;) {
    StencilPlan pl = status ? plan_detail::refused(status) : stencil_plan(r, k0);
    if (at + STENCIL_PLAN_INTS > plan_len) return QMG_ERR_INVALID;
    const int v[STENCIL_PLAN_INTS] = {pl.family, pl.storage, pl.NC, pl.P, pl.K, pl.flags, pl.S, pl.H, pl.smem, pl.gx, pl.gy, pl.nk};
    for (int i = 0; i < STENCIL_PLAN_INTS; i++) plan_out[at + i] = v[i];
    at += STENCIL_PLAN_INTS;
    if (pl.family != SF_MFMA) break;
    k0 += pl.nk;
  }
  return QMG_SUCCESS;
}
