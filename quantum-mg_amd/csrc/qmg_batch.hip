// qmg_batch.hip -- lock-step batches of independent right-hand sides ("independent right-hand sides"; up to 16
// systems per GPU advance through the same Krylov / K-cycle iteration together).
//
// Why: every coarse-level kernel of the K-cycle streams the SAME matrices (stencil) or the SAME null vectors (transfer)
// for every right-hand side.  Solving k systems one after the other reads them k times; solving them in lock step reads
// them once and turns the coarse apply into an (nc x nc).(nc x k) contraction (kernel C of qmg_stencil_mfma.hip, f64 MFMA).
//
// Layout: a batch vector is `nrhs` vectors of `n` complex128 at a common `stride` (complex elements).  Every entry point
// takes a bit mask of ACTIVE systems: a system that has converged inside an inner solve is frozen -- neither read nor
// written -- while the others continue, so each system sees exactly the iteration it would see alone.
//
// ONE system is a batch of one: the single-vector BLAS-1 and sum reductions of the C ABI (qmg_caxpy, qmg_norm2sq, qmg_multidot, ...) are
// entry points of this file too and run these kernels at nrhs = 1, mask = 1, complex<double> (the end of the file).  A system's arithmetic does
// not depend on the batch it is in: the element-wise operation order is DESIGN 4's table, and a reduction's block partition and fixed-order
// second stage are per system, so an inner product has the same bits alone and in any batch.
#include <string.h>
#include <time.h>

#include <initializer_list>
#include <vector>

#include "qmg_batch_plan.h"
#include "qmg_common.h"

namespace qmg {

// ---------------- element-wise ----------------
// T = storage scalar (double | float), W = elements per 16-byte access (1 for double; 2 for float when the arrays are
// 16-byte aligned with even n and stride, else 1).  Arithmetic is fp64 in registers for both T.
struct BatchCoef { cplx a[BATCH_MAX], b[BATCH_MAX]; };   // indexed by system id

// read-only operands of a batch whose active systems add up to `blas_nt_mb` MiB or more are streamed non-temporally (+8-10 % on vectors
// the caches cannot hold anyway: a five-stream read of 12 GB runs at 6.96 TB/s with the hint and 6.37 without, tools/membw4.hip); the in/out
// operand never is (a non-temporal read of a line about to be stored loses 3 %).  A run-time, launch-uniform choice (the plan's `nt`).
template <typename T, int W>
__device__ __forceinline__ void ldb(const void* p, long i, cplx (&v)[W], bool nt) {
  if (nt) ldc_pack_nt<T, W>(p, i, v);
  else ldc_pack<T, W>(p, i, v);
}
// The same choice at compile time, for the kernels that one system of 256 MiB and more runs through (k_bblas, k_breduce, k_bmultidot: their loops exist
// twice and the kernel picks one by the plan's bit).  Under the run-time form the compiler merges the two loads of a complex<double> element -- same
// type, same address -- into ONE plain load: none of the complex<double> kernels that use ldb has an `nt` on a load in its ISA, which costs
// 9-12 % at 512 MiB per vector (profiles/blas_one_engine.txt; the complex<float> forms differ in type and keep theirs).
template <typename T, int W, bool NT>
__device__ __forceinline__ void ldp(const void* p, long i, cplx (&v)[W]) {
  if (NT) ldc_pack_nt<T, W>(p, i, v);
  else ldc_pack<T, W>(p, i, v);
}

// the non-temporal store of a result that is no operand of its own pass (+4 % on vectors the caches cannot hold; on an in/out operand it gains nothing)
template <typename T, int W>
__device__ __forceinline__ void stc_pack_nt(void* base, long ipack, const cplx (&v)[W]) {
  if constexpr (sizeof(T) == 4 && W == 2) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    const f4 r = {(float)v[0].x, (float)v[0].y, (float)v[W - 1].x, (float)v[W - 1].y};
    __builtin_nontemporal_store(r, reinterpret_cast<f4*>(base) + ipack);
  } else {
    typename CStore<T>::type* p = reinterpret_cast<typename CStore<T>::type*>(base) + ipack;
    __builtin_nontemporal_store((T)v[0].x, &p->x);
    __builtin_nontemporal_store((T)v[0].y, &p->y);
  }
}
// NT / YNT: x / y are read non-temporally; with both, z of the ops that do not read z is stored non-temporally
template <int OP, typename T, int W, bool NT, bool YNT>
__device__ __forceinline__ void bblas_run(typename CStore<T>::type* z, const typename CStore<T>::type* x, const typename CStore<T>::type* y, cplx a, cplx b, long np) {
  for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < np; i += (long)gridDim.x * BLOCK) {
    cplx r[W], u[W], v[W];
    if (OP == QMG_BOP_CAX || OP == QMG_BOP_CAXPY || OP == QMG_BOP_CXPY || OP == QMG_BOP_CXPAY || OP == QMG_BOP_CAXPBY) ldc_pack<T, W>(z, i, r);
    if (OP != QMG_BOP_ZERO && OP != QMG_BOP_CAX) ldp<T, W, NT>(x, i, u);
    if (OP == QMG_BOP_CAXPBYZ || OP == QMG_BOP_CXPYZ) ldp<T, W, YNT>(y, i, v);
#pragma unroll
    for (int w = 0; w < W; w++) {
      if (OP == QMG_BOP_ZERO) r[w] = cmake(0.0, 0.0);
      else if (OP == QMG_BOP_COPY) r[w] = u[w];
      else if (OP == QMG_BOP_CAX) r[w] = cmul(a, r[w]);
      else if (OP == QMG_BOP_CAXPY) cmac(r[w], a, u[w]);
      else if (OP == QMG_BOP_CXPY) r[w] = cadd(r[w], u[w]);
      else if (OP == QMG_BOP_CAXY) r[w] = cmul(a, u[w]);
      else if (OP == QMG_BOP_CXPAY) { const cplx t = r[w]; r[w] = u[w]; cmac(r[w], a, t); }
      else if (OP == QMG_BOP_CAXPBY) { r[w] = cmul(b, r[w]); cmac(r[w], a, u[w]); }
      else if (OP == QMG_BOP_CXPYZ) r[w] = cadd(u[w], v[w]);
      else { r[w] = cmul(a, u[w]); cmac(r[w], b, v[w]); }   // CAXPBYZ
    }
    constexpr bool reads_z = OP == QMG_BOP_CAX || OP == QMG_BOP_CAXPY || OP == QMG_BOP_CXPY || OP == QMG_BOP_CXPAY || OP == QMG_BOP_CAXPBY;
    constexpr bool reads_y = OP == QMG_BOP_CAXPBYZ || OP == QMG_BOP_CXPYZ;
    if (NT && !reads_z && (YNT || !reads_y)) stc_pack_nt<T, W>(z, i, r);
    else stc_pack<T, W>(z, i, r);
  }
}
template <int OP, typename T, int W>
__global__ __launch_bounds__(BLOCK) void k_bblas(void* __restrict__ z_, const void* __restrict__ x_, const void* __restrict__ y_, const BatchCoef c,
                                                 const BatchIdx bi, long n, long stride) {
  typedef typename CStore<T>::type ct;
  const int k = bi.id[blockIdx.y];
  ct* z = reinterpret_cast<ct*>(z_) + (long)k * stride;
  const ct* x = reinterpret_cast<const ct*>(x_) + (long)k * stride;
  const ct* y = reinterpret_cast<const ct*>(y_) + (long)k * stride;
  const cplx a = c.a[k], b = c.b[k];
  const long np = n / W;
  constexpr bool reads_y = OP == QMG_BOP_CAXPBYZ || OP == QMG_BOP_CXPYZ;
  if (!bi.nt) bblas_run<OP, T, W, false, false>(z, x, y, a, b, np);
  else if (reads_y && y_ == z_) bblas_run<OP, T, W, true, false>(z, x, y, a, b, np);   // (z = a x + b z is the common aliased use: then y is the in/out operand)
  else bblas_run<OP, T, W, true, reads_y>(z, x, y, a, b, np);
}

// y_k += sum_j a[j][k] x_j,k for up to BMAXPY_J = 8 vector sets per launch (coefficients travel as kernel arguments)
struct BatchMultiAxpy { const void* x[BMAXPY_J]; cplx a[BMAXPY_J][BATCH_MAX]; };
// The NJ vector sets' loads are all requested (in storage form) before the first is widened and used: with a loop over nj and a branch on the
// coefficient around each load, every load waited for the one before it.  A zero coefficient means "this system does not use vector
// set j" (systems of a batch own different numbers of directions): the slot may hold stale pool memory, whose VALUE must not enter the sum
// (0 * inf = nan) -- it is loaded like the others and replaced by zero.
template <typename T, int W, int NJ, bool NT>
__device__ __forceinline__ void bmulti_caxpy_run(typename CStore<T>::type* y, const BatchMultiAxpy& m, int k, long off, long np) {
  typedef typename CStore<T>::type ct;
  typedef typename RawP<T, W>::type raw;
  cplx c[NJ];
  bool use[NJ];
#pragma unroll
  for (int j = 0; j < NJ; j++) { c[j] = m.a[j][k]; use[j] = c[j].x != 0.0 || c[j].y != 0.0; }
  for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < np; i += (long)gridDim.x * BLOCK) {
    raw ur[NJ];
#pragma unroll
    for (int j = 0; j < NJ; j++) {
      const void* xb = reinterpret_cast<const ct*>(m.x[j]) + off;
      ur[j] = NT ? ld_rawp_nt<T, W>(xb, i) : ld_rawp<T, W>(xb, i);
    }
    cplx acc[W];
    ldc_pack<T, W>(y, i, acc);
#pragma unroll
    for (int j = 0; j < NJ; j++) {
      cplx u[W];
      widen_rawp<T, W>(ur[j], u);
#pragma unroll
      for (int w = 0; w < W; w++) cmac(acc[w], c[j], use[j] ? u[w] : cmake(0.0, 0.0));
    }
    stc_pack<T, W>(y, i, acc);
  }
}
// the short-vector form (coarse levels: a launch of a few microseconds, where the unrolled form's longer prologue costs more than its loads gain)
template <typename T, int W>
__global__ __launch_bounds__(BLOCK) void k_bmulti_caxpy_small(void* __restrict__ y_, const BatchMultiAxpy m, int nj, const BatchIdx bi, long n, long stride) {
  typedef typename CStore<T>::type ct;
  const int k = bi.id[blockIdx.y];
  const long off = (long)k * stride;
  ct* y = reinterpret_cast<ct*>(y_) + off;
  const long np = n / W;
  for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < np; i += (long)gridDim.x * BLOCK) {
    cplx acc[W];
    ldc_pack<T, W>(y, i, acc);
    for (int j = 0; j < nj; j++) {
      const cplx c = m.a[j][k];
      if (c.x != 0.0 || c.y != 0.0) {   // (a zero coefficient: the slot may hold stale pool memory, which must not be read)
        cplx u[W];
        ldb<T, W>(reinterpret_cast<const ct*>(m.x[j]) + off, i, u, bi.nt);
#pragma unroll
        for (int w = 0; w < W; w++) cmac(acc[w], c, u[w]);
      }
    }
    stc_pack<T, W>(y, i, acc);
  }
}
template <typename T, int W>
__global__ __launch_bounds__(BLOCK) void k_bmulti_caxpy(void* __restrict__ y_, const BatchMultiAxpy m, int nj, const BatchIdx bi, long n, long stride) {
  typedef typename CStore<T>::type ct;
  const int k = bi.id[blockIdx.y];
  const long off = (long)k * stride;
  ct* y = reinterpret_cast<ct*>(y_) + off;
  const long np = n / W;
#define QMG_MAXPY_CASE(NJ) case NJ: if (bi.nt) bmulti_caxpy_run<T, W, NJ, true>(y, m, k, off, np); else bmulti_caxpy_run<T, W, NJ, false>(y, m, k, off, np); break;
  switch (nj) {
    QMG_MAXPY_CASE(1) QMG_MAXPY_CASE(2) QMG_MAXPY_CASE(3) QMG_MAXPY_CASE(4) QMG_MAXPY_CASE(5) QMG_MAXPY_CASE(6) QMG_MAXPY_CASE(7)
    default: if (bi.nt) bmulti_caxpy_run<T, W, 8, true>(y, m, k, off, np); else bmulti_caxpy_run<T, W, 8, false>(y, m, k, off, np); break;
  }
#undef QMG_MAXPY_CASE
}

// The flexible GCR's three vector updates of one iteration in ONE pass (bgcr_core): w += sum_j c_j W_j (Gram-Schmidt), r += a w (a = -alpha; the w
// just stored, in its storage precision), z_next = r (optional: the next search direction of an un-preconditioned GCR).  Operation for operation
// k_bmulti_caxpy_small, k_bblas<CAXPY>, k_bblas<COPY> -- the same bits -- with one launch and one read of w and r instead of three launches.
struct BatchCoefA { cplx a[BATCH_MAX]; };
template <typename T, int W>
__global__ __launch_bounds__(BLOCK) void k_bgcr_update(void* __restrict__ w_, const BatchMultiAxpy m, int nj, const BatchCoefA ar, void* __restrict__ r_,
                                                       void* __restrict__ zn_, const BatchIdx bi, long n, long stride) {
  typedef typename CStore<T>::type ct;
  const int k = bi.id[blockIdx.y];
  const long off = (long)k * stride;
  ct* wv = reinterpret_cast<ct*>(w_) + off;
  ct* rv = reinterpret_cast<ct*>(r_) + off;
  ct* zn = zn_ ? reinterpret_cast<ct*>(zn_) + off : nullptr;
  const cplx a = ar.a[k];
  const long np = n / W;
  for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < np; i += (long)gridDim.x * BLOCK) {
    cplx acc[W], rr[W];
    ldc_pack<T, W>(wv, i, acc);
    ldc_pack<T, W>(rv, i, rr);
    for (int j = 0; j < nj; j++) {
      const cplx c = m.a[j][k];
      if (c.x != 0.0 || c.y != 0.0) {   // (a zero coefficient: the slot may hold stale pool memory, which must not be read)
        cplx u[W];
        ldb<T, W>(reinterpret_cast<const ct*>(m.x[j]) + off, i, u, bi.nt);
#pragma unroll
        for (int q = 0; q < W; q++) cmac(acc[q], c, u[q]);
      }
    }
    if (nj > 0) stc_pack<T, W>(wv, i, acc);
#pragma unroll
    for (int q = 0; q < W; q++) {
      if (sizeof(T) == 4) acc[q] = cmake((double)(float)acc[q].x, (double)(float)acc[q].y);   // what a separate pass would read back
      cmac(rr[q], a, acc[q]);
    }
    stc_pack<T, W>(rv, i, rr);
    if (zn) stc_pack<T, W>(zn, i, rr);
  }
}

// Multi-shift CG's vector updates of one iteration in ONE pass (bcg_m_core): for every shift s that system k still iterates,
//   x[s] += a[s] p[s] ;  p[s] = z[s] r + c[s] p[s]        (a, z, c real: the coefficients of CG on a Hermitian operator)
// r is read once per element and serves every shift: 1 + 2 S reads and 2 S writes where the k_bblas passes (CAXPY on x[s], CAXPBYZ on r, p[s]) make
// 4 S reads and 2 S writes.  Operation for operation those two passes with coefficients (a, 0), (z, 0), (c, 0) -- cmac / cmul with the zero imaginary
// part kept, because dropping it changes the sign of a zero result -- so the same bits; the kernel is bound by its loads (64 bytes per shift and
// element against 12 FMAs).  A (system, shift) pair that has converged is not in the system's list: neither read nor written.  Shifts are
// taken CGM_CHUNK at a time, all 2 CGM_CHUNK loads of a chunk requested in storage form before the first is used (as bmulti_caxpy_run: 8 loads in flight).
struct BatchCgm {
  void* x[CGM_J];
  void* p[CGM_J];
  double a[CGM_J][BATCH_MAX], z[CGM_J][BATCH_MAX], c[CGM_J][BATCH_MAX];
  unsigned char na[BATCH_MAX];            // per system: how many of the launch's shifts it still iterates
  unsigned char idx[BATCH_MAX][CGM_J];    // ... and which (slots of x / p / a / z / c)
};
template <typename T, int W, int NJ>
__device__ __forceinline__ void bcgm_chunk(const BatchCgm& m, int k, int j0, long off, long i, const cplx (&rr)[W]) {
  typedef typename CStore<T>::type ct;
  typedef typename RawP<T, W>::type raw;
  raw xr[NJ], pr[NJ];
  int s[NJ];
#pragma unroll
  for (int j = 0; j < NJ; j++) {
    s[j] = m.idx[k][j0 + j];
    xr[j] = ld_rawp<T, W>(reinterpret_cast<const ct*>(m.x[s[j]]) + off, i);
    pr[j] = ld_rawp<T, W>(reinterpret_cast<const ct*>(m.p[s[j]]) + off, i);
  }
#pragma unroll
  for (int j = 0; j < NJ; j++) {
    const cplx a = cmake(m.a[s[j]][k], 0.0), z = cmake(m.z[s[j]][k], 0.0), c = cmake(m.c[s[j]][k], 0.0);
    cplx xv[W], pv[W], pn[W];
    widen_rawp<T, W>(xr[j], xv);
    widen_rawp<T, W>(pr[j], pv);
#pragma unroll
    for (int w = 0; w < W; w++) {
      cmac(xv[w], a, pv[w]);                          // k_bblas<CAXPY>
      pn[w] = cmul(z, rr[w]); cmac(pn[w], c, pv[w]);  // k_bblas<CAXPBYZ>
    }
    stc_pack<T, W>(reinterpret_cast<ct*>(m.x[s[j]]) + off, i, xv);
    stc_pack<T, W>(reinterpret_cast<ct*>(m.p[s[j]]) + off, i, pn);
  }
}
template <typename T, int W>
__global__ __launch_bounds__(BLOCK) void k_bcgm_update(const BatchCgm m, const void* __restrict__ r_, const BatchIdx bi, long n, long stride) {
  typedef typename CStore<T>::type ct;
  const int k = bi.id[blockIdx.y];
  const int na = m.na[k];
  const long off = (long)k * stride;
  const ct* rv = reinterpret_cast<const ct*>(r_) + off;
  const long np = n / W;
  for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < np; i += (long)gridDim.x * BLOCK) {
    cplx rr[W];
    ldb<T, W>(rv, i, rr, bi.nt);
    int j0 = 0;
    for (; j0 + CGM_CHUNK <= na; j0 += CGM_CHUNK) bcgm_chunk<T, W, CGM_CHUNK>(m, k, j0, off, i, rr);
    switch (na - j0) {
      case 1: bcgm_chunk<T, W, 1>(m, k, j0, off, i, rr); break;
      case 2: bcgm_chunk<T, W, 2>(m, k, j0, off, i, rr); break;
      case 3: bcgm_chunk<T, W, 3>(m, k, j0, off, i, rr); break;
      default: break;
    }
  }
}

// ---------------- reductions ----------------
// Two-stage and DETERMINISTIC: each lane accumulates a grid-strided slice in fp64, wave_reduce_many sums the wavefront, LDS the four
// wavefronts of the block (block_reduce_store, qmg_common.h), the block writes one partial, and a second tiny launch sums the (fixed number
// of) partials in a fixed order -- no float atomics, so two runs give bit-identical inner products.
template <int OP, typename T, int W, bool NT>
__device__ __forceinline__ void breduce_run(const typename CStore<T>::type* x, const typename CStore<T>::type* y, long np, double (&v)[2]) {
  for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < np; i += (long)gridDim.x * BLOCK) {
    cplx av[W], bv[W];
    ldp<T, W, NT>(x, i, av);
    if (OP != QMG_BRED_NORM2) ldp<T, W, NT>(y, i, bv);
#pragma unroll
    for (int w = 0; w < W; w++) {
      const cplx a = av[w];
      if (OP == QMG_BRED_NORM2) { v[0] = fma(a.x, a.x, v[0]); v[0] = fma(a.y, a.y, v[0]); }
      else if (OP == QMG_BRED_DOT) {
        const cplx b = bv[w];
        v[0] = fma(a.x, b.x, v[0]); v[0] = fma(a.y, b.y, v[0]);
        v[1] = fma(a.x, b.y, v[1]); v[1] = fma(-a.y, b.x, v[1]);
      } else {
        const cplx b = bv[w];
        const double dx = a.x - b.x, dy = a.y - b.y;
        v[0] = fma(dx, dx, v[0]); v[0] = fma(dy, dy, v[0]);
      }
    }
  }
}
// partials layout: [system slot s][block][2*width]
template <int OP, typename T, int W>
__global__ __launch_bounds__(BLOCK) void k_breduce(const void* __restrict__ x_, const void* __restrict__ y_, long n, long stride, const BatchIdx bi,
                                                   double* __restrict__ partials) {
  typedef typename CStore<T>::type ct;
  const long off = (long)bi.id[blockIdx.y] * stride;
  const ct* x = reinterpret_cast<const ct*>(x_) + off;
  const ct* y = reinterpret_cast<const ct*>(y_) + off;
  double v[2] = {0.0, 0.0};
  if (bi.nt) breduce_run<OP, T, W, true>(x, y, n / W, v);
  else breduce_run<OP, T, W, false>(x, y, n / W, v);
  block_reduce_store<2>(v, partials + ((long)blockIdx.y * gridDim.x + blockIdx.x) * 2);
}
struct BatchPtrs { const void* x[BDOT_MAX]; };
template <int KT, typename T, int W, bool NT>
__device__ __forceinline__ void bmultidot_run(const BatchPtrs& xs, int j0, const typename CStore<T>::type* y, long off, long np, double (&v)[2 * KT]) {
  typedef typename CStore<T>::type ct;
  for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < np; i += (long)gridDim.x * BLOCK) {
    cplx bv[W];
    ldp<T, W, NT>(y, i, bv);
#pragma unroll
    for (int q = 0; q < KT; q++) {
      cplx av[W];
      ldp<T, W, NT>(reinterpret_cast<const ct*>(xs.x[j0 + q]) + off, i, av);
#pragma unroll
      for (int w = 0; w < W; w++) {
        const cplx a = av[w], b = bv[w];
        v[2 * q] = fma(a.x, b.x, v[2 * q]); v[2 * q] = fma(a.y, b.y, v[2 * q]);
        v[2 * q + 1] = fma(a.x, b.y, v[2 * q + 1]); v[2 * q + 1] = fma(-a.y, b.x, v[2 * q + 1]);
      }
    }
  }
}
// KT dots <x_j,k , y_k> per system in one pass over y_k
template <int KT, typename T, int W>
__global__ __launch_bounds__(BLOCK) void k_bmultidot(const BatchPtrs xs, int j0, const void* __restrict__ y_, long n, long stride, const BatchIdx bi,
                                                     double* __restrict__ partials, int jtot) {
  typedef typename CStore<T>::type ct;
  const long off = (long)bi.id[blockIdx.y] * stride;
  const ct* y = reinterpret_cast<const ct*>(y_) + off;
  double v[2 * KT];
#pragma unroll
  for (int q = 0; q < 2 * KT; q++) v[q] = 0.0;
  if (bi.nt) bmultidot_run<KT, T, W, true>(xs, j0, y, off, n / W, v);
  else bmultidot_run<KT, T, W, false>(xs, j0, y, off, n / W, v);
  block_reduce_store<2 * KT>(v, partials + ((long)blockIdx.y * gridDim.x + blockIdx.x) * 2 * jtot + 2 * j0);
}

// stage 2: block (q, s) sums the nparts partials of output q of system slot s in a fixed order
// done / flag / seq (flag != nullptr): the LAST block to finish publishes `seq` in a host-visible word after the results (system-scope
// fences on both sides of the block count), so the host can pick the results up by polling that word instead of waiting for the
// stream's completion signal (wait_results below).
__global__ __launch_bounds__(BLOCK) void k_breduce_final(const double* __restrict__ partials, int nparts, int width, const BatchIdx bi, int out_width,
                                                         double* __restrict__ out, unsigned* done = nullptr, unsigned long long* flag = nullptr,
                                                         unsigned long long seq = 0) {
  __shared__ double sm[BLOCK / WAVE];
  const int q = blockIdx.x, s = blockIdx.y;
  const double* p = partials + (long)s * nparts * width;
  double t = 0.0;
  for (int i = threadIdx.x; i < nparts; i += BLOCK) t += p[(long)i * width + q];
  t = wave_sum(t);
  if ((threadIdx.x & (WAVE - 1)) == 0) sm[threadIdx.x / WAVE] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    double r = sm[0];
#pragma unroll
    for (int w = 1; w < BLOCK / WAVE; w++) r += sm[w];
    out[(long)bi.id[s] * out_width + q] = r;
    if (flag) {
      __threadfence_system();
      if (atomicAdd(done, 1u) == gridDim.x * gridDim.y - 1) {
        atomicExch(done, 0u);
        __threadfence_system();
        __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
  }
}

// MR(omega) update with the step length formed ON THE DEVICE from the dots the previous launches left in `dots` ([system][4]:
// Re<p,r>, Im<p,r>, <p,p>): alpha = omega conj(<p,r>)... written as krylov.hpp writes it, alpha = omega * <r,p>^* / <p,p> with
// <p,r> = conj(<r,p>); 0 when <p,p> == 0 (the host loop's breakdown `break`: the system is left as it is).
//   x (+)= alpha r_in ;  r_out = r_in - alpha p   (r_out == nullptr: not wanted; r_out may alias r_in)
// XSET: x = alpha r_in (the first step of a smoother that starts from x0 = 0: no zero-fill, no read of x).
template <typename T, int W, bool XSET>
__global__ __launch_bounds__(BLOCK) void k_bmr_update(void* __restrict__ x_, const void* __restrict__ rin_, void* rout_, const void* __restrict__ p_,
                                                      const double* __restrict__ dots, double omega, const BatchIdx bi, long n, long stride) {
  typedef typename CStore<T>::type ct;
  const int k = bi.id[blockIdx.y];
  const long off = (long)k * stride;
  ct* x = reinterpret_cast<ct*>(x_) + off;
  const ct* rin = reinterpret_cast<const ct*>(rin_) + off;
  ct* rout = rout_ ? reinterpret_cast<ct*>(rout_) + off : nullptr;
  const ct* p = reinterpret_cast<const ct*>(p_) + off;
  const double prx = dots[4 * k], pry = dots[4 * k + 1], pp = dots[4 * k + 2];   // <p,r> = (prx, pry)
  // alpha = omega * <p,r> / <p,p> in the host loop's operation order: (omega * pr) / pp
  const cplx alpha = (pp == 0.0) ? cmake(0.0, 0.0) : cmake((omega * prx) / pp, (omega * pry) / pp);
  const cplx malpha = cmake(-alpha.x, -alpha.y);
  const long np = n / W;
  for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < np; i += (long)gridDim.x * BLOCK) {
    cplx xv[W], rv[W], pv[W];
    ldc_pack<T, W>(rin, i, rv);
    if (!XSET) ldc_pack<T, W>(x, i, xv);
#pragma unroll
    for (int w = 0; w < W; w++) { if (XSET) xv[w] = cmake(0.0, 0.0); cmac(xv[w], alpha, rv[w]); }   // (XSET: the accumulate on an explicit zero, bit for bit)
    stc_pack<T, W>(x, i, xv);
    if (rout) {
      ldb<T, W>(p, i, pv, bi.nt);
#pragma unroll
      for (int w = 0; w < W; w++) cmac(rv[w], malpha, pv[w]);
      stc_pack<T, W>(rout, i, rv);
    }
  }
}

// stage 2 of the MR dots: out[system][4] <- {sum of partial q = 0, 1 (<r,p>: conjugated into <p,r>), q = 3 (<p,p>)}; one block per system
__global__ __launch_bounds__(BLOCK) void k_bmr_final(const double* __restrict__ partials, int nparts, const BatchIdx bi, double* __restrict__ out) {
  __shared__ double sm[3][BLOCK / WAVE];
  const int s = blockIdx.x;
  const double* p = partials + (long)s * nparts * 4;   // multidot of {r, p} against p: [part][4] = Re<r,p>, Im<r,p>, <p,p>, 0
  double t[3] = {0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < nparts; i += BLOCK) { t[0] += p[(long)i * 4]; t[1] += p[(long)i * 4 + 1]; t[2] += p[(long)i * 4 + 2]; }
#pragma unroll
  for (int q = 0; q < 3; q++) {
    const double w = wave_sum(t[q]);
    if ((threadIdx.x & (WAVE - 1)) == 0) sm[q][threadIdx.x / WAVE] = w;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    double r = sm[threadIdx.x][0];
#pragma unroll
    for (int w = 1; w < BLOCK / WAVE; w++) r += sm[threadIdx.x][w];
    // <p,r> = conj(<r,p>): the imaginary part changes sign (krylov.hpp: pr = conj(d2[0]))
    out[4 * bi.id[s] + threadIdx.x] = (threadIdx.x == 1) ? -r : r;
  }
}

static thread_local BatchWorkspace g_bws;

int get_bws(BatchWorkspace** out) {
  int dev = 0;
  QMG_HIP_CHECK(hipGetDevice(&dev));
  if (g_bws.device != dev) {
    QMG_HIP_CHECK(hipMalloc((void**)&g_bws.partials, sizeof(double) * WS_PARTIALS));
    if (const int rc = poison_new_scratch(g_bws.partials, sizeof(double) * WS_PARTIALS)) return rc;
    QMG_HIP_CHECK(hipHostMalloc((void**)&g_bws.pinned, sizeof(double) * WS_RESULTS, hipHostMallocCoherent));
    QMG_HIP_CHECK(hipHostMalloc((void**)&g_bws.flag, 64, hipHostMallocCoherent));
    *g_bws.flag = 0;
    g_bws.seq = 0;
    QMG_HIP_CHECK(hipMalloc((void**)&g_bws.done, sizeof(unsigned)));
    QMG_HIP_CHECK(hipMemset(g_bws.done, 0, sizeof(unsigned)));
    QMG_HIP_CHECK(hipMalloc((void**)&g_bws.result, sizeof(double) * WS_RESULTS));
    QMG_HIP_CHECK(hipMemset(g_bws.result, 0, sizeof(double) * WS_RESULTS));
    QMG_HIP_CHECK(hipMalloc((void**)&g_bws.mr, sizeof(double) * BATCH_MAX * 4));
    QMG_HIP_CHECK(hipMemset(g_bws.mr, 0, sizeof(double) * BATCH_MAX * 4));
    // The three memsets are null-stream work, and the thread's first reduction may be on a non-blocking stream, which is not ordered behind
    // them: `done` is that reduction's arrival counter.  Once per thread, as in poison_new_scratch.
    QMG_HIP_CHECK(hipDeviceSynchronize());
    g_bws.device = dev;
  }
  *out = &g_bws;
  return QMG_SUCCESS;
}

void release_batch_workspace() {   // qmg_shutdown (qmg_runtime.hip)
  if (g_bws.partials) hipFree(g_bws.partials);
  if (g_bws.result) hipFree(g_bws.result);
  if (g_bws.pinned) hipHostFree(g_bws.pinned);
  if (g_bws.mr) hipFree(g_bws.mr);
  if (g_bws.epi_part) hipFree(g_bws.epi_part);
  if (g_bws.done) hipFree(g_bws.done);
  if (g_bws.flag) hipHostFree(g_bws.flag);
  g_bws = BatchWorkspace();
}

// How a reduction's results reach the host.  A solver iteration is a chain of short kernels with one or two host decisions in it, and
// hipStreamSynchronize costs ~15 us of completion-signal handling per decision on top of the kernels' own latency (profiles/r03_n13_solve_phase.json:
// 8244 gaps of 22.8 us after k_breduce_final = 16 % of the C3 solve).  With "reduce_spin" (default 1) the final stage's last block publishes a
// sequence number in coherent host memory behind its results and the host polls that word; the stream is NOT synchronised (later launches
// are ordered behind the kernel anyway).  A poll that sees nothing for 2 s falls back to the synchronise, which also surfaces a launch error.
int g_reduce_spin = 1;
static inline bool spin_results(const BatchWorkspace* ws) { return g_reduce_spin != 0 && ws->flag != nullptr; }
static int wait_results(BatchWorkspace* ws, bool flagged, hipStream_t st) {
  if (flagged) {
    const unsigned long long want = ws->seq;
    volatile unsigned long long* f = ws->flag;
    for (long spins = 0;; spins++) {
      if (__atomic_load_n(f, __ATOMIC_ACQUIRE) == want) return QMG_SUCCESS;
      if ((spins & 0xfff) == 0xfff) {
        static thread_local double t0 = 0;
        timespec ts;
        clock_gettime(CLOCK_MONOTONIC, &ts);
        const double now = ts.tv_sec + 1e-9 * ts.tv_nsec;
        if (spins == 0xfff) t0 = now;
        else if (now - t0 > 2.0) break;
      }
    }
  }
  QMG_HIP_CHECK(hipStreamSynchronize(st));
  return QMG_SUCCESS;
}

double* result_slot(BatchWorkspace* ws, double* out_dev) { return out_dev ? out_dev : (dist_reductions_on() ? ws->result : ws->pinned); }
int results_to_host(BatchWorkspace* ws, const double* res, int count, bool flagged, hipStream_t st) {
  if (res != ws->pinned) QMG_HIP_CHECK(hipMemcpyAsync(ws->pinned, res, sizeof(double) * count, hipMemcpyDeviceToHost, st));
  return wait_results(ws, flagged, st);
}

double* mr_epilogue_begin(int nsys, long npart) {
  BatchWorkspace* ws;
  if (get_bws(&ws) != QMG_SUCCESS) return nullptr;
  const size_t need = (size_t)nsys * (size_t)npart * 4;
  if (ws->epi_cap < need) {
    if (ws->epi_part) { if (hipFree(ws->epi_part) != hipSuccess) return nullptr; }   // (synchronises: nothing still writes the old buffer)
    ws->epi_part = nullptr; ws->epi_cap = 0;
    if (hipMalloc((void**)&ws->epi_part, sizeof(double) * need) != hipSuccess) return nullptr;
    if (poison_new_scratch(ws->epi_part, sizeof(double) * need) != QMG_SUCCESS) return nullptr;
    ws->epi_cap = need;
  }
  return ws->epi_part;
}

int mr_epilogue_finish(const unsigned char* ids, int n, long npart, hipStream_t st) {
  BatchWorkspace* ws;
  int rc = get_bws(&ws);
  if (rc) return rc;
  if (n < 1 || n > BATCH_MAX || !ws->epi_part) return QMG_ERR_INVALID;
  BatchIdx bi;
  bi.n = n; bi.nt = 0;
  for (int k = 0; k < BATCH_MAX; k++) bi.id[k] = (k < n) ? ids[k] : (unsigned char)0;
  const bool dist = dist_reductions_on();
  if (dist) QMG_HIP_CHECK(hipMemsetAsync(ws->mr, 0, sizeof(double) * 4 * BATCH_MAX, st));   // inactive slots must not accumulate over the ranks call after call
  k_bmr_final<<<(unsigned)n, BLOCK, 0, st>>>(ws->epi_part, (int)npart, bi, ws->mr);
  QMG_LAUNCH_CHECK();
  if (dist) { rc = dist_allreduce(ws->mr, 4 * BATCH_MAX, false, st); if (rc) return rc; }
  return QMG_SUCCESS;
}

// What batch_plan (qmg_batch_plan.h) reads of a call, at the current "blas_nt_mb".  Every launcher below asks the plan and switches on its answer.
static bool all_aligned16(std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs) if (p && !aligned16(p)) return false;
  return true;
}
static bool all_aligned16(const void* const* ptrs, int first, int count) {
  for (int j = first; j < first + count; j++) if (ptrs[j] && !aligned16(ptrs[j])) return false;
  return true;
}
static BatchPlanRequest batch_request(int entry, int dtype, size_t n, size_t stride, int nrhs, unsigned mask, bool aligned) {
  BatchPlanRequest r = {};
  r.entry = entry; r.dtype = dtype; r.n = n; r.stride = stride; r.nrhs = nrhs; r.mask = mask;
  r.aligned = aligned;
  r.nt_bytes = g_blas_nt_bytes;
  return r;
}
// the systems of a launch and its non-temporal bit, as the kernels take them
static BatchIdx batch_idx(const BatchPass& pl, int nrhs) {
  BatchIdx bi = expand_mask(pl.systems, nrhs);
  bi.nt = pl.nt;
  return bi;
}

}  // namespace qmg

using namespace qmg;

// dispatch on (dtype, access width): K(T, W) expands to one kernel launch
#define QMG_DISPATCH_TW(dtype, W_, K)                         \
  do {                                                        \
    if ((dtype) == QMG_C32) { if ((W_) == 2) { K(float, 2); } else { K(float, 1); } } \
    else { K(double, 1); }                                    \
  } while (0)

extern "C" {

int qmg_batch_blas_t(int dtype, int op, const double* a, const double* b, const void* x, const void* y, void* z, size_t n, int nrhs, size_t stride,
                     unsigned mask, void* stream) {
  if (!valid_dtype(dtype) || nrhs < 1 || nrhs > BATCH_MAX || (!z && n)) return QMG_ERR_INVALID;
  if (op < QMG_BOP_ZERO || op > QMG_BOP_CXPYZ) return QMG_ERR_INVALID;
  const bool reads_x = op != QMG_BOP_ZERO && op != QMG_BOP_CAX, reads_y = op == QMG_BOP_CAXPBYZ || op == QMG_BOP_CXPYZ;
  const bool uses_b = op == QMG_BOP_CAXPBYZ || op == QMG_BOP_CAXPBY;
  const bool uses_a = uses_b || op == QMG_BOP_CAX || op == QMG_BOP_CAXPY || op == QMG_BOP_CAXY || op == QMG_BOP_CXPAY;
  if ((reads_x && !x && n) || (reads_y && !y && n) || (uses_a && !a) || (uses_b && !b)) return QMG_ERR_INVALID;
  BatchPlanRequest rq = batch_request(QMG_BE_BLAS, dtype, n, stride, nrhs, mask, all_aligned16({x, y, z}));
  rq.op = op;
  const BatchPass pl = batch_plan(rq);
  if (pl.family == BF_NOTHING) return QMG_SUCCESS;
  const BatchIdx bi = batch_idx(pl, nrhs);
  BatchCoef c;
  for (int k = 0; k < BATCH_MAX; k++) {
    c.a[k] = (a && k < nrhs) ? make_double2(a[2 * k], a[2 * k + 1]) : make_double2(0.0, 0.0);
    c.b[k] = (b && k < nrhs) ? make_double2(b[2 * k], b[2 * k + 1]) : make_double2(0.0, 0.0);
  }
  const int W = pl.W;
  dim3 grid(grid_1d(n / W), (unsigned)bi.n);
  hipStream_t st = as_stream(stream);
#define QMG_OP(OP, T, WW) case OP: k_bblas<OP, T, WW><<<grid, BLOCK, 0, st>>>(z, x, y, c, bi, (long)n, (long)stride); break;
#define QMG_K(T, WW)                                                                                                         \
  switch (pl.variant) {                                                                                                      \
    QMG_OP(QMG_BOP_ZERO, T, WW) QMG_OP(QMG_BOP_COPY, T, WW) QMG_OP(QMG_BOP_CAX, T, WW) QMG_OP(QMG_BOP_CAXPY, T, WW) QMG_OP(QMG_BOP_CXPY, T, WW) \
    QMG_OP(QMG_BOP_CAXY, T, WW) QMG_OP(QMG_BOP_CXPAY, T, WW) QMG_OP(QMG_BOP_CAXPBY, T, WW) QMG_OP(QMG_BOP_CXPYZ, T, WW)      \
    default: k_bblas<QMG_BOP_CAXPBYZ, T, WW><<<grid, BLOCK, 0, st>>>(z, x, y, c, bi, (long)n, (long)stride); break;          \
  }
  QMG_DISPATCH_TW(dtype, W, QMG_K);
#undef QMG_K
#undef QMG_OP
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}
int qmg_batch_blas(int op, const double* a, const double* b, const void* x, const void* y, void* z, size_t n, int nrhs, size_t stride,
                   unsigned mask, void* stream) {
  return qmg_batch_blas_t(QMG_C64, op, a, b, x, y, z, n, nrhs, stride, mask, stream);
}

// coeffs[(j*nrhs + k)*2 + {0,1}]: coefficient of vector set j for system k
int qmg_batch_multi_caxpy_t(int dtype, const double* coeffs, const void* const* xs, int nj, void* y, size_t n, int nrhs, size_t stride, unsigned mask,
                            void* stream) {
  if (!valid_dtype(dtype) || nrhs < 1 || nrhs > BATCH_MAX || nj < 0 || (nj > 0 && (!coeffs || !xs)) || (!y && n)) return QMG_ERR_INVALID;
  BatchPlanRequest rq = batch_request(QMG_BE_MULTI_CAXPY, dtype, n, stride, nrhs, mask, all_aligned16({y}) && all_aligned16(xs, 0, nj));
  rq.nj = nj;
  BatchPass pl = batch_plan(rq);
  if (pl.family == BF_NOTHING) return QMG_SUCCESS;
  // one fp64 system on long vectors (a single outer solve on the fine lattice): k_multi_caxpy (qmg_blas.hip), which takes up to 32 vector sets
  // per pass over y instead of 8 -- the same sums in the same order
  // -- on the vector sets whose coefficient is not zero, in their order: a zero coefficient means "not read" here as in the batch kernels, and
  // that kernel multiplies whatever it is given (0 * nan = nan)
  if (pl.family == BF_MAXPY_SINGLE) {
    std::vector<double> cf;
    std::vector<const void*> used;
    for (int j = 0; j < nj; j++) {
      if (!xs[j]) return QMG_ERR_INVALID;
      if (coeffs[2 * j] == 0.0 && coeffs[2 * j + 1] == 0.0) continue;
      cf.push_back(coeffs[2 * j]); cf.push_back(coeffs[2 * j + 1]);
      used.push_back(xs[j]);
    }
    return qmg_multi_caxpy(cf.data(), used.data(), (int)used.size(), y, n, stream);
  }
  for (int j = 0; j < nj; j++) if (!xs[j]) return QMG_ERR_INVALID;
  const BatchIdx bi = batch_idx(pl, nrhs);
  const int W = pl.W;
  dim3 grid(grid_1d(n / W), (unsigned)bi.n);
  for (;; pl = batch_plan(rq, pl.next)) {
    const int j0 = pl.at, jj = pl.J;
    BatchMultiAxpy m;
    for (int j = 0; j < BMAXPY_J; j++) {
      m.x[j] = (j < jj) ? xs[j0 + j] : nullptr;
      for (int k = 0; k < BATCH_MAX; k++)
        m.a[j][k] = (j < jj && k < nrhs) ? make_double2(coeffs[((size_t)(j0 + j) * nrhs + k) * 2], coeffs[((size_t)(j0 + j) * nrhs + k) * 2 + 1])
                                         : make_double2(0.0, 0.0);
    }
    // long vectors: all loads of a chunk in flight (BATCH_LONG_BYTES, qmg_batch_plan.h)
    const bool big = pl.family == BF_MAXPY_LONG;
#define QMG_K(T, WW) if (big) k_bmulti_caxpy<T, WW><<<grid, BLOCK, 0, as_stream(stream)>>>(y, m, jj, bi, (long)n, (long)stride); \
                     else k_bmulti_caxpy_small<T, WW><<<grid, BLOCK, 0, as_stream(stream)>>>(y, m, jj, bi, (long)n, (long)stride)
    QMG_DISPATCH_TW(dtype, W, QMG_K);
#undef QMG_K
    QMG_LAUNCH_CHECK();
    if (pl.next < 0) break;
  }
  return QMG_SUCCESS;
}
int qmg_batch_multi_caxpy(const double* coeffs, const void* const* xs, int nj, void* y, size_t n, int nrhs, size_t stride, unsigned mask, void* stream) {
  return qmg_batch_multi_caxpy_t(QMG_C64, coeffs, xs, nj, y, n, nrhs, stride, mask, stream);
}

// w_k += sum_j c[j][k] ws[j]_k ; r_k += a[k] w_k ; z_next_k = r_k (z_next != NULL) for the active systems: see k_bgcr_update
int qmg_batch_gcr_update_t(int dtype, const double* coeffs, const void* const* ws, int nj, void* w, const double* a, void* r, void* z_next, size_t n, int nrhs,
                           size_t stride, unsigned mask, void* stream) {
  if (!valid_dtype(dtype) || nrhs < 1 || nrhs > BATCH_MAX || nj < 0 || (nj > 0 && (!coeffs || !ws)) || !a || ((!w || !r) && n)) return QMG_ERR_INVALID;
  if (w == r || (z_next && (z_next == w || z_next == r))) return QMG_ERR_INVALID;
  BatchPlanRequest rq = batch_request(QMG_BE_GCR_UPDATE, dtype, n, stride, nrhs, mask, true);
  rq.nj = nj;
  rq.flags = z_next ? BPV_ZNEXT : 0;
  if (batch_plan(rq).family == BF_NOTHING) return QMG_SUCCESS;
  // all but the last chunk of 8 vector sets: the plain multi-axpy.  Long vectors (an outer solve on the fine lattice): every chunk through it -- its
  // long-vector form keeps a chunk's loads in flight, which is worth more there than the saved launch (C5 shape: 2 % of the solve)
  const int lead = batch_gcr_lead(rq);
  if (lead > 0) { const int rc = qmg_batch_multi_caxpy_t(dtype, coeffs, ws, lead, w, n, nrhs, stride, mask, stream); if (rc) return rc; }
  const int jj = nj - lead;
  rq.aligned = all_aligned16({w, r, z_next}) && (jj == 0 || all_aligned16(ws, lead, jj));   // (the pointers this launch reads)
  const BatchPass pl = batch_plan(rq, lead);
  const BatchIdx bi = batch_idx(pl, nrhs);
  const int W = pl.W;
  BatchMultiAxpy m;
  for (int j = 0; j < BMAXPY_J; j++) {
    m.x[j] = (j < jj) ? ws[lead + j] : nullptr;
    if (j < jj && !ws[lead + j]) return QMG_ERR_INVALID;
    for (int k = 0; k < BATCH_MAX; k++)
      m.a[j][k] = (j < jj && k < nrhs) ? make_double2(coeffs[((size_t)(lead + j) * nrhs + k) * 2], coeffs[((size_t)(lead + j) * nrhs + k) * 2 + 1]) : make_double2(0.0, 0.0);
  }
  BatchCoefA ar;
  for (int k = 0; k < BATCH_MAX; k++) ar.a[k] = (k < nrhs) ? make_double2(a[2 * k], a[2 * k + 1]) : make_double2(0.0, 0.0);
  dim3 grid(grid_1d(n / W), (unsigned)bi.n);
#define QMG_K(T, WW) k_bgcr_update<T, WW><<<grid, BLOCK, 0, as_stream(stream)>>>(w, m, jj, ar, r, z_next, bi, (long)n, (long)stride)
  QMG_DISPATCH_TW(dtype, W, QMG_K);
#undef QMG_K
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

// x[s]_k += a[s][k] p[s]_k ; p[s]_k = z[s][k] r_k + c[s][k] p[s]_k for every shift s < ns and every system k of mask & shift_masks[s]: see k_bcgm_update.
// a, z, c: [s * nrhs + k], real.  More than 8 shifts take one launch per 8 (r is read once per launch).
int qmg_batch_cgm_update_t(int dtype, const void* const* xs, const void* const* ps, int ns, const double* a, const double* z, const double* c,
                           const unsigned* shift_masks, const void* r, size_t n, int nrhs, size_t stride, unsigned mask, void* stream) {
  if (!valid_dtype(dtype) || nrhs < 1 || nrhs > BATCH_MAX || ns < 1 || ns > BATCH_MAX || !xs || !ps || !a || !z || !c || !shift_masks || (!r && n)) return QMG_ERR_INVALID;
  for (int s = 0; s < ns; s++) {
    if (n && (!xs[s] || !ps[s] || xs[s] == r || ps[s] == r || xs[s] == ps[s])) return QMG_ERR_INVALID;
    for (int t = 0; t < s; t++) if (n && (xs[s] == xs[t] || ps[s] == ps[t] || xs[s] == ps[t] || ps[s] == xs[t])) return QMG_ERR_INVALID;
  }
  if (n == 0) return QMG_SUCCESS;
  BatchPlanRequest rq = batch_request(QMG_BE_CGM_UPDATE, dtype, n, stride, nrhs, mask, all_aligned16({r}) && all_aligned16(xs, 0, ns) && all_aligned16(ps, 0, ns));
  rq.nj = ns;
  rq.shift_masks = shift_masks;
  for (BatchPass pl = batch_plan(rq);; pl = batch_plan(rq, pl.next)) {
    if (pl.family == BF_NOTHING) {   // a launch none of whose shifts is iterated any more
      if (pl.next < 0) break;
      continue;
    }
    const int s0 = pl.at, sj = pl.J, W = pl.W;
    BatchCgm m;
    memset(&m, 0, sizeof(m));
    for (int j = 0; j < sj; j++) {
      m.x[j] = const_cast<void*>(xs[s0 + j]);
      m.p[j] = const_cast<void*>(ps[s0 + j]);
      const unsigned act = mask & shift_masks[s0 + j];
      for (int k = 0; k < nrhs; k++) {
        m.a[j][k] = a[(size_t)(s0 + j) * nrhs + k]; m.z[j][k] = z[(size_t)(s0 + j) * nrhs + k]; m.c[j][k] = c[(size_t)(s0 + j) * nrhs + k];
        if ((act >> k) & 1u) m.idx[k][m.na[k]++] = (unsigned char)j;
      }
    }
    const BatchIdx bi = batch_idx(pl, nrhs);   // a system none of whose shifts is iterated any more launches no block
    dim3 grid(grid_1d(n / W), (unsigned)bi.n);
#define QMG_K(T, WW) k_bcgm_update<T, WW><<<grid, BLOCK, 0, as_stream(stream)>>>(m, r, bi, (long)n, (long)stride)
    QMG_DISPATCH_TW(dtype, W, QMG_K);
#undef QMG_K
    QMG_LAUNCH_CHECK();
    if (pl.next < 0) break;
  }
  return QMG_SUCCESS;
}

// Stage 2 of a sum reduction and the way of its results, shared by every launcher below: block (q, system) of the final stage writes output q
// (of `width`; the partials hold `pwidth` per block) of every active system k to res[k * width + q], res being the caller's device pointer
// or the workspace's slot (result_slot).  Under distributed reductions the results are summed over the ranks where they are (every rank has
// the same active mask: the lock-step decisions are taken on these very sums).  out_host == NULL: that is all, nothing waits.  Else the
// active systems' results are on the host when this returns (wait_results); inactive entries of out_host are left untouched.
static int reduce_finish(BatchWorkspace* ws, unsigned nparts, int pwidth, int width, const BatchIdx& bi, int nrhs, double* out_dev, double* out_host,
                         hipStream_t st) {
  double* res = result_slot(ws, out_dev);
  const bool flagged = res == ws->pinned && spin_results(ws);
  const dim3 grid(width, (unsigned)bi.n);
  if (flagged) k_breduce_final<<<grid, BLOCK, 0, st>>>(ws->partials, (int)nparts, pwidth, bi, width, res, ws->done, ws->flag, ++ws->seq);
  else k_breduce_final<<<grid, BLOCK, 0, st>>>(ws->partials, (int)nparts, pwidth, bi, width, res);
  QMG_LAUNCH_CHECK();
  if (dist_reductions_on()) { const int rc = dist_allreduce(res, width * nrhs, false, st); if (rc) return rc; }
  if (!out_host) return QMG_SUCCESS;
  const int rc = results_to_host(ws, res, width * nrhs, flagged, st);
  if (rc) return rc;
  for (int s = 0; s < bi.n; s++) memcpy(out_host + (size_t)bi.id[s] * width, ws->pinned + (size_t)bi.id[s] * width, sizeof(double) * width);
  return QMG_SUCCESS;
}

// `width` doubles per system (2: re, im; 1: a real result alone) to out_dev and / or out_host (reduce_finish); the caller has checked the arguments
static int reduce_run(int dtype, int op, const void* x, const void* y, size_t n, int nrhs, size_t stride, unsigned mask, int width, double* out_dev,
                      double* out_host, void* stream) {
  BatchPlanRequest rq = batch_request(QMG_BE_REDUCE, dtype, n, stride, nrhs, mask, all_aligned16({x, y}));
  rq.op = op;
  const BatchPass pl = batch_plan(rq);
  if (pl.family == BF_NOTHING) return QMG_SUCCESS;
  const BatchIdx bi = batch_idx(pl, nrhs);
  BatchWorkspace* ws;
  int rc = get_bws(&ws);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  const int W = pl.W;
  const unsigned g = red_grid((long)(n / W));
  dim3 grid(g, (unsigned)bi.n);
#define QMG_K(T, WW)                                                                                                                      \
  if (op == QMG_BRED_NORM2) k_breduce<QMG_BRED_NORM2, T, WW><<<grid, BLOCK, 0, st>>>(x, nullptr, (long)n, (long)stride, bi, ws->partials); \
  else if (op == QMG_BRED_DOT) k_breduce<QMG_BRED_DOT, T, WW><<<grid, BLOCK, 0, st>>>(x, y, (long)n, (long)stride, bi, ws->partials);      \
  else k_breduce<QMG_BRED_DIFFNORM2, T, WW><<<grid, BLOCK, 0, st>>>(x, y, (long)n, (long)stride, bi, ws->partials)
  QMG_DISPATCH_TW(dtype, W, QMG_K);
#undef QMG_K
  QMG_LAUNCH_CHECK();
  return reduce_finish(ws, g, 2, width, bi, nrhs, out_dev, out_host, st);
}

// out_host[2*k + {0,1}] for every ACTIVE system k (inactive entries are left untouched); returns when they are on the host (wait_results)
int qmg_batch_reduce_t(int dtype, int op, const void* x, const void* y, size_t n, int nrhs, size_t stride, unsigned mask, double* out_host, void* stream) {
  if (!valid_dtype(dtype) || nrhs < 1 || nrhs > BATCH_MAX || !x || !out_host) return QMG_ERR_INVALID;
  if (op < QMG_BRED_NORM2 || op > QMG_BRED_DIFFNORM2) return QMG_ERR_INVALID;
  if (op != QMG_BRED_NORM2 && !y) return QMG_ERR_INVALID;
  return reduce_run(dtype, op, x, y, n, nrhs, stride, mask, 2, nullptr, out_host, stream);
}
int qmg_batch_reduce(int op, const void* x, const void* y, size_t n, int nrhs, size_t stride, unsigned mask, double* out_host, void* stream) {
  return qmg_batch_reduce_t(QMG_C64, op, x, y, n, nrhs, stride, mask, out_host, stream);
}

// <xs[j]_k , y_k> for 1 <= nj <= BDOT_MAX vector sets, 2 nj doubles per system, to out_dev and / or out_host (reduce_finish); the caller has checked the arguments
static int multidot_run(int dtype, const void* const* xs, int nj, const void* y, size_t n, int nrhs, size_t stride, unsigned mask, double* out_dev,
                        double* out_host, void* stream) {
  BatchPlanRequest rq = batch_request(QMG_BE_MULTIDOT, dtype, n, stride, nrhs, mask, all_aligned16({y}) && all_aligned16(xs, 0, nj));
  rq.nj = nj;
  BatchPass pl = batch_plan(rq);
  if (pl.family == BF_NOTHING) return QMG_SUCCESS;
  const BatchIdx bi = batch_idx(pl, nrhs);
  BatchWorkspace* ws;
  int rc = get_bws(&ws);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  BatchPtrs p;
  const int W = pl.W;
  for (int j = 0; j < BDOT_MAX; j++) {
    p.x[j] = (j < nj) ? xs[j] : nullptr;
    if (j < nj && !xs[j]) return QMG_ERR_INVALID;
  }
  const unsigned g = red_grid((long)(n / W));
  dim3 grid(g, (unsigned)bi.n);
  for (;; pl = batch_plan(rq, pl.next)) {   // chunks of 8 / 4 / 2 / 1 dots (batch_plan)
    const int j0 = pl.at, kt = pl.J;
#define QMG_K(T, WW)                                                                                                  \
    if (kt == 8) k_bmultidot<8, T, WW><<<grid, BLOCK, 0, st>>>(p, j0, y, (long)n, (long)stride, bi, ws->partials, nj);   \
    else if (kt == 4) k_bmultidot<4, T, WW><<<grid, BLOCK, 0, st>>>(p, j0, y, (long)n, (long)stride, bi, ws->partials, nj);   \
    else if (kt == 2) k_bmultidot<2, T, WW><<<grid, BLOCK, 0, st>>>(p, j0, y, (long)n, (long)stride, bi, ws->partials, nj); \
    else k_bmultidot<1, T, WW><<<grid, BLOCK, 0, st>>>(p, j0, y, (long)n, (long)stride, bi, ws->partials, nj)
    QMG_DISPATCH_TW(dtype, W, QMG_K);
#undef QMG_K
    QMG_LAUNCH_CHECK();
    if (pl.next < 0) break;
  }
  return reduce_finish(ws, g, 2 * nj, 2 * nj, bi, nrhs, out_dev, out_host, st);
}

// out_host[(k*nj + j)*2 + {0,1}] = <xs[j]_k , y_k> for every active system k; returns when they are on the host (wait_results)
int qmg_batch_multidot_t(int dtype, const void* const* xs, int nj, const void* y, size_t n, int nrhs, size_t stride, unsigned mask, double* out_host,
                         void* stream) {
  if (!valid_dtype(dtype) || nrhs < 1 || nrhs > BATCH_MAX || nj < 1 || nj > BDOT_MAX || !xs || !y || !out_host) return QMG_ERR_INVALID;
  return multidot_run(dtype, xs, nj, y, n, nrhs, stride, mask, nullptr, out_host, stream);
}
int qmg_batch_multidot(const void* const* xs, int nj, const void* y, size_t n, int nrhs, size_t stride, unsigned mask, double* out_host, void* stream) {
  return qmg_batch_multidot_t(QMG_C64, xs, nj, y, n, nrhs, stride, mask, out_host, stream);
}

// ---- MR(omega) with every scalar on the device (the smoothers of the K-cycle: fixed iteration counts, no host decision) ----
// qmg_batch_mr_dots_t: <p_k, r_k> and <p_k, p_k> of the active systems into the calling thread's device slot (one pass over p and r,
// the same two-stage deterministic reduction as qmg_batch_multidot of {r, p} against p, summed over ranks under distributed
// reductions).  Nothing comes back to the host; nothing synchronises.
int qmg_batch_mr_dots_t(int dtype, const void* r, const void* p, size_t n, int nrhs, size_t stride, unsigned mask, void* stream) {
  if (!valid_dtype(dtype) || nrhs < 1 || nrhs > BATCH_MAX || !r || !p) return QMG_ERR_INVALID;
  const BatchPass pl = batch_plan(batch_request(QMG_BE_MR_DOTS, dtype, n, stride, nrhs, mask, all_aligned16({r, p})));
  if (pl.family == BF_NOTHING) return QMG_SUCCESS;
  const BatchIdx bi = batch_idx(pl, nrhs);
  BatchWorkspace* ws;
  int rc = get_bws(&ws);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  BatchPtrs ptr;
  for (int j = 0; j < BDOT_MAX; j++) ptr.x[j] = nullptr;
  ptr.x[0] = r; ptr.x[1] = p;
  const int W = pl.W;
  const unsigned g = red_grid((long)(n / W));
  dim3 grid(g, (unsigned)bi.n);
#define QMG_K(T, WW) k_bmultidot<2, T, WW><<<grid, BLOCK, 0, st>>>(ptr, 0, p, (long)n, (long)stride, bi, ws->partials, 2)
  QMG_DISPATCH_TW(dtype, W, QMG_K);
#undef QMG_K
  QMG_LAUNCH_CHECK();
  const bool dist = dist_reductions_on();
  if (dist) QMG_HIP_CHECK(hipMemsetAsync(ws->mr, 0, sizeof(double) * 4 * BATCH_MAX, st));   // inactive slots must not accumulate over the ranks call after call
  k_bmr_final<<<(unsigned)bi.n, BLOCK, 0, st>>>(ws->partials, (int)g, bi, ws->mr);
  QMG_LAUNCH_CHECK();
  if (dist) { rc = dist_allreduce(ws->mr, 4 * BATCH_MAX, false, st); if (rc) return rc; }
  return QMG_SUCCESS;
}

// qmg_batch_mr_update_t: with alpha_k = omega <p_k, r_k> / <p_k, p_k> formed on the device from the slot qmg_batch_mr_dots_t (or a stencil
// apply with the MR epilogue) filled on this stream:   x (+)= alpha r_in ;  r_out = r_in - alpha p.
//   x_set != 0: x = alpha r_in (first step from x0 = 0: x is written, never read);  r_out == NULL: the new residual is not wanted;
//   r_out may alias r_in.  <p,p> == 0 leaves the system unchanged (alpha = 0), as the host loop's breakdown exit does.
int qmg_batch_mr_update_t(int dtype, double omega, void* x, const void* r_in, void* r_out, const void* p, int x_set, size_t n, int nrhs, size_t stride,
                          unsigned mask, void* stream) {
  if (!valid_dtype(dtype) || nrhs < 1 || nrhs > BATCH_MAX || !x || !r_in || (r_out && !p)) return QMG_ERR_INVALID;
  BatchPlanRequest rq = batch_request(QMG_BE_MR_UPDATE, dtype, n, stride, nrhs, mask, all_aligned16({x, r_in, r_out, p}));
  rq.flags = (x_set ? BPV_XSET : 0) | (r_out ? BPV_ROUT : 0);
  const BatchPass pl = batch_plan(rq);
  if (pl.family == BF_NOTHING) return QMG_SUCCESS;
  const BatchIdx bi = batch_idx(pl, nrhs);
  BatchWorkspace* ws;
  int rc = get_bws(&ws);
  if (rc) return rc;
  const int W = pl.W;
  dim3 grid(grid_1d(n / W), (unsigned)bi.n);
  hipStream_t st = as_stream(stream);
#define QMG_K(T, WW)                                                                                                               \
  if (pl.variant & BPV_XSET) k_bmr_update<T, WW, true><<<grid, BLOCK, 0, st>>>(x, r_in, r_out, p, ws->mr, omega, bi, (long)n, (long)stride);        \
  else k_bmr_update<T, WW, false><<<grid, BLOCK, 0, st>>>(x, r_in, r_out, p, ws->mr, omega, bi, (long)n, (long)stride)
  QMG_DISPATCH_TW(dtype, W, QMG_K);
#undef QMG_K
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

// the slot itself (4 doubles per system: Re<p,r>, Im<p,r>, <p,p>, -) copied to the host: tests and diagnostics; synchronises
int qmg_batch_mr_read_dots(double* out_host, int nrhs, void* stream) {
  if (!out_host || nrhs < 1 || nrhs > BATCH_MAX) return QMG_ERR_INVALID;
  BatchWorkspace* ws;
  int rc = get_bws(&ws);
  if (rc) return rc;
  QMG_HIP_CHECK(hipMemcpyAsync(out_host, ws->mr, sizeof(double) * 4 * nrhs, hipMemcpyDeviceToHost, as_stream(stream)));
  QMG_HIP_CHECK(hipStreamSynchronize(as_stream(stream)));
  return QMG_SUCCESS;
}

// The plan of a call (include/qmg_hip.h): the entry point's own argument checks, then what batch_plan -- the function every launcher above switches
// on -- answers pass by pass.  No HIP call.
int qmg_batch_plan(int entry, int dtype, int op, size_t n, size_t stride, int nrhs, unsigned mask, int nj, const unsigned* shift_masks, int flags,
                   int aligned16_, int* plan_out, int max_passes) {
  if (!plan_out || max_passes < 1 || !valid_dtype(dtype) || nrhs < 1 || nrhs > BATCH_MAX) return QMG_ERR_INVALID;
  switch (entry) {
    case QMG_BE_BLAS: if (op < QMG_BOP_ZERO || op > QMG_BOP_CXPYZ || nj || flags) return QMG_ERR_INVALID; break;
    case QMG_BE_MULTI_CAXPY: if (nj < 0 || op || flags) return QMG_ERR_INVALID; break;
    case QMG_BE_GCR_UPDATE: if (nj < 0 || op || (flags & ~BPV_ZNEXT)) return QMG_ERR_INVALID; break;
    case QMG_BE_CGM_UPDATE: if (nj < 1 || nj > BATCH_MAX || !shift_masks || op || flags) return QMG_ERR_INVALID; break;
    case QMG_BE_REDUCE: if (op < QMG_BRED_NORM2 || op > QMG_BRED_DIFFNORM2 || nj || flags) return QMG_ERR_INVALID; break;
    case QMG_BE_MULTIDOT: if (nj < 1 || nj > BDOT_MAX || op || flags) return QMG_ERR_INVALID; break;
    case QMG_BE_MR_DOTS: if (nj || op || flags) return QMG_ERR_INVALID; break;
    case QMG_BE_MR_UPDATE: if (nj || op || (flags & ~(BPV_XSET | BPV_ROUT))) return QMG_ERR_INVALID; break;
    default: return QMG_ERR_INVALID;
  }
  BatchPlanRequest rq = batch_request(entry, dtype, n, stride, nrhs, mask, aligned16_ != 0);
  rq.op = op; rq.nj = nj; rq.shift_masks = shift_masks; rq.flags = flags;
  for (int i = 0; i < BATCH_PLAN_INTS * max_passes; i++) plan_out[i] = -1;
  int passes = 0;
  for (int at = 0; at >= 0; passes++) {
    if (passes == max_passes) return QMG_ERR_INVALID;
    const BatchPass pl = batch_plan(rq, at);
    const int v[BATCH_PLAN_INTS] = {pl.family, pl.W, pl.nt, pl.J, pl.variant};
    for (int i = 0; i < BATCH_PLAN_INTS; i++) plan_out[BATCH_PLAN_INTS * passes + i] = v[i];
    at = pl.next;
  }
  return QMG_SUCCESS;
}

// ---- ONE system: the single-vector BLAS-1 and sum reductions of the C ABI are the launchers above at nrhs = 1, mask = 1, complex<double>.
// (qmg_multi_caxpy, qmg_norminf and the per-timeslice sums have no batch form: qmg_blas.hip.)
static int blas1(int op, double ar, double ai, double br, double bi, const void* x, const void* y, void* z, size_t n, void* s) {
  const double a[2] = {ar, ai}, b[2] = {br, bi};
  return qmg_batch_blas_t(QMG_C64, op, a, b, x, y, z, n, 1, 0, 1u, s);   // (its argument checks are the single-vector ones: a NULL vector only with n = 0)
}
int qmg_zero_vector(void* x, size_t n, void* s) { return blas1(QMG_BOP_ZERO, 0, 0, 0, 0, nullptr, nullptr, x, n, s); }
int qmg_copy_vector(void* dst, const void* src, size_t n, void* s) { return blas1(QMG_BOP_COPY, 0, 0, 0, 0, src, nullptr, dst, n, s); }
int qmg_cax(double ar, double ai, void* x, size_t n, void* s) { return blas1(QMG_BOP_CAX, ar, ai, 0, 0, nullptr, nullptr, x, n, s); }
int qmg_caxy(double ar, double ai, const void* x, void* y, size_t n, void* s) { return blas1(QMG_BOP_CAXY, ar, ai, 0, 0, x, nullptr, y, n, s); }
int qmg_caxpy(double ar, double ai, const void* x, void* y, size_t n, void* s) { return blas1(QMG_BOP_CAXPY, ar, ai, 0, 0, x, nullptr, y, n, s); }
int qmg_cxpy(const void* x, void* y, size_t n, void* s) { return blas1(QMG_BOP_CXPY, 0, 0, 0, 0, x, nullptr, y, n, s); }
int qmg_cxpay(const void* x, double ar, double ai, void* y, size_t n, void* s) { return blas1(QMG_BOP_CXPAY, ar, ai, 0, 0, x, nullptr, y, n, s); }
int qmg_caxpby(double ar, double ai, const void* x, double br, double bi, void* y, size_t n, void* s) {
  return blas1(QMG_BOP_CAXPBY, ar, ai, br, bi, x, nullptr, y, n, s);
}
int qmg_cxpyz(const void* x, const void* y, void* z, size_t n, void* s) { return blas1(QMG_BOP_CXPYZ, 0, 0, 0, 0, x, y, z, n, s); }
int qmg_caxpbyz(double ar, double ai, const void* x, double br, double bi, const void* y, void* z, size_t n, void* s) {
  return blas1(QMG_BOP_CAXPBYZ, ar, ai, br, bi, x, y, z, n, s);
}

// out_dev: written by the final stage, nothing waits; out_host: makes the call synchronous (reduce_finish)
static int reduce1(int op, int width, const void* x, const void* y, size_t n, double* od, double* oh, void* s) {
  if (!x || (op != QMG_BRED_NORM2 && !y) || (!od && !oh)) return QMG_ERR_INVALID;
  return reduce_run(QMG_C64, op, x, y, n, 1, 0, 1u, width, od, oh, s);
}
int qmg_norm2sq(const void* x, size_t n, double* od, double* oh, void* s) { return reduce1(QMG_BRED_NORM2, 1, x, nullptr, n, od, oh, s); }
int qmg_dot(const void* x, const void* y, size_t n, double* od, double* oh, void* s) { return reduce1(QMG_BRED_DOT, 2, x, y, n, od, oh, s); }
int qmg_diffnorm2sq(const void* x, const void* y, size_t n, double* od, double* oh, void* s) { return reduce1(QMG_BRED_DIFFNORM2, 1, x, y, n, od, oh, s); }

// up to 64 vectors: BDOT_MAX per pass of the launcher (each dot is its own accumulation: the split changes no digit)
int qmg_multidot(const void* const* xs, int k, const void* y, size_t n, double* out_dev, double* out_host, void* stream) {
  if (!xs || !y || k < 1 || k > 2 * BDOT_MAX || (!out_dev && !out_host)) return QMG_ERR_INVALID;
  for (int i = 0; i < k; i++) if (!xs[i]) return QMG_ERR_INVALID;
  for (int k0 = 0; k0 < k; k0 += BDOT_MAX) {
    const int rc = multidot_run(QMG_C64, xs + k0, k - k0 < BDOT_MAX ? k - k0 : BDOT_MAX, y, n, 1, 0, 1u, out_dev ? out_dev + 2 * k0 : nullptr,
                                out_host ? out_host + 2 * k0 : nullptr, stream);
    if (rc) return rc;
  }
  return QMG_SUCCESS;
}

}  // extern "C"
