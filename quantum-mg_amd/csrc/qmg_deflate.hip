// qmg_deflate.hip -- one basis V shared by every system of a batch (coarsest-level deflation, the Lanczos eigensolver of
// include/qmg/eigen.hpp): C = V^dagger B, B += V C, and the deflated guess E = V diag(1/lambda) V^dagger B.
//
// The batch entry points of qmg_batch.hip take one vector set PER SYSTEM (at the batch's stride, at most 32 vectors).  Here the
// nv <= 128 basis vectors (contiguous, leading dimension ldv) are the same for all nrhs <= 16 systems, so one pass reads every
// element of V once and every element of B once, whatever nv and the number of active systems are:
//   dot     a block stages a chunk of R rows of all nv basis vectors and of all active systems in LDS, and each thread keeps its
//           (j, k) pairs' running sums in registers over the block's chunks (pairs x row slices fill the 256 threads); the slices are
//           summed in LDS in a fixed order, the blocks' partials by a second kernel in a fixed order: the same bits run to run.
//   update  a thread owns one row of every active system and walks the nv basis vectors once; the coefficients sit in LDS.
// Storage complex<double> or complex<float> (dtype); arithmetic and accumulation are fp64 for both, as in the other _t kernels.
#include <string.h>

#include "qmg_common.h"

namespace qmg {

constexpr int BASIS_MAX = 128;                    // basis vectors per call
constexpr int BASIS_BLOCKS = 1024;                // partials per pair
constexpr int BASIS_PAIRS = BASIS_MAX * BATCH_MAX;
constexpr int BASIS_PAIRS_PER_THREAD = BASIS_PAIRS / BLOCK;   // 8

// rows per staged chunk: as many as fit 48 KiB of LDS, 16 to 64
static inline int basis_rows(int nv, int nact) {
  const int per_row = (nv + nact) * (int)sizeof(cplx);
  int r = 64;
  while (r > 16 && r * per_row > 48 * 1024) r /= 2;
  return r;
}

// stage 1: partials[block][pair][2], pair p = j * nact + s (s: slot of the active system)
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_basis_dot(const void* __restrict__ V_, long ldv, int nv, const void* __restrict__ B_, long stride,
                                                     const BatchIdx bi, long n, int R, double* __restrict__ partials) {
  typedef typename CStore<T>::type ct;
  extern __shared__ cplx sm_basis[];
  const ct* V = reinterpret_cast<const ct*>(V_);
  const ct* B = reinterpret_cast<const ct*>(B_);
  const int nact = bi.n;
  const int P = nv * nact;
  const int S = (P >= BLOCK) ? 1 : BLOCK / P;   // row slices per pair
  const int t = threadIdx.x;
  const int slice = (S > 1) ? t / P : 0;
  const bool owner = (S > 1) ? (t < S * P) : true;
  cplx* sV = sm_basis;              // [nv][R]
  cplx* sB = sm_basis + nv * R;     // [nact][R]
  cplx acc[BASIS_PAIRS_PER_THREAD];
#pragma unroll
  for (int q = 0; q < BASIS_PAIRS_PER_THREAD; q++) acc[q] = cmake(0.0, 0.0);
  const long nchunks = (n + R - 1) / R;
  for (long c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const long i0 = c * R;
    for (int e = t; e < (nv + nact) * R; e += BLOCK) {
      const int row = e / R, r = e - row * R;
      const long i = i0 + r;
      cplx v = cmake(0.0, 0.0);
      if (i < n) v = (row < nv) ? ldc<T>(V, (long)row * ldv + i) : ldc<T>(B, (long)bi.id[row - nv] * stride + i);
      sm_basis[e] = v;
    }
    __syncthreads();
    if (owner) {
      if (S > 1) {
        const int p = t - slice * P;
        const int j = p / nact, s = p - j * nact;
        for (int r = slice; r < R; r += S) cmac_conj(acc[0], sV[j * R + r], sB[s * R + r]);
      } else {
#pragma unroll
        for (int q = 0; q < BASIS_PAIRS_PER_THREAD; q++) {
          const int p = t + q * BLOCK;
          if (p < P) {
            const int j = p / nact, s = p - j * nact;
            for (int r = 0; r < R; r++) cmac_conj(acc[q], sV[j * R + r], sB[s * R + r]);
          }
        }
      }
    }
    __syncthreads();
  }
  double* out = partials + (long)blockIdx.x * P * 2;
  if (S > 1) {   // the slices of a pair, summed in slice order
    if (owner) sm_basis[t] = acc[0];
    __syncthreads();
    if (t < P) {
      cplx r = sm_basis[t];
      for (int sl = 1; sl < S; sl++) r = cadd(r, sm_basis[sl * P + t]);
      out[2 * t] = r.x; out[2 * t + 1] = r.y;
    }
  } else {
#pragma unroll
    for (int q = 0; q < BASIS_PAIRS_PER_THREAD; q++) {
      const int p = t + q * BLOCK;
      if (p < P) { out[2 * p] = acc[q].x; out[2 * p + 1] = acc[q].y; }
    }
  }
}

// stage 2: block p sums pair p over the nparts blocks in a fixed order; out[(id[s] * nv + j) * 2 + {0,1}] (times inv_lambda[j] if given)
__global__ __launch_bounds__(BLOCK) void k_basis_dot_final(const double* __restrict__ partials, int nparts, int nv, const BatchIdx bi,
                                                           const double* __restrict__ inv_lambda, double* __restrict__ out) {
  __shared__ double sm[2][BLOCK / WAVE];
  const int p = blockIdx.x, P = nv * bi.n;
  double tr = 0.0, ti = 0.0;
  for (int b = threadIdx.x; b < nparts; b += BLOCK) { tr += partials[((long)b * P + p) * 2]; ti += partials[((long)b * P + p) * 2 + 1]; }
  tr = wave_sum(tr);
  ti = wave_sum(ti);
  if ((threadIdx.x & (WAVE - 1)) == 0) { sm[0][threadIdx.x / WAVE] = tr; sm[1][threadIdx.x / WAVE] = ti; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double re = sm[0][0], im = sm[1][0];
#pragma unroll
    for (int w = 1; w < BLOCK / WAVE; w++) { re += sm[0][w]; im += sm[1][w]; }
    const int j = p / bi.n, s = p - j * bi.n;
    if (inv_lambda) { re *= inv_lambda[j]; im *= inv_lambda[j]; }
    const long o = ((long)bi.id[s] * nv + j) * 2;
    out[o] = re; out[o + 1] = im;
  }
}

// b_k (+)= sum_j C[k][j] v_j for the active systems; C[(k * nv + j) * 2 + {0,1}] in device memory; OVERWRITE: b_k = sum_j ... (b not read)
template <typename T, int KMAX, bool OVERWRITE>
__global__ __launch_bounds__(BLOCK) void k_basis_update(const double* __restrict__ coef, const void* __restrict__ V_, long ldv, int nv, void* __restrict__ B_,
                                                        long stride, const BatchIdx bi, long n) {
  typedef typename CStore<T>::type ct;
  __shared__ cplx sc[BASIS_MAX * KMAX];   // [j][s]
  const ct* V = reinterpret_cast<const ct*>(V_);
  ct* B = reinterpret_cast<ct*>(B_);
  const int nact = bi.n;
  for (int e = threadIdx.x; e < nv * KMAX; e += BLOCK) {
    const int j = e / KMAX, s = e - j * KMAX;
    sc[e] = (s < nact) ? cmake(coef[((long)bi.id[s] * nv + j) * 2], coef[((long)bi.id[s] * nv + j) * 2 + 1]) : cmake(0.0, 0.0);
  }
  __syncthreads();
  for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * BLOCK) {
    cplx acc[KMAX];
#pragma unroll
    for (int s = 0; s < KMAX; s++) acc[s] = (!OVERWRITE && s < nact) ? ldc<T>(B, (long)bi.id[s] * stride + i) : cmake(0.0, 0.0);
#pragma unroll 4
    for (int j = 0; j < nv; j++) {
      const cplx v = ldc<T>(V, (long)j * ldv + i);
#pragma unroll
      for (int s = 0; s < KMAX; s++) cmac(acc[s], sc[j * KMAX + s], v);
    }
#pragma unroll
    for (int s = 0; s < KMAX; s++) if (s < nact) stc<T>(B, (long)bi.id[s] * stride + i, acc[s]);
  }
}

struct DeflateWorkspace {
  double* partials = nullptr;   // BASIS_BLOCKS * BASIS_PAIRS * 2 doubles, grown on demand
  size_t partials_cap = 0;
  double* coef = nullptr;       // device coefficients: BATCH_MAX * BASIS_MAX * 2 doubles
  double* pinned = nullptr;     // host-pinned results of a dot whose results go to the host
  int device = -1;
};
static thread_local DeflateWorkspace g_dws;

static int get_dws(DeflateWorkspace** out, size_t partials_need) {
  int dev = 0;
  QMG_HIP_CHECK(hipGetDevice(&dev));
  if (g_dws.device != dev) {
    QMG_HIP_CHECK(hipMalloc((void**)&g_dws.coef, sizeof(double) * BASIS_PAIRS * 2));
    if (const int rc = poison_new_scratch(g_dws.coef, sizeof(double) * BASIS_PAIRS * 2)) return rc;
    QMG_HIP_CHECK(hipHostMalloc((void**)&g_dws.pinned, sizeof(double) * BASIS_PAIRS * 2, hipHostMallocCoherent));
    g_dws.device = dev;
  }
  if (g_dws.partials_cap < partials_need) {
    if (g_dws.partials) QMG_HIP_CHECK(hipFree(g_dws.partials));   // (synchronises: nothing still reads the old buffer)
    g_dws.partials = nullptr; g_dws.partials_cap = 0;
    QMG_HIP_CHECK(hipMalloc((void**)&g_dws.partials, sizeof(double) * partials_need));
    if (const int rc = poison_new_scratch(g_dws.partials, sizeof(double) * partials_need)) return rc;
    g_dws.partials_cap = partials_need;
  }
  *out = &g_dws;
  return QMG_SUCCESS;
}

void release_deflate_workspace() {   // qmg_shutdown (qmg_runtime.hip)
  if (g_dws.partials) hipFree(g_dws.partials);
  if (g_dws.coef) hipFree(g_dws.coef);
  if (g_dws.pinned) hipHostFree(g_dws.pinned);
  g_dws = DeflateWorkspace();
}

static int basis_args(int dtype, const void* V, int nv, size_t ldv, const void* B, size_t n, int nrhs) {
  if (!valid_dtype(dtype) || nv < 1 || nv > BASIS_MAX || nrhs < 1 || nrhs > BATCH_MAX || ldv < n) return QMG_ERR_INVALID;
  if (n > 0 && (!V || !B)) return QMG_ERR_INVALID;
  if (dist_reductions_on()) return QMG_ERR_UNSUPPORTED;   // one lattice's slabs: the dots would have to be summed over the ranks
  return QMG_SUCCESS;
}

// stage 1 + stage 2 on the stream; the results (scaled by inv_lambda if given) go to out_dev (device)
static int basis_dot_launch(int dtype, const void* V, int nv, size_t ldv, const void* B, size_t n, size_t stride, const BatchIdx& bi,
                            const double* inv_lambda, double* out_dev, hipStream_t st) {
  const int R = basis_rows(nv, bi.n);
  const long nchunks = ((long)n + R - 1) / R;
  const unsigned g = (unsigned)(nchunks < BASIS_BLOCKS ? (nchunks > 0 ? nchunks : 1) : BASIS_BLOCKS);
  const int P = nv * bi.n;
  DeflateWorkspace* ws;
  int rc = get_dws(&ws, (size_t)g * P * 2);
  if (rc) return rc;
  size_t lds = (size_t)(nv + bi.n) * R * sizeof(cplx);
  if (lds < BLOCK * sizeof(cplx)) lds = BLOCK * sizeof(cplx);   // the slice reduction reuses the staging area
  if (dtype == QMG_C32) k_basis_dot<float><<<g, BLOCK, lds, st>>>(V, (long)ldv, nv, B, (long)stride, bi, (long)n, R, ws->partials);
  else k_basis_dot<double><<<g, BLOCK, lds, st>>>(V, (long)ldv, nv, B, (long)stride, bi, (long)n, R, ws->partials);
  QMG_LAUNCH_CHECK();
  k_basis_dot_final<<<(unsigned)P, BLOCK, 0, st>>>(ws->partials, (int)g, nv, bi, inv_lambda, out_dev);
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

static int basis_update_launch(int dtype, const double* coef_dev, const void* V, int nv, size_t ldv, void* B, size_t n, size_t stride, const BatchIdx& bi,
                               bool overwrite, hipStream_t st) {
  const unsigned g = grid_1d(n);
  const int kmax = bi.n <= 1 ? 1 : bi.n <= 2 ? 2 : bi.n <= 4 ? 4 : bi.n <= 8 ? 8 : 16;
#define QMG_UPD(T, K)                                                                                                                             \
  if (overwrite) k_basis_update<T, K, true><<<g, BLOCK, 0, st>>>(coef_dev, V, (long)ldv, nv, B, (long)stride, bi, (long)n);                          \
  else k_basis_update<T, K, false><<<g, BLOCK, 0, st>>>(coef_dev, V, (long)ldv, nv, B, (long)stride, bi, (long)n)
#define QMG_UPD_K(T)                                                                                                                              \
  switch (kmax) { case 1: QMG_UPD(T, 1); break; case 2: QMG_UPD(T, 2); break; case 4: QMG_UPD(T, 4); break; case 8: QMG_UPD(T, 8); break; default: QMG_UPD(T, 16); break; }
  if (dtype == QMG_C32) { QMG_UPD_K(float); } else { QMG_UPD_K(double); }
#undef QMG_UPD_K
#undef QMG_UPD
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

}  // namespace qmg

using namespace qmg;

extern "C" {

int qmg_basis_dot_t(int dtype, const void* V, int nv, size_t ldv, const void* B, size_t n, int nrhs, size_t stride, unsigned mask, double* out,
                    int out_on_device, void* stream) {
  int rc = basis_args(dtype, V, nv, ldv, B, n, nrhs);
  if (rc) return rc;
  if (!out) return QMG_ERR_INVALID;
  const BatchIdx bi = expand_mask(mask, nrhs);
  if (bi.n == 0) return QMG_SUCCESS;
  hipStream_t st = as_stream(stream);
  if (out_on_device) return basis_dot_launch(dtype, V, nv, ldv, B, n, stride, bi, nullptr, out, st);
  DeflateWorkspace* ws;
  rc = get_dws(&ws, 0);
  if (rc) return rc;
  rc = basis_dot_launch(dtype, V, nv, ldv, B, n, stride, bi, nullptr, ws->coef, st);
  if (rc) return rc;
  QMG_HIP_CHECK(hipMemcpyAsync(ws->pinned, ws->coef, sizeof(double) * 2 * nv * nrhs, hipMemcpyDeviceToHost, st));
  QMG_HIP_CHECK(hipStreamSynchronize(st));
  for (int s = 0; s < bi.n; s++) memcpy(out + (size_t)bi.id[s] * 2 * nv, ws->pinned + (size_t)bi.id[s] * 2 * nv, sizeof(double) * 2 * nv);
  return QMG_SUCCESS;
}

int qmg_basis_update_t(int dtype, const double* coeffs, int coeffs_on_device, const void* V, int nv, size_t ldv, void* B, size_t n, int nrhs, size_t stride,
                       unsigned mask, void* stream) {
  const int rc0 = basis_args(dtype, V, nv, ldv, B, n, nrhs);
  if (rc0) return rc0;
  if (!coeffs) return QMG_ERR_INVALID;
  const BatchIdx bi = expand_mask(mask, nrhs);
  if (bi.n == 0 || n == 0) return QMG_SUCCESS;
  hipStream_t st = as_stream(stream);
  const double* c = coeffs;
  if (!coeffs_on_device) {
    DeflateWorkspace* ws;
    const int rc = get_dws(&ws, 0);
    if (rc) return rc;
    // (pageable source: the call returns once the host array has been consumed; the copy is ordered behind the stream's earlier work)
    QMG_HIP_CHECK(hipMemcpyAsync(ws->coef, coeffs, sizeof(double) * 2 * nv * nrhs, hipMemcpyHostToDevice, st));
    c = ws->coef;
  }
  return basis_update_launch(dtype, c, V, nv, ldv, B, n, stride, bi, false, st);
}

int qmg_batch_deflate_t(int dtype, const void* V, int nv, size_t ldv, const double* inv_lambda, const void* B, void* E, size_t n, int nrhs, size_t stride,
                        unsigned mask, void* stream) {
  int rc = basis_args(dtype, V, nv, ldv, B, n, nrhs);
  if (rc) return rc;
  if (!inv_lambda || (n > 0 && !E) || E == B) return QMG_ERR_INVALID;
  const BatchIdx bi = expand_mask(mask, nrhs);
  if (bi.n == 0 || n == 0) return QMG_SUCCESS;
  hipStream_t st = as_stream(stream);
  DeflateWorkspace* ws;
  rc = get_dws(&ws, 0);
  if (rc) return rc;
  rc = basis_dot_launch(dtype, V, nv, ldv, B, n, stride, bi, inv_lambda, ws->coef, st);
  if (rc) return rc;
  return basis_update_launch(dtype, ws->coef, V, nv, ldv, E, n, stride, bi, true, st);
}

}  // extern "C"
