// qmg_blas.hip -- the BLAS-1 leaves and reductions that have no batch form: the 32-vector multi-axpy, the shuffle pattern, the Gaussian fills,
// the maximum norm and the per-timeslice sums.
//
// The reference takes its BLAS-1 from quantum-linalg (absent; semantics inferred from call sites).  The streaming leaves
// (caxpy / cxpay / caxpbyz / ...) and the Krylov inner products (norm2sq / dot / diffnorm2sq / multidot) are the batch kernels of qmg_batch.hip
// on a batch of one; their entry points are there.  The two reductions here use that file's workspace (qmg_common.h) and its first stage
// (block_reduce_store): deterministic, no float atomics.
#include "qmg_common.h"

namespace qmg {

// vectors of at least this many bytes are streamed with non-temporal loads (tuning key "blas_nt_mb", in MiB; 0 = never)
long g_blas_nt_bytes = 256l << 20;
static inline bool blas_nt(size_t n_complex) { return g_blas_nt_bytes > 0 && (long)(n_complex * sizeof(cplx)) >= g_blas_nt_bytes; }

// NT: the operands are read with the non-temporal hint.  A five-stream read of 12 GB runs at 6.96 TB/s with it and 6.37 without
// (tools/membw4.hip; sc0 / sc1 make no difference), and a vector larger than the 256 MB Infinity Cache is gone before anyone reads it again
// anyway -- so the launchers ask for it from `g_blas_nt_bytes` per vector upwards and leave smaller vectors to the caches.
template <bool NT> __device__ __forceinline__ cplx ldx(const cplx* p, long i) { return NT ? ldc_nt<double>(p, i) : p[i]; }

// y += sum_i a_i x_i for up to 32 vectors in ONE pass (GCR orthogonalisation: 2k separate caxpy launches -> 2)
constexpr int MAXPY_K = 32;
struct MultiAxpy { const cplx* x[MAXPY_K]; cplx a[MAXPY_K]; };
// NJ vectors' elements requested together, then accumulated in order j (the sum's order is that of the plain loop: bit-identical results).  A loop of one
// load and one multiply-add per trip kept a single 16-byte load in flight per lane: 0.58 of the HBM rate on the outer GCR's 4096^2 updates.
template <bool NT, int NJ>
__device__ __forceinline__ void maxpy_chunk(cplx& acc, const MultiAxpy& m, int j0, long i) {
  cplx u[NJ];
#pragma unroll
  for (int j = 0; j < NJ; j++) u[j] = ldx<NT>(m.x[j0 + j], i);
#pragma unroll
  for (int j = 0; j < NJ; j++) cmac(acc, m.a[j0 + j], u[j]);
}
template <bool NT>
__global__ __launch_bounds__(BLOCK) void k_multi_caxpy(cplx* __restrict__ y, MultiAxpy m, int k, long n) {
  for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * BLOCK) {
    cplx acc = y[i];
    int j = 0;
    for (; j + 8 <= k; j += 8) maxpy_chunk<NT, 8>(acc, m, j, i);
    if (k - j >= 4) { maxpy_chunk<NT, 4>(acc, m, j, i); j += 4; }
    if (k - j >= 2) { maxpy_chunk<NT, 2>(acc, m, j, i); j += 2; }
    if (k - j >= 1) maxpy_chunk<NT, 1>(acc, m, j, i);
    y[i] = acc;
  }
}

struct Pattern { double scale[64]; int shuffle[64]; };
__global__ __launch_bounds__(BLOCK) void k_pattern(cplx* __restrict__ y, const cplx* __restrict__ x, long nsite, int nc, Pattern pat) {
  const long n = nsite * nc;
  for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * BLOCK) {
    const long site = i / nc;
    const int c = (int)(i - site * nc);
    const cplx v = x[site * nc + pat.shuffle[c]];
    y[i] = cmake(pat.scale[c] * v.x, pat.scale[c] * v.y);
  }
}

// counter-based Gaussian: splitmix64 -> two uniforms -> Box-Muller; the draw of global element gi depends only on (seed, gi)
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
struct BoxMuller { double rad, angle; };   // the complex draw is rad (cos angle, sin angle)
__device__ __forceinline__ BoxMuller box_muller(unsigned long long seed, unsigned long long gi) {
  const unsigned long long h1 = splitmix64(seed * 0xD1342543DE82EF95ull + 2ull * gi);
  const unsigned long long h2 = splitmix64(h1 + 2ull * gi + 1ull);
  const double u1 = ((double)(h1 >> 11) + 1.0) * (1.0 / 9007199254740992.0);   // (0,1]
  const double u2 = (double)(h2 >> 11) * (1.0 / 9007199254740992.0);
  BoxMuller d;
  d.rad = sqrt(-2.0 * log(u1));
  d.angle = 6.283185307179586476925286766559 * u2;
  return d;
}
__global__ __launch_bounds__(BLOCK) void k_gaussian(cplx* __restrict__ x, long n, unsigned long long seed) {
  for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * BLOCK) {
    const BoxMuller d = box_muller(seed, (unsigned long long)i);
    double sn, cs;
    sincos(d.angle, &sn, &cs);
    x[i] = cmake(d.rad * cs, d.rad * sn);
  }
}

// the same numbers for the rows [y0, y0 + Ly_l) of a (cv) vector over the lattice Lx x Ly_g: element i of the slab takes the value
// the element at its GLOBAL position would get from k_gaussian -- a slab-decomposed run draws the single-domain run's vectors
__global__ __launch_bounds__(BLOCK) void k_gaussian_slab(cplx* __restrict__ x, int hr, int Ly_g, int y0, int Ly_l, int nc, unsigned long long seed) {
  const long row = (long)hr * nc, n = 2 * row * Ly_l;
  for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * BLOCK) {
    const long q = i / (row * Ly_l), rem = i - q * row * Ly_l;          // parity, offset inside the slab's half
    const BoxMuller d = box_muller(seed, (unsigned long long)((q * Ly_g + y0) * row + rem));
    double sn, cs;
    sincos(d.angle, &sn, &cs);
    x[i] = cmake(d.rad * cs, d.rad * sn);
  }
}

// ---------------- the maximum norm: max_i |x_i|, the one global reduction that is no sum ----------------
template <bool NT>
__global__ __launch_bounds__(BLOCK) void k_norminf(const cplx* __restrict__ x, long n, double* __restrict__ partials) {
  double v = 0.0;
  for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * BLOCK) {
    const cplx a = ldx<NT>(x, i);
    v = fmax(v, a.x * a.x + a.y * a.y);
  }
  block_reduce_store<1, true>(&v, partials + blockIdx.x);
}
// stage 2, one block: out = sqrt of the largest partial
__global__ __launch_bounds__(BLOCK) void k_norminf_final(const double* __restrict__ partials, int nparts, double* __restrict__ out) {
  __shared__ double res;
  double v = 0.0;
  for (int i = threadIdx.x; i < nparts; i += BLOCK) v = fmax(v, partials[i]);
  block_reduce_store<1, true>(&v, &res);
  if (threadIdx.x == 0) out[0] = sqrt(res);
}

// gaussian_wall_source (reductions/reductions.h:90-162): a REAL Gaussian (mean + deviation N(0,1), imaginary part 0) on the elements with
// y == timeslice and component == color, zero everywhere else.  The draw of element i is the real Box-Muller value k_gaussian gives it.
__global__ __launch_bounds__(BLOCK) void k_wall_source(cplx* __restrict__ x, int hr, int Ly, int nc, int timeslice, int color, unsigned long long seed, double deviation, double mean) {
  const long n = 2l * hr * Ly * nc;
  for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * BLOCK) {
    const long site = i / nc;
    const int c = (int)(i - site * nc);
    const int y = (int)((site / hr) % Ly);   // site = (y + p Ly) hr + j
    cplx v = cmake(0.0, 0.0);
    if (c == color && y == timeslice) {
      const BoxMuller d = box_muller(seed, (unsigned long long)i);
      v.x = mean + deviation * (d.rad * cos(d.angle));
    }
    x[i] = v;
  }
}

// per-timeslice reductions (reductions/reductions.h:24-87): sum over x and c for each y.
// In the even-odd layout row y is two contiguous runs (one per parity) of hr*nc elements.
// MODE 0: |a|^2 (norm2sq_cv_timeslice, :24-41); 1: conj(a) b, re and im (dot_cv_timeslice, :69-87); 2: Re conj(a) b (redot_cv_timeslice, :47-66)
template <int MODE>
__global__ __launch_bounds__(BLOCK) void k_timeslice(const cplx* __restrict__ a, const cplx* __restrict__ b, int hr, int Ly, int nc, double* __restrict__ out) {
  const int y = blockIdx.x;
  const long half_cv = (long)hr * Ly * nc;
  const long run = (long)hr * nc;
  double v[2] = {0.0, 0.0};
  for (int p = 0; p < 2; p++) {
    const cplx* ap = a + p * half_cv + (long)y * run;
    const cplx* bp = MODE ? b + p * half_cv + (long)y * run : nullptr;
    for (long i = threadIdx.x; i < run; i += BLOCK) {
      const cplx u = ap[i];
      if (MODE) {
        const cplx w = bp[i];
        v[0] = fma(u.x, w.x, v[0]); v[0] = fma(u.y, w.y, v[0]);
        if (MODE == 1) { v[1] = fma(u.x, w.y, v[1]); v[1] = fma(-u.y, w.x, v[1]); }
      } else { v[0] = fma(u.x, u.x, v[0]); v[0] = fma(u.y, u.y, v[0]); }
    }
  }
  double part[2];
  __shared__ double res[2];
  block_reduce_store<2, false>(v, res);
  __syncthreads();
  part[0] = res[0]; part[1] = res[1];
  if (threadIdx.x == 0) {
    if (MODE == 1) { out[2 * y] = part[0]; out[2 * y + 1] = part[1]; }
    else out[y] = part[0];
  }
}

// The three per-timeslice entry points: out_dev (Ly doubles; 2 Ly for MODE 1) is written asynchronously; a result wanted on the host alone goes
// through the reduction workspace's partials.
template <int MODE>
static int timeslice_run(const void* a, const void* b, int Lx, int Ly, int nc, double* out_dev, double* out_host, void* stream) {
  if (!a || (MODE && !b) || !valid_lattice(Lx, Ly) || nc < 1 || (!out_dev && !out_host)) return QMG_ERR_INVALID;
  const size_t width = (MODE == 1 ? 2 : 1) * (size_t)Ly;
  double* res = out_dev;
  if (!res) {
    if (width > WS_PARTIALS) return QMG_ERR_INVALID;
    BatchWorkspace* ws;
    const int rc = get_bws(&ws);
    if (rc) return rc;
    res = ws->partials;
  }
  hipStream_t st = as_stream(stream);
  k_timeslice<MODE><<<Ly, BLOCK, 0, st>>>((const cplx*)a, (const cplx*)b, Lx / 2, Ly, nc, res);
  QMG_LAUNCH_CHECK();
  if (out_host) {
    QMG_HIP_CHECK(hipMemcpyAsync(out_host, res, sizeof(double) * width, hipMemcpyDeviceToHost, st));
    QMG_HIP_CHECK(hipStreamSynchronize(st));
  }
  return QMG_SUCCESS;
}

}  // namespace qmg

using namespace qmg;

extern "C" {

int qmg_multi_caxpy(const double* coeffs, const void* const* xs, int k, void* y, size_t n, void* s) {
  if (k < 0 || (k > 0 && (!coeffs || !xs)) || (!y && n)) return QMG_ERR_INVALID;
  if (n == 0) return QMG_SUCCESS;
  int done = 0;
  while (done < k) {
    const int kk = (k - done > MAXPY_K) ? MAXPY_K : k - done;
    MultiAxpy m;
    for (int j = 0; j < kk; j++) {
      if (!xs[done + j]) return QMG_ERR_INVALID;
      m.x[j] = (const cplx*)xs[done + j];
      m.a[j] = make_double2(coeffs[2 * (done + j)], coeffs[2 * (done + j) + 1]);
    }
    if (blas_nt(n)) k_multi_caxpy<true><<<grid_1d(n), BLOCK, 0, as_stream(s)>>>((cplx*)y, m, kk, (long)n);
    else k_multi_caxpy<false><<<grid_1d(n), BLOCK, 0, as_stream(s)>>>((cplx*)y, m, kk, (long)n);
    QMG_LAUNCH_CHECK();
    done += kk;
  }
  return QMG_SUCCESS;
}

int qmg_caxy_pattern(const double* scale, const int* shuffle, int nc, const void* x, void* y, size_t nsite, void* s) {
  if (!scale || !shuffle || nc < 1 || nc > 64 || !x || !y || x == y) return QMG_ERR_INVALID;
  Pattern pat;
  for (int c = 0; c < nc; c++) {
    if (shuffle[c] < 0 || shuffle[c] >= nc) return QMG_ERR_INVALID;
    pat.scale[c] = scale[c];
    pat.shuffle[c] = shuffle[c];
  }
  if (nsite == 0) return QMG_SUCCESS;
  k_pattern<<<grid_1d(nsite * nc), BLOCK, 0, as_stream(s)>>>((cplx*)y, (const cplx*)x, (long)nsite, nc, pat);
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

int qmg_gaussian(void* x, size_t n, unsigned long long seed, void* s) {
  if (!x && n) return QMG_ERR_INVALID;
  if (n == 0) return QMG_SUCCESS;
  k_gaussian<<<grid_1d(n), BLOCK, 0, as_stream(s)>>>((cplx*)x, (long)n, seed);
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

int qmg_gaussian_slab(void* x, int Lx, int Ly_global, int y0, int Ly_local, int nc, unsigned long long seed, void* s) {
  if (!x || !valid_lattice(Lx, Ly_global) || !valid_lattice(Lx, Ly_local) || nc < 1 || y0 < 0 || y0 + Ly_local > Ly_global) return QMG_ERR_INVALID;
  k_gaussian_slab<<<grid_1d((size_t)Lx * Ly_local * nc), BLOCK, 0, as_stream(s)>>>((cplx*)x, Lx / 2, Ly_global, y0, Ly_local, nc, seed);
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

int qmg_gaussian_wall_source(void* cv, int Lx, int Ly, int nc, int timeslice, int color, unsigned long long seed, double deviation, double mean, void* s) {
  if (!cv || !valid_lattice(Lx, Ly) || nc < 1) return QMG_ERR_INVALID;
  if (timeslice < 0 || timeslice >= Ly || color < 0 || color >= nc) return QMG_ERR_INVALID;   // the facade prints the reference's messages (:94-107)
  k_wall_source<<<grid_1d((size_t)Lx * Ly * nc), BLOCK, 0, as_stream(s)>>>((cplx*)cv, Lx / 2, Ly, nc, timeslice, color, seed, deviation, mean);
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

// out_dev: written by the final stage, nothing waits; out_host: makes the call synchronous.  Slabs of one lattice: the maximum over the ranks
// is taken before the value leaves HBM.
int qmg_norminf(const void* x, size_t n, double* out_dev, double* out_host, void* stream) {
  if (!x || (!out_dev && !out_host)) return QMG_ERR_INVALID;
  BatchWorkspace* ws;
  int rc = get_bws(&ws);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  const unsigned g = red_grid((long)n);
  if (blas_nt(n)) k_norminf<true><<<g, BLOCK, 0, st>>>((const cplx*)x, (long)n, ws->partials);
  else k_norminf<false><<<g, BLOCK, 0, st>>>((const cplx*)x, (long)n, ws->partials);
  QMG_LAUNCH_CHECK();
  double* res = result_slot(ws, out_dev);
  k_norminf_final<<<1, BLOCK, 0, st>>>(ws->partials, (int)g, res);
  QMG_LAUNCH_CHECK();
  if (dist_reductions_on()) { rc = dist_allreduce(res, 1, true, st); if (rc) return rc; }
  if (!out_host) return QMG_SUCCESS;
  rc = results_to_host(ws, res, 1, false, st);
  if (rc) return rc;
  *out_host = ws->pinned[0];
  return QMG_SUCCESS;
}

// reductions/reductions.h:24-87: norm2sq_cv_timeslice (:24-41), dot_cv_timeslice (:69-87), redot_cv_timeslice (:47-66: sum[y] = Re sum_{x,c} conj(a) b)
int qmg_norm2sq_cv_timeslice(const void* cv, int Lx, int Ly, int nc, double* out_dev, double* out_host, void* stream) {
  return timeslice_run<0>(cv, nullptr, Lx, Ly, nc, out_dev, out_host, stream);
}
int qmg_dot_cv_timeslice(const void* a, const void* b, int Lx, int Ly, int nc, double* out_dev, double* out_host, void* stream) {
  return timeslice_run<1>(a, b, Lx, Ly, nc, out_dev, out_host, stream);
}
int qmg_redot_cv_timeslice(const void* a, const void* b, int Lx, int Ly, int nc, double* out_dev, double* out_host, void* stream) {
  return timeslice_run<2>(a, b, Lx, Ly, nc, out_dev, out_host, stream);
}

}  // extern "C"
