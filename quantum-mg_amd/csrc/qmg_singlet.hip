// qmg_singlet.hip -- what turns a lock-step batch of solves into flavour-singlet loops: Z4 noise that is a function of (seed, element) and is
// never stored, its dilution into a batch of sources in one launch, and S, P, N of every timeslice of every active system in one pass over
// the solutions.
//
//   noise      eta_i = i^(h >> 62),  h = splitmix64(seed * 0xD1342543DE82EF95 + 2 i): the first hash box_muller (qmg_blas.hip) takes for element i
//   dilution   class d(i) = ((y mod nt) ncs + (spin ? c : 0)) neo + (eo ? p : 0)  (singlet_class, qmg_singlet_plan.h); system k of a batch
//              carries class first_class + k:  out_k(i) = eta_i where d(i) = first_class + k, zero elsewhere
//   loops      S_k(y) = sum_{i in row y, d(i) = d_k} conj(eta_i) psi_k(i),   P_k(y) the same with the sign g(i) of gamma5,
//              N_k(y) = sum_{i in row y} |psi_k(i)|^2 over the WHOLE row;  out[(k Ly + y) 5 + {0..4}] = Re S, Im S, Re P, Im P, N
//
// Lane mapping of the loops: a block of 256 lanes per (timeslice y, active system) -- k_timeslice (qmg_blas.hip) with the systems over
// grid.x.  The block walks the even run of row y and then the odd one; a lane takes elements tid, tid + 256, ... of a run, four loads
// requested in front of their arithmetic, and keeps its component c by adding 256 mod nc instead of dividing.  Whether the row
// (y mod nt) and the run (p) belong to the system's class is the same for the whole block; only the component test is per lane, and the hash
// is evaluated behind all three.  Five fp64 sums per lane go through block_reduce_store (wavefronts by recursive halving, then the four
// wavefronts in index order) and lanes 0..4 store them: one launch, no atomics, and a system's numbers depend on nothing but its own vector
// -- not on the batch, the mask or a second run.  Frozen systems get no block, and no lane steps past the end of a run.
// 16 nc B/site per system in fp64, 8 nc in fp32; nothing else is read.
#include "qmg_singlet_plan.h"

namespace qmg {

// (the library's counter-based generator, restated: qmg_blas.hip keeps its own copy beside box_muller)
__device__ __forceinline__ unsigned long long sg_splitmix64(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// the power q of eta_i = i^q
__device__ __forceinline__ int z4_power(unsigned long long seed, unsigned long long i) {
  return (int)(sg_splitmix64(seed * 0xD1342543DE82EF95ull + 2ull * i) >> 62);
}
__device__ __forceinline__ cplx z4_value(int q) { return cmake(q == 0 ? 1.0 : q == 2 ? -1.0 : 0.0, q == 1 ? 1.0 : q == 3 ? -1.0 : 0.0); }

__global__ __launch_bounds__(BLOCK) void k_noise_z4(cplx* __restrict__ eta, long n, unsigned long long seed) {
  for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * BLOCK) eta[i] = z4_value(z4_power(seed, (unsigned long long)i));
}

// what the two kernels know of a call's dilution
struct Dilute { int nt, ncs, neo, spin, eo, first_class; };
// the (y mod nt, c, p) of class d; c and p are 0 where the class does not fix them
struct ClassOf { int t, c, p; };
__device__ __forceinline__ ClassOf class_of(const Dilute& dl, int d) {
  ClassOf k;
  k.p = d % dl.neo;
  k.c = (d / dl.neo) % dl.ncs;
  k.t = d / (dl.neo * dl.ncs);
  return k;
}

// out_k(i) for every element of the active systems: grid.y = the active systems, grid.x strides over the elements
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_noise_dilute(void* __restrict__ out, int hr, int Ly, int nc, Dilute dl, unsigned long long seed, long stride, BatchIdx ids) {
  const int k = ids.id[blockIdx.y];
  const ClassOf cl = class_of(dl, dl.first_class + k);
  const long n = 2l * hr * Ly * nc;
  char* dst = reinterpret_cast<char*>(out) + (long)k * stride * (long)(2 * sizeof(T));
  for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * BLOCK) {
    const long site = i / nc;
    const int c = (int)(i - site * nc);
    const long row = site / hr;                        // site = (y + p Ly) hr + j
    const int p = (int)(row / Ly), y = (int)(row - (long)p * Ly);
    cplx v = cmake(0.0, 0.0);
    if (y % dl.nt == cl.t && (!dl.spin || c == cl.c) && (!dl.eo || p == cl.p)) v = z4_value(z4_power(seed, (unsigned long long)i));
    stc<T>(dst, i, v);
  }
}

// one element's share of the five sums; `hit`: the element is in the system's support, gneg: g(i) = -1
__device__ __forceinline__ void loop_acc(double (&v)[SINGLET_RED], cplx a, bool hit, bool gneg, unsigned long long seed, unsigned long long i) {
  v[4] = fma(a.x, a.x, v[4]); v[4] = fma(a.y, a.y, v[4]);
  if (hit) {
    const int q = z4_power(seed, i);
    // conj(eta) psi = (-i)^q psi: psi, -i psi, -psi, i psi
    const double re = q == 0 ? a.x : q == 1 ? a.y : q == 2 ? -a.x : -a.y;
    const double im = q == 0 ? a.y : q == 1 ? -a.x : q == 2 ? -a.y : a.x;
    v[0] += re; v[1] += im;
    v[2] += gneg ? -re : re; v[3] += gneg ? -im : im;
  }
}

template <typename T, bool NT>
__global__ __launch_bounds__(BLOCK) void k_loops_timeslice(const void* __restrict__ psi, int hr, int Ly, int nc, Dilute dl, unsigned long long seed, int g5_mode,
                                                           long stride, BatchIdx ids, double* __restrict__ out) {
  typedef typename RawC<T>::type raw_t;
  __shared__ double res[SINGLET_RED];
  const int k = ids.id[blockIdx.x];
  const ClassOf cl = class_of(dl, dl.first_class + k);
  const int run = hr * nc;
  const int tid = threadIdx.x;
  const int c0 = tid % nc, cstep = BLOCK % nc;
  const char* x = reinterpret_cast<const char*>(psi) + (long)k * stride * (long)(2 * sizeof(T));
  for (int y = blockIdx.y; y < Ly; y += gridDim.y) {
    const bool row_in = (y % dl.nt) == cl.t;
    double v[SINGLET_RED] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int p = 0; p < 2; p++) {
      const long first = ((long)p * Ly + y) * run;     // the run's first element: its index in the vector is what the hash takes
      const bool run_in = row_in && (!dl.eo || p == cl.p);
      int r = tid, c = c0;
      auto in_class = [&](int cc) { return run_in && (!dl.spin || cc == cl.c); };
      auto minus = [&](int cc) { return g5_mode ? p == 1 : 2 * cc >= nc; };
      auto next_c = [&](int cc) { cc += cstep; return cc >= nc ? cc - nc : cc; };
      for (; r + 3 * BLOCK < run; r += 4 * BLOCK) {    // four elements in flight
        raw_t w[4];
#pragma unroll
        for (int u = 0; u < 4; u++) w[u] = NT ? ld_raw_nt<T>(x, first + r + u * BLOCK) : ld_raw<T>(x, first + r + u * BLOCK);
#pragma unroll
        for (int u = 0; u < 4; u++) {
          loop_acc(v, widen_rawc<T>(w[u]), in_class(c), minus(c), seed, (unsigned long long)(first + r + u * BLOCK));
          c = next_c(c);
        }
      }
      for (; r < run; r += BLOCK) {
        const raw_t w = NT ? ld_raw_nt<T>(x, first + r) : ld_raw<T>(x, first + r);
        loop_acc(v, widen_rawc<T>(w), in_class(c), minus(c), seed, (unsigned long long)(first + r));
        c = next_c(c);
      }
    }
    block_reduce_store<SINGLET_RED, false>(v, res);
    __syncthreads();
    if (tid < SINGLET_OUT) out[((long)k * Ly + y) * SINGLET_OUT + tid] = res[tid];
  }
}

// the calling thread's result slab of a qmg_loops_timeslice_batch that has no out_dev, held until qmg_shutdown
static thread_local ThreadScratch g_singlet;
void release_singlet_workspace() { g_singlet.release(); }

static Dilute make_dilute(int nc, int nt, int spin, int eo, int first_class) {
  Dilute dl;
  dl.nt = nt; dl.ncs = spin ? nc : 1; dl.neo = eo ? 2 : 1; dl.spin = spin; dl.eo = eo; dl.first_class = first_class;
  return dl;
}
// the vectors of a batch: nrhs of them, `stride` elements apart, none shorter than the lattice
static bool batch_ok(int dtype, const void* p, int Lx, int Ly, int nc, int nrhs, size_t stride) {
  if (!valid_dtype(dtype) || !p || !aligned16(p)) return false;
  return nrhs == 1 || stride >= (size_t)Lx * Ly * nc;
}

}  // namespace qmg

using namespace qmg;

extern "C" {

int qmg_singlet_plan(int Lx, int Ly, int nc, int nt, int spin, int eo, int first_class, int nrhs, unsigned mask, int* out, int n_out) {
  if (!out || n_out < SINGLET_PLAN_INTS) return QMG_ERR_INVALID;
  const SingletPlan pl = singlet_plan(Lx, Ly, nc, nt, spin, eo, first_class, nrhs, mask);
  const int v[SINGLET_PLAN_INTS] = {pl.family, pl.block, pl.gx, pl.gy, pl.walk, pl.lds, pl.doubles, pl.dgx, pl.dgy, pl.dwalk, pl.nk, pl.classes};
  for (int i = 0; i < n_out; i++) out[i] = i < SINGLET_PLAN_INTS ? v[i] : -1;
  return pl.status;
}

int qmg_noise_z4(void* eta, size_t n, unsigned long long seed, void* stream) {
  if (!eta && n) return QMG_ERR_INVALID;
  if (n == 0) return QMG_SUCCESS;
  k_noise_z4<<<grid_1d(n), BLOCK, 0, as_stream(stream)>>>((cplx*)eta, (long)n, seed);
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

int qmg_noise_dilute_batch(int dtype, void* out, int Lx, int Ly, int nc, int nt, int spin, int eo, int first_class, unsigned long long seed, int nrhs,
                           size_t stride, unsigned mask, void* stream) {
  const SingletPlan pl = singlet_plan(Lx, Ly, nc, nt, spin, eo, first_class, nrhs, mask);
  if (pl.family == SGF_INVALID || !batch_ok(dtype, out, Lx, Ly, nc, nrhs, stride)) return QMG_ERR_INVALID;
  if (pl.family == SGF_NONE) return QMG_SUCCESS;
  const Dilute dl = make_dilute(nc, nt, spin, eo, first_class);
  const BatchIdx ids = expand_mask(mask, nrhs);
  const dim3 grid((unsigned)pl.dgx, (unsigned)pl.dgy);
  hipStream_t st = as_stream(stream);
  if (dtype == QMG_C64) k_noise_dilute<double><<<grid, pl.block, 0, st>>>(out, Lx / 2, Ly, nc, dl, seed, (long)stride, ids);
  else k_noise_dilute<float><<<grid, pl.block, 0, st>>>(out, Lx / 2, Ly, nc, dl, seed, (long)stride, ids);
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

int qmg_loops_timeslice_batch(int dtype, const void* psi, int Lx, int Ly, int nc, int nt, int spin, int eo, int first_class, unsigned long long seed,
                              int g5_mode, int nrhs, size_t stride, unsigned mask, double* out_dev, double* out_host, void* stream) {
  const SingletPlan pl = singlet_plan(Lx, Ly, nc, nt, spin, eo, first_class, nrhs, mask);
  if (pl.family == SGF_INVALID || !batch_ok(dtype, psi, Lx, Ly, nc, nrhs, stride) || (!out_dev && !out_host)) return QMG_ERR_INVALID;
  if ((g5_mode != 0 && g5_mode != 1) || (g5_mode == 0 && (nc & 1))) return QMG_ERR_INVALID;
  if (pl.family == SGF_NONE) return QMG_SUCCESS;
  const size_t per_sys = (size_t)SINGLET_OUT * Ly;
  double* res = out_dev;
  if (!res)
    if (int rc = g_singlet.grow(per_sys * nrhs * sizeof(double), &res)) return rc;
  const Dilute dl = make_dilute(nc, nt, spin, eo, first_class);
  const BatchIdx ids = expand_mask(mask, nrhs);
  const size_t n = (size_t)Lx * Ly * nc;
  const bool nt_loads = g_blas_nt_bytes > 0 && (long)(n * dtype_size(dtype) * ids.n) >= g_blas_nt_bytes;
  const dim3 grid((unsigned)pl.gx, (unsigned)pl.gy);
  hipStream_t st = as_stream(stream);
  const int hr = Lx / 2;
  if (dtype == QMG_C64) {
    if (nt_loads) k_loops_timeslice<double, true><<<grid, pl.block, 0, st>>>(psi, hr, Ly, nc, dl, seed, g5_mode, (long)stride, ids, res);
    else k_loops_timeslice<double, false><<<grid, pl.block, 0, st>>>(psi, hr, Ly, nc, dl, seed, g5_mode, (long)stride, ids, res);
  } else {
    if (nt_loads) k_loops_timeslice<float, true><<<grid, pl.block, 0, st>>>(psi, hr, Ly, nc, dl, seed, g5_mode, (long)stride, ids, res);
    else k_loops_timeslice<float, false><<<grid, pl.block, 0, st>>>(psi, hr, Ly, nc, dl, seed, g5_mode, (long)stride, ids, res);
  }
  QMG_LAUNCH_CHECK();
  if (out_host) {   // the active systems only, runs of neighbours in one copy: a frozen system's entries stay as they are
    for (int a = 0; a < ids.n;) {
      int b = a + 1;
      while (b < ids.n && ids.id[b] == ids.id[b - 1] + 1) b++;
      const size_t off = per_sys * ids.id[a];
      QMG_HIP_CHECK(hipMemcpyAsync(out_host + off, res + off, per_sys * (size_t)(b - a) * sizeof(double), hipMemcpyDeviceToHost, st));
      a = b;
    }
    QMG_HIP_CHECK(hipStreamSynchronize(st));
  }
  return QMG_SUCCESS;
}

}  // extern "C"
