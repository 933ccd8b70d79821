// qmg_dwf_meas.hip -- what turns a domain-wall solve into physical numbers: the wall source of a 4D field, the wall and midpoint projections of
// a 5D field, and the per-timeslice, per-slice norms N(y, s, sigma) = sum_x |psi(x, y; s, sigma)|^2 in one pass over the vector.
//
// Component c = 2 s + sigma; sigma = 0 is the P_+ component (it hops s -> s+1 and crosses the wall as out(0, 0) += m psi(Ls-1, 0)), sigma = 1 P_-.
//   wall source    B(x; 0, 0) = eta(x, 0),  B(x; Ls-1, 1) = eta(x, 1),  zero elsewhere            32 Ls + 32 B/site in fp64
//   physical q     q(x, 0) = psi(x; Ls-1, 0),  q(x, 1) = psi(x; 0, 1)                             reads the two half chunks it needs
//   midpoint q     q(x, 0) = psi(x; Ls/2-1, 0),  q(x, 1) = psi(x; Ls/2, 1)   (even Ls)
//   slice norms    out[sys][y][s][sigma], fp64 accumulation in both precisions                    32 Ls B/site in fp64
//
// Lane mapping of the source and the norms: kernel D's (qmg_dwf.hip) -- one lane per (site, s) with the two spin components as one chunk,
// lanes along c and then along x, rows (parity, y) over grid.y with block-uniform bases; the systems of a batch over grid.z.  The
// projections take one lane per (site, sigma).
// The norms: the block is Ls floor(256 / Ls) lanes and the gx = pbr blocks of a row stride over the half row by gx whole blocks, so a lane
// keeps its s and carries two fp64 accumulators.  The lanes of a block with the same s are summed through LDS in lane order by the first
// 2 Ls lanes (nothing depends on how Ls divides the wavefront), which write one partial per (system, row, block, c) into the calling thread's
// device scratch; a second launch adds the 2 pbr partials of a timeslice -- even row first, blocks in index order.  Two plain launches, no
// atomics: the result is the same bits on every run.
#include "qmg_dwf_meas_plan.h"
#include "qmg_lane.h"   // uni, gld

namespace qmg {

template <typename T>
__global__ __launch_bounds__(DWF_BLOCK_MAX) void k_dwf_wall_source(void* __restrict__ psi5, const void* __restrict__ eta4, int hr, int Ls, int nrows,
                                                                        long stride5_bytes, long stride4_bytes) {
  typedef T v4 __attribute__((ext_vector_type(4)));   // a lane's chunk: (sigma 0 re, im, sigma 1 re, im)
  typedef T v2 __attribute__((ext_vector_type(2)));
  constexpr unsigned CH = 4u * sizeof(T);
  const dwf::Lane ln = dwf::lane_of<false>(hr, Ls);
  if (!ln.live) return;
  const int t = ln.t, j = ln.j, s = ln.s;
  const long row5 = (long)hr * Ls * CH, row4 = (long)hr * CH;   // a 4D site is one chunk too
  char* out = reinterpret_cast<char*>(psi5) + blockIdx.z * stride5_bytes;
  const char* in = reinterpret_cast<const char*>(eta4) + blockIdx.z * stride4_bytes;
  for (int row = blockIdx.y; row < nrows; row += gridDim.y) {
    const gchar* src = uni(in + row * row4);
    gchar* dst = uni(out + row * row5);
    v4 o = {(T)0, (T)0, (T)0, (T)0};
    if (s == 0) { const v2 e = gld<v2>(src, (unsigned)j * CH); o.x = e.x; o.y = e.y; }
    if (s == Ls - 1) { const v2 e = gld<v2>(src, (unsigned)j * CH + CH / 2); o.z = e.x; o.w = e.y; }
    // a plain store: the non-temporal one takes 0.44 ms against 0.28 ms at 2048^2, Ls = 8 in fp64 (profiles/dwf_meas_bench.txt)
    *(__attribute__((address_space(1))) v4*)(dst + (unsigned)t * CH) = o;
  }
}

// s0, s1: the slices sigma = 0 and sigma = 1 are taken from
template <typename T>
__global__ __launch_bounds__(DWF_BLOCK_MAX) void k_dwf_wall_project(void* __restrict__ q4, const void* __restrict__ psi5, int hr, int Ls, int nrows, int s0, int s1,
                                                                         long stride4_bytes, long stride5_bytes) {
  typedef T v2 __attribute__((ext_vector_type(2)));
  constexpr unsigned CH = 4u * sizeof(T);
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= hr * 2) return;
  const int j = t >> 1, sg = t & 1;
  const unsigned off_src = (unsigned)(j * Ls + (sg ? s1 : s0)) * CH + (unsigned)sg * (CH / 2);
  const long row5 = (long)hr * Ls * CH, row4 = (long)hr * CH;
  char* out = reinterpret_cast<char*>(q4) + blockIdx.z * stride4_bytes;
  const char* in = reinterpret_cast<const char*>(psi5) + blockIdx.z * stride5_bytes;
  for (int row = blockIdx.y; row < nrows; row += gridDim.y) {
    const v2 e = gld<v2>(uni(in + row * row5), off_src);
    *(__attribute__((address_space(1))) v2*)(uni(out + row * row4) + (unsigned)t * (CH / 2)) = e;
  }
}

// part[((sys * nrows + row) * gridDim.x + blockIdx.x) * 2 Ls + c]
template <typename T>
__global__ __launch_bounds__(DWF_BLOCK_MAX) void k_dwf_slice_norms(const void* __restrict__ psi5, int hr, int Ls, int nrows, long stride5_bytes,
                                                                        double* __restrict__ part) {
  typedef T v4 __attribute__((ext_vector_type(4)));
  constexpr unsigned CH = 4u * sizeof(T);
  __shared__ double sm[DWF_BLOCK_MAX][2];
  const int tid = threadIdx.x;
  const int lanes = hr * Ls;                         // of a half row
  const int step = gridDim.x * blockDim.x;           // a multiple of Ls: the lane keeps its s
  const int t0 = blockIdx.x * blockDim.x + tid;
  const int groups = blockDim.x / Ls;                // sites of a block
  const long row5 = (long)lanes * CH;
  const char* x = reinterpret_cast<const char*>(psi5) + blockIdx.z * stride5_bytes;
  for (int row = blockIdx.y; row < nrows; row += gridDim.y) {
    const gchar* base = uni(x + row * row5);
    double a0 = 0.0, a1 = 0.0;
    int t = t0;
    for (; t + 3 * step < lanes; t += 4 * step) {    // four chunks in flight
      v4 v[4];
#pragma unroll
      for (int u = 0; u < 4; u++) v[u] = gld<v4>(base, (unsigned)(t + u * step) * CH);
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const double re0 = (double)v[u].x, im0 = (double)v[u].y, re1 = (double)v[u].z, im1 = (double)v[u].w;
        a0 = fma(re0, re0, a0); a0 = fma(im0, im0, a0);
        a1 = fma(re1, re1, a1); a1 = fma(im1, im1, a1);
      }
    }
    for (; t < lanes; t += step) {
      const v4 v = gld<v4>(base, (unsigned)t * CH);
      const double re0 = (double)v.x, im0 = (double)v.y, re1 = (double)v.z, im1 = (double)v.w;
      a0 = fma(re0, re0, a0); a0 = fma(im0, im0, a0);
      a1 = fma(re1, re1, a1); a1 = fma(im1, im1, a1);
    }
    sm[tid][0] = a0; sm[tid][1] = a1;
    __syncthreads();
    if (tid < 2 * Ls) {                              // c = tid: lane g Ls + s holds (s, 0) and (s, 1), i.e. doubles g 2 Ls + c of sm
      const double* col = &sm[0][0] + tid;
      double r = 0.0;
      for (int g = 0; g < groups; g++) r += col[g * 2 * Ls];
      part[(((long)blockIdx.z * nrows + row) * gridDim.x + blockIdx.x) * (2 * Ls) + tid] = r;
    }
    __syncthreads();
  }
}

// out[sys][y][c] = the partials of the even row y, then of the odd row y, blocks in index order
__global__ __launch_bounds__(BLOCK) void k_dwf_slice_sum(const double* __restrict__ part, int Ly, int nc, int pbr, long total, double* __restrict__ out) {
  for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < total; i += (long)gridDim.x * BLOCK) {
    const int c = (int)(i % nc);
    const long sy = i / nc;
    const int y = (int)(sy % Ly);
    const long sys = sy / Ly;
    double r = 0.0;
    for (int p = 0; p < 2; p++) {
      const double* src = part + ((sys * 2 * Ly + (long)p * Ly + y) * pbr) * nc + c;
      for (int b = 0; b < pbr; b++) r += src[(long)b * nc];
    }
    out[i] = r;
  }
}

// the calling thread's partial slab and result of qmg_dwf_slice_norms, held until qmg_shutdown
static thread_local ThreadScratch g_meas;
void release_dwf_meas_workspace() { g_meas.release(); }

// what every entry checks before the plan is asked; has4: the entry takes 4D vectors too
static int meas_valid(int dtype, int Lx, int Ly, int Ls, int nsys, size_t stride5, size_t stride4, bool has4) {
  if (!valid_lattice(Lx, Ly)) return QMG_ERR_INVALID;
  return dwf_entry_check(dtype, Lx, Ly, Ls, nsys, stride5, stride4, has4);
}

}  // namespace qmg

using namespace qmg;

extern "C" {

int qmg_dwf_meas_plan(int dtype, int Lx, int Ly, int Ls, int kernel, int nsys, int* plan_out, int plan_len) {
  if (!plan_out || plan_len < DWF_MEAS_PLAN_INTS) return QMG_ERR_INVALID;
  const DwfMeasPlan pl = dwf_meas_plan(dtype, Lx, Ly, Ls, kernel, nsys);
  const int v[DWF_MEAS_PLAN_INTS] = {pl.family, pl.lps, pl.block, pl.gx, pl.gy, pl.pbr, pl.lds, pl.nk};
  export_plan_ints(v, DWF_MEAS_PLAN_INTS, plan_out, plan_len);
  return QMG_SUCCESS;
}

int qmg_dwf_wall_source(int dtype, int Lx, int Ly, int Ls, void* psi5, const void* eta4, int nsys, size_t stride5, size_t stride4, void* stream) {
  if (!psi5 || !eta4 || !aligned16(psi5) || !aligned16(eta4)) return QMG_ERR_INVALID;
  if (int rc = meas_valid(dtype, Lx, Ly, Ls, nsys, stride5, stride4, true)) return rc;
  const DwfMeasPlan pl = dwf_meas_plan(dtype, Lx, Ly, Ls, DMK_SOURCE, nsys);
  if (pl.family != DMF_SOURCE) return pl.status;
  const long eb = (long)dtype_size(dtype);
  const dim3 grid((unsigned)pl.gx, (unsigned)pl.gy, (unsigned)pl.nk);
  hipStream_t st = as_stream(stream);
  if (dtype == QMG_C64) k_dwf_wall_source<double><<<grid, pl.block, 0, st>>>(psi5, eta4, Lx / 2, Ls, 2 * Ly, (long)stride5 * eb, (long)stride4 * eb);
  else k_dwf_wall_source<float><<<grid, pl.block, 0, st>>>(psi5, eta4, Lx / 2, Ls, 2 * Ly, (long)stride5 * eb, (long)stride4 * eb);
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

int qmg_dwf_wall_project(int dtype, int Lx, int Ly, int Ls, void* q4, const void* psi5, int which, int nsys, size_t stride4, size_t stride5, void* stream) {
  if (!q4 || !psi5 || !aligned16(q4) || !aligned16(psi5) || (which != 0 && which != 1)) return QMG_ERR_INVALID;
  if (int rc = meas_valid(dtype, Lx, Ly, Ls, nsys, stride5, stride4, true)) return rc;
  const DwfMeasPlan pl = dwf_meas_plan(dtype, Lx, Ly, Ls, which ? DMK_PROJECT_MID : DMK_PROJECT_WALL, nsys);
  if (pl.family != DMF_PROJECT) return pl.status;
  const int s0 = which ? Ls / 2 - 1 : Ls - 1, s1 = which ? Ls / 2 : 0;
  const long eb = (long)dtype_size(dtype);
  const dim3 grid((unsigned)pl.gx, (unsigned)pl.gy, (unsigned)pl.nk);
  hipStream_t st = as_stream(stream);
  if (dtype == QMG_C64) k_dwf_wall_project<double><<<grid, pl.block, 0, st>>>(q4, psi5, Lx / 2, Ls, 2 * Ly, s0, s1, (long)stride4 * eb, (long)stride5 * eb);
  else k_dwf_wall_project<float><<<grid, pl.block, 0, st>>>(q4, psi5, Lx / 2, Ls, 2 * Ly, s0, s1, (long)stride4 * eb, (long)stride5 * eb);
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

int qmg_dwf_slice_norms(int dtype, int Lx, int Ly, int Ls, const void* psi5, int nsys, size_t stride5, double* out_dev, double* out_host, void* stream) {
  if (!psi5 || !aligned16(psi5) || (!out_dev && !out_host)) return QMG_ERR_INVALID;
  if (int rc = meas_valid(dtype, Lx, Ly, Ls, nsys, stride5, 0, false)) return rc;
  const DwfMeasPlan pl = dwf_meas_plan(dtype, Lx, Ly, Ls, DMK_NORMS, nsys);
  if (pl.family != DMF_NORMS) return pl.status;
  const int nc = 2 * Ls, nrows = 2 * Ly;
  const size_t n_part = (size_t)nsys * nrows * pl.pbr * nc, n_out = (size_t)nsys * Ly * nc;
  double* part;
  if (int rc = g_meas.grow((n_part + n_out) * sizeof(double), &part)) return rc;
  double* res = out_dev ? out_dev : part + n_part;
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)pl.gx, (unsigned)pl.gy, (unsigned)pl.nk);
  const long sb = (long)stride5 * (long)dtype_size(dtype);
  if (dtype == QMG_C64) k_dwf_slice_norms<double><<<grid, pl.block, 0, st>>>(psi5, Lx / 2, Ls, nrows, sb, part);
  else k_dwf_slice_norms<float><<<grid, pl.block, 0, st>>>(psi5, Lx / 2, Ls, nrows, sb, part);
  QMG_LAUNCH_CHECK();
  k_dwf_slice_sum<<<grid_1d(n_out), BLOCK, 0, st>>>(part, Ly, nc, pl.pbr, (long)n_out, res);
  QMG_LAUNCH_CHECK();
  if (out_host) {
    QMG_HIP_CHECK(hipMemcpyAsync(out_host, res, n_out * sizeof(double), hipMemcpyDeviceToHost, st));
    QMG_HIP_CHECK(hipStreamSynchronize(st));
  }
  return QMG_SUCCESS;
}

}  // extern "C"
