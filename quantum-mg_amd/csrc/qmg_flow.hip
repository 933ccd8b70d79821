// qmg_flow.hip -- gradient (Wilson) flow and planar Wilson / Polyakov loops for compact U(1) in two dimensions; fp64 only, single domain.
// Not in the reference (u1/u1_utils.h stops at plaquette, topology and APE): the independent statement is tests/flow_numpy.py.
//
//   d theta_mu(x) / dt = - dS_w / d theta_mu(x),   S_w = sum_x (1 - cos P(x)),   P(x) = theta_x(x) + theta_y(x+xhat) - theta_x(x+yhat) - theta_y(x)
//   dS_w/dtheta_x(x) = sin P(x) - sin P(x-yhat)          dS_w/dtheta_y(x) = -sin P(x) + sin P(x-xhat)
// -- the gauge force of qmg_hmc_momentum_update (qmg_hmc.hip) at beta = 1.  Luescher's third-order Runge-Kutta scheme (JHEP 08 (2010) 071,
// appendix C), which for an abelian group needs two registers per link: with Z(theta) = -eps dS_w/dtheta,
//   stage 1:  A = Z(theta)                      theta += A / 4
//   stage 2:  A = 8/9 Z(theta) - 17/36 A        theta += A
//   stage 3:  A = 3/4 Z(theta) - A              theta += A
//
// Layouts (lattice.h:75-81): site (x, y) has index (y + p Ly) Lx/2 + x/2, p = (x + y) & 1; phases, accumulator and links are [mu][site].
#include "qmg_common.h"

namespace qmg {

__device__ __forceinline__ double flow_im_plaq(cplx a, cplx b, cplx c, cplx d) {   // Im[ a b conj(c) conj(d) ]
  const cplx ab = cmul(a, b), cd = cmul(c, d);
  return fma(ab.y, cd.x, -ab.x * cd.y);
}

// the two-register update of one link; returns the new phase
template <int STAGE>
__device__ __forceinline__ double flow_link(double th, double* __restrict__ acc, long i, double a_old, double z) {
  double a;
  if (STAGE == 1) a = z;
  else if (STAGE == 2) a = fma(8.0 / 9.0, z, -(17.0 / 36.0) * a_old);
  else a = fma(0.75, z, -a_old);
  acc[i] = a;
  return (STAGE == 1) ? fma(0.25, a, th) : th + a;
}

// One Runge-Kutta stage in one pass.  The thread mapping of k_ape_smear (qmg_u1.hip) and k_hmc_momentum_update (qmg_hmc.hip): a thread owns the
// two sites (2 xh, y) and (2 xh + 1, y) -- one of each parity, at the same offset xh of their rows, so every load and store of a wave is one
// contiguous run -- and updates all four of their links.  It loads 15 links of `in` (the five plaquettes P(a), P(b), P(a-y), P(b-y), P(a-x);
// P(b-x) = P(a)), four phases and, from stage 2 on, four accumulators; all loads are unconditional and sit in front of the arithmetic
// (DESIGN 10.6b); every index is a wrapped lattice coordinate, so nothing is read or written outside the fields.  sin P is the imaginary
// part of the plaquette of the links: the only trigonometry is the sincos of the four new phases.  out != in (neighbours are read from in).
// Byte model: 128 B/site -- theta read and written (32), acc read and written (32; stage 1 only writes), two links read (32), two written (32).
template <int STAGE>
__global__ __launch_bounds__(BLOCK) void k_flow_stage(double* __restrict__ theta, double* __restrict__ acc, cplx* __restrict__ out,
                                                      const cplx* __restrict__ in, int Lx, int Ly, double eps) {
  const long V = (long)Lx * Ly;
  const int h = Lx >> 1;
  const long npairs = V / 2;
  const cplx* __restrict__ Ux = in;
  const cplx* __restrict__ Uy = in + V;
  for (long t = (long)blockIdx.x * BLOCK + threadIdx.x; t < npairs; t += (long)gridDim.x * BLOCK) {
    const int xh = (int)(t % h), y = (int)(t / h);
    const int yp = (y + 1 == Ly) ? 0 : y + 1, ym = (y == 0) ? Ly - 1 : y - 1;
    const int xl = (xh == 0) ? h - 1 : xh - 1, xr = (xh + 1 == h) ? 0 : xh + 1;
    // a: the even-x site of the pair, b: the odd-x one; l: the odd-x site left of a, r: the even-x site right of b
    const int q = y & 1, qp = yp & 1, qm = ym & 1;
    const long ra = (long)(y + q * Ly) * h, rb = (long)(y + (1 - q) * Ly) * h;          // rows of even-x / odd-x sites at y
    const long rap = (long)(yp + qp * Ly) * h, rbp = (long)(yp + (1 - qp) * Ly) * h;    // at y + 1
    const long ram = (long)(ym + qm * Ly) * h, rbm = (long)(ym + (1 - qm) * Ly) * h;    // at y - 1
    const long sa = ra + xh, sb = rb + xh;
    const double tax = theta[sa], tay = theta[V + sa], tbx = theta[sb], tby = theta[V + sb];
    double aax = 0.0, aay = 0.0, abx = 0.0, aby = 0.0;
    if (STAGE != 1) { aax = acc[sa]; aay = acc[V + sa]; abx = acc[sb]; aby = acc[V + sb]; }
    const cplx ax = Ux[sa], ay = Uy[sa], bx = Ux[sb], by = Uy[sb];
    const cplx apx = Ux[rap + xh], bpx = Ux[rbp + xh];
    const cplx amx = Ux[ram + xh], amy = Uy[ram + xh], bmx = Ux[rbm + xh], bmy = Uy[rbm + xh];
    const cplx lx = Ux[rb + xl], ly = Uy[rb + xl], lpx = Ux[rbp + xl];
    const cplx ry = Uy[ra + xr], rmy = Uy[ram + xr];

    // sin P: a + x = b, a + y = ap, b + x = r, (a-y) + x = b-y, (a-y) + y = a, l + x = a
    const double sPa = flow_im_plaq(ax, by, apx, ay), sPb = flow_im_plaq(bx, ry, bpx, by);
    const double sPam = flow_im_plaq(amx, bmy, ax, amy), sPbm = flow_im_plaq(bmx, rmy, bx, bmy);
    const double sPl = flow_im_plaq(lx, ay, lpx, ly);
    const double nax = flow_link<STAGE>(tax, acc, sa, aax, -eps * (sPa - sPam));
    const double nay = flow_link<STAGE>(tay, acc, V + sa, aay, -eps * (sPl - sPa));
    const double nbx = flow_link<STAGE>(tbx, acc, sb, abx, -eps * (sPb - sPbm));
    const double nby = flow_link<STAGE>(tby, acc, V + sb, aby, -eps * (sPa - sPb));
    double s, c;
    theta[sa] = nax;     sincos(nax, &s, &c); out[sa] = cmake(c, s);
    theta[V + sa] = nay; sincos(nay, &s, &c); out[V + sa] = cmake(c, s);
    theta[sb] = nbx;     sincos(nbx, &s, &c); out[sb] = cmake(c, s);
    theta[V + sb] = nby; sincos(nby, &s, &c); out[V + sb] = cmake(c, s);
  }
}

// ---------------- Wilson loops from running line products ----------------
// Thread t is STORAGE index t: row = t / h = y + p Ly, so x = 2 (t % h) + (p ^ (y & 1)).  Every access below is a contiguous run of a wave
// (a shifted row of the same or the other parity), up to the wrap in x.
__device__ __forceinline__ long flow_eo(int x, int y, int h, int Ly) {
  const int p = (x + y) & 1;
  return (long)(y + p * Ly) * h + (x >> 1);
}

// out(x) = line(x) U_mu(x + k mu)   (line == nullptr: out = U_mu, k = 0).  In place is allowed: the kernel is pointwise in `line`.
__global__ __launch_bounds__(BLOCK) void k_line_extend(cplx* out, const cplx* line, const cplx* __restrict__ U, int Lx, int Ly, int mu, int k) {
  const long V = (long)Lx * Ly;
  const int h = Lx >> 1;
  for (long t = (long)blockIdx.x * BLOCK + threadIdx.x; t < V; t += (long)gridDim.x * BLOCK) {
    const int row = (int)(t / h), xh = (int)(t % h);
    const int p = row >= Ly, y = row - p * Ly, x = 2 * xh + (p ^ (y & 1));
    const int xs = (mu == 0) ? (x + k) % Lx : x, ys = (mu == 0) ? y : (y + k) % Ly;
    const cplx u = U[flow_eo(xs, ys, h, Ly)];
    out[t] = line ? cmul(line[t], u) : u;
  }
}

// per-block partial sums of W_{R,T}(x) = LX_R(x) LY_T(x + R xhat) conj LX_R(x + T yhat) conj LY_T(x): four 16-byte reads per site
__global__ __launch_bounds__(BLOCK) void k_wilson_loop(const cplx* __restrict__ LX, const cplx* __restrict__ LY, int Lx, int Ly, int R, int T, double* __restrict__ partials) {
  const long V = (long)Lx * Ly;
  const int h = Lx >> 1;
  double v[2] = {0.0, 0.0};
  for (long t = (long)blockIdx.x * BLOCK + threadIdx.x; t < V; t += (long)gridDim.x * BLOCK) {
    const int row = (int)(t / h), xh = (int)(t % h);
    const int p = row >= Ly, y = row - p * Ly, x = 2 * xh + (p ^ (y & 1));
    const cplx a = LX[t], d = LY[t];
    const cplx b = LY[flow_eo((x + R) % Lx, y, h, Ly)], c = LX[flow_eo(x, (y + T) % Ly, h, Ly)];
    const cplx ab = cmul(a, b), cd = cmul(c, d);   // W = ab conj(cd)
    v[0] += fma(ab.x, cd.x, ab.y * cd.y);
    v[1] += fma(ab.y, cd.x, -ab.x * cd.y);
  }
  __shared__ double sm[2][BLOCK / WAVE];
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
#pragma unroll
  for (int q = 0; q < 2; q++) {
    const double w = wave_sum(v[q]);
    if (lane == 0) sm[q][wv] = w;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    double t = 0.0;
    for (int w = 0; w < BLOCK / WAVE; w++) t += sm[threadIdx.x][w];
    partials[(long)blockIdx.x * 2 + threadIdx.x] = t;
  }
}
// second stage, as k_sum3 of the plaquette (qmg_u1.hip): a fixed order, so the result is deterministic; out = sum * scale
__global__ void k_loop_sum2(const double* __restrict__ partials, int nparts, double scale, double* __restrict__ out) {
  if (threadIdx.x < 2) {
    double t = 0.0;
    for (int i = 0; i < nparts; i++) t += partials[(long)i * 2 + threadIdx.x];
    out[threadIdx.x] = t * scale;
  }
}

// Polyakov loops: thread l < Ly multiplies the x-links of row y = l, thread Ly + l the y-links of column x = l; the products go to
// lines[l] and lines[Ly + l] and are averaged by the caller's k_polyakov_mean.  O(V) reads in all: an observable, not a hot path.
__global__ __launch_bounds__(BLOCK) void k_polyakov_lines(const cplx* __restrict__ gauge, int Lx, int Ly, cplx* __restrict__ lines) {
  const long V = (long)Lx * Ly;
  const int h = Lx >> 1;
  const int l = blockIdx.x * BLOCK + threadIdx.x;
  if (l >= Lx + Ly) return;
  cplx p = cmake(1.0, 0.0);
  if (l < Ly) for (int x = 0; x < Lx; x++) p = cmul(p, gauge[flow_eo(x, l, h, Ly)]);
  else for (int y = 0; y < Ly; y++) p = cmul(p, gauge[V + flow_eo(l - Ly, y, h, Ly)]);
  lines[l] = p;
}
__global__ void k_polyakov_mean(const cplx* __restrict__ lines, int Lx, int Ly, double* __restrict__ out) {
  if (threadIdx.x < 2) {   // thread 0: x direction (Ly lines), thread 1: y direction (Lx lines); fixed order
    const int n = threadIdx.x ? Lx : Ly, first = threadIdx.x ? Ly : 0;
    double re = 0.0, im = 0.0;
    for (int i = 0; i < n; i++) { re += lines[first + i].x; im += lines[first + i].y; }
    out[2 * threadIdx.x] = re / n;
    out[2 * threadIdx.x + 1] = im / n;
  }
}

// the calling thread's scratch of qmg_u1_flow (a link field and the accumulator) and of qmg_u1_wilson_loops (two line-product fields),
// grown on demand and held until qmg_shutdown like the APE scratch field
struct FlowScratch { void* buf = nullptr; size_t bytes = 0; int device = -1; };
static thread_local FlowScratch g_flow;

static int flow_scratch(size_t bytes, void** out) {
  int dev = 0;
  QMG_HIP_CHECK(hipGetDevice(&dev));
  if (g_flow.device != dev || g_flow.bytes < bytes) {
    if (g_flow.buf && g_flow.device == dev) QMG_HIP_CHECK(hipFree(g_flow.buf));   // waits for the device: nothing still reads it
    g_flow = FlowScratch();
    QMG_HIP_CHECK(hipMalloc(&g_flow.buf, bytes));
    g_flow.bytes = bytes;
    g_flow.device = dev;
  }
  *out = g_flow.buf;
  return QMG_SUCCESS;
}

void release_flow_workspace() {   // qmg_shutdown (qmg_runtime.hip)
  if (g_flow.buf) hipFree(g_flow.buf);
  g_flow = FlowScratch();
}

static bool fields_overlap(const void* a, size_t abytes, const void* b, size_t bbytes) {
  return (const char*)a < (const char*)b + bbytes && (const char*)b < (const char*)a + abytes;
}

static int launch_stage(double* theta, double* acc, cplx* out, const cplx* in, int Lx, int Ly, double eps, int stage, hipStream_t st) {
  const unsigned g = grid_1d((size_t)Lx * Ly / 2);
  if (stage == 1) k_flow_stage<1><<<g, BLOCK, 0, st>>>(theta, acc, out, in, Lx, Ly, eps);
  else if (stage == 2) k_flow_stage<2><<<g, BLOCK, 0, st>>>(theta, acc, out, in, Lx, Ly, eps);
  else k_flow_stage<3><<<g, BLOCK, 0, st>>>(theta, acc, out, in, Lx, Ly, eps);
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

}  // namespace qmg

using namespace qmg;

extern "C" {

// One stage (1, 2 or 3) of the Runge-Kutta step, one launch: Z = -eps dS_w/dtheta from the links gauge_in, the accumulator and the phases
// updated in place (stage 1 does not read acc), gauge_out = exp(i theta).  theta, acc: DEVICE double[2 Lx Ly]; gauge_in, gauge_out: DEVICE
// complex<double>[2 Lx Ly], DIFFERENT buffers (neighbours are read from gauge_in); gauge_in must hold exp(i theta).
int qmg_u1_flow_stage(double* theta, double* acc, void* gauge_out, const void* gauge_in, int Lx, int Ly, double eps, int stage, void* stream) {
  if (!theta || !acc || !gauge_out || !gauge_in || !valid_lattice(Lx, Ly) || eps != eps || stage < 1 || stage > 3) return QMG_ERR_INVALID;
  const size_t n = 2 * (size_t)Lx * Ly;
  if (fields_overlap(gauge_out, sizeof(cplx) * n, gauge_in, sizeof(cplx) * n) || fields_overlap(theta, sizeof(double) * n, acc, sizeof(double) * n)) return QMG_ERR_INVALID;
  return launch_stage(theta, acc, (cplx*)gauge_out, (const cplx*)gauge_in, Lx, Ly, eps, stage, as_stream(stream));
}

// n_steps Runge-Kutta steps of size eps: flow time n_steps * eps.  theta: DEVICE double[2 Lx Ly]; gauge: DEVICE complex<double>[2 Lx Ly], exp(i theta)
// on entry (qmg_u1_phase_to_gauge) and on return.  The 3 n_steps launches ping-pong between `gauge` and the calling thread's scratch link
// field; an odd n_steps ends there and is copied over.  n_steps == 0 or eps == 0 leave both fields as they are, bit for bit.
int qmg_u1_flow(double* theta, void* gauge, int Lx, int Ly, double eps, int n_steps, void* stream) {
  if (!theta || !gauge || !valid_lattice(Lx, Ly) || eps != eps || n_steps < 0) return QMG_ERR_INVALID;
  if (n_steps == 0 || eps == 0.0) return QMG_SUCCESS;
  const size_t n = 2 * (size_t)Lx * Ly;
  void* buf = nullptr;
  int rc = flow_scratch((sizeof(cplx) + sizeof(double)) * n, &buf);
  if (rc) return rc;
  cplx* ends[2] = {(cplx*)gauge, (cplx*)buf};
  double* acc = (double*)((cplx*)buf + n);
  hipStream_t st = as_stream(stream);
  int src = 0;
  for (int i = 0; i < n_steps; i++)
    for (int stage = 1; stage <= 3; stage++) {
      rc = launch_stage(theta, acc, ends[1 - src], ends[src], Lx, Ly, eps, stage, st);
      if (rc) return rc;
      src = 1 - src;
    }
  return src ? qmg_copy_vector(gauge, buf, n, stream) : QMG_SUCCESS;
}

// Lattice averages of the planar R x T Wilson loops, 1 <= R <= r_max <= Lx/2, 1 <= T <= t_max <= Ly/2:
// out_host[2 ((R-1) t_max + (T-1))] and [.. + 1] are the real and imaginary part.  Running line products LX_R(x) = prod_{k<R} U_x(x + k xhat),
// LY_T(x) = prod_{k<T} U_y(x + k yhat) are extended in place by one link per pass, so a pair (R, T) costs two passes over the lattice (the
// extension of LY and the loop itself) whatever its perimeter.  Synchronous; the line products live in the calling thread's scratch.
int qmg_u1_wilson_loops(const void* gauge, int Lx, int Ly, int r_max, int t_max, double* out_host, void* stream) {
  if (!gauge || !out_host || !valid_lattice(Lx, Ly) || r_max < 1 || t_max < 1 || r_max > Lx / 2 || t_max > Ly / 2) return QMG_ERR_INVALID;
  const size_t V = (size_t)Lx * Ly, npairs = (size_t)r_max * t_max;
  const unsigned g = grid_1d(V);
  unsigned nb = (unsigned)((V + BLOCK - 1) / BLOCK);
  if (nb > 1024) nb = 1024;
  void* buf = nullptr;
  int rc = flow_scratch(sizeof(cplx) * 2 * V + sizeof(double) * 2 * (nb + npairs), &buf);
  if (rc) return rc;
  cplx* LX = (cplx*)buf;
  cplx* LY = LX + V;
  double* partials = (double*)(LY + V);
  double* results = partials + 2 * nb;
  const cplx* Ux = (const cplx*)gauge;
  const cplx* Uy = Ux + V;
  hipStream_t st = as_stream(stream);
  for (int R = 1; R <= r_max; R++) {
    k_line_extend<<<g, BLOCK, 0, st>>>(LX, R == 1 ? nullptr : LX, Ux, Lx, Ly, 0, R - 1);
    for (int T = 1; T <= t_max; T++) {
      k_line_extend<<<g, BLOCK, 0, st>>>(LY, T == 1 ? nullptr : LY, Uy, Lx, Ly, 1, T - 1);
      k_wilson_loop<<<nb, BLOCK, 0, st>>>(LX, LY, Lx, Ly, R, T, partials);
      k_loop_sum2<<<1, 64, 0, st>>>(partials, (int)nb, 1.0 / (double)V, results + 2 * ((size_t)(R - 1) * t_max + (T - 1)));
    }
  }
  QMG_LAUNCH_CHECK();
  QMG_HIP_CHECK(hipMemcpyAsync(out_host, results, sizeof(double) * 2 * npairs, hipMemcpyDeviceToHost, st));
  QMG_HIP_CHECK(hipStreamSynchronize(st));
  return QMG_SUCCESS;
}

// Polyakov loops, the line products at full length: out_host[0..1] = average over y of prod_x U_x(x, y), out_host[2..3] = average over x of
// prod_y U_y(x, y).  Synchronous.
int qmg_u1_polyakov(const void* gauge, int Lx, int Ly, double* out_host, void* stream) {
  if (!gauge || !out_host || !valid_lattice(Lx, Ly)) return QMG_ERR_INVALID;
  void* buf = nullptr;
  const int rc = flow_scratch(sizeof(cplx) * ((size_t)Lx + Ly) + sizeof(double) * 4, &buf);
  if (rc) return rc;
  cplx* lines = (cplx*)buf;
  double* res = (double*)(lines + Lx + Ly);
  hipStream_t st = as_stream(stream);
  k_polyakov_lines<<<(unsigned)((Lx + Ly + BLOCK - 1) / BLOCK), BLOCK, 0, st>>>((const cplx*)gauge, Lx, Ly, lines);
  k_polyakov_mean<<<1, 64, 0, st>>>(lines, Lx, Ly, res);
  QMG_LAUNCH_CHECK();
  QMG_HIP_CHECK(hipMemcpyAsync(out_host, res, sizeof(double) * 4, hipMemcpyDeviceToHost, st));
  QMG_HIP_CHECK(hipStreamSynchronize(st));
  return QMG_SUCCESS;
}

}  // extern "C"
