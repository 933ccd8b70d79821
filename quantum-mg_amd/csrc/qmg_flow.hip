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
#include "qmg_u1_pair.h"

namespace qmg {

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

// One Runge-Kutta stage in one pass, on the site pairs of qmg_u1_pair.h: a thread updates the four links of its pair from the 15 links of `in`,
// four phases and, from stage 2 on, four accumulators, all loaded in front of the arithmetic.  sin P is the imaginary part of the plaquette
// of the links: the only trigonometry is the sincos of the four new phases.  out != in (neighbours are read from in).
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
    const PairGeom g = pair_geom(t, h, Ly);
    const long sa = g.sa, sb = g.sb;
    const double tax = theta[sa], tay = theta[V + sa], tbx = theta[sb], tby = theta[V + sb];
    double aax = 0.0, aay = 0.0, abx = 0.0, aby = 0.0;
    if (STAGE != 1) { aax = acc[sa]; aay = acc[V + sa]; abx = acc[sb]; aby = acc[V + sb]; }
    const PairForce d = pair_sin_diffs(pair_links(Ux, Uy, g));

    const double nax = flow_link<STAGE>(tax, acc, sa, aax, -eps * d.ax);
    const double nay = flow_link<STAGE>(tay, acc, V + sa, aay, -eps * d.ay);
    const double nbx = flow_link<STAGE>(tbx, acc, sb, abx, -eps * d.bx);
    const double nby = flow_link<STAGE>(tby, acc, V + sb, aby, -eps * d.by);
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

// out(x) = line(x) U_mu(x + k mu)   (line == nullptr: out = U_mu, k = 0).  In place is allowed: the kernel is pointwise in `line`.
__global__ __launch_bounds__(BLOCK) void k_line_extend(cplx* out, const cplx* line, const cplx* __restrict__ U, int Lx, int Ly, int mu, int k) {
  const long V = (long)Lx * Ly;
  const int h = Lx >> 1;
  for (long t = (long)blockIdx.x * BLOCK + threadIdx.x; t < V; t += (long)gridDim.x * BLOCK) {
    const int row = (int)(t / h), xh = (int)(t % h);
    const int p = row >= Ly, y = row - p * Ly, x = 2 * xh + (p ^ (y & 1));
    const int xs = (mu == 0) ? (x + k) % Lx : x, ys = (mu == 0) ? y : (y + k) % Ly;
    const cplx u = U[eo_index(xs, ys, Lx, Ly)];
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
    const cplx b = LY[eo_index((x + R) % Lx, y, Lx, Ly)], c = LX[eo_index(x, (y + T) % Ly, Lx, Ly)];
    const cplx ab = cmul(a, b), cd = cmul(c, d);   // W = ab conj(cd)
    v[0] += fma(ab.x, cd.x, ab.y * cd.y);
    v[1] += fma(ab.y, cd.x, -ab.x * cd.y);
  }
  __shared__ double sm[2][BLOCK / WAVE];
  block_partials<2>(v, sm, partials);
}

// Polyakov loops: thread l < Ly multiplies the x-links of row y = l, thread Ly + l the y-links of column x = l; the products go to
// lines[l] and lines[Ly + l] and are averaged by the caller's k_polyakov_mean.  O(V) reads in all: an observable, not a hot path.
__global__ __launch_bounds__(BLOCK) void k_polyakov_lines(const cplx* __restrict__ gauge, int Lx, int Ly, cplx* __restrict__ lines) {
  const long V = (long)Lx * Ly;
  const int l = blockIdx.x * BLOCK + threadIdx.x;
  if (l >= Lx + Ly) return;
  cplx p = cmake(1.0, 0.0);
  if (l < Ly) for (int x = 0; x < Lx; x++) p = cmul(p, gauge[eo_index(x, l, Lx, Ly)]);
  else for (int y = 0; y < Ly; y++) p = cmul(p, gauge[V + eo_index(l - Ly, y, Lx, Ly)]);
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

// the calling thread's scratch of qmg_u1_flow (a link field and the accumulator), of qmg_u1_wilson_loops (two line-product fields) and of
// qmg_u1_polyakov; its own buffer, not the APE scratch field's, so that a thread may smear on one stream while it flows on another
static thread_local ThreadScratch g_flow;

void release_flow_workspace() { g_flow.release(); }   // qmg_shutdown (qmg_runtime.hip)

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
  int rc = g_flow.grow((sizeof(cplx) + sizeof(double)) * n, &buf);
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
  int rc = g_flow.grow(sizeof(cplx) * 2 * V + sizeof(double) * 2 * (nb + npairs), &buf);
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
      k_sum_partials<2><<<1, 64, 0, st>>>(partials, (int)nb, 1.0 / (double)V, results + 2 * ((size_t)(R - 1) * t_max + (T - 1)));
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
  const int rc = g_flow.grow(sizeof(cplx) * ((size_t)Lx + Ly) + sizeof(double) * 4, &buf);
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
