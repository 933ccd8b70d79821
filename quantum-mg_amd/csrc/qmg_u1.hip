// qmg_u1.hip -- U(1) gauge-field generation and observables on the device (reference: u1/u1_utils.h).
//
// The reference generates its quenched U(1) fields with a SEQUENTIAL non-compact heatbath on the host
// (heatbath_noncompact_update, u1_utils.h:607-757; its own comment: "This algorithm can't be parallelized as is... We
// would need subsets").  The subsets exist: with the non-compact action S = beta/2 sum_p theta_p^2, theta_p = A_x(x) +
// A_y(x+xhat) - A_x(x+yhat) - A_y(x), the conditional distribution of a link given the rest is Gaussian,
//     A_mu(x) ~ N(-staple/2, 1/(2 beta)),
// and the staple of an x-link at (x, y) (u1_utils.h:644-650) contains x-links only from rows y+1 and y-1, the staple of a
// y-link at (x, y) (:658-664) y-links only from columns x+1 and x-1.  So all x-links of the EVEN rows are conditionally
// independent given everything else, likewise the odd rows, and y-links by even / odd columns: one sweep is four
// launches, each a perfectly parallel exact heatbath step of a quarter of the links.  Same stationary distribution as
// the sequential sweep (each step samples a conditional of the same Gibbs measure), different update order and random
// stream -- configurations are not reproduced link by link, the ENSEMBLE is (tests pin plaquette and m_pi).
//
// Layout: phase field = two real nc=1 lattice fields (mu = 0, 1), phase[mu*V + site], site = even-odd index
// (lattice.h:75-81), as `gauge_coord_to_index` gives it; compact links U = exp(i A) in the same order (complex).
//
// Field tools (u1_utils.h:183-383, 545-603): hot / Gaussian fields and random gauge transforms, the gauge transform itself,
// APE smearing and the two instantons.  All are site-local or nearest-neighbour.  The random ones draw from the counter-based
// generator below, keyed by (seed, mu, site): the field depends on neither the launch geometry nor the call order, and -- as
// with the heatbath -- it is the DISTRIBUTION of the reference that is reproduced, not its std::mt19937 stream.
// lorentz_gauge_fix_u1 (:511-542) is an unfinished stub in the reference (its loop has no body and never ends): not here.
#include <string.h>

#include "qmg_u1_pair.h"

namespace qmg {

__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// one N(0,1) draw keyed by (seed, counter): counter-based, so the field does not depend on the launch geometry
__device__ __forceinline__ double gaussian_draw(unsigned long long seed, unsigned long long counter) {
  const unsigned long long h1 = mix64(seed * 0xD1342543DE82EF95ull + 2ull * counter);
  const unsigned long long h2 = mix64(h1 + 2ull * counter + 1ull);
  const double u1 = ((double)(h1 >> 11) + 1.0) * (1.0 / 9007199254740992.0);   // (0,1]
  const double u2 = (double)(h2 >> 11) * (1.0 / 9007199254740992.0);
  return sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925286766559 * u2);
}

// mu = 0: x-links of the rows with y & 1 == line ; mu = 1: y-links of the columns with x & 1 == line
__global__ __launch_bounds__(BLOCK) void k_heatbath_noncompact(double* __restrict__ phase, int Lx, int Ly, int mu, int line, double width,
                                                               unsigned long long seed, unsigned long long sweep) {
  const long V = (long)Lx * Ly;
  const long nlinks = V / 2;
  double* Ax = phase;
  double* Ay = phase + V;
  for (long t = (long)blockIdx.x * BLOCK + threadIdx.x; t < nlinks; t += (long)gridDim.x * BLOCK) {
    int x, y;
    if (mu == 0) { x = (int)(t % Lx); y = 2 * (int)(t / Lx) + line; }
    else { y = (int)(t % Ly); x = 2 * (int)(t / Ly) + line; }
    const int xp = (x + 1 == Lx) ? 0 : x + 1, xm = (x == 0) ? Lx - 1 : x - 1;
    const int yp = (y + 1 == Ly) ? 0 : y + 1, ym = (y == 0) ? Ly - 1 : y - 1;
    double staple;
    if (mu == 0) {   // u1_utils.h:644-650
      staple = Ay[eo_index(xp, y, Lx, Ly)] - Ax[eo_index(x, yp, Lx, Ly)] - Ay[eo_index(x, y, Lx, Ly)]
             - Ay[eo_index(xp, ym, Lx, Ly)] - Ax[eo_index(x, ym, Lx, Ly)] + Ay[eo_index(x, ym, Lx, Ly)];
    } else {         // :658-664
      staple = Ax[eo_index(x, yp, Lx, Ly)] - Ay[eo_index(xp, y, Lx, Ly)] - Ax[eo_index(x, y, Lx, Ly)]
             - Ax[eo_index(xm, yp, Lx, Ly)] - Ay[eo_index(xm, y, Lx, Ly)] + Ax[eo_index(xm, y, Lx, Ly)];
    }
    const long site = eo_index(x, y, Lx, Ly);
    const double g = gaussian_draw(seed, (sweep * 2ull + (unsigned long long)mu) * (unsigned long long)V + (unsigned long long)site);
    (mu == 0 ? Ax : Ay)[site] = width * g - 0.5 * staple;
  }
}

// U = exp(i A) (polar_vector)
__global__ __launch_bounds__(BLOCK) void k_phase_to_gauge(cplx* __restrict__ gauge, const double* __restrict__ phase, long n) {
  for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * BLOCK) {
    double s, c;
    sincos(phase[i], &s, &c);
    gauge[i] = cmake(c, s);
  }
}
// A = arg U
__global__ __launch_bounds__(BLOCK) void k_gauge_to_phase(double* __restrict__ phase, const cplx* __restrict__ gauge, long n) {
  for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * BLOCK) phase[i] = atan2(gauge[i].y, gauge[i].x);
}

// one uniform draw in (-pi, pi) keyed by (seed, counter); 53 bits, centred so that neither end point is reached
__device__ __forceinline__ double uniform_phase_draw(unsigned long long seed, unsigned long long counter) {
  const unsigned long long h = mix64(mix64(seed * 0xD1342543DE82EF95ull + 2ull * counter) + 2ull * counter + 1ull);
  const double u = ((double)(h >> 11) + 0.5) * (1.0 / 9007199254740992.0);   // (0,1)
  return 3.14159265358979323846 * (2.0 * u - 1.0);
}

// rand_gauge_u1 / rand_trans_u1 (u1_utils.h:185-237; width < 0: uniform phases) and gauss_gauge_u1 (:200-223; N(0, width^2) phases),
// then U = exp(i A).  Element i = mu * V + site is draw number i of `seed`.
__global__ __launch_bounds__(BLOCK) void k_random_u1(cplx* __restrict__ out, long n, double width, unsigned long long seed) {
  for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * BLOCK) {
    const double a = (width < 0.0) ? uniform_phase_draw(seed, (unsigned long long)i) : width * gaussian_draw(seed, (unsigned long long)i);
    double s, c;
    sincos(a, &s, &c);
    out[i] = cmake(c, s);
  }
}

// apply_gauge_trans_u1 (u1_utils.h:241-272): U_mu(x) <- g(x) U_mu(x) conj g(x + mu), both directions in one pass
__global__ __launch_bounds__(BLOCK) void k_gauge_transform(cplx* __restrict__ gauge, const cplx* __restrict__ trans, int Lx, int Ly) {
  const long V = (long)Lx * Ly;
  for (long t = (long)blockIdx.x * BLOCK + threadIdx.x; t < V; t += (long)gridDim.x * BLOCK) {
    const int x = (int)(t % Lx), y = (int)(t / Lx);
    const int xp = (x + 1 == Lx) ? 0 : x + 1, yp = (y + 1 == Ly) ? 0 : y + 1;
    const long s = eo_index(x, y, Lx, Ly);
    const cplx g = trans[s];
    gauge[s] = cmul(cmul(g, gauge[s]), cconj(trans[eo_index(xp, y, Lx, Ly)]));
    gauge[V + s] = cmul(cmul(g, gauge[V + s]), cconj(trans[eo_index(x, yp, Lx, Ly)]));
  }
}

// P[z] = exp(i arg z), P[0] = 1 (arg_vector + polar, u1_utils.h:371-372).  z / |z| costs one rsqrt and two multiplies per link
// where atan2 + sincos cost a few hundred fp64 operations -- comparable to the time the link's 64 bytes take from HBM
// (profiles/u1_smear_bench.txt has both).  -DQMG_U1_APE_TRIG builds the trigonometric form for that comparison only.
__device__ __forceinline__ cplx project_u1(cplx z) {
#ifdef QMG_U1_APE_TRIG
  double s, c;
  sincos(atan2(z.y, z.x), &s, &c);
  return cmake(c, s);
#else
  const double n2 = fma(z.x, z.x, z.y * z.y);
  if (!(n2 > 0.0)) return cmake(1.0, 0.0);
  const double r = rsqrt(n2);
  return cmake(z.x * r, z.y * r);
#endif
}

// One APE iteration (u1_utils.h:292-375), out != in, on the site pairs of qmg_u1_pair.h: all four links of a pair from its 15.
//   U'_x(s) = P[ U_x(s) + alpha ( U_y(s) U_x(s+y) conj U_y(s+x) + conj U_y(s-y) U_x(s-y) U_y(s+x-y) ) ]
//   U'_y(s) = P[ U_y(s) + alpha ( U_x(s) U_y(s+x) conj U_x(s+y) + conj U_x(s-x) U_y(s-x) U_x(s-x+y) ) ]
__global__ __launch_bounds__(BLOCK) void k_ape_smear(cplx* __restrict__ out, const cplx* __restrict__ in, int Lx, int Ly, double alpha) {
  const long V = (long)Lx * Ly;
  const int h = Lx >> 1;
  const long npairs = V / 2;
  const cplx* __restrict__ Ux = in;
  const cplx* __restrict__ Uy = in + V;
  for (long t = (long)blockIdx.x * BLOCK + threadIdx.x; t < npairs; t += (long)gridDim.x * BLOCK) {
    const PairGeom g = pair_geom(t, h, Ly);
    const int xh = g.xh, xl = g.xl, xr = g.xr;
    const long ra = g.ra, rb = g.rb, rap = g.rap, rbp = g.rbp, ram = g.ram, rbm = g.rbm;
    // pair_links(Ux, Uy, g), written out: through the helper's struct the kernel kept its occupancy (92 VGPRs for 96) but got another schedule,
    // and an iteration at 4096^2 took 0.2255 ms for the parent's 0.2108 (profiles/u1_pair_refactor.txt)
    const cplx ax = Ux[ra + xh], ay = Uy[ra + xh], bx = Ux[rb + xh], by = Uy[rb + xh];
    const cplx apx = Ux[rap + xh], bpx = Ux[rbp + xh];
    const cplx amx = Ux[ram + xh], amy = Uy[ram + xh], bmx = Ux[rbm + xh], bmy = Uy[rbm + xh];
    const cplx lx = Ux[rb + xl], ly = Uy[rb + xl], lpx = Ux[rbp + xl];
    const cplx ry = Uy[ra + xr], rmy = Uy[ram + xr];

    cplx st;
    // site a: x + xhat = b, x - xhat = l
    st = cadd(cmul(cmul(ay, apx), cconj(by)), cmul(cmul(cconj(amy), amx), bmy));
    out[ra + xh] = project_u1(cmake(fma(alpha, st.x, ax.x), fma(alpha, st.y, ax.y)));
    st = cadd(cmul(cmul(ax, by), cconj(apx)), cmul(cmul(cconj(lx), ly), lpx));
    out[V + ra + xh] = project_u1(cmake(fma(alpha, st.x, ay.x), fma(alpha, st.y, ay.y)));
    // site b: x + xhat = r, x - xhat = a
    st = cadd(cmul(cmul(by, bpx), cconj(ry)), cmul(cmul(cconj(bmy), bmx), rmy));
    out[rb + xh] = project_u1(cmake(fma(alpha, st.x, bx.x), fma(alpha, st.y, bx.y)));
    st = cadd(cmul(cmul(bx, ry), cconj(bpx)), cmul(cmul(cconj(ax), ay), apx));
    out[V + rb + xh] = project_u1(cmake(fma(alpha, st.x, by.x), fma(alpha, st.y, by.y)));
  }
}

// create_instanton_u1 (u1_utils.h:545-572): the site (x, y) of the reference's loop, displaced by r = (x - Lx/2 + 1/2, y - Ly/2 + 1/2)
// from the centre, lands on ((x - Lx/2 + x0 + 3 Lx) % Lx, (y - Ly/2 + y0 + 3 Ly) % Ly); U_x *= exp(i Q r_y / r^2), U_y *= exp(-i Q r_x / r^2).
// The map (x, y) -> target is a bijection for every x0, y0 that keeps the reference's % arguments non-negative.
__global__ __launch_bounds__(BLOCK) void k_instanton(cplx* __restrict__ gauge, int Lx, int Ly, double Q, int x0, int y0) {
  const long V = (long)Lx * Ly;
  for (long t = (long)blockIdx.x * BLOCK + threadIdx.x; t < V; t += (long)gridDim.x * BLOCK) {
    const int x = (int)(t % Lx), y = (int)(t / Lx);
    const double rx = x - Lx / 2 + 0.5, ry = y - Ly / 2 + 0.5;
    const double r2 = rx * rx + ry * ry;
    const long s = eo_index((x - Lx / 2 + x0 + 3 * Lx) % Lx, (y - Ly / 2 + y0 + 3 * Ly) % Ly, Lx, Ly);
    double sn, cs;
    sincos(Q * ry / r2, &sn, &cs);
    gauge[s] = cmul(gauge[s], cmake(cs, sn));
    sincos(-Q * rx / r2, &sn, &cs);
    gauge[V + s] = cmul(gauge[V + s], cmake(cs, sn));
  }
}

// create_noncompact_instanton_u1 (u1_utils.h:575-603), with the reference's ten-digit literal for pi
__global__ __launch_bounds__(BLOCK) void k_noncompact_instanton(double* __restrict__ phase, int Lx, int Ly, double Q) {
  const long V = (long)Lx * Ly;
  for (long t = (long)blockIdx.x * BLOCK + threadIdx.x; t < V; t += (long)gridDim.x * BLOCK) {
    const int x = (int)(t % Lx), y = (int)(t / Lx);
    const long s = eo_index(x, y, Lx, Ly);
    phase[s] += -Q * 3.1415926535 * y / (double)V;
    if (y == Ly - 1) phase[V + s] += Q * 3.1415926535 * x / Lx;
  }
}

// Per-block partial sums of: plaquette (re, im), topological charge density arg(P)/2pi, and -- from a phase field --
// the non-compact plaquette angle squared.  MODE 0: compact links; MODE 1: phases.
template <int MODE>
__global__ __launch_bounds__(BLOCK) void k_plaquette(const cplx* __restrict__ gauge, const double* __restrict__ phase, int Lx, int Ly, double* __restrict__ partials) {
  const long V = (long)Lx * Ly;
  double v[3] = {0.0, 0.0, 0.0};
  for (long t = (long)blockIdx.x * BLOCK + threadIdx.x; t < V; t += (long)gridDim.x * BLOCK) {
    const int x = (int)(t % Lx), y = (int)(t / Lx);
    const int xp = (x + 1 == Lx) ? 0 : x + 1, yp = (y + 1 == Ly) ? 0 : y + 1;
    const long s = eo_index(x, y, Lx, Ly), sx = eo_index(xp, y, Lx, Ly), sy = eo_index(x, yp, Lx, Ly);
    if (MODE == 0) {   // U_x(x) U_y(x+xhat) U_x^*(x+yhat) U_y^*(x)   (u1_utils.h:424-462)
      cplx p = cmul(gauge[s], gauge[V + sx]);
      p = cmul(p, cconj(gauge[sy]));
      p = cmul(p, cconj(gauge[V + s]));
      v[0] += p.x; v[1] += p.y;
      v[2] += atan2(p.y, p.x);   // get_topo_u1 (:465-508): sum arg / 2 pi
    } else {           // theta_p = A_x(x) + A_y(x+xhat) - A_x(x+yhat) - A_y(x)   (get_noncompact_action_u1, :386-421)
      const double th = phase[s] + phase[V + sx] - phase[sy] - phase[V + s];
      v[0] += th * th;
    }
  }
  __shared__ double sm[3][BLOCK / WAVE];
  block_partials<3>(v, sm, partials);
}

static int plaquette_sums(const void* gauge, const double* phase, int Lx, int Ly, double out[3], void* stream, int mode) {
  if (!valid_lattice(Lx, Ly)) return QMG_ERR_INVALID;
  hipStream_t st = as_stream(stream);
  const long V = (long)Lx * Ly;
  long nb = (V + BLOCK - 1) / BLOCK;
  if (nb > 1024) nb = 1024;
  double* buf = nullptr;
  QMG_HIP_CHECK(hipMalloc((void**)&buf, sizeof(double) * (3 * nb + 3)));
  if (const int rc = poison_new_scratch(buf, sizeof(double) * (3 * nb + 3))) { hipFree(buf); return rc; }
  if (mode == 0) k_plaquette<0><<<(unsigned)nb, BLOCK, 0, st>>>((const cplx*)gauge, nullptr, Lx, Ly, buf);
  else k_plaquette<1><<<(unsigned)nb, BLOCK, 0, st>>>(nullptr, phase, Lx, Ly, buf);
  k_sum_partials<3><<<1, 64, 0, st>>>(buf, (int)nb, 1.0, buf + 3 * nb);
  hipError_t e = hipMemcpyAsync(out, buf + 3 * nb, sizeof(double) * 3, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  hipFree(buf);
  if (e != hipSuccess) { set_hip_error(e, "plaquette_sums"); return QMG_ERR_HIP; }
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

static thread_local ThreadScratch g_smear;   // the calling thread's scratch field of qmg_u1_ape_smear

void release_u1_workspace() { g_smear.release(); }   // qmg_shutdown (qmg_runtime.hip)

}  // namespace qmg

using namespace qmg;

extern "C" {

// heatbath_noncompact_update (u1_utils.h:607-757) as a four-colour parallel heatbath: n_update sweeps of {x-links even rows,
// x-links odd rows, y-links even columns, y-links odd columns}.  phase: DEVICE double[2 Lx Ly].  `seed` + the running sweep
// index `first_sweep` key the counter-based generator (pass the number of sweeps already done to continue a stream).
int qmg_u1_heatbath_noncompact(double* phase, int Lx, int Ly, double beta, int n_update, unsigned long long seed, unsigned long long first_sweep, void* stream) {
  if (!phase || !valid_lattice(Lx, Ly) || !(beta > 0.0) || n_update < 0) return QMG_ERR_INVALID;
  const double width = sqrt(0.5 / beta);
  const long nlinks = (long)Lx * Ly / 2;
  const unsigned g = grid_1d((size_t)nlinks);
  hipStream_t st = as_stream(stream);
  for (int i = 0; i < n_update; i++) {
    const unsigned long long sweep = first_sweep + (unsigned long long)i;
    k_heatbath_noncompact<<<g, BLOCK, 0, st>>>(phase, Lx, Ly, 0, 0, width, seed, sweep);
    k_heatbath_noncompact<<<g, BLOCK, 0, st>>>(phase, Lx, Ly, 0, 1, width, seed, sweep);
    k_heatbath_noncompact<<<g, BLOCK, 0, st>>>(phase, Lx, Ly, 1, 0, width, seed, sweep);
    k_heatbath_noncompact<<<g, BLOCK, 0, st>>>(phase, Lx, Ly, 1, 1, width, seed, sweep);
  }
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

// polar_vector(phases, gauge_field, size_gauge): U = exp(i A); and its inverse A = arg U (the phases write_gauge_u1 stores)
int qmg_u1_phase_to_gauge(void* gauge, const double* phase, size_t n, void* stream) {
  if ((!gauge || !phase) && n) return QMG_ERR_INVALID;
  if (n == 0) return QMG_SUCCESS;
  k_phase_to_gauge<<<grid_1d(n), BLOCK, 0, as_stream(stream)>>>((cplx*)gauge, phase, (long)n);
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}
int qmg_u1_gauge_to_phase(double* phase, const void* gauge, size_t n, void* stream) {
  if ((!gauge || !phase) && n) return QMG_ERR_INVALID;
  if (n == 0) return QMG_SUCCESS;
  k_gauge_to_phase<<<grid_1d(n), BLOCK, 0, as_stream(stream)>>>(phase, (const cplx*)gauge, (long)n);
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

// get_plaquette_u1 (u1_utils.h:424-462): volume average of the plaquette (re, im) -> out_host[0..1];
// get_topo_u1 (:465-508): sum_p arg(P) / 2 pi -> out_host[2].  Synchronous.
int qmg_u1_plaquette(const void* gauge, int Lx, int Ly, double* out_host, void* stream) {
  if (!gauge || !out_host) return QMG_ERR_INVALID;
  double s[3];
  const int rc = plaquette_sums(gauge, nullptr, Lx, Ly, s, stream, 0);
  if (rc) return rc;
  const double V = (double)Lx * Ly;
  out_host[0] = s[0] / V; out_host[1] = s[1] / V; out_host[2] = s[2] * 0.5 / 3.14159265358979323846;
  return QMG_SUCCESS;
}
// get_noncompact_action_u1 (:386-421): beta/2 sum_p theta_p^2
int qmg_u1_noncompact_action(const double* phase, int Lx, int Ly, double beta, double* out_host, void* stream) {
  if (!phase || !out_host) return QMG_ERR_INVALID;
  double s[3];
  const int rc = plaquette_sums(nullptr, phase, Lx, Ly, s, stream, 1);
  if (rc) return rc;
  *out_host = 0.5 * beta * s[0];
  return QMG_SUCCESS;
}

// rand_gauge_u1 (u1_utils.h:185-195): hot start, phases uniform in (-pi, pi).  gauge: DEVICE complex<double>[2 Lx Ly].
int qmg_u1_hot_gauge(void* gauge, int Lx, int Ly, unsigned long long seed, void* stream) {
  if (!gauge || !valid_lattice(Lx, Ly)) return QMG_ERR_INVALID;
  const long n = 2L * Lx * Ly;
  k_random_u1<<<grid_1d((size_t)n), BLOCK, 0, as_stream(stream)>>>((cplx*)gauge, n, -1.0, seed);
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}
// gauss_gauge_u1 (:200-223): phases N(0, 1/|beta|); beta == 0 is the hot start
int qmg_u1_gauss_gauge(void* gauge, int Lx, int Ly, double beta, unsigned long long seed, void* stream) {
  if (!gauge || !valid_lattice(Lx, Ly) || beta != beta) return QMG_ERR_INVALID;
  if (beta == 0.0) return qmg_u1_hot_gauge(gauge, Lx, Ly, seed, stream);
  const long n = 2L * Lx * Ly;
  k_random_u1<<<grid_1d((size_t)n), BLOCK, 0, as_stream(stream)>>>((cplx*)gauge, n, 1.0 / sqrt(fabs(beta)), seed);
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}
// rand_trans_u1 (:227-237): trans: DEVICE complex<double>[Lx Ly], phases uniform in (-pi, pi)
int qmg_u1_random_trans(void* trans, int Lx, int Ly, unsigned long long seed, void* stream) {
  if (!trans || !valid_lattice(Lx, Ly)) return QMG_ERR_INVALID;
  const long n = (long)Lx * Ly;
  k_random_u1<<<grid_1d((size_t)n), BLOCK, 0, as_stream(stream)>>>((cplx*)trans, n, -1.0, seed);
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

// apply_gauge_trans_u1 (:241-272), in place
int qmg_u1_gauge_transform(void* gauge, const void* trans, int Lx, int Ly, void* stream) {
  if (!gauge || !trans || !valid_lattice(Lx, Ly)) return QMG_ERR_INVALID;
  k_gauge_transform<<<grid_1d((size_t)Lx * Ly), BLOCK, 0, as_stream(stream)>>>((cplx*)gauge, (const cplx*)trans, Lx, Ly);
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

// apply_ape_smear_u1 (:276-383): n_iter iterations of one launch each, ping-ponging between `smeared` and the calling thread's scratch
// field so that the last one lands in `smeared`.  smeared == gauge is allowed (the reference copies first); n_iter == 0 is a copy.
// The scratch field grows on demand (the only synchronous step, and only when it grows) and is held until qmg_shutdown, like the
// reduction workspaces; calls of one host thread on different streams share it and must not overlap.
int qmg_u1_ape_smear(void* smeared, const void* gauge, int Lx, int Ly, double alpha, int n_iter, void* stream) {
  if (!smeared || !gauge || !valid_lattice(Lx, Ly) || n_iter < 0 || alpha != alpha) return QMG_ERR_INVALID;
  const size_t n = 2 * (size_t)Lx * Ly, bytes = sizeof(cplx) * n;
  const bool in_place = (smeared == gauge);
  if (!in_place && fields_overlap(smeared, bytes, gauge, bytes)) return QMG_ERR_INVALID;   // partial overlap
  if (n_iter == 0) return in_place ? QMG_SUCCESS : qmg_copy_vector(smeared, gauge, n, stream);
  cplx* tmp = nullptr;
  if (in_place || n_iter > 1) {
    const int rc = g_smear.grow(bytes, &tmp);
    if (rc) return rc;
  }
  // targets alternate and end on `smeared`; in place with an odd count the roles swap (the first target cannot be the
  // source) and the result is copied over from the scratch field
  const bool swapped = in_place && (n_iter & 1);
  cplx* ends[2] = {swapped ? tmp : (cplx*)smeared, swapped ? (cplx*)smeared : tmp};
  const unsigned g = grid_1d((size_t)Lx * Ly / 2);
  const cplx* src = (const cplx*)gauge;
  for (int i = 0; i < n_iter; i++) {
    cplx* dst = ends[(n_iter - 1 - i) & 1];
    k_ape_smear<<<g, BLOCK, 0, as_stream(stream)>>>(dst, src, Lx, Ly, alpha);
    src = dst;
  }
  QMG_LAUNCH_CHECK();
  return swapped ? qmg_copy_vector(smeared, tmp, n, stream) : QMG_SUCCESS;
}

// create_instanton_u1 (:545-572), in place: charge Q centred between the sites around (x0, y0)
int qmg_u1_instanton(void* gauge, int Lx, int Ly, double Q, int x0, int y0, void* stream) {
  if (!gauge || !valid_lattice(Lx, Ly)) return QMG_ERR_INVALID;
  // the reference's (x - Lx/2 + x0 + 3 Lx) % Lx needs a non-negative argument (and no int overflow) to be a lattice coordinate
  if (x0 < -2 * (long)Lx - Lx / 2 || y0 < -2 * (long)Ly - Ly / 2 || x0 > (1 << 30) || y0 > (1 << 30)) return QMG_ERR_INVALID;
  k_instanton<<<grid_1d((size_t)Lx * Ly), BLOCK, 0, as_stream(stream)>>>((cplx*)gauge, Lx, Ly, Q, x0, y0);
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}
// create_noncompact_instanton_u1 (:575-603), in place on a phase field
int qmg_u1_noncompact_instanton(double* phase, int Lx, int Ly, double Q, void* stream) {
  if (!phase || !valid_lattice(Lx, Ly)) return QMG_ERR_INVALID;
  k_noncompact_instanton<<<grid_1d((size_t)Lx * Ly), BLOCK, 0, as_stream(stream)>>>(phase, Lx, Ly, Q);
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

}  // extern "C"
