// qmg_stout.hip -- stout-smeared links for the Wilson fermions of the Schwinger-model HMC, and the chain rule of their force; fp64 only.
// Not in the reference, which has neither HMC nor a differentiable smearing: the driver is include/qmg/hmc.hpp (SchwingerHMC with stout_levels > 0,
// through include/qmg/stout.hpp), the independent statement tests/stout_numpy.py.
//
//   P(x) = theta_x(x) + theta_y(x+xhat) - theta_x(x+yhat) - theta_y(x),   S_w = sum_x (1 - cos P),   U_mu(x) = exp(i theta_mu(x))
//   curl:       (C F)(x) = F_x(x) + F_y(x+xhat) - F_x(x+yhat) - F_y(x)                    (link field -> plaquette field)
//   transpose:  (C^T g)_x(x) = g(x) - g(x-yhat),   (C^T g)_y(x) = -g(x) + g(x-xhat)       (so dS_w/dtheta = C^T sin P)
//
// One stout level is an Euler step of the Wilson flow of length rho:  theta^(k+1) = theta^(k) - rho C^T sin P^(k), in links
// U^(k+1)_mu(x) = U^(k)_mu(x) exp(-i rho (C^T sin P^(k))_mu(x)); it is gauge covariant.  The fermions see V = U^(n), the gauge action the thin
// links U = U^(0).  The Jacobian of a level, J_k = 1 - rho C^T diag(cos P^(k)) C, is symmetric, so the force on the thin links is
//   F^(n) = sum_j w_j Ff(X_j, Y_j) with the links V (the bilinear of qmg_hmc.hip),   F^(k) = J_k F^(k+1),  k = n-1 .. 0,
//   pi -= dt (beta C^T sin P^(0) + F^(0)).
// sin P and cos P are the imaginary and the real part of the plaquette of the complex links: the only trigonometry is the sincos of the
// four rotations of a smearing step.
//
// All four kernels run on the site pairs of qmg_u1_pair.h with its loaders: a thread owns the four links of its pair and reads the 15 links
// around it (and the 15 values of a force field at the same links), all loaded in front of the arithmetic.  No LDS, no atomics.
// Layouts (lattice.h:75-81): site (x, y) has index (y + p Ly) Lx/2 + x/2, p = (x + y) & 1; links and forces are [mu][site], spinors [site][2].
#include <cmath>

#include "qmg_hmc_bilinear.h"
#include "qmg_u1_pair.h"

namespace qmg {

// One level: out = in exp(-i rho C^T sin P[in]).  out != in (neighbours are read from in).
// Byte model: 64 B/site -- two links read (32), two written (32); the neighbours are expected from cache.
__global__ __launch_bounds__(BLOCK) void k_stout_smear(cplx* __restrict__ out, const cplx* __restrict__ in, int Lx, int Ly, double rho) {
  const long V = (long)Lx * Ly;
  const int h = Lx >> 1;
  const long npairs = V / 2;
  const cplx* __restrict__ Ux = in;
  const cplx* __restrict__ Uy = in + V;
  for (long t = (long)blockIdx.x * BLOCK + threadIdx.x; t < npairs; t += (long)gridDim.x * BLOCK) {
    const PairGeom g = pair_geom(t, h, Ly);
    const PairLinks u = pair_links(Ux, Uy, g);
    const PairForce d = pair_sin_diffs(u);
    double s, c;
    sincos(-rho * d.ax, &s, &c); out[g.sa] = cmul(u.ax, cmake(c, s));
    sincos(-rho * d.ay, &s, &c); out[V + g.sa] = cmul(u.ay, cmake(c, s));
    sincos(-rho * d.bx, &s, &c); out[g.sb] = cmul(u.bx, cmake(c, s));
    sincos(-rho * d.by, &s, &c); out[V + g.sb] = cmul(u.by, cmake(c, s));
  }
}

// F = sum_j w_j Ff(X_j, Y_j) as a link field: the pole loop of k_hmc_momentum_update_poles (its loads, its expressions, its order) without
// the momenta and the gauge force.  FIRST writes the sum, the launches after the first (more than HMC_POLES_J poles) add to what is there.
// Byte model: 48 + 64 n B/site -- two links (32), F written (16; read as well after the first launch), per pole X_j and Y_j (64).
template <bool FIRST>
__global__ __launch_bounds__(BLOCK) void k_hmc_fermion_force(double* __restrict__ F, const cplx* __restrict__ gauge, const HmcPoles poles, int n_poles, int Lx, int Ly) {
  const long V = (long)Lx * Ly;
  const int h = Lx >> 1;
  const long npairs = V / 2;
  const cplx* __restrict__ Ux = gauge;
  const cplx* __restrict__ Uy = gauge + V;
  for (long t = (long)blockIdx.x * BLOCK + threadIdx.x; t < npairs; t += (long)gridDim.x * BLOCK) {
    const PairGeom g = pair_geom(t, h, Ly);
    const long sa = g.sa, sb = g.sb;
    const PairOwn o = pair_own_links(Ux, Uy, g);
    // The pole sum starts from -0.0, the one number that fma(w, f, .) leaves every w f at, signed zeros included; or from the sum so far.
    double fax = -0.0, fay = -0.0, fbx = -0.0, fby = -0.0;
    if (!FIRST) { fax = F[sa]; fay = F[V + sa]; fbx = F[sb]; fby = F[V + sb]; }
    const long sr = g.ra + g.xr, sap = g.rap + g.xh, sbp = g.rbp + g.xh;
    for (int j = 0; j < n_poles; j++) {
      const cplx* __restrict__ X = poles.X[j];
      const cplx* __restrict__ Y = poles.Y[j];
      const double w = poles.w[j];
      const cplx xa0 = X[2 * sa], xa1 = X[2 * sa + 1], ya0 = Y[2 * sa], ya1 = Y[2 * sa + 1];
      const cplx xb0 = X[2 * sb], xb1 = X[2 * sb + 1], yb0 = Y[2 * sb], yb1 = Y[2 * sb + 1];
      const cplx xr0 = X[2 * sr], xr1 = X[2 * sr + 1], yr0 = Y[2 * sr], yr1 = Y[2 * sr + 1];
      const cplx xap0 = X[2 * sap], xap1 = X[2 * sap + 1], yap0 = Y[2 * sap], yap1 = Y[2 * sap + 1];
      const cplx xbp0 = X[2 * sbp], xbp1 = X[2 * sbp + 1], ybp0 = Y[2 * sbp], ybp1 = Y[2 * sbp + 1];
      fax = fma(w, link_force(o.ax, ydag_hx(ya0, ya1, xb0, xb1, 1.0), ydag_hx(yb0, yb1, xa0, xa1, -1.0)), fax);
      fay = fma(w, link_force(o.ay, ydag_hy(ya0, ya1, xap0, xap1, 1.0), ydag_hy(yap0, yap1, xa0, xa1, -1.0)), fay);
      fbx = fma(w, link_force(o.bx, ydag_hx(yb0, yb1, xr0, xr1, 1.0), ydag_hx(yr0, yr1, xb0, xb1, -1.0)), fbx);
      fby = fma(w, link_force(o.by, ydag_hy(yb0, yb1, xbp0, xbp1, 1.0), ydag_hy(ybp0, ybp1, xb0, xb1, -1.0)), fby);
    }
    F[sa] = fax;
    F[V + sa] = fay;
    F[sb] = fbx;
    F[V + sb] = fby;
  }
}

// F_out = J_k F_in = F_in - rho C^T [cos P^(k) . (C F_in)] in one pass: the pair's 15 links of level k and the 15 values of F_in at the same
// links.  F_out != F_in (neighbours are read from F_in).
// Byte model: 64 B/site -- two links (32), F_in (16), F_out (16); the neighbours are expected from cache.
__global__ __launch_bounds__(BLOCK) void k_stout_force_level(double* __restrict__ F_out, const double* __restrict__ F_in, const cplx* __restrict__ gauge, int Lx, int Ly,
                                                             double rho) {
  const long V = (long)Lx * Ly;
  const int h = Lx >> 1;
  const long npairs = V / 2;
  const cplx* __restrict__ Ux = gauge;
  const cplx* __restrict__ Uy = gauge + V;
  for (long t = (long)blockIdx.x * BLOCK + threadIdx.x; t < npairs; t += (long)gridDim.x * BLOCK) {
    const PairGeom g = pair_geom(t, h, Ly);
    const PairLinks u = pair_links(Ux, Uy, g);
    const PairReals f = pair_reals(F_in, F_in + V, g);
    const PairForce d = pair_cos_curl_diffs(u, f);
    F_out[g.sa] = fma(-rho, d.ax, f.ax);
    F_out[V + g.sa] = fma(-rho, d.ay, f.ay);
    F_out[g.sb] = fma(-rho, d.bx, f.bx);
    F_out[V + g.sb] = fma(-rho, d.by, f.by);
  }
}

// pi -= dt (beta C^T sin P + J_0 F_in), every link in one pass over the thin links: the five plaquettes of a pair give their imaginary parts
// to the gauge force and their real parts to the Jacobian from the same 15 loads.
// Byte model: 80 B/site -- pi read and written (32), two links (32), F_in (16); the neighbours are expected from cache.
__global__ __launch_bounds__(BLOCK) void k_hmc_momentum_update_stout(double* __restrict__ pi, const cplx* __restrict__ gauge, const double* __restrict__ F_in, int Lx,
                                                                     int Ly, double beta, double rho, double dt) {
  const long V = (long)Lx * Ly;
  const int h = Lx >> 1;
  const long npairs = V / 2;
  const cplx* __restrict__ Ux = gauge;
  const cplx* __restrict__ Uy = gauge + V;
  for (long t = (long)blockIdx.x * BLOCK + threadIdx.x; t < npairs; t += (long)gridDim.x * BLOCK) {
    const PairGeom g = pair_geom(t, h, Ly);
    const long sa = g.sa, sb = g.sb;
    const double pax = pi[sa], pay = pi[V + sa], pbx = pi[sb], pby = pi[V + sb];
    const PairLinks u = pair_links(Ux, Uy, g);
    const PairReals f = pair_reals(F_in, F_in + V, g);
    const PairForce sd = pair_sin_diffs(u);
    const PairForce cd = pair_cos_curl_diffs(u, f);
    const double fax = fma(beta, sd.ax, fma(-rho, cd.ax, f.ax)), fay = fma(beta, sd.ay, fma(-rho, cd.ay, f.ay));
    const double fbx = fma(beta, sd.bx, fma(-rho, cd.bx, f.bx)), fby = fma(beta, sd.by, fma(-rho, cd.by, f.by));
    pi[sa] = fma(-dt, fax, pax);
    pi[V + sa] = fma(-dt, fay, pay);
    pi[sb] = fma(-dt, fbx, pbx);
    pi[V + sb] = fma(-dt, fby, pby);
  }
}

}  // namespace qmg

using namespace qmg;

extern "C" {

// levels[k] = level k + 1 of the stout smearing of `gauge`, k = 0 .. n_levels - 1, each from the one before (level 0 is `gauge` itself, which
// is not copied); one launch per level.  levels: DEVICE complex<double>[n_levels][2 Lx Ly]; gauge: DEVICE complex<double>[2 Lx Ly]; they must
// not overlap.  n_levels == 0 does nothing (levels is not read and may be null).
int qmg_u1_stout_smear(void* levels, const void* gauge, int Lx, int Ly, double rho, int n_levels, void* stream) {
  if (!gauge || !valid_lattice(Lx, Ly) || !std::isfinite(rho) || n_levels < 0) return QMG_ERR_INVALID;
  if (n_levels == 0) return QMG_SUCCESS;
  const size_t n = 2 * (size_t)Lx * Ly;
  if (!levels || fields_overlap(levels, sizeof(cplx) * n * (size_t)n_levels, gauge, sizeof(cplx) * n)) return QMG_ERR_INVALID;
  const unsigned g = grid_1d((size_t)Lx * Ly / 2);
  const cplx* in = (const cplx*)gauge;
  cplx* out = (cplx*)levels;
  for (int k = 0; k < n_levels; k++) {
    k_stout_smear<<<g, BLOCK, 0, as_stream(stream)>>>(out, in, Lx, Ly, rho);
    QMG_LAUNCH_CHECK();
    in = out;
    out += n;
  }
  return QMG_SUCCESS;
}

// F = sum_j weights[j] Ff(X[j], Y[j]) with the links `gauge`, written (not accumulated) to F: DEVICE double[2 Lx Ly].  X, Y: HOST arrays of
// n_poles DEVICE spinors; weights: HOST double[n_poles] -- the pole lists of qmg_hmc_momentum_update_poles.  Up to 16 poles go in one launch;
// further poles take further launches that add to F.  n_poles = 0 zeroes F (X, Y, weights are not read and may be null).  Two flavours is one
// pole of weight 1.  F must not overlap the other fields.
int qmg_hmc_fermion_force(double* F, const void* gauge, const void* const* X, const void* const* Y, const double* weights, int n_poles, int Lx, int Ly, void* stream) {
  if (!F || !gauge || !valid_lattice(Lx, Ly) || n_poles < 0) return QMG_ERR_INVALID;
  if (n_poles == 0) return qmg_memset_zero(F, sizeof(double) * 2 * (size_t)Lx * Ly, stream);
  if (!pole_lists_valid(X, Y, weights, n_poles)) return QMG_ERR_INVALID;
  const unsigned g = grid_1d((size_t)Lx * Ly / 2);
  return launch_pole_chunks<HMC_POLES_J>(n_poles, [&](int j0, int nj, bool first) {
    HmcPoles p;
    for (int j = 0; j < HMC_POLES_J; j++) {
      p.X[j] = j < nj ? (const cplx*)X[j0 + j] : nullptr;
      p.Y[j] = j < nj ? (const cplx*)Y[j0 + j] : nullptr;
      p.w[j] = j < nj ? weights[j0 + j] : 0.0;
    }
    if (first) k_hmc_fermion_force<true><<<g, BLOCK, 0, as_stream(stream)>>>(F, (const cplx*)gauge, p, nj, Lx, Ly);
    else k_hmc_fermion_force<false><<<g, BLOCK, 0, as_stream(stream)>>>(F, (const cplx*)gauge, p, nj, Lx, Ly);
  });
}

// F_out = J_k F_in = F_in - rho C^T [cos P . (C F_in)], P the plaquette angles of the links gauge_k: one step of the chain rule through a
// stout level.  F_out, F_in: DEVICE double[2 Lx Ly], DIFFERENT buffers (neighbours are read from F_in); F_out is overwritten.
int qmg_u1_stout_force_level(double* F_out, const double* F_in, const void* gauge_k, int Lx, int Ly, double rho, void* stream) {
  if (!F_out || !F_in || !gauge_k || !valid_lattice(Lx, Ly) || !std::isfinite(rho)) return QMG_ERR_INVALID;
  const size_t n = 2 * (size_t)Lx * Ly;
  if (fields_overlap(F_out, sizeof(double) * n, F_in, sizeof(double) * n)) return QMG_ERR_INVALID;
  k_stout_force_level<<<grid_1d((size_t)Lx * Ly / 2), BLOCK, 0, as_stream(stream)>>>(F_out, F_in, (const cplx*)gauge_k, Lx, Ly, rho);
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

// pi -= dt (beta C^T sin P + J_0 F_in) in ONE pass over the thin links `gauge`: the gauge force and the last step of the chain rule, F_in the
// force at level 1 (qmg_hmc_fermion_force on the fat links, then qmg_u1_stout_force_level down to level 1).  dt = 0 returns the momenta bit for
// bit; rho = 0 is the gauge kick plus F_in.  pi must not overlap F_in.
int qmg_hmc_momentum_update_stout(double* pi, const void* gauge, const double* F_in, int Lx, int Ly, double beta, double rho, double dt, void* stream) {
  if (!pi || !gauge || !F_in || !valid_lattice(Lx, Ly) || beta != beta || dt != dt || !std::isfinite(rho)) return QMG_ERR_INVALID;
  const size_t n = 2 * (size_t)Lx * Ly;
  if (fields_overlap(pi, sizeof(double) * n, F_in, sizeof(double) * n)) return QMG_ERR_INVALID;
  k_hmc_momentum_update_stout<<<grid_1d((size_t)Lx * Ly / 2), BLOCK, 0, as_stream(stream)>>>(pi, (const cplx*)gauge, F_in, Lx, Ly, beta, rho, dt);
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

}  // extern "C"
