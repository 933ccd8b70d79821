// qmg_hmc.hip -- molecular dynamics of two-flavour Wilson HMC for compact U(1) in two dimensions (the Schwinger model); fp64 only.
// Not in the reference, which has no HMC: the driver is include/qmg/hmc.hpp (SchwingerHMC), the independent statement tests/hmc_numpy.py.
//
//   H = 1/2 sum pi^2 + S_g + S_f,   S_g = beta sum_x (1 - cos P(x)),   S_f = phi^dag (D^dag D)^-1 phi,   U_mu(x) = exp(i theta_mu(x))
//   P(x) = theta_x(x) + theta_y(x+xhat) - theta_x(x+yhat) - theta_y(x),   D: Wilson2D (wilson_coeff 1; tests/coordspace.py::wilson_apply)
//
// Forces F = dS/dtheta, with X = (D^dag D)^-1 phi, Y = D X, Hp_mu = (-1 + sigma_mu)/2, Hm_mu = (-1 - sigma_mu)/2:
//   Fg_x(x) = beta [ sin P(x) - sin P(x-yhat) ]          Fg_y(x) = beta [ -sin P(x) + sin P(x-xhat) ]
//   Ff_mu(x) = 2 Im[ U_mu(x) Y(x)^dag Hp_mu X(x+mu)  -  conj(U_mu(x)) Y(x+mu)^dag Hm_mu X(x) ]
// sin P is the imaginary part of the plaquette of the complex links, so the force kernel needs no trigonometry.
//
// Layouts (lattice.h:75-81): site (x, y) has index (y + p Ly) Lx/2 + x/2, p = (x + y) & 1; phases, momenta and links are [mu][site],
// spinors [site][2].
#include "qmg_hmc_bilinear.h"   // ydag_hx, ydag_hy, link_force, HmcPoles, launch_pole_chunks
#include "qmg_hmc_dwf_plan.h"
#include "qmg_lane.h"   // uni, gld
#include "qmg_u1_pair.h"

namespace qmg {

// pi -= dt (Fg + Ff), every link in one pass, on the site pairs of qmg_u1_pair.h (its geometry; the loads are the kernel's own, see below): a
// thread updates the four momenta of its pair from the pair's 15 links and, with fermions, X and Y at five sites (a, b, the site right of b and the two above), all loaded in front of the arithmetic.
// Byte model: 128 B/site -- pi read and written (32), two links (32), X and Y (64); the neighbours are expected from cache.
template <bool FERMIONS>
__global__ __launch_bounds__(BLOCK) void k_hmc_momentum_update(double* __restrict__ pi, const cplx* __restrict__ gauge, const cplx* __restrict__ X,
                                                               const cplx* __restrict__ Y, int Lx, int Ly, double beta, double dt) {
  const long V = (long)Lx * Ly;
  const int h = Lx >> 1;
  const long npairs = V / 2;
  const cplx* __restrict__ Ux = gauge;
  const cplx* __restrict__ Uy = gauge + V;
  for (long t = (long)blockIdx.x * BLOCK + threadIdx.x; t < npairs; t += (long)gridDim.x * BLOCK) {
    const PairGeom g = pair_geom(t, h, Ly);
    const long sa = g.sa, sb = g.sb;
    const double pax = pi[sa], pay = pi[V + sa], pbx = pi[sb], pby = pi[V + sb];
    const int xh = g.xh, xl = g.xl, xr = g.xr;
    const long ra = g.ra, rb = g.rb, rap = g.rap, rbp = g.rbp, ram = g.ram, rbm = g.rbm;
    // pair_links and pair_sin_diffs, written out: through the helpers the two-flavour kernel kept its registers and occupancy but grew from 599
    // to 617 instructions (more 64-bit address arithmetic, three more s_waitcnt), and n of its launches back to back at 2048^2 took 1 to 2 %
    // longer than the parent's in every session measured (profiles/u1_pair_refactor.txt).  Written out, its device code is the parent's text.
    const cplx ax = Ux[sa], ay = Uy[sa], bx = Ux[sb], by = Uy[sb];
    const cplx apx = Ux[rap + xh], bpx = Ux[rbp + xh];
    const cplx amx = Ux[ram + xh], amy = Uy[ram + xh], bmx = Ux[rbm + xh], bmy = Uy[rbm + xh];
    const cplx lx = Ux[rb + xl], ly = Uy[rb + xl], lpx = Ux[rbp + xl];
    const cplx ry = Uy[ra + xr], rmy = Uy[ram + xr];
    cplx xa0, xa1, ya0, ya1, xb0, xb1, yb0, yb1, xr0, xr1, yr0, yr1, xap0, xap1, yap0, yap1, xbp0, xbp1, ybp0, ybp1;
    if (FERMIONS) {
      const long sr = ra + xr, sap = rap + xh, sbp = rbp + xh;
      xa0 = X[2 * sa]; xa1 = X[2 * sa + 1]; ya0 = Y[2 * sa]; ya1 = Y[2 * sa + 1];
      xb0 = X[2 * sb]; xb1 = X[2 * sb + 1]; yb0 = Y[2 * sb]; yb1 = Y[2 * sb + 1];
      xr0 = X[2 * sr]; xr1 = X[2 * sr + 1]; yr0 = Y[2 * sr]; yr1 = Y[2 * sr + 1];
      xap0 = X[2 * sap]; xap1 = X[2 * sap + 1]; yap0 = Y[2 * sap]; yap1 = Y[2 * sap + 1];
      xbp0 = X[2 * sbp]; xbp1 = X[2 * sbp + 1]; ybp0 = Y[2 * sbp]; ybp1 = Y[2 * sbp + 1];
    }

    // sin P: a + x = b, a + y = ap, b + x = r, (a-y) + x = b-y, (a-y) + y = a, l + x = a
    const double sPa = im_plaq(ax, by, apx, ay), sPb = im_plaq(bx, ry, bpx, by);
    const double sPam = im_plaq(amx, bmy, ax, amy), sPbm = im_plaq(bmx, rmy, bx, bmy);
    const double sPl = im_plaq(lx, ay, lpx, ly);
    double fax = beta * (sPa - sPam), fay = beta * (sPl - sPa);
    double fbx = beta * (sPb - sPbm), fby = beta * (sPa - sPb);
    if (FERMIONS) {
      fax += link_force(ax, ydag_hx(ya0, ya1, xb0, xb1, 1.0), ydag_hx(yb0, yb1, xa0, xa1, -1.0));
      fay += link_force(ay, ydag_hy(ya0, ya1, xap0, xap1, 1.0), ydag_hy(yap0, yap1, xa0, xa1, -1.0));
      fbx += link_force(bx, ydag_hx(yb0, yb1, xr0, xr1, 1.0), ydag_hx(yr0, yr1, xb0, xb1, -1.0));
      fby += link_force(by, ydag_hy(yb0, yb1, xbp0, xbp1, 1.0), ydag_hy(ybp0, ybp1, xb0, xb1, -1.0));
    }
    pi[sa] = fma(-dt, fax, pax);
    pi[V + sa] = fma(-dt, fay, pay);
    pi[sb] = fma(-dt, fbx, pbx);
    pi[V + sb] = fma(-dt, fby, pby);
  }
}

// pi -= dt (Fg + sum_j w_j Ff(X_j, Y_j)), every link in one pass: the kick of a rational pseudofermion action
//   S = c0 phi^dag (1 + sum_j rho_j (D^dag D + mu_j^2)^-1) phi,   X_j = (D^dag D + mu_j^2)^-1 phi,  Y_j = D X_j,  w_j = c0 rho_j.
// The site pairs (qmg_u1_pair.h) and the expressions of k_hmc_momentum_update, so that one pole of weight 1 gives its bits: the gauge part
// first, from its 15 links, of which only the pair's four own links live on into the pole loop; then, pole by pole, the 20 spinor loads in
// front of that pole's arithmetic and four fused multiply-adds onto the pole sum, to which the gauge part is added last.
// GAUGE = false (the launches after the first when there are more than HMC_POLES_J poles) loads the four own links alone.
// Byte model: 64 + 64 n B/site -- pi read and written (32), two links (32), per pole X_j and Y_j (64).
template <bool GAUGE>
__global__ __launch_bounds__(BLOCK) void k_hmc_momentum_update_poles(double* __restrict__ pi, const cplx* __restrict__ gauge, const HmcPoles poles, int n_poles,
                                                                     int Lx, int Ly, double beta, double dt) {
  const long V = (long)Lx * Ly;
  const int h = Lx >> 1;
  const long npairs = V / 2;
  const cplx* __restrict__ Ux = gauge;
  const cplx* __restrict__ Uy = gauge + V;
  for (long t = (long)blockIdx.x * BLOCK + threadIdx.x; t < npairs; t += (long)gridDim.x * BLOCK) {
    const PairGeom g = pair_geom(t, h, Ly);
    const long sa = g.sa, sb = g.sb;
    const double pax = pi[sa], pay = pi[V + sa], pbx = pi[sb], pby = pi[V + sb];
    const PairOwn o = pair_own_links(Ux, Uy, g);
    PairForce d = {0.0, 0.0, 0.0, 0.0};   // the differences of sin P of the gauge force
    if (GAUGE) {
      d = pair_sin_diffs(pair_links(Ux, Uy, g, o));
      // Pin the four numbers here: they are used after the pole loop only, and left alone the compiler sinks the plaquettes below the loop
      // and carries the 15 links through it (212 VGPRs, 2 waves per SIMD instead of 4).
      asm volatile("" : "+v"(d.ax), "+v"(d.ay), "+v"(d.bx), "+v"(d.by));
    }
    // The pole sum starts from -0.0, the one number that fma(w, f, .) leaves every w f at, signed zeros included.
    double fax = -0.0, fay = -0.0, fbx = -0.0, fby = -0.0;
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
    // k_hmc_momentum_update's `beta * (...) + Ff` is contracted into one fma by the compiler; written out here so that the bits agree
    if (GAUGE) { fax = fma(beta, d.ax, fax); fay = fma(beta, d.ay, fay); fbx = fma(beta, d.bx, fbx); fby = fma(beta, d.by, fby); }
    pi[sa] = fma(-dt, fax, pax);
    pi[V + sa] = fma(-dt, fay, pay);
    pi[sb] = fma(-dt, fbx, pbx);
    pi[V + sb] = fma(-dt, fby, pby);
  }
}

// ---- staggered fermions (include/qmg/hmc_staggered.hpp; the independent statement is tests/stag_hmc_numpy.py) ----
// D = m + H, H psi(x) = -1/2 sum_mu eta_mu(x) [U_mu(x) psi(x+mu) - conj(U_mu(x-mu)) psi(x-mu)] (qmg_staggered_fill: eta_x = 1, eta_y = (-1)^x),
// A = m^2 - H^2, S_f = phi_e^dag (A_ee + sigma)^-1 phi_e.  With W = X_e (+) (H X_e)_o, X_e = (A_ee + sigma)^-1 phi_e and eps(x) = (-1)^(x+y):
//   Fs_mu(x) = dS_f/dtheta_mu(x) = eta_mu(x) eps(x) Im[ U_mu(x) conj(W(x)) W(x+mu) ]
// one complex number per site, two sites per link.
struct HmcStagPoles {   // the pole list of one launch of k_hmc_momentum_update_staggered, as HmcPoles
  const cplx* W[HMC_POLES_J];
  double w[HMC_POLES_J];
};
// Im[ u conj(a) b ]
__device__ __forceinline__ double im_u_adag_b(cplx u, cplx a, cplx b) {
  cplx c = cmake(0.0, 0.0);
  cmac_conj(c, a, b);
  return fma(u.x, c.y, u.y * c.x);
}

// pi -= dt (Fg + sum_j w_j Fs(W_j)), every link in one pass: the kick of two staggered tastes (one pole of weight 1) and of the rooted action
//   S = c0 phi_e^dag (1 + sum_j rho_j (A_ee + mu_j^2)^-1) phi_e,   w_j = c0 rho_j.
// The site pairs of qmg_u1_pair.h: a = (2 xh, y), b = (2 xh + 1, y), so eta_y is +1 on a and -1 on b and eps(a) = (-1)^y = -eps(b).  The gauge
// part comes first (pinned as in k_hmc_momentum_update_poles); then, pole by pole, five loads of W (a, b, the site right of b, the two above)
// in front of that pole's arithmetic and four fused multiply-adds onto the pole sum.  GAUGE = false (the launches after the
// first when there are more than HMC_POLES_J poles) loads the four own links alone.
// Byte model: 64 + 16 n B/site -- pi read and written (32), two links (32), per pole W_j (16).
template <bool GAUGE>
__global__ __launch_bounds__(BLOCK) void k_hmc_momentum_update_staggered(double* __restrict__ pi, const cplx* __restrict__ gauge, const HmcStagPoles poles, int n_poles,
                                                                         int Lx, int Ly, double beta, double dt) {
  const long V = (long)Lx * Ly;
  const int h = Lx >> 1;
  const long npairs = V / 2;
  const cplx* __restrict__ Ux = gauge;
  const cplx* __restrict__ Uy = gauge + V;
  for (long t = (long)blockIdx.x * BLOCK + threadIdx.x; t < npairs; t += (long)gridDim.x * BLOCK) {
    const PairGeom g = pair_geom(t, h, Ly);
    const long sa = g.sa, sb = g.sb;
    const double pax = pi[sa], pay = pi[V + sa], pbx = pi[sb], pby = pi[V + sb];
    const PairOwn o = pair_own_links(Ux, Uy, g);
    PairForce d = {0.0, 0.0, 0.0, 0.0};   // the differences of sin P of the gauge force
    if (GAUGE) {
      d = pair_sin_diffs(pair_links(Ux, Uy, g, o));
      asm volatile("" : "+v"(d.ax), "+v"(d.ay), "+v"(d.bx), "+v"(d.by));   // keep the 15 links out of the pole loop, as in k_hmc_momentum_update_poles
    }
    const double ea = g.q ? -1.0 : 1.0;   // eps(a); eta_x eps = ea, -ea on (a, b); eta_y eps = ea on both
    double fax = -0.0, fay = -0.0, fbx = -0.0, fby = -0.0;
    const long sr = g.ra + g.xr, sap = g.rap + g.xh, sbp = g.rbp + g.xh;
    for (int j = 0; j < n_poles; j++) {
      const cplx* __restrict__ W = poles.W[j];
      const double wa = ea * poles.w[j];
      const cplx a = W[sa], b = W[sb], r = W[sr], ap = W[sap], bp = W[sbp];
      fax = fma(wa, im_u_adag_b(o.ax, a, b), fax);
      fay = fma(wa, im_u_adag_b(o.ay, a, ap), fay);
      fbx = fma(-wa, im_u_adag_b(o.bx, b, r), fbx);
      fby = fma(wa, im_u_adag_b(o.by, b, bp), fby);
    }
    if (GAUGE) { fax = fma(beta, d.ax, fax); fay = fma(beta, d.ay, fay); fbx = fma(beta, d.bx, fbx); fby = fma(beta, d.by, fby); }
    pi[sa] = fma(-dt, fax, pax);
    pi[V + sa] = fma(-dt, fay, pay);
    pi[sb] = fma(-dt, fbx, pbx);
    pi[V + sb] = fma(-dt, fby, pby);
  }
}

// ---- domain-wall fermions (include/qmg/hmc_dwf.hpp; the independent statement is tests/dwf_hmc_numpy.py) ----
// The force of S_f = phi^dag P (M^dag M)^-1 P^dag phi is the Wilson bilinear Ff above summed over the Ls slices of pairs of FIVE-dimensional
// full-lattice vectors (the hops of the domain-wall operator are diagonal in s and are the Wilson hops on every slice):
//   pi -= dt (Fg + sum_j w_j sum_s Ff(X_j(.; s), Y_j(.; s)))
// The vectors are nc = 2 Ls in the even-odd layout, c = 2 s + sigma: the chunk (sigma 0, sigma 1) of (site, s) is 32 bytes at (site Ls + s) 32.
// G5Y reads Y_j as Gamma5 Y_j: the chunk of slice Ls-1-s with the sign of sigma 1 flipped.
//
// Lane mapping: kernels D and K's -- one lane per (site, s), rows (parity, y) over grid.y, block-uniform row bases, so every chunk load of a
// wave is one contiguous run.  A site owns its two forward links: a lane loads X and Y at its site, at x + xhat (the other parity's row y) and
// at x + yhat (the other parity's row y + 1) -- six chunks per pair, in front of that pair's arithmetic -- and forms its slice's share of the two
// forces, pair by pair in the order given.  The shares go into LDS; after one barrier lane s = 0 adds the Ls shares of the x link in the order
// s = 0 .. Ls-1, lane s = 1 those of the y link, each adds the gauge force of its link (from the ten links around the site, loaded in front of the
// pair loop) and updates its momentum.  The order is fixed and there is no atomic: two runs give the same bits.  The block is
// Ls floor(256 / Ls) lanes, so a site never straddles a block whatever Ls is; lanes past the end of a half row stay for the barrier, load what
// lane (0, s) loads and store nothing.  Two LDS buffers alternate, so one barrier per row suffices: 2 x 256 x 16 B = 8 KiB per block.
// GAUGE = false (the launches after the first when there are more than HMC_DWF_PAIRS pairs) loads the two own links alone.
// Byte model: 64 + 64 Ls n B/site -- pi read and written (32), two links (32), per pair X_j and Y_j (2 x 32 Ls); the neighbours from cache.
struct HmcDwfPairs {
  const char* X[HMC_DWF_PAIRS];
  const char* Y[HMC_DWF_PAIRS];
  double w[HMC_DWF_PAIRS];
};

template <bool GAUGE>
__global__ __launch_bounds__(DWF_BLOCK_MAX) void k_hmc_momentum_update_dwf(double* __restrict__ pi, const cplx* __restrict__ gauge, const HmcDwfPairs pr, int n_pairs,
                                                                               int g5y, int hr, int Ly, int Ls, double beta, double dt) {
  typedef double v4 __attribute__((ext_vector_type(4)));   // a lane's chunk: (sigma 0 re, im, sigma 1 re, im)
  constexpr unsigned CH = 32u;
  __shared__ double2 share[2][DWF_BLOCK_MAX];
  const int tid = threadIdx.x;
  const dwf::Lane ln = dwf::lane_of<true>(hr, Ls);   // a site is live or not as a whole: the block and the half row are multiples of Ls lanes
  const int j = ln.j, s = ln.s;
  const bool live = ln.live;
  const int base = tid - s;               // the site's shares in LDS: base .. base + Ls - 1, all in this block
  const int sy = g5y ? Ls - 1 - s : s;
  const double g5 = g5y ? -1.0 : 1.0;
  const long half_vol = (long)hr * Ly, V = 2 * half_vol;
  const long row_bytes = (long)hr * Ls * CH;
  const cplx* __restrict__ Ux = gauge;
  const cplx* __restrict__ Uy = gauge + V;
  const bool writer = live && s < 2;      // s = 0: the x link, s = 1: the y link
  int buf = 0;
  for (int row = blockIdx.y; row < 2 * Ly; row += gridDim.y) {
    const int p = row & 1, y = row >> 1;
    // dwf::row_of<double, false>'s geometry, written out, in row indices (the links are indexed by site): through the helper both
    // instantiations keep their 470 / 605 lines of device code but not their order (profiles/dwf_lane_refactor.txt).
    const int sx = (y + p) & 1;
    int jp = j + sx;     if (jp == hr) jp = 0;
    int jm = j + sx - 1; if (jm < 0) jm = hr - 1;
    const int yp = (y + 1 == Ly) ? 0 : y + 1;
    const int ym = (y == 0) ? Ly - 1 : y - 1;
    const long r_own = (long)p * Ly + y, r_x = (long)(1 - p) * Ly + y, r_yp = (long)(1 - p) * Ly + yp;
    const long site = r_own * hr + j;
    const cplx ux = Ux[site], uy = Uy[site];
    double p_old = 0.0, dg = 0.0;
    double* dst = pi + (s == 1 ? V : 0) + site;
    if (writer) {
      p_old = *dst;
      if (GAUGE) {
        // sin P(x) and, for the x link, sin P(x - yhat); for the y link, sin P(x - xhat)
        const long s_xp = r_x * hr + jp, s_yp = r_yp * hr + j;
        const double sP = im_plaq(ux, Uy[s_xp], Ux[s_yp], uy);
        if (s == 0) {
          const long s_ym = ((long)(1 - p) * Ly + ym) * hr + j, s_ymxp = ((long)p * Ly + ym) * hr + jp;
          dg = im_plaq(Ux[s_ym], Uy[s_ymxp], ux, Uy[s_ym]);
          dg = sP - dg;
        } else {
          const long s_xm = r_x * hr + jm, s_xmyp = ((long)p * Ly + yp) * hr + jm;
          dg = im_plaq(Ux[s_xm], uy, Ux[s_xmyp], Uy[s_xm]);
          dg = dg - sP;
        }
        asm volatile("" : "+v"(dg));   // keep the links out of the pair loop, as in k_hmc_momentum_update_poles
      }
    }
    const unsigned ox_own = (unsigned)(j * Ls + s) * CH, oy_own = (unsigned)(j * Ls + sy) * CH;
    const unsigned ox_xp = (unsigned)(jp * Ls + s) * CH, oy_xp = (unsigned)(jp * Ls + sy) * CH;
    // The pair sum starts from -0.0, the one number that fma(w, f, .) leaves every w f at, signed zeros included.
    double fx = -0.0, fy = -0.0;
    for (int k = 0; k < n_pairs; k++) {
      const char* X = pr.X[k];
      const char* Y = pr.Y[k];
      const double w = pr.w[k];
      const gchar* xo = uni(X + r_own * row_bytes);
      const gchar* xx = uni(X + r_x * row_bytes);
      const gchar* xy = uni(X + r_yp * row_bytes);
      const gchar* yo = uni(Y + r_own * row_bytes);
      const gchar* yx = uni(Y + r_x * row_bytes);
      const gchar* yy = uni(Y + r_yp * row_bytes);
      const v4 xa = gld<v4>(xo, ox_own), xb = gld<v4>(xx, ox_xp), xc = gld<v4>(xy, ox_own);
      v4 ya = gld<v4>(yo, oy_own), yb = gld<v4>(yx, oy_xp), yc = gld<v4>(yy, oy_own);
      __builtin_amdgcn_sched_barrier(0);
      ya.z *= g5; ya.w *= g5; yb.z *= g5; yb.w *= g5; yc.z *= g5; yc.w *= g5;
      const cplx xa0 = cmake(xa.x, xa.y), xa1 = cmake(xa.z, xa.w), xb0 = cmake(xb.x, xb.y), xb1 = cmake(xb.z, xb.w), xc0 = cmake(xc.x, xc.y), xc1 = cmake(xc.z, xc.w);
      const cplx ya0 = cmake(ya.x, ya.y), ya1 = cmake(ya.z, ya.w), yb0 = cmake(yb.x, yb.y), yb1 = cmake(yb.z, yb.w), yc0 = cmake(yc.x, yc.y), yc1 = cmake(yc.z, yc.w);
      fx = fma(w, link_force(ux, ydag_hx(ya0, ya1, xb0, xb1, 1.0), ydag_hx(yb0, yb1, xa0, xa1, -1.0)), fx);
      fy = fma(w, link_force(uy, ydag_hy(ya0, ya1, xc0, xc1, 1.0), ydag_hy(yc0, yc1, xa0, xa1, -1.0)), fy);
    }
    share[buf][tid] = make_double2(fx, fy);
    __syncthreads();
    if (writer) {
      double f = -0.0;
      for (int k = 0; k < Ls; k++) {
        const double2 v = share[buf][base + k];
        f += s == 0 ? v.x : v.y;
      }
      if (GAUGE) f = fma(beta, dg, f);
      *dst = fma(-dt, f, p_old);
    }
    buf ^= 1;
  }
}

// theta += dt pi ; U = exp(i theta), one pass over the 2 V links.  One fma: the phases are within one rounding of a host `theta + dt * pi`.
__global__ __launch_bounds__(BLOCK) void k_hmc_link_update(double* __restrict__ theta, cplx* __restrict__ gauge, const double* __restrict__ pi, long n, double dt) {
  for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * BLOCK) {
    const double th = fma(dt, pi[i], theta[i]);
    double s, c;
    sincos(th, &s, &c);
    theta[i] = th;
    gauge[i] = cmake(c, s);
  }
}

// One step of the pure-gauge inner loop of a two-scale integrator in one pass, on the site pairs of qmg_u1_pair.h:
//   pi -= dt_kick beta C^T sin P(in) ;  theta += dt_drift pi ;  out = exp(i theta)
// A thread owns the four links of its pair: four momenta, four phases and the pair's 15 links of `in`, all loaded in front of the arithmetic.
// The kick is k_hmc_momentum_update<false>'s expression (beta times the difference of sin P, one fma onto the momentum), the drift and the
// sincos are k_hmc_link_update's, so the three fields carry the bits of those two launches.  out != in: neighbours are read from `in`.
// Byte model: 128 B/site -- pi read and written (32), theta read and written (32), two links read (32), two written (32).
// Blocks of 128 threads (grid_1d with that block): at 2048^2 a step took 0.114 ms against 0.127 ms in blocks of 256 (profiles/hmc_gauge_step_bench.txt).
constexpr int GAUGE_STEP_BLOCK = 128;
__global__ __launch_bounds__(GAUGE_STEP_BLOCK) void k_hmc_gauge_step(double* __restrict__ theta, cplx* __restrict__ out, const cplx* __restrict__ in, double* __restrict__ pi,
                                                          int Lx, int Ly, double beta, double dt_kick, double dt_drift) {
  const long V = (long)Lx * Ly;
  const int h = Lx >> 1;
  const long npairs = V / 2;
  const cplx* __restrict__ Ux = in;
  const cplx* __restrict__ Uy = in + V;
  for (long t = (long)blockIdx.x * GAUGE_STEP_BLOCK + threadIdx.x; t < npairs; t += (long)gridDim.x * GAUGE_STEP_BLOCK) {
    const PairGeom g = pair_geom(t, h, Ly);
    const long sa = g.sa, sb = g.sb;
    const double pax = pi[sa], pay = pi[V + sa], pbx = pi[sb], pby = pi[V + sb];
    const double tax = theta[sa], tay = theta[V + sa], tbx = theta[sb], tby = theta[V + sb];
    const PairForce d = pair_sin_diffs(pair_links(Ux, Uy, g));

    const double fax = beta * d.ax, fay = beta * d.ay, fbx = beta * d.bx, fby = beta * d.by;
    const double nax = fma(-dt_kick, fax, pax), nay = fma(-dt_kick, fay, pay), nbx = fma(-dt_kick, fbx, pbx), nby = fma(-dt_kick, fby, pby);
    const double hax = fma(dt_drift, nax, tax), hay = fma(dt_drift, nay, tay), hbx = fma(dt_drift, nbx, tbx), hby = fma(dt_drift, nby, tby);
    // The eight real stores first, so that only the four new phases live on into the sincos calls, and those in a loop that stays rolled: 92
    // VGPRs and 5 waves per SIMD, where the four calls written out between the stores took 138 and 3 (profiles/hmc_gauge_step_resource_usage.txt).
    pi[sa] = nax; pi[V + sa] = nay; pi[sb] = nbx; pi[V + sb] = nby;
    theta[sa] = hax; theta[V + sa] = hay; theta[sb] = hbx; theta[V + sb] = hby;
    const double hs[4] = {hax, hay, hbx, hby};
    const long is[4] = {sa, V + sa, sb, V + sb};
#pragma unroll 1
    for (int k = 0; k < 4; k++) {
      double s, c;
      sincos(hs[k], &s, &c);
      out[is[k]] = cmake(c, s);
    }
  }
}

}  // namespace qmg

using namespace qmg;

// What the two pole kicks (qmg_hmc_momentum_update_poles, _staggered) check first; the pole lists they check after the pure-gauge case has
// left are pole_lists_valid's (qmg_hmc_bilinear.h).
static bool pole_kick_args_valid(const double* pi, const void* gauge, int Lx, int Ly, double beta, double dt, int n_poles, unsigned flags) {
  return pi && gauge && valid_lattice(Lx, Ly) && beta == beta && dt == dt && n_poles >= 0 && !(flags & ~(unsigned)QMG_HMC_GAUGE_ONLY);
}

extern "C" {

// pi -= dt (Fg + Ff).  pi: DEVICE double[2 Lx Ly]; gauge: DEVICE complex<double>[2 Lx Ly], the links exp(i theta) that qmg_hmc_link_update
// keeps beside the phases; X = (D^dag D)^-1 phi and Y = D X: DEVICE complex<double>[2 Lx Ly] spinors.  flags & QMG_HMC_GAUGE_ONLY drops
// the fermion force (X and Y are not read and may be null).  pi must not overlap the other fields.
int qmg_hmc_momentum_update(double* pi, const void* gauge, const void* X, const void* Y, int Lx, int Ly, double beta, double dt, unsigned flags, void* stream) {
  if (!pi || !gauge || !valid_lattice(Lx, Ly) || beta != beta || dt != dt || (flags & ~(unsigned)QMG_HMC_GAUGE_ONLY)) return QMG_ERR_INVALID;
  const bool fermions = !(flags & QMG_HMC_GAUGE_ONLY);
  if (fermions && (!X || !Y)) return QMG_ERR_INVALID;
  const unsigned g = grid_1d((size_t)Lx * Ly / 2);
  if (fermions) k_hmc_momentum_update<true><<<g, BLOCK, 0, as_stream(stream)>>>(pi, (const cplx*)gauge, (const cplx*)X, (const cplx*)Y, Lx, Ly, beta, dt);
  else k_hmc_momentum_update<false><<<g, BLOCK, 0, as_stream(stream)>>>(pi, (const cplx*)gauge, nullptr, nullptr, Lx, Ly, beta, dt);
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

// pi -= dt (Fg + sum_j weights[j] Ff(X[j], Y[j])) in one pass over the momenta and links.  X, Y: HOST arrays of n_poles DEVICE spinors
// (X[j] = (D^dag D + mu_j^2)^-1 phi, Y[j] = D X[j]); weights: HOST double[n_poles].  Up to 16 poles go in one launch; further poles take
// further launches without the gauge force.  n_poles = 0 or flags & QMG_HMC_GAUGE_ONLY is the pure-gauge kick (X, Y, weights are not read
// and may be null).  One pole of weight 1 gives the bits of qmg_hmc_momentum_update.  pi must not overlap the other fields.
int qmg_hmc_momentum_update_poles(double* pi, const void* gauge, const void* const* X, const void* const* Y, const double* weights, int n_poles, int Lx, int Ly,
                                  double beta, double dt, unsigned flags, void* stream) {
  if (!pole_kick_args_valid(pi, gauge, Lx, Ly, beta, dt, n_poles, flags)) return QMG_ERR_INVALID;
  if ((flags & QMG_HMC_GAUGE_ONLY) || n_poles == 0) return qmg_hmc_momentum_update(pi, gauge, nullptr, nullptr, Lx, Ly, beta, dt, QMG_HMC_GAUGE_ONLY, stream);
  if (!pole_lists_valid(X, Y, weights, n_poles)) return QMG_ERR_INVALID;
  const unsigned g = grid_1d((size_t)Lx * Ly / 2);
  return launch_pole_chunks<HMC_POLES_J>(n_poles, [&](int j0, int nj, bool first) {
    HmcPoles p;
    for (int j = 0; j < HMC_POLES_J; j++) {
      p.X[j] = j < nj ? (const cplx*)X[j0 + j] : nullptr;
      p.Y[j] = j < nj ? (const cplx*)Y[j0 + j] : nullptr;
      p.w[j] = j < nj ? weights[j0 + j] : 0.0;
    }
    if (first) k_hmc_momentum_update_poles<true><<<g, BLOCK, 0, as_stream(stream)>>>(pi, (const cplx*)gauge, p, nj, Lx, Ly, beta, dt);
    else k_hmc_momentum_update_poles<false><<<g, BLOCK, 0, as_stream(stream)>>>(pi, (const cplx*)gauge, p, nj, Lx, Ly, beta, dt);
  });
}

// pi -= dt (Fg + sum_j weights[j] Fs(W[j])) in one pass over the momenta and links, Fs the staggered force above.  W: HOST array of n_poles
// DEVICE complex<double>[Lx Ly] vectors (nc = 1, even-odd layout; even half (A_ee + mu_j^2)^-1 phi_e, odd half its hopping apply); weights:
// HOST double[n_poles].  Up to 16 poles go in one launch; further poles take further launches without the gauge force.  n_poles = 0 or
// flags & QMG_HMC_GAUGE_ONLY is the pure-gauge kick of qmg_hmc_momentum_update (W, weights are not read and may be null).  pi must not
// overlap the other fields.
int qmg_hmc_momentum_update_staggered(double* pi, const void* gauge, const void* const* W, const double* weights, int n_poles, int Lx, int Ly, double beta, double dt,
                                      unsigned flags, void* stream) {
  if (!pole_kick_args_valid(pi, gauge, Lx, Ly, beta, dt, n_poles, flags)) return QMG_ERR_INVALID;
  if ((flags & QMG_HMC_GAUGE_ONLY) || n_poles == 0) return qmg_hmc_momentum_update(pi, gauge, nullptr, nullptr, Lx, Ly, beta, dt, QMG_HMC_GAUGE_ONLY, stream);
  if (!pole_lists_valid(W, W, weights, n_poles)) return QMG_ERR_INVALID;
  const unsigned g = grid_1d((size_t)Lx * Ly / 2);
  return launch_pole_chunks<HMC_POLES_J>(n_poles, [&](int j0, int nj, bool first) {
    HmcStagPoles p;
    for (int j = 0; j < HMC_POLES_J; j++) {
      p.W[j] = j < nj ? (const cplx*)W[j0 + j] : nullptr;
      p.w[j] = j < nj ? weights[j0 + j] : 0.0;
    }
    if (first) k_hmc_momentum_update_staggered<true><<<g, BLOCK, 0, as_stream(stream)>>>(pi, (const cplx*)gauge, p, nj, Lx, Ly, beta, dt);
    else k_hmc_momentum_update_staggered<false><<<g, BLOCK, 0, as_stream(stream)>>>(pi, (const cplx*)gauge, p, nj, Lx, Ly, beta, dt);
  });
}

// pi -= dt (Fg + sum_j weights[j] sum_s Ff(X[j](.; s), Y[j](.; s))) in one pass over the momenta and links: the kick of domain-wall pseudofermions.
// X, Y: HOST arrays of n_pairs DEVICE complex<double>[2 Ls Lx Ly] vectors (nc = 2 Ls, c = 2 s + sigma, even-odd layout), 16-byte aligned;
// weights: HOST double[n_pairs], any sign.  flags & QMG_HMC_DWF_G5_Y reads every Y[j] as Gamma5 Y[j].  Up to HMC_DWF_PAIRS pairs go in one
// launch; further pairs take further launches without the gauge force.  n_pairs = 0 or flags & QMG_HMC_GAUGE_ONLY is the pure-gauge kick of
// qmg_hmc_momentum_update (X, Y, weights are not read and may be null).  pi must not overlap the other fields.
int qmg_hmc_momentum_update_dwf(double* pi, const void* gauge, const void* const* X, const void* const* Y, const double* weights, int n_pairs, int Ls, int Lx, int Ly,
                                double beta, double dt, unsigned flags, void* stream) {
  const HmcDwfPlan pl = hmc_dwf_plan(Lx, Ly, Ls, n_pairs, flags);
  if (pl.family == HDF_INVALID || pl.family == HDF_UNSUPPORTED) return pl.status;
  if (!pi || !gauge || beta != beta || dt != dt) return QMG_ERR_INVALID;
  if (pl.family == HDF_GAUGE) return qmg_hmc_momentum_update(pi, gauge, nullptr, nullptr, Lx, Ly, beta, dt, QMG_HMC_GAUGE_ONLY, stream);
  if (!pole_lists_valid(X, Y, weights, n_pairs)) return QMG_ERR_INVALID;
  for (int j = 0; j < n_pairs; j++)
    if (!aligned16(X[j]) || !aligned16(Y[j])) return QMG_ERR_INVALID;
  const dim3 grid((unsigned)pl.gx, (unsigned)pl.gy);
  const int g5y = (flags & QMG_HMC_DWF_G5_Y) ? 1 : 0;
  return launch_pole_chunks<HMC_DWF_PAIRS>(n_pairs, [&](int j0, int nj, bool first) {
    HmcDwfPairs p;
    for (int j = 0; j < HMC_DWF_PAIRS; j++) {
      p.X[j] = j < nj ? (const char*)X[j0 + j] : nullptr;
      p.Y[j] = j < nj ? (const char*)Y[j0 + j] : nullptr;
      p.w[j] = j < nj ? weights[j0 + j] : 0.0;
    }
    if (first) k_hmc_momentum_update_dwf<true><<<grid, (unsigned)pl.block, 0, as_stream(stream)>>>(pi, (const cplx*)gauge, p, nj, g5y, Lx / 2, Ly, Ls, beta, dt);
    else k_hmc_momentum_update_dwf<false><<<grid, (unsigned)pl.block, 0, as_stream(stream)>>>(pi, (const cplx*)gauge, p, nj, g5y, Lx / 2, Ly, Ls, beta, dt);
  });
}

// What qmg_hmc_momentum_update_dwf launches for a request (host only): plan_out = (family, lanes per site, block, gx, gy, LDS bytes, launches,
// pairs per launch); entries past the eighth are -1.
int qmg_hmc_dwf_plan(int Lx, int Ly, int Ls, int n_pairs, unsigned flags, int* plan_out, int plan_len) {
  if (!plan_out || plan_len < HMC_DWF_PLAN_INTS) return QMG_ERR_INVALID;
  const HmcDwfPlan pl = hmc_dwf_plan(Lx, Ly, Ls, n_pairs, flags);
  const int v[HMC_DWF_PLAN_INTS] = {pl.family, pl.lps, pl.block, pl.gx, pl.gy, pl.lds, pl.launches, pl.per_launch};
  export_plan_ints(v, HMC_DWF_PLAN_INTS, plan_out, plan_len);
  return QMG_SUCCESS;
}

// theta += dt pi ; gauge = exp(i theta).  theta, pi: DEVICE double[n]; gauge: DEVICE complex<double>[n]; n = 2 Lx Ly links.
int qmg_hmc_link_update(double* theta, void* gauge, const double* pi, size_t n, double dt, void* stream) {
  if ((!theta || !gauge || !pi) && n) return QMG_ERR_INVALID;
  if (dt != dt) return QMG_ERR_INVALID;
  if (n == 0) return QMG_SUCCESS;
  k_hmc_link_update<<<grid_1d(n), BLOCK, 0, as_stream(stream)>>>(theta, (cplx*)gauge, pi, (long)n, dt);
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

// pi -= dt_kick beta C^T sin P(gauge_in) ; theta += dt_drift pi ; gauge_out = exp(i theta), one launch: the bits of qmg_hmc_momentum_update with
// QMG_HMC_GAUGE_ONLY and dt_kick followed by qmg_hmc_link_update with dt_drift.  theta, pi: DEVICE double[2 Lx Ly]; gauge_in, gauge_out: DEVICE
// complex<double>[2 Lx Ly], DIFFERENT buffers (neighbours are read from gauge_in); no two of the four fields may overlap.
int qmg_hmc_gauge_step(double* theta, void* gauge_out, const void* gauge_in, double* pi, int Lx, int Ly, double beta, double dt_kick, double dt_drift, void* stream) {
  if (!theta || !gauge_out || !gauge_in || !pi || !valid_lattice(Lx, Ly) || beta != beta || dt_kick != dt_kick || dt_drift != dt_drift) return QMG_ERR_INVALID;
  const size_t n = 2 * (size_t)Lx * Ly, nr = sizeof(double) * n, nc = sizeof(cplx) * n;
  if (fields_overlap(gauge_out, nc, gauge_in, nc) || fields_overlap(theta, nr, pi, nr) || fields_overlap(theta, nr, gauge_in, nc) || fields_overlap(theta, nr, gauge_out, nc) ||
      fields_overlap(pi, nr, gauge_in, nc) || fields_overlap(pi, nr, gauge_out, nc))
    return QMG_ERR_INVALID;
  k_hmc_gauge_step<<<grid_1d((size_t)Lx * Ly / 2, GAUGE_STEP_BLOCK), GAUGE_STEP_BLOCK, 0, as_stream(stream)>>>(theta, (cplx*)gauge_out, (const cplx*)gauge_in, pi, Lx, Ly, beta, dt_kick, dt_drift);
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

// Momentum refresh: pi ~ N(0, 1) per link, a function of (seed, trajectory) alone.  The n doubles are filled as n/2 complex numbers by
// qmg_gaussian, whose Box-Muller pair has unit variance in EACH real component; n must be even (it is 2 Lx Ly).
int qmg_hmc_momentum_refresh(double* pi, size_t n, unsigned long long seed, unsigned long long trajectory, void* stream) {
  if ((!pi && n) || (n & 1)) return QMG_ERR_INVALID;
  return qmg_gaussian(pi, n / 2, qmg_hmc_stream_seed(seed, trajectory, 0), stream);
}

// The seed of random field number `field` of trajectory `trajectory` (0: momenta, 1: pseudofermion noise, 2: Metropolis number): an
// injective-looking 64-bit mix of the three, so that neither trajectories nor the fields of one trajectory share a stream.
unsigned long long qmg_hmc_stream_seed(unsigned long long seed, unsigned long long trajectory, int field) {
  unsigned long long z = seed * 0x9E3779B97F4A7C15ull + (3ull * trajectory + (unsigned long long)field + 1ull) * 0xD1B54A32D192ED03ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

}  // extern "C"
