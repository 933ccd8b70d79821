// qmg_u1_pair.h -- the site-pair thread mapping of the U(1) link kernels: k_ape_smear (qmg_u1.hip), the three momentum kicks (qmg_hmc.hip),
// k_flow_stage (qmg_flow.hip) and the four stout kernels (qmg_stout.hip).
//
// Even-odd layout (lattice.h:75-81): site (x, y) has index (y + p Ly) Lx/2 + x/2, p = (x + y) & 1, so the sites of one parity of a row y are
// Lx/2 consecutive elements.  Thread t owns the PAIR of sites a = (2 xh, y) and b = (2 xh + 1, y), xh = t % (Lx/2), y = t / (Lx/2): one of each
// parity, at the same offset xh of their two rows, so every load and store of a wave is one contiguous run.  The thread writes all four links
// (or momenta, or phases) of its pair from the 15 links around it:
//
//     lp--lpx--ap--apx--bp--bpx---+          a, b : the pair;   l : the odd-x site left of a;   r : the even-x site right of b
//     |        |        |         |          lp, ap, bp : the sites above l, a, b (y + 1);   am, bm, rm : below a, b, r (y - 1)
//     ly P(l)  ay P(a)  by P(b)   ry         ..x, ..y : the x-link and the y-link that START at the site
//     |        |        |         |
//     l---lx---a---ax---b---bx----r          the five plaquettes behind the pair's four links:  P(a), P(b), P(a-y) = P(am), P(b-y) = P(bm),
//              |        |         |          P(a-x) = P(l);  P(b-x) is P(a) again -- which is why a pair needs 15 links where two single
//              amy P(am) bmy P(bm) rmy       sites need 20
//              |        |         |
//              am--amx--bm--bmx---rm
//
// Rows: the even-x sites at height y' have parity y' & 1, the odd-x sites the other one; ra, rb are the row offsets of a and b (r sits in a's row,
// l in b's), rap, rbp those of the rows above, ram, rbm below.  Every y' and every xl, xr is wrapped, so each index is a lattice site and nothing
// is read or written outside the fields; on the thinnest lattices (Lx = 2: xl = xr = xh; Ly = 2: yp = ym) neighbours coincide and the same
// expressions hold.  The loads are unconditional and the kernels place them in front of their arithmetic.
#ifndef QMG_U1_PAIR_H
#define QMG_U1_PAIR_H

#include "qmg_common.h"

namespace qmg {

__device__ __forceinline__ long eo_index(int x, int y, int Lx, int Ly) {
  const int p = (x + y) & 1;
  return (long)(y + p * Ly) * (Lx >> 1) + (x >> 1);
}

__device__ __forceinline__ double im_plaq(cplx a, cplx b, cplx c, cplx d) {   // Im[ a b conj(c) conj(d) ]
  const cplx ab = cmul(a, b), cd = cmul(c, d);
  return fma(ab.y, cd.x, -ab.x * cd.y);
}

struct PairGeom {
  int xh, xl, xr;       // offset of the pair in its rows, and of l and r in theirs
  int q;                // y & 1: eps(a) = (-1)^q = -eps(b)
  long ra, rb;          // rows of the even-x / odd-x sites at y
  long rap, rbp;        // at y + 1
  long ram, rbm;        // at y - 1
  long sa, sb;          // the pair's own two sites, ra + xh and rb + xh
};
__device__ __forceinline__ PairGeom pair_geom(long t, int h, int Ly) {   // h = Lx / 2
  const int xh = (int)(t % h), y = (int)(t / h);
  const int yp = (y + 1 == Ly) ? 0 : y + 1, ym = (y == 0) ? Ly - 1 : y - 1;
  const int xl = (xh == 0) ? h - 1 : xh - 1, xr = (xh + 1 == h) ? 0 : xh + 1;
  const int q = y & 1, qp = yp & 1, qm = ym & 1;
  PairGeom g;
  g.xh = xh; g.xl = xl; g.xr = xr; g.q = q;
  g.ra = (long)(y + q * Ly) * h;        g.rb = (long)(y + (1 - q) * Ly) * h;
  g.rap = (long)(yp + qp * Ly) * h;     g.rbp = (long)(yp + (1 - qp) * Ly) * h;
  g.ram = (long)(ym + qm * Ly) * h;     g.rbm = (long)(ym + (1 - qm) * Ly) * h;
  g.sa = g.ra + xh;
  g.sb = g.rb + xh;
  return g;
}

struct PairOwn { cplx ax, ay, bx, by; };   // the four links the pair owns
struct PairLinks { cplx ax, ay, bx, by, apx, bpx, amx, amy, bmx, bmy, lx, ly, lpx, ry, rmy; };

__device__ __forceinline__ PairOwn pair_own_links(const cplx* __restrict__ Ux, const cplx* __restrict__ Uy, const PairGeom& g) {
  PairOwn o;
  o.ax = Ux[g.sa]; o.ay = Uy[g.sa]; o.bx = Ux[g.sb]; o.by = Uy[g.sb];
  return o;
}
// the eleven links around the pair, behind its own four
__device__ __forceinline__ PairLinks pair_links(const cplx* __restrict__ Ux, const cplx* __restrict__ Uy, const PairGeom& g, const PairOwn o) {
  PairLinks u;
  u.ax = o.ax; u.ay = o.ay; u.bx = o.bx; u.by = o.by;
  u.apx = Ux[g.rap + g.xh]; u.bpx = Ux[g.rbp + g.xh];
  u.amx = Ux[g.ram + g.xh]; u.amy = Uy[g.ram + g.xh]; u.bmx = Ux[g.rbm + g.xh]; u.bmy = Uy[g.rbm + g.xh];
  u.lx = Ux[g.rb + g.xl]; u.ly = Uy[g.rb + g.xl]; u.lpx = Ux[g.rbp + g.xl];
  u.ry = Uy[g.ra + g.xr]; u.rmy = Uy[g.ram + g.xr];
  return u;
}
__device__ __forceinline__ PairLinks pair_links(const cplx* __restrict__ Ux, const cplx* __restrict__ Uy, const PairGeom& g) {
  return pair_links(Ux, Uy, g, pair_own_links(Ux, Uy, g));
}

// dS/dtheta of S = sum_x (1 - cos P(x)) at the pair's four links: the differences of sin P = Im of the plaquette of the links.
//   a + x = b, a + y = ap, b + x = r, (a-y) + x = b-y, (a-y) + y = a, l + x = a
// For the two pole kicks and k_flow_stage; k_hmc_momentum_update writes the same loads and expressions out (see there), k_ape_smear its loads.
struct PairForce { double ax, ay, bx, by; };
__device__ __forceinline__ PairForce pair_sin_diffs(const PairLinks& u) {
  const double sPa = im_plaq(u.ax, u.by, u.apx, u.ay), sPb = im_plaq(u.bx, u.ry, u.bpx, u.by);
  const double sPam = im_plaq(u.amx, u.bmy, u.ax, u.amy), sPbm = im_plaq(u.bmx, u.rmy, u.bx, u.bmy);
  const double sPl = im_plaq(u.lx, u.ay, u.lpx, u.ly);
  PairForce d;
  d.ax = sPa - sPam; d.ay = sPl - sPa;
  d.bx = sPb - sPbm; d.by = sPa - sPb;
  return d;
}

// ---- for the stout kernels (qmg_stout.hip): the real part of the plaquettes, and a real link field on the pair's 15 links ----
__device__ __forceinline__ double re_plaq(cplx a, cplx b, cplx c, cplx d) {   // Re[ a b conj(c) conj(d) ]
  const cplx ab = cmul(a, b), cd = cmul(c, d);
  return fma(ab.x, cd.x, ab.y * cd.y);
}

// A real link field F (a force: [mu][site] doubles) at the 15 links of PairLinks, by the same indices.
struct PairReals { double ax, ay, bx, by, apx, bpx, amx, amy, bmx, bmy, lx, ly, lpx, ry, rmy; };
__device__ __forceinline__ PairReals pair_reals(const double* __restrict__ Fx, const double* __restrict__ Fy, const PairGeom& g) {
  PairReals f;
  f.ax = Fx[g.sa]; f.ay = Fy[g.sa]; f.bx = Fx[g.sb]; f.by = Fy[g.sb];
  f.apx = Fx[g.rap + g.xh]; f.bpx = Fx[g.rbp + g.xh];
  f.amx = Fx[g.ram + g.xh]; f.amy = Fy[g.ram + g.xh]; f.bmx = Fx[g.rbm + g.xh]; f.bmy = Fy[g.rbm + g.xh];
  f.lx = Fx[g.rb + g.xl]; f.ly = Fy[g.rb + g.xl]; f.lpx = Fx[g.rbp + g.xl];
  f.ry = Fy[g.ra + g.xr]; f.rmy = Fy[g.ram + g.xr];
  return f;
}

// (C^T [cos P . (C F)]) at the pair's four links, C the lattice curl (C F)(x) = F_x(x) + F_y(x+xhat) - F_x(x+yhat) - F_y(x): the five
// plaquettes of pair_sin_diffs with cos P = Re of the plaquette of the links and the curl of F on the same four links, and its differences.
__device__ __forceinline__ PairForce pair_cos_curl_diffs(const PairLinks& u, const PairReals& f) {
  const double ga = re_plaq(u.ax, u.by, u.apx, u.ay) * (f.ax + f.by - f.apx - f.ay);
  const double gb = re_plaq(u.bx, u.ry, u.bpx, u.by) * (f.bx + f.ry - f.bpx - f.by);
  const double gam = re_plaq(u.amx, u.bmy, u.ax, u.amy) * (f.amx + f.bmy - f.ax - f.amy);
  const double gbm = re_plaq(u.bmx, u.rmy, u.bx, u.bmy) * (f.bmx + f.rmy - f.bx - f.bmy);
  const double gl = re_plaq(u.lx, u.ay, u.lpx, u.ly) * (f.lx + f.ay - f.lpx - f.ly);
  PairForce d;
  d.ax = ga - gam; d.ay = gl - ga;
  d.bx = gb - gbm; d.by = ga - gb;
  return d;
}

}  // namespace qmg

#endif
