// qmg_mobius_eo.hip -- the 4D even-odd Schur complement of the Moebius domain-wall operator and its dagger, STRAIGHT FROM THE GAUGE LINKS.
//
// D = A + H B (qmg_mobius.hip): A = alpha + kappa L and B = b5 + c5 L are site-local, the same at every site of a parity (alpha_p = alpha +
// shift +- eo_shift) and commute with each other, H changes parity and does not commute with them.  With p the parity of the system:
//   M_p        = A_p - H_{p,1-p} B A_{1-p}^-1 H_{1-p,p} B
//   M_p^dagger = Gamma5 [A'_p - B' H_{p,1-p} A'_{1-p}^-1 B' H_{1-p,p}] Gamma5            ': conj(m), conj(shifts)
// Gamma5 M Gamma5 is NOT M^dagger (B stands on the other side of H), so the dagger has kernels of its own.  On the sigma 0 block L^Ls = -m:
// every function of L is a twisted circulant f(L) = sum_{k < Ls} f_k L^k, (L^k h)(s) = h(s-k) for s >= k and -m h(s-k+Ls) below; sigma 1 is
// the mirror under s -> Ls-1-s.  The tables of 1, A^-1 and A^-1 B are formed on the host in long double (qmg_mobius_eo_plan.h:
// mobius_eo_coef), rounded once to the kernel's scalar and come in by value, with -m f_k next to f_k.  The kernels:
//   k_mobius_eo_mix           lhs_p (+)= scale S h,  h = H_{p,1-p} (R [Gamma5] rhs_{1-p}) or rhs_p.  R = B is formed ON THE LOAD as k_mobius_load
//                             does it (the two fifth-dimension halves of each neighbour next to its chunk); S goes through LDS as kernel K's
//                             scan does (qmg_dwf_eo.hip): the chunk h into LDS, one barrier, then 2 Ls complex FMAs per lane with the
//                             UNIFORM coefficients f_k (inside) or -m f_k (wrapped).  Stage 1 of M and of M^dagger, prepare, reconstruct.
//   k_mobius_eo_schur2        lhs_p = A_p x_p + H_{p,1-p} (B t_{1-p}):  k_mobius_load with x and t behind separate pointers; no LDS, 256 lanes.
//   k_mobius_eo_schur2_dagger lhs_p = Gamma5 [A'_p Gamma5 x_p + B' (H_{p,1-p} t_{1-p})]:  k_mobius_result with x and t behind separate pointers:
//                             the hop sum of a slice exchanged along s in LDS, Gamma5 on the load of x and on the store.
// Lane mapping: qmg_lane.h's -- one lane per (site, s) with the two spin components as one chunk, rows (parity, y) over grid.y, block-uniform
// bases, links loaded once per row and kept across the systems of a batch.  The kernels with an exchange run blocks of Ls floor(256 / Ls)
// lanes, so that a site never straddles a block; a lane past the end of a half row stays for the barrier as lane (0, s) and stores nothing.
// Two LDS buffers alternate, so one barrier per (row, system) suffices: 16 KiB per block in fp64, 8 KiB in fp32.
#include "qmg_lane.h"   // uni, gld, fmac2, dwf::lane_of, row_py, row_of, hop_acc
#include "qmg_mobius_eo_plan.h"

namespace qmg {

// T: the kernel's scalar.  Every coefficient arrives in it, rounded once on the host from the values of mobius_eo_coef.
template <typename T>
struct MobiusEoArgs {
  const void* gauge;       // [mu][site] complex<T>
  void* lhs;
  const void* rhs;         // k_mobius_eo_mix: the source; the second stages: x
  const void* aux;         // the second stages: t
  int hr, Ly, Ls;
  long half_vol;
  unsigned pieces;
  int nrhs;                // active systems
  long vec_stride;
  int par_first, par_count, nrows;
  int g5_in;
  T hw, sx, sy;            // -w/2, scale
  T b5, c5, kappa;
  T wk[2], wc[2];          // across the wall: -m kappa and -m c5 (conj(m) for the dagger)
  T al[2][2];              // alpha_p (conjugated for the dagger)
  T tab[2][DWF_LS_MAX][2];    // S on parity p: f_k
  T tabw[2][DWF_LS_MAX][2];   // -m f_k
  int ridx[16];
};

// ---- lhs_p (+)= scale S h,  h = H_{p,1-p} (R [Gamma5] rhs_{1-p}) (HOP) or rhs_p (!HOP) ----
template <typename T, bool HOP, bool RMIX, bool ZERO, bool BATCH>
__global__ __launch_bounds__(DWF_BLOCK_MAX) void k_mobius_eo_mix(const MobiusEoArgs<T> a) {
  using namespace dwf;
  typedef T R;
  typedef T v4 __attribute__((ext_vector_type(4)));   // a lane's chunk: (sigma 0 re, im, sigma 1 re, im)
  typedef T v2 __attribute__((ext_vector_type(2)));   // half a chunk
  constexpr unsigned CH = 4u * sizeof(T);
  __shared__ v4 xch[2][DWF_BLOCK_MAX];
  const int tid = threadIdx.x;
  const Lane ln = lane_of<true>(a.hr, a.Ls);      // a site is live or not as a whole: the block and the half row are multiples of Ls lanes
  const bool live = ln.live;
  const int j = ln.j, s = ln.s;
  const int base = tid - s;                       // the site's chunks in LDS: base .. base + Ls - 1, all in this block
  const int rev = a.Ls - 1;
  const int s_lo = s > 0 ? s - 1 : rev, s_hi = s + 1 < a.Ls ? s + 1 : 0;
  const bool g5 = HOP && a.g5_in;
  const R g5s = g5 ? (R)-1 : (R)1;                // Gamma5 on the load: the slices the source comes from and the sign of its sigma 1
  const unsigned in_src = (unsigned)(g5 ? rev - s : s) * CH, in_lo = (unsigned)(g5 ? rev - s_lo : s_lo) * CH, in_hi = (unsigned)(g5 ? rev - s_hi : s_hi) * CH + CH / 2;
  const unsigned in_own = (unsigned)s * CH;
  // R = B: c5 inside, -m c5 across the wall
  const R clx = s > 0 ? a.c5 : a.wc[0], cly = s > 0 ? (R)0 : a.wc[1];
  const R chx = s + 1 < a.Ls ? a.c5 : a.wc[0], chy = s + 1 < a.Ls ? (R)0 : a.wc[1];
  const R b5 = a.b5, hw = a.hw, scx = a.sx, scy = a.sy;
  const long sys_bytes = a.vec_stride * (long)(2 * sizeof(T));
  const long row_bytes = (long)a.hr * a.Ls * CH;
  int buf = 0;
  for (int row = blockIdx.y; row < a.nrows; row += gridDim.y) {
    int p, y;
    row_py(a, row, p, y);
    const bool do_zero = ZERO || ((a.pieces >> (12 + p)) & 1u);
    const Row<T> r = row_of<T, HOP>(a, p, y, j, row_bytes);
    const unsigned site = (unsigned)(j * a.Ls) * CH, site_p = (unsigned)(r.jp * a.Ls) * CH, site_m = (unsigned)(r.jm * a.Ls) * CH;
    const int nsys = BATCH ? a.nrhs : 1;
    for (int k = 0; k < nsys; k++) {
      const long off = (long)a.ridx[k] * sys_bytes;
      const char* x = reinterpret_cast<const char*>(a.rhs) + off;
      char* out = reinterpret_cast<char*>(a.lhs) + off;
      __attribute__((address_space(1))) v4* dst = (__attribute__((address_space(1))) v4*)(uni(out + r.row_own) + site + in_own);
      v4 h;
      if (HOP) {
        const gchar* bx = uni(x + r.row_x);
        const gchar* byp = uni(x + r.row_yp);
        const gchar* bym = uni(x + r.row_ym);
        v4 xr[4];
        v2 xl[4], xh[4];
        xr[0] = gld<v4>(bx, site_p + in_src);
        xr[1] = gld<v4>(byp, site + in_src);
        xr[2] = gld<v4>(bx, site_m + in_src);
        xr[3] = gld<v4>(bym, site + in_src);
        if (RMIX) {
          xl[0] = gld<v2>(bx, site_p + in_lo); xh[0] = gld<v2>(bx, site_p + in_hi);
          xl[1] = gld<v2>(byp, site + in_lo);  xh[1] = gld<v2>(byp, site + in_hi);
          xl[2] = gld<v2>(bx, site_m + in_lo); xh[2] = gld<v2>(bx, site_m + in_hi);
          xl[3] = gld<v2>(bym, site + in_lo);  xh[3] = gld<v2>(bym, site + in_hi);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int d = 0; d < 4; d++) {
          if (RMIX) {   // chi = b5 phi + c5 L phi of the neighbour, phi = [Gamma5] rhs
            R c0x = b5 * xr[d].x, c0y = b5 * xr[d].y, c1x = b5 * xr[d].z, c1y = b5 * xr[d].w;
            fmac2<R>(c0x, c0y, clx, cly, xl[d].x, xl[d].y);
            fmac2<R>(c1x, c1y, chx, chy, xh[d].x, xh[d].y);
            xr[d] = (v4){c0x, c0y, g5s * c1x, g5s * c1y};
          } else {
            xr[d].z *= g5s; xr[d].w *= g5s;
          }
        }
        R a0x = (R)0, a0y = (R)0, a1x = (R)0, a1y = (R)0;
        hop_acc<T>(xr, r.lx, r.ly, hw, a0x, a0y, a1x, a1y);
        h = (v4){a0x, a0y, a1x, a1y};
      } else {
        h = gld<v4>(uni(x + r.row_own), site + in_own);
      }
      xch[buf][tid] = h;
      __syncthreads();
      // S h: distance k2 with the uniform coefficient f_k2, or -m f_k2 where the distance wraps around the wall
      const v2* half = reinterpret_cast<const v2*>(&xch[buf][base]);   // half[2 s'] = h(s', 0), half[2 s' + 1] = h(s', 1)
      R g0x = (R)0, g0y = (R)0, g1x = (R)0, g1y = (R)0;
#pragma unroll 1   // unrolled, the coefficients of several distances are held at once and the fp64 hop instantiations run out of scalar registers
      for (int k2 = 0; k2 < a.Ls; k2++) {
        const R fx = a.tab[p][k2][0], fy = a.tab[p][k2][1], wx = a.tabw[p][k2][0], wy = a.tabw[p][k2][1];
        const bool lo_in = k2 <= s, hi_in = s + k2 < a.Ls;
        const v2 vl = half[2 * (lo_in ? s - k2 : s - k2 + a.Ls)], vh = half[2 * (hi_in ? s + k2 : s + k2 - a.Ls) + 1];
        fmac2<R>(g0x, g0y, lo_in ? fx : wx, lo_in ? fy : wy, vl.x, vl.y);
        fmac2<R>(g1x, g1y, hi_in ? fx : wx, hi_in ? fy : wy, vh.x, vh.y);
      }
      v4 prev = {(R)0, (R)0, (R)0, (R)0};
      if (!do_zero && live) prev = *dst;
      R o0x = prev.x, o0y = prev.y, o1x = prev.z, o1y = prev.w;
      fmac2<R>(o0x, o0y, scx, scy, g0x, g0y);
      fmac2<R>(o1x, o1y, scx, scy, g1x, g1y);
      const v4 o = {o0x, o0y, o1x, o1y};
      if (live) __builtin_nontemporal_store(o, dst);
      buf ^= 1;
    }
  }
}

// ---- the second stage of M: lhs_p = A_p x_p + H_{p,1-p} (B t_{1-p}), overwriting; one parity ----
template <typename T, bool BATCH>
__global__ __launch_bounds__(BLOCK) void k_mobius_eo_schur2(const MobiusEoArgs<T> a) {
  using namespace dwf;
  typedef T R;
  typedef T v4 __attribute__((ext_vector_type(4)));
  typedef T v2 __attribute__((ext_vector_type(2)));
  constexpr unsigned CH = 4u * sizeof(T);
  const Lane ln = lane_of<false>(a.hr, a.Ls);
  if (!ln.live) return;
  const int j = ln.j, s = ln.s;
  const int s_lo = s > 0 ? s - 1 : a.Ls - 1, s_hi = s + 1 < a.Ls ? s + 1 : 0;
  const bool lo_in = s > 0, hi_in = s + 1 < a.Ls;
  const R klx = lo_in ? a.kappa : a.wk[0], kly = lo_in ? (R)0 : a.wk[1], khx = hi_in ? a.kappa : a.wk[0], khy = hi_in ? (R)0 : a.wk[1];
  const R clx = lo_in ? a.c5 : a.wc[0], cly = lo_in ? (R)0 : a.wc[1], chx = hi_in ? a.c5 : a.wc[0], chy = hi_in ? (R)0 : a.wc[1];
  const R b5 = a.b5, hw = a.hw;
  const unsigned in_own = (unsigned)s * CH, in_lo = (unsigned)s_lo * CH, in_hi = (unsigned)s_hi * CH + CH / 2;   // inside a site
  const long sys_bytes = a.vec_stride * (long)(2 * sizeof(T));
  const long row_bytes = (long)a.hr * a.Ls * CH;
  const int p = a.par_first;
  const R alx = a.al[p][0], aly = a.al[p][1];
  for (int y = blockIdx.y; y < a.Ly; y += gridDim.y) {
    const Row<T> r = row_of<T, true>(a, p, y, j, row_bytes);
    const unsigned site = (unsigned)(j * a.Ls) * CH, site_p = (unsigned)(r.jp * a.Ls) * CH, site_m = (unsigned)(r.jm * a.Ls) * CH;
    const int nsys = BATCH ? a.nrhs : 1;
    for (int k = 0; k < nsys; k++) {
      const long off = (long)a.ridx[k] * sys_bytes;
      const char* x = reinterpret_cast<const char*>(a.rhs) + off;
      const char* tv = reinterpret_cast<const char*>(a.aux) + off;
      char* out = reinterpret_cast<char*>(a.lhs) + off;
      const gchar* bx = uni(tv + r.row_x);
      const gchar* byp = uni(tv + r.row_yp);
      const gchar* bym = uni(tv + r.row_ym);
      const gchar* bo = uni(x + r.row_own);
      v4 xr[4];
      v2 xl[4], xh[4];
      xr[0] = gld<v4>(bx, site_p + in_own); xl[0] = gld<v2>(bx, site_p + in_lo); xh[0] = gld<v2>(bx, site_p + in_hi);
      xr[1] = gld<v4>(byp, site + in_own);  xl[1] = gld<v2>(byp, site + in_lo);  xh[1] = gld<v2>(byp, site + in_hi);
      xr[2] = gld<v4>(bx, site_m + in_own); xl[2] = gld<v2>(bx, site_m + in_lo); xh[2] = gld<v2>(bx, site_m + in_hi);
      xr[3] = gld<v4>(bym, site + in_own);  xl[3] = gld<v2>(bym, site + in_lo);  xh[3] = gld<v2>(bym, site + in_hi);
      const v4 own = gld<v4>(bo, site + in_own);
      const v2 lo = gld<v2>(bo, site + in_lo), hi = gld<v2>(bo, site + in_hi);
      __builtin_amdgcn_sched_barrier(0);
      // chi = b5 t + c5 L t of the four neighbours, in registers
#pragma unroll
      for (int d = 0; d < 4; d++) {
        R c0x = b5 * xr[d].x, c0y = b5 * xr[d].y, c1x = b5 * xr[d].z, c1y = b5 * xr[d].w;
        fmac2<R>(c0x, c0y, clx, cly, xl[d].x, xl[d].y);
        fmac2<R>(c1x, c1y, chx, chy, xh[d].x, xh[d].y);
        xr[d] = (v4){c0x, c0y, c1x, c1y};
      }
      R a0x = (R)0, a0y = (R)0, a1x = (R)0, a1y = (R)0;
      fmac2<R>(a0x, a0y, alx, aly, own.x, own.y);
      fmac2<R>(a1x, a1y, alx, aly, own.z, own.w);
      fmac2<R>(a0x, a0y, klx, kly, lo.x, lo.y);
      fmac2<R>(a1x, a1y, khx, khy, hi.x, hi.y);
      hop_acc<T>(xr, r.lx, r.ly, hw, a0x, a0y, a1x, a1y);
      const v4 o = {a0x, a0y, a1x, a1y};
      __builtin_nontemporal_store(o, (__attribute__((address_space(1))) v4*)(uni(out + r.row_own) + site + in_own));
    }
  }
}

// ---- the second stage of M^dagger: lhs_p = Gamma5 [A'_p Gamma5 x_p + B' (H_{p,1-p} t_{1-p})], overwriting; one parity ----
// The lane of slice s works on phi = Gamma5 x: it reads slice Ls-1-s of x (sigma 1 negated) for A', slice s of t's neighbours for the hop sum
// g(s), puts g(s) into LDS, takes g(s-1, 0) and g(s+1, 1) of its site from there, and stores (sigma 1 negated) to slice Ls-1-s.
template <typename T, bool BATCH>
__global__ __launch_bounds__(DWF_BLOCK_MAX) void k_mobius_eo_schur2_dagger(const MobiusEoArgs<T> a) {
  using namespace dwf;
  typedef T R;
  typedef T v4 __attribute__((ext_vector_type(4)));
  typedef T v2 __attribute__((ext_vector_type(2)));
  constexpr unsigned CH = 4u * sizeof(T);
  __shared__ v4 xch[2][DWF_BLOCK_MAX];
  const int tid = threadIdx.x;
  const Lane ln = lane_of<true>(a.hr, a.Ls);
  const bool live = ln.live;
  const int j = ln.j, s = ln.s;
  const int base = tid - s;
  const int rev = a.Ls - 1;
  const int s_lo = s > 0 ? s - 1 : rev, s_hi = s + 1 < a.Ls ? s + 1 : 0;
  const bool lo_in = s > 0, hi_in = s + 1 < a.Ls;
  const R klx = lo_in ? a.kappa : a.wk[0], kly = lo_in ? (R)0 : a.wk[1], khx = hi_in ? a.kappa : a.wk[0], khy = hi_in ? (R)0 : a.wk[1];
  const R clx = lo_in ? a.c5 : a.wc[0], cly = lo_in ? (R)0 : a.wc[1], chx = hi_in ? a.c5 : a.wc[0], chy = hi_in ? (R)0 : a.wc[1];
  const R b5 = a.b5, hw = a.hw;
  const unsigned in_t = (unsigned)s * CH;                                                                                                  // t: never reflected
  const unsigned in_own = (unsigned)(rev - s) * CH, in_lo = (unsigned)(rev - s_lo) * CH, in_hi = (unsigned)(rev - s_hi) * CH + CH / 2;   // x: Gamma5 on the load
  const long sys_bytes = a.vec_stride * (long)(2 * sizeof(T));
  const long row_bytes = (long)a.hr * a.Ls * CH;
  const int p = a.par_first;
  const R alx = a.al[p][0], aly = a.al[p][1];
  int buf = 0;
  for (int y = blockIdx.y; y < a.Ly; y += gridDim.y) {
    const Row<T> r = row_of<T, true>(a, p, y, j, row_bytes);
    const unsigned site = (unsigned)(j * a.Ls) * CH, site_p = (unsigned)(r.jp * a.Ls) * CH, site_m = (unsigned)(r.jm * a.Ls) * CH;
    const int nsys = BATCH ? a.nrhs : 1;
    for (int k = 0; k < nsys; k++) {
      const long off = (long)a.ridx[k] * sys_bytes;
      const char* x = reinterpret_cast<const char*>(a.rhs) + off;
      const char* tv = reinterpret_cast<const char*>(a.aux) + off;
      char* out = reinterpret_cast<char*>(a.lhs) + off;
      __attribute__((address_space(1))) v4* dst = (__attribute__((address_space(1))) v4*)(uni(out + r.row_own) + site + in_own);   // Gamma5 on the store
      const gchar* bx = uni(tv + r.row_x);
      const gchar* bo = uni(x + r.row_own);
      v4 xr[4];
      xr[0] = gld<v4>(bx, site_p + in_t);
      xr[1] = gld<v4>(uni(tv + r.row_yp), site + in_t);
      xr[2] = gld<v4>(bx, site_m + in_t);
      xr[3] = gld<v4>(uni(tv + r.row_ym), site + in_t);
      const v4 own = gld<v4>(bo, site + in_own);                                     // x(Ls-1-s): phi(s) up to the sign of sigma 1
      const v2 lo = gld<v2>(bo, site + in_lo), hi = gld<v2>(bo, site + in_hi);       // phi(s_lo, 0) and -phi(s_hi, 1)
      __builtin_amdgcn_sched_barrier(0);
      R g0x = (R)0, g0y = (R)0, g1x = (R)0, g1y = (R)0;
      hop_acc<T>(xr, r.lx, r.ly, hw, g0x, g0y, g1x, g1y);
      xch[buf][tid] = (v4){g0x, g0y, g1x, g1y};
      __syncthreads();
      const v4 gl = xch[buf][base + s_lo], gh = xch[buf][base + s_hi];
      // A' phi + B' g on slice s
      R a0x = (R)0, a0y = (R)0, a1x = (R)0, a1y = (R)0;
      fmac2<R>(a0x, a0y, alx, aly, own.x, own.y);
      fmac2<R>(a1x, a1y, alx, aly, -own.z, -own.w);
      fmac2<R>(a0x, a0y, klx, kly, lo.x, lo.y);
      fmac2<R>(a1x, a1y, khx, khy, -hi.x, -hi.y);
      fmac2<R>(a0x, a0y, b5, (R)0, g0x, g0y);
      fmac2<R>(a1x, a1y, b5, (R)0, g1x, g1y);
      fmac2<R>(a0x, a0y, clx, cly, gl.x, gl.y);
      fmac2<R>(a1x, a1y, chx, chy, gh.z, gh.w);
      const v4 o = {a0x, a0y, -a1x, -a1y};                                           // Gamma5 on the store
      if (live) __builtin_nontemporal_store(o, dst);
      buf ^= 1;
    }
  }
}

template <typename T>
static void launch_mobius_eo(const MobiusEoArgs<T>& a, const MobiusEoPlan& pl, hipStream_t st) {
  const dim3 grid((unsigned)pl.gx, (unsigned)pl.gy);
  const unsigned bl = (unsigned)pl.block;
  const bool zero = pl.flags & DPF_ZERO, batch = pl.flags & DPF_BATCH, rmix = pl.flags & MEPF_RMIX;
  if (pl.family == MEF_SCHUR2) {
    if (batch) k_mobius_eo_schur2<T, true><<<grid, bl, 0, st>>>(a); else k_mobius_eo_schur2<T, false><<<grid, bl, 0, st>>>(a);
  } else if (pl.family == MEF_SCHUR2_DAGGER) {
    if (batch) k_mobius_eo_schur2_dagger<T, true><<<grid, bl, 0, st>>>(a); else k_mobius_eo_schur2_dagger<T, false><<<grid, bl, 0, st>>>(a);
  } else if (pl.family == MEF_MIX) {
    if (batch) k_mobius_eo_mix<T, false, false, true, true><<<grid, bl, 0, st>>>(a); else k_mobius_eo_mix<T, false, false, true, false><<<grid, bl, 0, st>>>(a);
  } else if (rmix) {
    if (zero) { if (batch) k_mobius_eo_mix<T, true, true, true, true><<<grid, bl, 0, st>>>(a); else k_mobius_eo_mix<T, true, true, true, false><<<grid, bl, 0, st>>>(a); }
    else { if (batch) k_mobius_eo_mix<T, true, true, false, true><<<grid, bl, 0, st>>>(a); else k_mobius_eo_mix<T, true, true, false, false><<<grid, bl, 0, st>>>(a); }
  } else {
    if (zero) { if (batch) k_mobius_eo_mix<T, true, false, true, true><<<grid, bl, 0, st>>>(a); else k_mobius_eo_mix<T, true, false, true, false><<<grid, bl, 0, st>>>(a); }
    else { if (batch) k_mobius_eo_mix<T, true, false, false, true><<<grid, bl, 0, st>>>(a); else k_mobius_eo_mix<T, true, false, false, false><<<grid, bl, 0, st>>>(a); }
  }
}

// one launch of a planned request
template <typename T>
static void meo_launch(const qmg_stencil_desc* d, const MobiusEoPlan& pl, const MobiusEoCoef& co, const void* gauge, int Ls, double w, void* lhs, const void* rhs,
                       const void* aux, unsigned pieces, double sr, double si, unsigned flags, const BatchIdx& b, size_t vec_stride, hipStream_t st) {
  MobiusEoArgs<T> a;
  dwf_fill_rows(a, gauge, lhs, rhs, d->Lx, d->Ly, Ls, pieces, b, vec_stride, pl.par_first, pl.par_count);
  a.aux = aux;
  a.g5_in = (flags & QMG_DWF_G5_IN) ? 1 : 0;
  a.hw = (T)(-0.5 * w); a.sx = (T)sr; a.sy = (T)si;
  a.b5 = (T)co.b5; a.c5 = (T)co.c5; a.kappa = (T)co.kappa;
  for (int c = 0; c < 2; c++) { a.wk[c] = (T)co.wk[c]; a.wc[c] = (T)co.wc[c]; }
  for (int p = 0; p < 2; p++)
    for (int c = 0; c < 2; c++) {
      a.al[p][c] = (T)co.al[p][c];
      for (int k = 0; k < DWF_LS_MAX; k++) { a.tab[p][k][c] = (T)co.tab[p][k][c]; a.tabw[p][k][c] = (T)co.tabw[p][k][c]; }
    }
  launch_mobius_eo<T>(a, pl, st);
}
static int meo_run(int dtype, const qmg_stencil_desc* d, const MobiusEoPlan& pl, const MobiusEoCoef& co, const void* gauge, int Ls, double w, void* lhs,
                   const void* rhs, const void* aux, unsigned pieces, double sr, double si, unsigned flags, const BatchIdx& b, size_t vec_stride, hipStream_t st) {
  if (dtype == QMG_C64) meo_launch<double>(d, pl, co, gauge, Ls, w, lhs, rhs, aux, pieces, sr, si, flags, b, vec_stride, st);
  else meo_launch<float>(d, pl, co, gauge, Ls, w, lhs, rhs, aux, pieces, sr, si, flags, b, vec_stride, st);
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

}  // namespace qmg

using namespace qmg;

extern "C" {

int qmg_mobius_eo_plan(int dtype, int Lx, int Ly, int Ls, int kernel, unsigned pieces, int table, int source, int n_active, int inplace, int* plan_out,
                       int plan_len) {
  const MobiusEoPlan pl = mobius_eo_plan(dtype, Lx, Ly, Ls, kernel, pieces, table, source, n_active, inplace);
  return export_dw_plan(pl, pl.lds, plan_out, plan_len);
}

int qmg_mobius_inv5(int dtype, const qmg_stencil_desc* d, int Ls, double mass_re, double mass_im, double wilson_coeff, double M5, double b5, double c5, void* lhs,
                    const void* rhs, unsigned pieces, int table, double scale_re, double scale_im, int nrhs, size_t vec_stride, unsigned mask, void* stream) {
  if (!lhs || !rhs || !aligned16(lhs) || !aligned16(rhs) || !std::isfinite(scale_re) || !std::isfinite(scale_im)) return QMG_ERR_INVALID;
  if (int rc = dw_eo_valid(dtype, d, Ls, nrhs, vec_stride)) return rc;
  const BatchIdx b = expand_mask(mask, nrhs);
  const MobiusEoPlan pl = mobius_eo_plan(dtype, d->Lx, d->Ly, Ls, MEK_INV5, pieces, table, MES_ONE, b.n, lhs == rhs);
  if (dw_eo_refused(pl)) return pl.status;
  MobiusEoCoef co;
  if (int rc = mobius_eo_coef(d, Ls, mass_re, mass_im, wilson_coeff, M5, b5, c5, false, table, dw_eo_need(pl), &co)) return rc;
  if (pl.family == MEF_NOTHING) return QMG_SUCCESS;
  return meo_run(dtype, d, pl, co, 0, Ls, wilson_coeff, lhs, rhs, 0, pieces, scale_re, scale_im, 0, b, vec_stride, as_stream(stream));
}

int qmg_mobius_hops_inv5(int dtype, const qmg_stencil_desc* d, const void* gauge, int Ls, double mass_re, double mass_im, double wilson_coeff, double M5, double b5,
                         double c5, void* lhs, const void* rhs, unsigned pieces, int table, int source, double scale_re, double scale_im, unsigned flags, int nrhs,
                         size_t vec_stride, unsigned mask, void* stream) {
  if (!gauge || !lhs || !rhs || !aligned16(gauge) || !aligned16(lhs) || !aligned16(rhs)) return QMG_ERR_INVALID;
  if (!std::isfinite(scale_re) || !std::isfinite(scale_im) || (flags & ~(unsigned)QMG_DWF_G5_IN)) return QMG_ERR_INVALID;
  if (int rc = dw_eo_valid(dtype, d, Ls, nrhs, vec_stride)) return rc;
  const BatchIdx b = expand_mask(mask, nrhs);
  const MobiusEoPlan pl = mobius_eo_plan(dtype, d->Lx, d->Ly, Ls, MEK_HOPS_INV5, pieces, table, source, b.n, lhs == rhs);
  if (dw_eo_refused(pl)) return pl.status;
  MobiusEoCoef co;
  if (int rc = mobius_eo_coef(d, Ls, mass_re, mass_im, wilson_coeff, M5, b5, c5, false, table, dw_eo_need(pl), &co)) return rc;
  if (pl.family == MEF_NOTHING) return QMG_SUCCESS;
  return meo_run(dtype, d, pl, co, gauge, Ls, wilson_coeff, lhs, rhs, 0, pieces, scale_re, scale_im, flags, b, vec_stride, as_stream(stream));
}

int qmg_mobius_schur_apply(int dtype, const qmg_stencil_desc* d, const void* gauge, int Ls, double mass_re, double mass_im, double wilson_coeff, double M5,
                           double b5, double c5, void* lhs, const void* rhs, void* tmp, int parity, int op, int nrhs, size_t vec_stride, unsigned mask,
                           void* stream) {
  if (!gauge || !lhs || !rhs || !tmp || !aligned16(gauge) || !aligned16(lhs) || !aligned16(rhs) || !aligned16(tmp)) return QMG_ERR_INVALID;
  if ((parity != 0 && parity != 1) || (op != MOP_D && op != MOP_DAGGER) || lhs == rhs || tmp == rhs || tmp == lhs) return QMG_ERR_INVALID;
  if (int rc = dw_eo_valid(dtype, d, Ls, nrhs, vec_stride)) return rc;
  const BatchIdx b = expand_mask(mask, nrhs);
  const bool dag = op == MOP_DAGGER;
  // M:        stage 1  tmp_o = -A_o^-1 H_{o,p} (B rhs_p);               stage 2  lhs_p = A_p rhs_p + H_{p,o} (B tmp_o)
  // M^dagger: stage 1  tmp_o = -(A'_o^-1 B') H_{o,p} (Gamma5 rhs_p);    stage 2  lhs_p = Gamma5 [A'_p Gamma5 rhs_p + B' (H_{p,o} tmp_o)]
  const DwEoStages s = dw_eo_stages(parity);
  const int table = dag ? MET_AINV_B : MET_AINV;
  const MobiusEoPlan pl1 = mobius_eo_plan(dtype, d->Lx, d->Ly, Ls, MEK_HOPS_INV5, s.pieces1, table, dag ? MES_ONE : MES_B, b.n, 0);
  const MobiusEoPlan pl2 = mobius_eo_plan(dtype, d->Lx, d->Ly, Ls, dag ? MEK_SCHUR2_DAGGER : MEK_SCHUR2, s.pieces2, MET_ONE, MES_ONE, b.n, 0);
  if (dw_eo_refused(pl1)) return pl1.status;
  if (dw_eo_refused(pl2)) return pl2.status;
  MobiusEoCoef co;
  if (int rc = mobius_eo_coef(d, Ls, mass_re, mass_im, wilson_coeff, M5, b5, c5, dag, table, 1u << (1 - parity), &co)) return rc;
  if (pl1.family == MEF_NOTHING || pl2.family == MEF_NOTHING) return QMG_SUCCESS;
  hipStream_t st = as_stream(stream);
  if (int rc = meo_run(dtype, d, pl1, co, gauge, Ls, wilson_coeff, tmp, rhs, 0, s.pieces1, -1.0, 0.0, dag ? QMG_DWF_G5_IN : 0u, b, vec_stride, st)) return rc;
  return meo_run(dtype, d, pl2, co, gauge, Ls, wilson_coeff, lhs, rhs, tmp, s.pieces2, 1.0, 0.0, 0u, b, vec_stride, st);
}

}  // extern "C"
