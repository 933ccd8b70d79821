// qmg_lane.h -- what a lane of the kernels that work from the gauge links (and of the site kernel) uses to address and accumulate: the ONE copy
// of the block-uniform addressing (gchar, uni, gld, gld_nt) and of the complex multiply-add (fmac2), shared by csrc/qmg_wilson.hip (kernels
// W / W2), csrc/qmg_site.hip (kernel S) and the domain-wall units; and, in namespace dwf, the domain-wall (site, s) lane geometry of
// the lane decode (lane_of: kernels D, D2, stage 2, the wall source, the domain-wall kick), the row decode (row_py: kernels D, K,
// I), the rows and links of a site (row_of: kernels K, I, stage 2) and the hop sum (hop_acc: kernels K, stage 2).  The kernels are held to
// their device code text, so where a helper changed it the kernel keeps its lines and says so; profiles/dwf_lane_refactor.txt has the list.
// Device code only.
#ifndef QMG_LANE_H
#define QMG_LANE_H

#include "qmg_common.h"

namespace qmg {

// a block-uniform (row-uniform) pointer, told to the compiler: the loads then take the scalar-base + 32-bit-offset form
// (the result is a GLOBAL-address-space pointer: an integer cast to a plain pointer would make the accesses flat_load / flat_store)
typedef __attribute__((address_space(1))) char gchar;
__device__ __forceinline__ gchar* uni(const char* p) {
  const unsigned long long v = reinterpret_cast<unsigned long long>(p);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return (gchar*)(((unsigned long long)hi << 32) | lo);
}
template <typename V> __device__ __forceinline__ V gld(const gchar* base, unsigned off) { return *(const __attribute__((address_space(1))) V*)(base + off); }
template <typename V> __device__ __forceinline__ V gld_nt(const gchar* base, unsigned off) {
  return __builtin_nontemporal_load((const __attribute__((address_space(1))) V*)(base + off));
}
// acc += (mx + i my) (bx + i by)
template <typename R>
__device__ __forceinline__ void fmac2(R& ax, R& ay, R mx, R my, R bx, R by) {
  ax = fma(mx, bx, ax); ax = fma(-my, by, ax);
  ay = fma(mx, by, ay); ay = fma(my, bx, ay);
}

namespace dwf {
// ---- the (site, s) lane geometry: one lane per (site, s) of a half row, lanes along s and then along x; rows (parity, y) over grid.y ----
// The lane of a thread: t in the half row, its column j and slice s.  A lane past the end of the half row (!live) has j = 0.  KEEP: the kernels
// with a barrier keep such a lane (it loads what lane (0, s) loads and stores nothing); the others return on !live and, with KEEP = false,
// s is not formed for it (the division stays behind the kernel's exit, where it was).  hr and Ls come by reference, to be loaded here.
struct Lane {
  int t, j, s;
  bool live;
};
template <bool KEEP>
__device__ __forceinline__ Lane lane_of(const int& hr, const int& Ls) {
  Lane l = {};
  l.t = blockIdx.x * blockDim.x + threadIdx.x;
  l.live = l.t < hr * Ls;
  if (!KEEP && !l.live) return l;
  const int jt = l.t / Ls;
  l.s = l.t - jt * Ls;
  l.j = l.live ? jt : 0;
  return l;
}
// Row decode and row geometry read the kernel's argument struct `a` (hr, Ly, half_vol, gauge, par_first, par_count) where they use it and
// not through parameters: the kernels are held to their device code text, and values passed in are loaded in another order.
// row of the launch -> (parity, y): both parities interleaved, or the one processed parity
template <class Args>
__device__ __forceinline__ void row_py(const Args& a, int row, int& p, int& y) {
  p = (a.par_count == 2) ? (row & 1) : a.par_first;
  y = (a.par_count == 2) ? (row >> 1) : row;
}
// What a site of column j on row (p, y) reaches in the even-odd layout: the +x / -x columns jp / jm of the other parity's row y, the four row
// bases in bytes (own; the other parity's rows y, y + 1, y - 1; block-uniform) and, with LINKS, its four links.  Without LINKS the link
// members are not set and cost nothing.  (Three separate functions for the three parts gave the same instructions with commuted scalar
// multiplies in the eight hop instantiations of k_dwf_eo_inv5, so the parts are one function and a template parameter.)  Kernel D and the
// domain-wall kick keep their own lines for this (qmg_dwf.hip, qmg_hmc.hip say why).
template <typename T>
struct Row {
  int p, jp, jm;
  long row_own, row_x, row_yp, row_ym;
  T lx[4], ly[4];
};
template <typename T, bool LINKS, class Args>
__device__ __forceinline__ Row<T> row_of(const Args& a, int p, int y, int j, long row_bytes) {
  typedef T v2 __attribute__((ext_vector_type(2)));
  constexpr unsigned GB = 2u * sizeof(T);
  Row<T> r;
  r.p = p;
  const int sx = (y + p) & 1;
  r.jp = j + sx;     if (r.jp == a.hr) r.jp = 0;
  r.jm = j + sx - 1; if (r.jm < 0) r.jm = a.hr - 1;
  const int yp = (y + 1 == a.Ly) ? 0 : y + 1;
  const int ym = (y == 0) ? a.Ly - 1 : y - 1;
  r.row_own = ((long)p * a.Ly + y) * row_bytes;
  r.row_x = ((long)(1 - p) * a.Ly + y) * row_bytes;
  r.row_yp = ((long)(1 - p) * a.Ly + yp) * row_bytes;
  r.row_ym = ((long)(1 - p) * a.Ly + ym) * row_bytes;
  if (LINKS) {
    // links: own Ux, Uy and the -x / -y neighbours' (opposite parity), conjugated for the backward directions
    const long vol = 2 * a.half_vol;
    const char* gc = reinterpret_cast<const char*>(a.gauge);
    const gchar* g_own_x = uni(gc + ((long)p * a.half_vol + (long)y * a.hr) * GB);
    const gchar* g_own_y = uni(gc + (vol + (long)p * a.half_vol + (long)y * a.hr) * GB);
    const gchar* g_xm = uni(gc + ((long)(1 - p) * a.half_vol + (long)y * a.hr) * GB);
    const gchar* g_ym = uni(gc + (vol + (long)(1 - p) * a.half_vol + (long)ym * a.hr) * GB);
    const unsigned goff_j = (unsigned)j * GB;
    const v2 u0 = gld<v2>(g_own_x, goff_j), u1 = gld<v2>(g_own_y, goff_j), u2 = gld<v2>(g_xm, (unsigned)r.jm * GB), u3 = gld<v2>(g_ym, goff_j);
    r.lx[0] = u0.x; r.lx[1] = u1.x; r.lx[2] = u2.x; r.lx[3] = u3.x;
    r.ly[0] = u0.y; r.ly[1] = u1.y; r.ly[2] = -u2.y; r.ly[3] = -u3.y;
  }
  return r;
}
// the four hops of one (site, s) pair from its chunks xr = {+x, +y, -x, -y} and links (backward ones already conjugated), added to the two
// spin rows a0 (sigma 0) and a1 (sigma 1): the 2 x 2 spin blocks of the Wilson operator; hw = -w/2.  The even-odd kernels call this;
// dwf_site (qmg_dwf.hip) keeps its own copy of the loop: calling this one there gives the same instructions in another order and register
// assignment, and kernels D / D2 are held to their device code text (profiles/dwf_eo_device_code.txt).
template <typename T>
__device__ __forceinline__ void hop_acc(const T __attribute__((ext_vector_type(4))) (&xr)[4], const T (&lx)[4], const T (&ly)[4], T hw, T& a0x, T& a0y, T& a1x, T& a1y) {
  typedef T R;
  typedef T v4 __attribute__((ext_vector_type(4)));
  const R h = (R)0.5;
#pragma unroll
  for (int d = 0; d < 4; d++) {
    const R ux = lx[d], uy = ly[d];
    const R dx = hw * ux, dy = hw * uy;   // diagonal: -w/2 U
    R m01x, m01y, m10x, m10y;             // [0][1] and [1][0]
    if (d == 0) { m01x = h * ux; m01y = h * uy; m10x = m01x; m10y = m01y; }                           // +x: U/2 both
    else if (d == 2) { m01x = -h * ux; m01y = -h * uy; m10x = m01x; m10y = m01y; }                    // -x: -U/2 both
    else if (d == 1) { m01x = h * uy; m01y = -h * ux; m10x = -h * uy; m10y = h * ux; }                // +y: -i U/2, i U/2
    else { m01x = -h * uy; m01y = h * ux; m10x = h * uy; m10y = -h * ux; }                            // -y: i U/2, -i U/2
    const v4 v = xr[d];
    fmac2<R>(a0x, a0y, dx, dy, v.x, v.y);
    fmac2<R>(a0x, a0y, m01x, m01y, v.z, v.w);
    fmac2<R>(a1x, a1y, m10x, m10y, v.x, v.y);
    fmac2<R>(a1x, a1y, dx, dy, v.z, v.w);
  }
}
}  // namespace dwf
}  // namespace qmg

#endif
