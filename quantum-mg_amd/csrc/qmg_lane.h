// qmg_lane.h -- what a lane of the kernels that work from the gauge links (and of the site kernel) uses to address and accumulate: the ONE copy
// of the block-uniform addressing (gchar, uni, gld, gld_nt) and of the complex multiply-add (fmac2), shared by csrc/qmg_wilson.hip (kernels
// W / W2), csrc/qmg_site.hip (kernel S), csrc/qmg_dwf.hip (kernels D / D2) and csrc/qmg_dwf_eo.hip (the even-odd kernels), and the hop sum of a
// domain-wall site (dwf::hop_acc).  Device code only.
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
