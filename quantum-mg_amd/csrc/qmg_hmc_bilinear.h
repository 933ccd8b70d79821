// qmg_hmc_bilinear.h -- the Wilson fermion-force bilinear and the pole lists of the kicks, shared by qmg_hmc.hip (the fused kicks on the thin
// links) and qmg_stout.hip (the force as a link field of its own, for the chain rule through stout levels).
//
//   Ff_mu(x) = 2 Im[ U_mu(x) Y(x)^dag Hp_mu X(x+mu)  -  conj(U_mu(x)) Y(x+mu)^dag Hm_mu X(x) ],   Hp_mu = (-1 + sigma_mu)/2, Hm_mu = (-1 - sigma_mu)/2
#ifndef QMG_HMC_BILINEAR_H
#define QMG_HMC_BILINEAR_H

#include "qmg_common.h"

namespace qmg {

// Y^dag Hp_x X etc. without the factor 1/2 of the projectors (it cancels the 2 of 2 Im[...]).
//   Hp_x v = (-v0 + v1, v0 - v1)/2      Hm_x v = -(v0 + v1, v0 + v1)/2
//   Hp_y v = (-v0 - i v1, i v0 - v1)/2  Hm_y v = (-v0 + i v1, -i v0 - v1)/2
__device__ __forceinline__ cplx ydag_hx(cplx y0, cplx y1, cplx x0, cplx x1, double sgn) {   // sgn = +1: 2 Hp_x, -1: 2 Hm_x
  const cplx d = cmake(fma(sgn, x1.x, -x0.x), fma(sgn, x1.y, -x0.y));    // -x0 + sgn x1
  const cplx e = cmake(fma(sgn, x0.x, -x1.x), fma(sgn, x0.y, -x1.y));    // sgn x0 - x1
  cplx acc = cmake(0.0, 0.0);
  cmac_conj(acc, y0, d);
  cmac_conj(acc, y1, e);
  return acc;
}
__device__ __forceinline__ cplx ydag_hy(cplx y0, cplx y1, cplx x0, cplx x1, double sgn) {   // sgn = +1: 2 Hp_y, -1: 2 Hm_y
  const cplx d = cmake(fma(sgn, x1.y, -x0.x), fma(-sgn, x1.x, -x0.y));   // -x0 - sgn i x1
  const cplx e = cmake(fma(-sgn, x0.y, -x1.x), fma(sgn, x0.x, -x1.y));   // sgn i x0 - x1
  cplx acc = cmake(0.0, 0.0);
  cmac_conj(acc, y0, d);
  cmac_conj(acc, y1, e);
  return acc;
}
// Im[ U p - conj(U) m ]
__device__ __forceinline__ double link_force(cplx u, cplx p, cplx m) {
  return fma(u.x, p.y, u.y * p.x) - fma(u.x, m.y, -u.y * m.x);
}

// The pole list of one launch of k_hmc_momentum_update_poles and k_hmc_fermion_force: device pointers and weights travel as kernel arguments
// (the way BatchCgm of qmg_batch.hip carries its shift lists), so a launch needs no table in device memory.
#define HMC_POLES_J 16
struct HmcPoles {
  const cplx* X[HMC_POLES_J];
  const cplx* Y[HMC_POLES_J];
  double w[HMC_POLES_J];
};

// The pole lists the kicks check after the pure-gauge case has left: every vector present (B is the second list of vectors, or A again) and
// no weight a NaN.
static inline bool pole_lists_valid(const void* const* A, const void* const* B, const double* weights, int n_poles) {
  if (!A || !B || !weights) return false;
  for (int j = 0; j < n_poles; j++)
    if (!A[j] || !B[j] || weights[j] != weights[j]) return false;
  return true;
}
// Poles in chunks of CHUNK (HMC_POLES_J; HMC_DWF_PAIRS for the domain-wall pairs): launch(j0, nj, first) fills the list of poles
// j0 .. j0 + nj - 1 and launches its kernel, with the gauge force if `first` and without it after.
template <int CHUNK, class Launch> static int launch_pole_chunks(int n_poles, Launch launch) {
  for (int j0 = 0; j0 < n_poles; j0 += CHUNK) {
    launch(j0, n_poles - j0 < CHUNK ? n_poles - j0 : CHUNK, j0 == 0);
    QMG_LAUNCH_CHECK();
  }
  return QMG_SUCCESS;
}

}  // namespace qmg

#endif
