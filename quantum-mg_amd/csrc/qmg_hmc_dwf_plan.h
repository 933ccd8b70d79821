// qmg_hmc_dwf_plan.h -- which launches serve a request to qmg_hmc_momentum_update_dwf (csrc/qmg_hmc.hip): ONE host function (hmc_dwf_plan)
// that the entry switches on and that qmg_hmc_dwf_plan() exports, after qmg_dwf_eo_plan.h.  Host code only, no HIP call.
#ifndef QMG_HMC_DWF_PLAN_H
#define QMG_HMC_DWF_PLAN_H

#include "qmg_dwf_plan.h"

namespace qmg {

// families (the values are part of qmg_hmc_dwf_plan()'s output, include/qmg_hip.h)
enum HmcDwfFamily {
  HDF_UNSUPPORTED = 0,   // the entry point returns QMG_ERR_UNSUPPORTED
  HDF_FUSED = 1,         // k_hmc_momentum_update_dwf<GAUGE>: the first launch with the gauge force, further ones without
  HDF_GAUGE = 2,         // the pure-gauge kick of qmg_hmc_momentum_update (its kernel, its bits)
  HDF_INVALID = 3        // the entry point returns QMG_ERR_INVALID
};
enum { HMC_DWF_PLAN_INTS = 8, HMC_DWF_PAIRS = 4 };

// The first HMC_DWF_PLAN_INTS members, in this order, are what qmg_hmc_dwf_plan() writes.
struct HmcDwfPlan {
  int family;     // HmcDwfFamily
  int lps;        // lanes per site: Ls (HDF_FUSED), 0 for the pure-gauge kick (a thread per site pair)
  int block;      // threads per block: Ls * floor(256 / Ls), so that the Ls lanes of a site never straddle a block (the sum over s is in LDS)
  int gx, gy;     // gx blocks cover the lps * Lx/2 lanes of a half row; gy = min(2 Ly, 65535) blocks walk the (parity, y) rows
  int lds;        // bytes of LDS per block: two buffers of (fx, fy) per lane
  int launches;   // ceil(n_pairs / HMC_DWF_PAIRS)
  int per_launch; // HMC_DWF_PAIRS: pairs (X[j], Y[j]) one launch takes as kernel arguments
  // ----
  int status;
};

inline HmcDwfPlan hmc_dwf_plan(int Lx, int Ly, int Ls, int n_pairs, unsigned flags) {
  if (!dwf_dims_ok(Lx, Ly, Ls) || n_pairs < 0 || (flags & ~(unsigned)(QMG_HMC_GAUGE_ONLY | QMG_HMC_DWF_G5_Y)))
    return plan_refused<HmcDwfPlan>(QMG_ERR_INVALID, HDF_INVALID, HDF_UNSUPPORTED);
  HmcDwfPlan pl = {};
  pl.status = QMG_SUCCESS;
  if ((flags & QMG_HMC_GAUGE_ONLY) || n_pairs == 0) {
    pl.family = HDF_GAUGE;
    pl.block = BLOCK;
    pl.gx = (int)grid_1d((size_t)Lx * Ly / 2);
    pl.gy = 1;
    pl.launches = 1;
    return pl;
  }
  pl.family = HDF_FUSED;
  pl.lps = Ls;
  const HalfRowGrid g = half_row_grid(Lx, Ls, 2l * Ly, true);
  pl.block = g.block; pl.gx = g.gx; pl.gy = g.gy;
  pl.lds = 2 * DWF_BLOCK_MAX * 16;
  pl.launches = (n_pairs + HMC_DWF_PAIRS - 1) / HMC_DWF_PAIRS;
  pl.per_launch = HMC_DWF_PAIRS;
  return pl;
}

}  // namespace qmg

#endif
