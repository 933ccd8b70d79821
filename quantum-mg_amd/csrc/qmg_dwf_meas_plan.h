// qmg_dwf_meas_plan.h -- which launch serves a request to the domain-wall measurement entry points (qmg_dwf_wall_source,
// qmg_dwf_wall_project, qmg_dwf_slice_norms): ONE host function (dwf_meas_plan) that the three launches switch on and that
// qmg_dwf_meas_plan() exports, after qmg_dwf_eo_plan.h.  Host code only, no HIP call.
#ifndef QMG_DWF_MEAS_PLAN_H
#define QMG_DWF_MEAS_PLAN_H

#include "qmg_dwf_plan.h"

namespace qmg {

// the `kernel` argument of qmg_dwf_meas_plan()
enum DwfMeasKernel {
  DMK_SOURCE = 0,         // psi5 = the wall source of eta4
  DMK_PROJECT_WALL = 1,   // q4 = the physical quark field of psi5: (Ls-1, 0) and (0, 1)
  DMK_PROJECT_MID = 2,    // q4 = the midpoint field of psi5: (Ls/2-1, 0) and (Ls/2, 1); even Ls only
  DMK_NORMS = 3           // N(y, s, sigma) = sum_x |psi5(x, y; s, sigma)|^2
};
// families (the values are part of qmg_dwf_meas_plan()'s output, include/qmg_hip.h)
enum DwfMeasFamily {
  DMF_UNSUPPORTED = 0,   // the entry point returns QMG_ERR_UNSUPPORTED
  DMF_SOURCE = 1,        // k_dwf_wall_source<T>
  DMF_PROJECT = 2,       // k_dwf_wall_project<T>
  DMF_INVALID = 3,       // the entry point returns QMG_ERR_INVALID
  DMF_NORMS = 4          // k_dwf_slice_norms<T>, then k_dwf_slice_sum
};
enum { DWF_MEAS_PLAN_INTS = 8, DWF_MEAS_PBR_MAX = 4 };

// The first DWF_MEAS_PLAN_INTS members, in this order, are what qmg_dwf_meas_plan() writes.
struct DwfMeasPlan {
  int family;   // DwfMeasFamily
  int lps;      // lanes per site: Ls (source, norms: a lane owns one (site, s) pair with its two spin components) or 2 (projection: a
                // lane owns one spin component of a site)
  int block;    // threads per block: 256, for the norms Ls * floor(256 / Ls), so that a lane that strides by whole blocks keeps its s
  int gx, gy;   // gx blocks over the lps * Lx/2 lanes of a half row (norms: gx = pbr blocks, whose lanes stride over the half row by
                // gx * block); gy = min(2 Ly, 65535) blocks walk the (parity, y) rows; grid.z = the systems
  int pbr;      // partial sums per (parity, y) row that the second launch adds up: min(blocks that cover the half row, 4); 0 but for the norms
  int lds;      // bytes of LDS per block: two doubles per lane of the largest block for the norms, else 0
  int nk;       // systems served (all of them, in one launch)
  // ----
  int status;
};

inline DwfMeasPlan dwf_meas_plan(int dtype, int Lx, int Ly, int Ls, int kernel, int nsys) {
  const auto refused = [](int status) { return plan_refused<DwfMeasPlan>(status, DMF_INVALID, DMF_UNSUPPORTED); };
  if (!valid_dtype(dtype) || !dwf_dims_ok(Lx, Ly, Ls) || nsys < 1 || nsys > BATCH_MAX) return refused(QMG_ERR_INVALID);
  if (kernel < DMK_SOURCE || kernel > DMK_NORMS) return refused(QMG_ERR_INVALID);
  if (kernel == DMK_PROJECT_MID && (Ls & 1)) return refused(QMG_ERR_UNSUPPORTED);   // no midpoint between the walls
  DwfMeasPlan pl = {};
  pl.family = kernel == DMK_NORMS ? DMF_NORMS : kernel == DMK_SOURCE ? DMF_SOURCE : DMF_PROJECT;
  pl.lps = pl.family == DMF_PROJECT ? 2 : Ls;
  const HalfRowGrid g = half_row_grid(Lx, pl.lps, 2l * Ly, kernel == DMK_NORMS);
  pl.block = g.block; pl.gx = g.gx; pl.gy = g.gy;
  pl.nk = nsys;
  pl.status = QMG_SUCCESS;
  if (kernel == DMK_NORMS) {   // the blocks that would cover the half row, at most four, stride over it
    pl.pbr = g.gx > DWF_MEAS_PBR_MAX ? DWF_MEAS_PBR_MAX : g.gx;
    pl.gx = pl.pbr;
    pl.lds = DWF_BLOCK_MAX * 16;
  }
  return pl;
}

}  // namespace qmg

#endif
