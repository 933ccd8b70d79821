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
enum { DWF_MEAS_PLAN_INTS = 8, DWF_MEAS_BLOCK_MAX = 256, DWF_MEAS_PBR_MAX = 4 };

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

namespace dwf_meas_detail {
inline DwfMeasPlan refused(int status) {
  DwfMeasPlan pl = {};
  pl.family = status == QMG_ERR_INVALID ? DMF_INVALID : DMF_UNSUPPORTED;
  pl.status = status;
  return pl;
}
}  // namespace dwf_meas_detail

inline DwfMeasPlan dwf_meas_plan(int dtype, int Lx, int Ly, int Ls, int kernel, int nsys) {
  using namespace dwf_meas_detail;
  if (!valid_dtype(dtype) || !valid_lattice(Lx, Ly) || Ls < DWF_LS_MIN || Ls > DWF_LS_MAX || nsys < 1 || nsys > BATCH_MAX) return refused(QMG_ERR_INVALID);
  if (kernel < DMK_SOURCE || kernel > DMK_NORMS) return refused(QMG_ERR_INVALID);
  const long lanes5 = (long)(Lx / 2) * Ls;
  if (lanes5 * 32 > 0x7FFFFFFFl) return refused(QMG_ERR_INVALID);   // a half row of the vector is addressed with 32-bit byte offsets
  if (kernel == DMK_PROJECT_MID && (Ls & 1)) return refused(QMG_ERR_UNSUPPORTED);   // no midpoint between the walls
  const long nrows = 2l * Ly;
  DwfMeasPlan pl = {};
  pl.gy = nrows > 65535 ? 65535 : (int)nrows;
  pl.nk = nsys;
  pl.status = QMG_SUCCESS;
  if (kernel == DMK_NORMS) {
    pl.family = DMF_NORMS;
    pl.lps = Ls;
    pl.block = Ls * (DWF_MEAS_BLOCK_MAX / Ls);
    const long cover = (lanes5 + pl.block - 1) / pl.block;
    pl.pbr = cover > DWF_MEAS_PBR_MAX ? DWF_MEAS_PBR_MAX : (int)cover;
    pl.gx = pl.pbr;
    pl.lds = DWF_MEAS_BLOCK_MAX * 16;
    return pl;
  }
  pl.family = kernel == DMK_SOURCE ? DMF_SOURCE : DMF_PROJECT;
  pl.lps = kernel == DMK_SOURCE ? Ls : 2;
  pl.block = DWF_MEAS_BLOCK_MAX;
  const long lanes = (long)(Lx / 2) * pl.lps;
  pl.gx = (int)((lanes + pl.block - 1) / pl.block);
  return pl;
}

}  // namespace qmg

#endif
