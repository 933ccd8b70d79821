// qmg_singlet_plan.h -- what a request to the flavour-singlet entry points (qmg_noise_dilute_batch, qmg_loops_timeslice_batch) launches: ONE
// host function (singlet_plan) that both launches switch on and that qmg_singlet_plan() exports, after qmg_dwf_meas_plan.h.  The dilution
// classes (singlet_class) are here too: the one statement the two kernels share.  Host code only but for that function, no HIP call.
#ifndef QMG_SINGLET_PLAN_H
#define QMG_SINGLET_PLAN_H

#include "qmg_common.h"

namespace qmg {

// families (the values are part of qmg_singlet_plan()'s output, include/qmg_hip.h)
enum SingletFamily {
  SGF_INVALID = 0,   // the entry points return QMG_ERR_INVALID
  SGF_ROWS = 1,      // k_loops_timeslice<T, NT>: a block per (timeslice, active system); k_noise_dilute<T>: a lane per element
  SGF_NONE = 2       // no system is active: success with nothing launched
};
enum { SINGLET_PLAN_INTS = 12, SINGLET_ROWS_MAX = 65535, SINGLET_RED = 8, SINGLET_OUT = 5 };

// The first SINGLET_PLAN_INTS members, in this order, are what qmg_singlet_plan() writes.
struct SingletPlan {
  int family;     // SingletFamily
  int block;      // threads per block of both kernels: 256, whatever the row length (a row of Lx = 2 keeps 2 nc lanes of it busy)
  int gx, gy;     // the loops grid: gx = the active systems, gy = min(Ly, 65535) blocks over the timeslices
  int walk;       // timeslices walked per block: ceil(Ly / gy); block b takes y = b, b + gy, ... -- 1 unless Ly > 65535
  int lds;        // bytes of LDS per block of the loops kernel: 8 sums x 4 wavefronts, and the 8 block sums
  int doubles;    // doubles the loops entry writes: 5 Ly per active system
  int dgx, dgy;   // the dilution grid: dgx blocks of `block` lanes over the Lx Ly nc elements of a vector (at most 262144), dgy = the active systems
  int dwalk;      // elements walked per lane of the dilution kernel: ceil(n / (dgx block))
  int nk;         // active systems
  int classes;    // D = nt ncs neo
  // ----
  int status;
};

// the dilution class of element (y, c, p): ((y mod nt) ncs + (spin ? c : 0)) neo + (eo ? p : 0)
__host__ __device__ inline int singlet_class(int y, int c, int p, int nt, int nc, int spin, int eo) {
  const int ncs = spin ? nc : 1, neo = eo ? 2 : 1;
  return ((y % nt) * ncs + (spin ? c : 0)) * neo + (eo ? p : 0);
}

inline SingletPlan singlet_plan(int Lx, int Ly, int nc, int nt, int spin, int eo, int first_class, int nrhs, unsigned mask) {
  SingletPlan pl = {};
  pl.family = SGF_INVALID;
  pl.status = QMG_ERR_INVALID;
  if (!valid_lattice(Lx, Ly) || nc < 1 || nt < 1 || Ly % nt || (spin != 0 && spin != 1) || (eo != 0 && eo != 1)) return pl;
  if (nrhs < 1 || nrhs > BATCH_MAX || first_class < 0) return pl;
  const long run = (long)(Lx / 2) * nc;                // elements of a (parity, y) row: a lane counts them in an int
  if (run > 0x3FFFFFFFl) return pl;
  const long classes = (long)nt * (spin ? nc : 1) * (eo ? 2 : 1);
  if (classes > 0x7FFFFFFFl || (long)first_class + nrhs > classes) return pl;
  if ((long)SINGLET_OUT * Ly * BATCH_MAX > 0x7FFFFFFFl) return pl;
  const BatchIdx ids = expand_mask(mask, nrhs);
  pl.classes = (int)classes;
  pl.status = QMG_SUCCESS;
  if (ids.n < 1) { pl.family = SGF_NONE; return pl; }
  const size_t n = (size_t)Lx * Ly * nc;
  pl.family = SGF_ROWS;
  pl.block = BLOCK;
  pl.gx = ids.n;
  pl.gy = Ly > SINGLET_ROWS_MAX ? SINGLET_ROWS_MAX : Ly;
  pl.walk = (Ly + pl.gy - 1) / pl.gy;
  pl.lds = (int)sizeof(double) * (SINGLET_RED * (BLOCK / WAVE) + SINGLET_RED);
  pl.doubles = SINGLET_OUT * Ly * ids.n;
  pl.dgx = (int)grid_1d(n);
  pl.dgy = ids.n;
  pl.dwalk = (int)((n + (size_t)pl.dgx * BLOCK - 1) / ((size_t)pl.dgx * BLOCK));
  pl.nk = ids.n;
  return pl;
}

}  // namespace qmg

#endif
