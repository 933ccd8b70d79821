// qmg_dwf_plan.h -- which launch serves a request to qmg_dwf_apply_direct: ONE host function (dwf_plan) that the entry point switches on and
// that qmg_dwf_plan() exports, after the model of qmg_stencil_plan.h / qmg_transfer_plan.h: the tests ask for the answer to a request and hold
// the launch geometry to the lattice without a GPU (tests/test_host_dwf.py).  Host code only, no HIP call.
#ifndef QMG_DWF_PLAN_H
#define QMG_DWF_PLAN_H

#include "qmg_common.h"
#include "qmg_wilson_plan.h"   // links_piece_shape

namespace qmg {

// families (the values are part of qmg_dwf_plan()'s output, include/qmg_hip.h)
enum DwfFamily {
  DF_UNSUPPORTED = 0,   // the entry point returns QMG_ERR_UNSUPPORTED: a piece set the stored stencil serves
  DF_DIRECT = 1,        // k_dwf_direct<T, SHAPE, ZERO, BATCH>
  DF_NOTHING = 2,       // success with nothing launched (no piece asks for work, or no active system)
  DF_INVALID = 3,       // the entry point returns QMG_ERR_INVALID
  DF_PAIR = 4           // k_dwf_pair<T, ZERO, BATCH> (kernel D2): the full operator, both parities of a column per lane
};
// flags of the instantiation
enum {
  DPF_ZERO = 1,    // every processed parity is overwritten (compile-time ZERO; otherwise the kernel tests the bits per row)
  DPF_BATCH = 2,   // more than one active system: the links stay in registers across the systems
  DPF_F32 = 4      // complex<float> storage and arithmetic
};
enum { DWF_PLAN_INTS = 8, DWF_LS_MIN = 2, DWF_LS_MAX = 32 };

// The first DWF_PLAN_INTS members, in this order, are what qmg_dwf_plan() writes.
struct DwfPlan {
  int family;   // DwfFamily
  int lps;      // lanes per site: Ls, a lane owns one (site, s) pair with its two spin components
  int block;    // threads per block
  int gx, gy;   // grid: gx blocks cover the lps * Lx/2 lanes of a half row; gy = min(rows, 65535) blocks walk the rows: (parity, y) of the
                // processed parities for kernel D, y for kernel D2 (a lane serves both parities of its column)
  int flags;    // DPF_*
  int shape;    // 1: clover + every hop (+ shift) of the processed parities; 2: every hop alone
  int nk;       // active systems served (all of them, in one launch)
  // ----
  int status;   // QMG_SUCCESS, or what the entry point returns
  int par_first, par_count;
};

namespace dwf_detail {
inline DwfPlan refused(int status) {
  DwfPlan pl = {};
  pl.family = status == QMG_ERR_INVALID ? DF_INVALID : DF_UNSUPPORTED;
  pl.status = status;
  return pl;
}
inline DwfPlan nothing() {
  DwfPlan pl = {};
  pl.family = DF_NOTHING;
  return pl;
}
}  // namespace dwf_detail

// n_active: the systems of the call whose mask bit is set (0 .. 16); inplace: lhs == rhs
inline DwfPlan dwf_plan(int dtype, int Lx, int Ly, int Ls, unsigned pieces, int n_active, int inplace) {
  using namespace dwf_detail;
  if (!valid_dtype(dtype) || !valid_lattice(Lx, Ly) || Ls < DWF_LS_MIN || Ls > DWF_LS_MAX || n_active < 0 || n_active > BATCH_MAX) return refused(QMG_ERR_INVALID);
  const long lanes = (long)(Lx / 2) * Ls;
  if (lanes * 32 > 0x7FFFFFFFl) return refused(QMG_ERR_INVALID);   // a half row of the vector is addressed with 32-bit byte offsets
  if (n_active == 0) return nothing();
  const PieceShape ps = links_piece_shape(pieces);   // the sets kernel W serves (qmg_wilson_plan.h)
  if (ps.par_count == 0) return nothing();
  const int par_first = ps.par_first, par_count = ps.par_count, shape = ps.shape;
  const bool zero = ps.zero;
  if (shape == 0) return refused(QMG_ERR_UNSUPPORTED);
  if (inplace && (shape == 1 || par_count == 2)) return refused(QMG_ERR_INVALID);   // in place: one parity written from the other by hops alone
  const bool pair = shape == 1 && par_count == 2;   // the full operator: kernel D2
  const long nrows = pair ? (long)Ly : (long)Ly * par_count;
  DwfPlan pl = {};
  pl.family = pair ? DF_PAIR : DF_DIRECT;
  pl.lps = Ls;
  pl.block = BLOCK;
  pl.gx = (int)((lanes + BLOCK - 1) / BLOCK);
  pl.gy = nrows > 65535 ? 65535 : (int)nrows;
  pl.flags = (zero ? DPF_ZERO : 0) | (n_active > 1 ? DPF_BATCH : 0) | (dtype == QMG_C32 ? DPF_F32 : 0);
  pl.shape = shape;
  pl.nk = n_active;
  pl.status = QMG_SUCCESS;
  pl.par_first = par_first;
  pl.par_count = par_count;
  return pl;
}

}  // namespace qmg

#endif
