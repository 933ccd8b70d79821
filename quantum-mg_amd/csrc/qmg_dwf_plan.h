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
enum { DW_PLAN_INTS = 8, DWF_PLAN_INTS = DW_PLAN_INTS, DWF_LS_MIN = 2, DWF_LS_MAX = 32 };
constexpr int DWF_BLOCK_MAX = BLOCK;   // the largest block of a domain-wall kernel (launch bounds, LDS sized per lane)

// ---- what the four domain-wall plans (this one, qmg_dwf_eo_plan.h, qmg_dwf_meas_plan.h, qmg_hmc_dwf_plan.h) and their entries share ----
// the lattice, the Ls bounds, and a half row of a five-dimensional vector within reach of the kernels' 32-bit byte offsets
inline bool dwf_dims_ok(int Lx, int Ly, int Ls) {
  return valid_lattice(Lx, Ly) && Ls >= DWF_LS_MIN && Ls <= DWF_LS_MAX && (long)(Lx / 2) * Ls * 32 <= 0x7FFFFFFFl;
}
// The grid of the (site, s) lane mapping: gx blocks cover the lps * Lx/2 lanes of a half row, gy = min(rows, 65535) blocks walk
// the rows.  whole_sites: the block is lps * floor(256 / lps) lanes, so that the lanes of a site never straddle a block (kernels that
// exchange along s in LDS, or whose lanes stride by whole blocks and keep their s); else 256.
struct HalfRowGrid { int block, gx, gy; };
inline HalfRowGrid half_row_grid(int Lx, int lps, long rows, bool whole_sites) {
  HalfRowGrid g;
  g.block = whole_sites ? lps * (DWF_BLOCK_MAX / lps) : DWF_BLOCK_MAX;
  g.gx = (int)(((long)(Lx / 2) * lps + g.block - 1) / g.block);
  g.gy = rows_on_grid(rows);
  return g;
}
// a plan that launches nothing: refused with a status (the INVALID or the UNSUPPORTED family of the plan), or success with nothing to do
template <class Plan> inline Plan plan_refused(int status, int family_invalid, int family_unsupported) {
  Plan pl = {};
  pl.family = status == QMG_ERR_INVALID ? family_invalid : family_unsupported;
  pl.status = status;
  return pl;
}
template <class Plan> inline Plan plan_nothing(int family) {
  Plan pl = {};
  pl.family = family;
  return pl;
}
// What qmg_dwf_plan(), qmg_dwf_eo_plan(), qmg_mobius_plan() and qmg_mobius_eo_plan() write: {family, lps, block, gx, gy, flags, slot6, nk}, where
// slot6 is the plan's lds (its shape for qmg_dwf_plan()), then -1 beyond them.
template <class Plan> inline int export_dw_plan(const Plan& pl, int slot6, int* plan_out, int plan_len) {
  if (!plan_out || plan_len < DW_PLAN_INTS) return QMG_ERR_INVALID;
  const int v[DW_PLAN_INTS] = {pl.family, pl.lps, pl.block, pl.gx, pl.gy, pl.flags, slot6, pl.nk};
  export_plan_ints(v, DW_PLAN_INTS, plan_out, plan_len);
  return QMG_SUCCESS;
}
// What every entry checks before its plan is asked: dtype, Ls, the systems of the call and, with more than one, the stride between them --
// at least one five-dimensional vector (and, has4, one four-dimensional one), even in fp32 so that every system stays 16-byte aligned.
// Entries with a descriptor check d->nc == 2 Ls beside it.
inline int dwf_entry_check(int dtype, int Lx, int Ly, int Ls, int nsys, size_t stride5, size_t stride4 = 0, bool has4 = false) {
  if (!valid_dtype(dtype) || Ls < DWF_LS_MIN || Ls > DWF_LS_MAX || nsys < 1 || nsys > BATCH_MAX) return QMG_ERR_INVALID;
  if (nsys > 1) {
    const size_t site = (size_t)Lx * Ly;
    if (stride5 < site * 2 * Ls || (dtype == QMG_C32 && (stride5 & 1))) return QMG_ERR_INVALID;
    if (has4 && (stride4 < site * 2 || (dtype == QMG_C32 && (stride4 & 1)))) return QMG_ERR_INVALID;
  }
  return QMG_SUCCESS;
}
// the row members DwfArgs and DwfEoArgs<T> share (their order and types are part of the kernels' device code and stay the structs' own)
template <class Args>
inline void dwf_fill_rows(Args& a, const void* gauge, void* lhs, const void* rhs, int Lx, int Ly, int Ls, unsigned pieces, const BatchIdx& b, size_t vec_stride,
                          int par_first, int par_count) {
  a.gauge = gauge; a.lhs = lhs; a.rhs = rhs;
  a.hr = Lx / 2; a.Ly = Ly; a.Ls = Ls;
  a.half_vol = (long)a.hr * Ly;
  a.pieces = pieces; a.nrhs = b.n; a.vec_stride = (long)vec_stride;
  a.par_first = par_first; a.par_count = par_count; a.nrows = Ly * par_count;
  for (int k = 0; k < 16; k++) a.ridx[k] = b.id[k];
}

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

// n_active: the systems of the call whose mask bit is set (0 .. 16); inplace: lhs == rhs
inline DwfPlan dwf_plan(int dtype, int Lx, int Ly, int Ls, unsigned pieces, int n_active, int inplace) {
  const auto refused = [](int status) { return plan_refused<DwfPlan>(status, DF_INVALID, DF_UNSUPPORTED); };
  const auto nothing = [] { return plan_nothing<DwfPlan>(DF_NOTHING); };
  if (!valid_dtype(dtype) || !dwf_dims_ok(Lx, Ly, Ls) || n_active < 0 || n_active > BATCH_MAX) return refused(QMG_ERR_INVALID);
  if (n_active == 0) return nothing();
  const PieceShape ps = links_piece_shape(pieces);   // the sets kernel W serves (qmg_wilson_plan.h)
  if (ps.par_count == 0) return nothing();
  const int par_first = ps.par_first, par_count = ps.par_count, shape = ps.shape;
  const bool zero = ps.zero;
  if (shape == 0) return refused(QMG_ERR_UNSUPPORTED);
  if (inplace && (shape == 1 || par_count == 2)) return refused(QMG_ERR_INVALID);   // in place: one parity written from the other by hops alone
  const bool pair = shape == 1 && par_count == 2;   // the full operator: kernel D2
  const HalfRowGrid g = half_row_grid(Lx, Ls, pair ? (long)Ly : (long)Ly * par_count, false);
  DwfPlan pl = {};
  pl.family = pair ? DF_PAIR : DF_DIRECT;
  pl.lps = Ls;
  pl.block = g.block; pl.gx = g.gx; pl.gy = g.gy;
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
