// qmg_wilson_plan.h -- which launch serves a request to the Wilson applies from the gauge links (qmg_wilson_apply_direct, qmg_wilson_hops_direct
// and their _epi forms; csrc/qmg_wilson.hip): ONE host function (wilson_plan) that the entry point switches on and that qmg_wilson_plan()
// exports, after the model of qmg_dwf_plan.h; and the piece-set analysis every from-the-links plan shares (links_piece_shape).
// Host code only, no HIP call.
#ifndef QMG_WILSON_PLAN_H
#define QMG_WILSON_PLAN_H

#include "qmg_common.h"

namespace qmg {

// What a piece set asks of the kernels that work from the links.  par_count = 0: no piece names a parity.  shape, if every processed parity
// asks for the same complete set: 1 clover + every hop (+ shift), 2 every hop alone; 0: a partial set, or the parities differ.
// zero: every processed parity is overwritten (QMG_P_ZERO_p).
struct PieceShape { int par_first, par_count, shape; bool zero; };
inline PieceShape links_piece_shape(unsigned pieces) {
  const unsigned even_bits = QMG_P_CLOVER_E | QMG_P_EO | QMG_P_SHIFT_E | QMG_P_ZERO_E;
  const unsigned odd_bits = QMG_P_CLOVER_O | QMG_P_OE | QMG_P_SHIFT_O | QMG_P_ZERO_O;
  const bool ev = pieces & even_bits, od = pieces & odd_bits;
  PieceShape s = {ev ? 0 : 1, (ev ? 1 : 0) + (od ? 1 : 0), 0, true};
  int sh[2] = {0, 0};
  for (int q = 0; q < s.par_count; q++) {
    const int p = (s.par_count == 2) ? q : s.par_first;
    const bool cl = (pieces >> p) & 1u, shf = (pieces >> (10 + p)) & 1u;
    const unsigned hm = (pieces >> (2 + 4 * p)) & 0xFu;
    sh[q] = (hm == 0xFu) ? (cl ? 1 : (shf ? 0 : 2)) : 0;
    if (!((pieces >> (12 + p)) & 1u)) s.zero = false;
  }
  s.shape = (s.par_count == 2 && sh[0] != sh[1]) ? 0 : sh[0];
  return s;
}

// families (the values are part of qmg_wilson_plan()'s output, include/qmg_hip.h; 0 - 4 mean what they mean in qmg_dwf_plan.h)
enum WilsonFamily {
  WF_UNSUPPORTED = 0,   // the entry point returns QMG_ERR_UNSUPPORTED: the stored stencil serves the request
  WF_DIRECT = 1,        // k_wilson_direct<T, SHAPE, ZERO, BATCH, EPI> (kernel W): one site per lane group
  WF_NOTHING = 2,       // success with nothing launched
  WF_INVALID = 3,       // the entry point returns QMG_ERR_INVALID
  WF_PAIR = 4,          // k_wilson_pair<T, ZERO, BATCH, EPI> (kernel W2): the full operator, both parities of a column per lane group
  WF_PAIR2 = 5          // k_wilson_pair2<T, ZERO, EPI> (kernel W2 on two rows per lane group): one system, EPI 0 or 1
};
// flags of the instantiation
enum {
  WPF_ZERO = 1,    // every processed parity is overwritten (compile-time ZERO; otherwise the kernel tests the bits per row)
  WPF_BATCH = 2,   // more than one active system: the links stay in registers across the systems
  WPF_F32 = 4,     // complex<float> storage and arithmetic
  WPF_DOTS = 8     // the launch leaves the MR dots' partials (epilogue modes 1, 3, 4)
};
// what the launch needs to know of an epilogue (qmg_apply_epilogue): the `epi` member of a request
enum {
  WPE_ON = 1,              // the call has an epilogue
  WPE_OTHER = 2,           // epi->other is set
  WPE_DOTV = 4,            // epi->dotv is set
  WPE_DOTV_IS_OTHER = 8,   // ... and both are the same vector
  WPE_DOTV_IS_RHS = 16,    // epi->dotv is the right-hand side
  WPE_ALIASES_LHS = 32     // epi->other or epi->dotv is lhs
};
enum { WILSON_PLAN_INTS = 16 };

struct WilsonRequest {
  int dtype, Lx, Ly, nc;   // the vectors' lattice (a slab: its local rows)
  int gauge_Ly, y0;        // the gauge field's lattice and the slab's first row on it
  int halos;               // both y-slab halo buffers are given
  int layout_ok;           // what the entry point sees of the buffers: the halos come as a pair, the strides hold a vector / a halo row
  int scaled;              // the qmg_wilson_hops_direct* entries (SHAPE 3)
  unsigned pieces;
  int n_active;            // the systems of the call whose mask bit is set (0 .. 16)
  int inplace;             // lhs == rhs
  int rows;                // 0 all rows, 1 the interior, 2 the two boundary rows (qmg_stencil_apply_slab)
  int pair;                // the "wilson_pair" tuning knob
  unsigned epi;            // WPE_*
};

// The members, in this order, are what qmg_wilson_plan() writes.
struct WilsonPlan {
  int family;                // WilsonFamily
  int lps;                   // lanes per site: 2 in fp64 (a lane per spin component), 1 in fp32
  int block;                 // threads per block
  int gx, gy;                // grid: gx blocks cover the lps * Lx/2 lanes of a half row; gy blocks walk the rows -- (parity, y) for kernel W, y for
                             // W2, row pairs for W2 on two rows -- min(rows, 65535) of them, and with the dots at most max(1, 2048 / gx)
  int flags;                 // WPF_*
  int shape;                 // 1: clover + every hop (+ shift) of the processed parities; 2: every hop alone; 3: every hop alone, scaled
  int emode;                 // the kernels' EPI: 0 none, 1 dots against the right-hand side's own-site chunk, 2 combination, 3 combination + dots
                             // against the same vector, 4 dots against a separate vector
  int nk;                    // active systems served (all of them, in one launch)
  int y_first, y_count;      // the rows of the launch: y_first .. y_first + y_count - 1 ...
  int boundary_only;         // ... or, if set, rows 0 and Ly - 1 (y_count = 2)
  int npart;                 // partials of the MR epilogue per system: gx * gy * BLOCK / WAVE, one per wavefront; 0 without dots
  int status;                // QMG_SUCCESS, or what the entry point returns
  int par_first, par_count;
};

namespace wilson_detail {
inline WilsonPlan refused(int status) {
  WilsonPlan pl = {};
  pl.family = status == QMG_ERR_INVALID ? WF_INVALID : WF_UNSUPPORTED;
  pl.status = status;
  return pl;
}
inline WilsonPlan nothing() {
  WilsonPlan pl = {};
  pl.family = WF_NOTHING;
  return pl;
}
}  // namespace wilson_detail

// The status of a request, in this precedence (Stencil2D::run_route falls back to the stored stencil on QMG_ERR_UNSUPPORTED and on nothing
// else, so the order is a contract with the facade):
//    1. the hops entries refuse QMG_P_CLOVER | QMG_P_SHIFT pieces                                          UNSUPPORTED
//    2. dtype, rows, n_active, the two lattices, y0 (even, the slab inside the gauge lattice)              INVALID
//    3. nc != 2                                                                                            UNSUPPORTED
//    4. halos not a pair, a slab (gauge_Ly != Ly, or rows != 0) without halos, short strides               INVALID
//    5. no active system                                                                                   nothing
//    6. an epilogue with more than one active system                                                       UNSUPPORTED
//    7. an epilogue vector that is lhs                                                                     INVALID
//    8. two different epilogue vectors                                                                     UNSUPPORTED
//    9. no processed parity                                                                                nothing
//   10. y_count <= 0 (rows = 1 on Ly = 2)                                                                  nothing
//   11. shape 0, or a hops entry with a shape other than 2                                                 UNSUPPORTED
//   12. in place with shape 1 or both parities (in place: one parity written from the other by hops)       INVALID
//   13. an epilogue without overwrite on every processed parity, or in place                               INVALID
// Pointer-null checks are the entry point's and come between 1 and 2.
inline WilsonPlan wilson_plan(const WilsonRequest& q) {
  using namespace wilson_detail;
  if (q.scaled && (q.pieces & (QMG_P_CLOVER | QMG_P_SHIFT))) return refused(QMG_ERR_UNSUPPORTED);                                   // 1
  if (!valid_dtype(q.dtype) || q.rows < 0 || q.rows > 2 || q.n_active < 0 || q.n_active > BATCH_MAX) return refused(QMG_ERR_INVALID);   // 2
  if (!valid_lattice(q.Lx, q.Ly) || !valid_lattice(q.Lx, q.gauge_Ly) || q.y0 < 0 || (q.y0 & 1) || q.y0 + q.Ly > q.gauge_Ly) return refused(QMG_ERR_INVALID);
  if (q.nc != 2) return refused(QMG_ERR_UNSUPPORTED);                                                                                // 3
  if (!q.layout_ok || (!q.halos && (q.gauge_Ly != q.Ly || q.rows != 0))) return refused(QMG_ERR_INVALID);                            // 4
  if (q.n_active == 0) return nothing();                                                                                             // 5
  const bool epi = q.epi & WPE_ON, other = epi && (q.epi & WPE_OTHER), dotv = epi && (q.epi & WPE_DOTV);
  if (epi && q.n_active != 1) return refused(QMG_ERR_UNSUPPORTED);                                                                   // 6
  if (epi && (q.epi & WPE_ALIASES_LHS)) return refused(QMG_ERR_INVALID);                                                             // 7
  if (other && dotv && !(q.epi & WPE_DOTV_IS_OTHER)) return refused(QMG_ERR_UNSUPPORTED);                                            // 8
  const PieceShape ps = links_piece_shape(q.pieces);
  if (ps.par_count == 0) return nothing();                                                                                           // 9
  const int y_count = q.rows == 2 ? 2 : q.rows == 1 ? q.Ly - 2 : q.Ly;
  if (y_count <= 0) return nothing();                                                                                                // 10
  if (ps.shape == 0 || (q.scaled && ps.shape != 2)) return refused(QMG_ERR_UNSUPPORTED);                                             // 11
  const int shape = q.scaled ? 3 : ps.shape;
  if (q.inplace && (shape == 1 || ps.par_count == 2)) return refused(QMG_ERR_INVALID);                                               // 12
  if (epi && (!ps.zero || q.inplace)) return refused(QMG_ERR_INVALID);                                                               // 13
  WilsonPlan pl = {};
  pl.lps = q.dtype == QMG_C64 ? 2 : 1;
  pl.block = BLOCK;
  pl.gx = (int)(((long)(q.Lx / 2) * pl.lps + BLOCK - 1) / BLOCK);
  pl.flags = (ps.zero ? WPF_ZERO : 0) | (q.n_active > 1 ? WPF_BATCH : 0) | (q.dtype == QMG_C32 ? WPF_F32 : 0) | (dotv ? WPF_DOTS : 0);
  pl.shape = shape;
  // mode 1 needs the own-site chunk in registers (SHAPE 1), else the vector is loaded: mode 4; an epilogue with neither vector is a pure
  // scaling of the result (other_scale is moot): mode 2 with no vector
  pl.emode = !epi ? 0 : !dotv ? 2 : other ? 3 : ((q.epi & WPE_DOTV_IS_RHS) && shape == 1) ? 1 : 4;
  pl.nk = q.n_active;
  pl.y_first = q.rows == 1 ? 1 : 0;
  pl.y_count = y_count;
  pl.boundary_only = q.rows == 2;
  pl.par_first = ps.par_first;
  pl.par_count = ps.par_count;
  // The full operator goes to kernel W2; one system on an even run of consecutive rows to its two-row form -- unless the epilogue loads a
  // vector (modes 2-4): that would take the two-row form to 170-178 VGPRs, two wavefronts per SIMD, so those go through the one-row form.
  const bool full = shape == 1 && ps.par_count == 2;
  long nrows;
  if (full && q.pair >= 2 && q.n_active == 1 && !pl.boundary_only && y_count % 2 == 0 && pl.emode <= 1) { pl.family = WF_PAIR2; nrows = y_count / 2; }
  else if (full && q.pair) { pl.family = WF_PAIR; nrows = y_count; }
  else { pl.family = WF_DIRECT; nrows = (long)y_count * ps.par_count; }
  pl.gy = rows_on_grid(nrows);
  if (dotv) {
    // launches with the MR dots keep the number of partials (one per wavefront) small enough for the one-block second stage: the blocks
    // walk several rows each (every kernel W form has the row loop; capping grid.y costs nothing)
    const int cap = pl.gx >= 2048 ? 1 : 2048 / pl.gx;
    if (pl.gy > cap) pl.gy = cap;
    pl.npart = pl.gx * pl.gy * (BLOCK / WAVE);
  }
  return pl;
}

}  // namespace qmg

#endif
