// qmg_dwf_eo_plan.h -- which launch serves a request to the even-odd domain-wall entry points (qmg_dwf_inv5, qmg_dwf_hops_inv5,
// qmg_dwf_schur_apply, and their Moebius namesakes through qmg_mobius_eo_plan.h): ONE host function (dw_eo_plan) that the launches of both
// operators switch on and that qmg_dwf_eo_plan() / qmg_mobius_eo_plan() export, after qmg_dwf_plan.h; what the entries of both do around it;
// and the fifth-dimension coefficients the Shamir kernels take by value (dwf_eo_coef).  Host code only, no HIP call.
#ifndef QMG_DWF_EO_PLAN_H
#define QMG_DWF_EO_PLAN_H

#include <cmath>
#include <complex>

#include "qmg_dwf_plan.h"

namespace qmg {

// the `kernel` argument of qmg_dwf_eo_plan(); qmg_mobius_eo_plan() has the same three and a fourth (MobiusEoKernel)
enum DwfEoKernel {
  DEK_INV5 = 0,        // kernel I: lhs_p = alpha A_p^-1 rhs_p
  DEK_HOPS_INV5 = 1,   // kernel K: lhs_p (+)= alpha A_p^-1 H_{p,1-p} rhs_{1-p}
  DEK_SCHUR2 = 2       // second stage of M: lhs_p = A_p x_p + H_{p,1-p} t_{1-p}
};
// families (the values are part of qmg_dwf_eo_plan()'s and qmg_mobius_eo_plan()'s output, include/qmg_hip.h), under either operator's names
enum DwEoFamily {
  DEF_UNSUPPORTED = 0, MEF_UNSUPPORTED = 0,   // the entry point returns QMG_ERR_UNSUPPORTED
  DEF_HOPS_INV5 = 1, MEF_HOPS_MIX = 1,        // k_dwf_eo_inv5<T, true, ZERO, BATCH>; k_mobius_eo_mix<T, true, RMIX, ZERO, BATCH>
  DEF_NOTHING = 2, MEF_NOTHING = 2,           // success with nothing launched
  DEF_INVALID = 3, MEF_INVALID = 3,           // the entry point returns QMG_ERR_INVALID
  DEF_INV5 = 4, MEF_MIX = 4,                  // k_dwf_eo_inv5<T, false, true, BATCH>; k_mobius_eo_mix<T, false, false, true, BATCH>
  DEF_SCHUR2 = 5, MEF_SCHUR2 = 5,             // k_dwf_eo_schur2<T, BATCH>; k_mobius_eo_schur2<T, BATCH>
  MEF_SCHUR2_DAGGER = 6                       // k_mobius_eo_schur2_dagger<T, BATCH>
};
// MEPF_RMIX: a flag next to DPF_ZERO / DPF_BATCH / DPF_F32 -- the hop source is mixed on the load (Moebius only)
enum { DWF_EO_PLAN_INTS = DW_PLAN_INTS, MOBIUS_EO_PLAN_INTS = DW_PLAN_INTS, MEPF_RMIX = 8 };

// The first DW_PLAN_INTS members, in this order, are what the two exports write (export_dw_plan).
struct DwEoPlan {
  int family;   // DwEoFamily
  int lps;      // lanes per site: Ls
  int block;    // Ls * floor(256 / Ls) where the lanes of a site must not straddle a block (the exchange along s is in LDS), else 256
  int gx, gy;   // gx blocks cover the lps * Lx/2 lanes of a half row; gy = min(rows, 65535) blocks walk the (parity, y) rows
  int flags;    // DPF_ZERO / DPF_BATCH / DPF_F32 (qmg_dwf_plan.h) / MEPF_RMIX
  int lds;      // bytes of LDS per block: two buffers of one chunk per lane, 0 for the second stage of M
  int nk;       // active systems served (all of them, in one launch)
  // ----
  int status;
  int par_first, par_count;
};
typedef DwEoPlan DwfEoPlan;
typedef DwEoPlan MobiusEoPlan;

// the pieces of the two launches of a Schur apply of parity p (o = 1 - p): kernel 1 writes tmp_o from rhs_p, the second stage writes lhs_p
struct DwEoStages { unsigned pieces1, pieces2; };
inline DwEoStages dw_eo_stages(int p) {
  DwEoStages s;
  s.pieces1 = p ? QMG_P_EO | QMG_P_ZERO_E : QMG_P_OE | QMG_P_ZERO_O;
  s.pieces2 = p ? QMG_P_CLOVER_O | QMG_P_OE | QMG_P_SHIFT_O | QMG_P_ZERO_O : QMG_P_CLOVER_E | QMG_P_EO | QMG_P_SHIFT_E | QMG_P_ZERO_E;
  return s;
}

// pieces: kernel 0   QMG_P_CLOVER_E / _O name the parities;
//         kernel 1   all four hop bits of each processed parity (+ QMG_P_ZERO_*);
//         kernel 2   QMG_P_CLOVER_p | the four hops of p | QMG_P_SHIFT_p | QMG_P_ZERO_p of exactly one parity p; kernel 3 (the second stage of
//                    M^dagger, Moebius) takes kernel 2's.
// n_active: the systems whose mask bit is set (0 .. 16); inplace: lhs == rhs.  What the operator brings: kernel_max, its highest kernel number;
// rmix, whether a kernel-1 launch carries MEPF_RMIX; stage2_whole_sites, the block of kernel 2 -- Shamir's stage 2 runs whole-site blocks
// (Ls floor(256 / Ls)) although it exchanges nothing in LDS, Moebius's runs 256.  That is the launch geometry the two kernels were written
// and measured with: kept, not chosen here.
inline DwEoPlan dw_eo_plan(int dtype, int Lx, int Ly, int Ls, int kernel, int kernel_max, unsigned pieces, int n_active, int inplace, bool rmix,
                           bool stage2_whole_sites) {
  const auto refused = [](int status) { return plan_refused<DwEoPlan>(status, DEF_INVALID, DEF_UNSUPPORTED); };
  if (!valid_dtype(dtype) || !dwf_dims_ok(Lx, Ly, Ls) || n_active < 0 || n_active > BATCH_MAX) return refused(QMG_ERR_INVALID);
  if (kernel < DEK_INV5 || kernel > kernel_max) return refused(QMG_ERR_INVALID);
  if (n_active == 0 || pieces == 0) return plan_nothing<DwEoPlan>(DEF_NOTHING);
  int par_first = 0, par_count = 0;
  bool zero = true;
  if (kernel == DEK_INV5) {
    if (pieces & ~(unsigned)QMG_P_CLOVER) return refused(QMG_ERR_UNSUPPORTED);
    const bool ev = pieces & QMG_P_CLOVER_E, od = pieces & QMG_P_CLOVER_O;
    par_first = ev ? 0 : 1; par_count = (ev && od) ? 2 : 1;
  } else if (kernel == DEK_HOPS_INV5) {
    if (pieces & (QMG_P_CLOVER | QMG_P_SHIFT)) return refused(QMG_ERR_UNSUPPORTED);
    const PieceShape ps = links_piece_shape(pieces);   // no clover or shift bit is left: a parity is named by its hop or zero bits
    if (ps.shape != 2) return refused(QMG_ERR_UNSUPPORTED);   // a partial hop set
    par_first = ps.par_first; par_count = ps.par_count; zero = ps.zero;
    if (inplace && par_count == 2) return refused(QMG_ERR_INVALID);   // in place: one parity written from the other
  } else {
    const unsigned even = dw_eo_stages(0).pieces2, odd = dw_eo_stages(1).pieces2;
    if (pieces != even && pieces != odd) return refused(QMG_ERR_UNSUPPORTED);
    if (inplace) return refused(QMG_ERR_INVALID);
    par_first = pieces == even ? 0 : 1; par_count = 1;
  }
  const HalfRowGrid g = half_row_grid(Lx, Ls, (long)Ly * par_count, kernel != DEK_SCHUR2 || stage2_whole_sites);
  const int f32 = dtype == QMG_C32;
  DwEoPlan pl = {};
  pl.family = kernel == DEK_INV5 ? DEF_INV5 : kernel == DEK_HOPS_INV5 ? DEF_HOPS_INV5 : kernel == DEK_SCHUR2 ? DEF_SCHUR2 : MEF_SCHUR2_DAGGER;
  pl.lps = Ls;
  pl.block = g.block; pl.gx = g.gx; pl.gy = g.gy;
  pl.flags = (zero ? DPF_ZERO : 0) | (n_active > 1 ? DPF_BATCH : 0) | (f32 ? DPF_F32 : 0) | (kernel == DEK_HOPS_INV5 && rmix ? MEPF_RMIX : 0);
  pl.lds = kernel == DEK_SCHUR2 ? 0 : 2 * DWF_BLOCK_MAX * (f32 ? 16 : 32);
  pl.nk = n_active;
  pl.status = QMG_SUCCESS;
  pl.par_first = par_first;
  pl.par_count = par_count;
  return pl;
}
inline DwfEoPlan dwf_eo_plan(int dtype, int Lx, int Ly, int Ls, int kernel, unsigned pieces, int n_active, int inplace) {
  return dw_eo_plan(dtype, Lx, Ly, Ls, kernel, DEK_SCHUR2, pieces, n_active, inplace, false, true);
}

// ---- what the entries of both operators do around the plan ----
// what every entry checks before the plan is asked
inline int dw_eo_valid(int dtype, const qmg_stencil_desc* d, int Ls, int nrhs, size_t vec_stride) {
  if (!d || d->nc != 2 * Ls) return QMG_ERR_INVALID;
  return dwf_entry_check(dtype, d->Lx, d->Ly, Ls, nrhs, vec_stride);
}
// a plan that launches nothing and ends the entry with its status
inline bool dw_eo_refused(const DwEoPlan& pl) { return pl.family == DEF_UNSUPPORTED || pl.family == DEF_INVALID; }
// the `need` mask of a kernel-0 or kernel-1 request for the coefficients: bit p set when the site-local block of parity p is inverted
inline unsigned dw_eo_need(const DwEoPlan& pl) { return pl.family == DEF_NOTHING ? 0u : (pl.par_count == 2 ? 3u : 1u << pl.par_first); }

// ---- the site-local block A_p = d_p - (shift along s) + m (wall), d_p = 3 w + shift +- eo_shift, and what its inverse needs ----
//   sigma 0:  g_s = sum_{s' <= s} d^-(s-s'+1) h_s',   y_s = g_s - q d^-(s+1) g_{Ls-1},   q = m / (1 + m d^-Ls);   sigma 1: mirrored in s
struct DwfEoCoef {
  double d[2][2];                     // d_p (re, im)
  double q[2][2];                     // m / (1 + m d_p^-Ls)
  double pw[2][DWF_LS_MAX + 1][2];    // d_p^-k, k = 0 .. Ls
};
// need: bit p set when A_p is inverted or applied.  QMG_SUCCESS, or the refusal the entry points document.
inline int dwf_eo_coef(const qmg_stencil_desc* d, int Ls, double mr, double mi, double w, unsigned need, DwfEoCoef* out) {
  typedef std::complex<double> C;
  const double all[] = {mr, mi, w, d->shift[0], d->shift[1], d->eo_shift[0], d->eo_shift[1], d->dof_shift[0], d->dof_shift[1]};
  for (double v : all)
    if (!std::isfinite(v)) return QMG_ERR_INVALID;
  if (d->dof_shift[0] != 0.0 || d->dof_shift[1] != 0.0) return QMG_ERR_UNSUPPORTED;   // the diagonal is no longer constant along s
  const C m(mr, mi);
  DwfEoCoef c = {};
  for (int p = 0; p < 2; p++) {
    const double sg = p ? -1.0 : 1.0;
    const C dp(3.0 * w + d->shift[0] + sg * d->eo_shift[0], d->shift[1] + sg * d->eo_shift[1]);
    c.d[p][0] = dp.real(); c.d[p][1] = dp.imag();
    if (!((need >> p) & 1u)) continue;
    if (!(std::abs(dp) > 1.0)) return QMG_ERR_UNSUPPORTED;   // outside the domain-wall regime: the scan's powers would grow
    const C inv = 1.0 / dp;
    C pk(1.0, 0.0);
    for (int k = 0; k <= Ls; k++) { c.pw[p][k][0] = pk.real(); c.pw[p][k][1] = pk.imag(); pk *= inv; }
    const C den = 1.0 + m * C(c.pw[p][Ls][0], c.pw[p][Ls][1]);
    if (den == C(0.0, 0.0)) return QMG_ERR_INVALID;
    const C q = m / den;
    if (!std::isfinite(q.real()) || !std::isfinite(q.imag())) return QMG_ERR_INVALID;
    c.q[p][0] = q.real(); c.q[p][1] = q.imag();
  }
  *out = c;
  return QMG_SUCCESS;
}

}  // namespace qmg

#endif
