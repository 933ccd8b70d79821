// qmg_mobius_plan.h -- which launch serves a request to qmg_mobius_apply_direct: ONE host function (mobius_plan) that the entry point switches
// on and that qmg_mobius_plan() exports, after qmg_dwf_eo_plan.h; and the coefficients of the Moebius operator the kernels and the fill take
// by value (mobius_coef).  Host code only, no HIP call.
#ifndef QMG_MOBIUS_PLAN_H
#define QMG_MOBIUS_PLAN_H

#include <cmath>

#include "qmg_dwf_plan.h"

namespace qmg {

// the `op` argument
enum MobiusOp { MOP_D = 0, MOP_DAGGER = 1 };
// families (the values are part of qmg_mobius_plan()'s output, include/qmg_hip.h)
enum MobiusFamily {
  MF_UNSUPPORTED = 0,   // the entry point returns QMG_ERR_UNSUPPORTED: a piece set the stored stencil serves
  MF_LOAD = 1,          // k_mobius_load<T, ZERO, BATCH>: D, the hop source mixed along s on the load
  MF_NOTHING = 2,       // success with nothing launched
  MF_INVALID = 3,       // the entry point returns QMG_ERR_INVALID
  MF_RESULT = 4         // k_mobius_result<T, ZERO, BATCH>: D^dagger, the hop sum mixed along s in LDS
};
enum { MOBIUS_PLAN_INTS = DW_PLAN_INTS };

// The first MOBIUS_PLAN_INTS members, in this order, are what qmg_mobius_plan() writes (export_dw_plan; the layout of DwEoPlan).
struct MobiusPlan {
  int family;   // MobiusFamily
  int lps;      // lanes per site: Ls
  int block;    // 256 for op 0; Ls * floor(256 / Ls) for op 1, so that the Ls lanes of a site never straddle a block
  int gx, gy;   // gx blocks cover the lps * Lx/2 lanes of a half row; gy = min(2 Ly, 65535) blocks walk the (parity, y) rows
  int flags;    // DPF_ZERO (both parities overwritten) / DPF_BATCH / DPF_F32 (qmg_dwf_plan.h)
  int lds;      // bytes of LDS per block: 0 for op 0, two buffers of one chunk per lane for op 1
  int nk;       // active systems served (all of them, in one launch)
  // ----
  int status;
};

// pieces: QMG_P_CLOVER | QMG_P_HOPPING, with QMG_P_SHIFT_E / _O and QMG_P_ZERO_E / _O optional; n_active: the systems whose mask bit is set
// (0 .. 16); inplace: lhs == rhs
inline MobiusPlan mobius_plan(int dtype, int Lx, int Ly, int Ls, int op, unsigned pieces, int n_active, int inplace) {
  const auto refused = [](int status) { return plan_refused<MobiusPlan>(status, MF_INVALID, MF_UNSUPPORTED); };
  if (!valid_dtype(dtype) || !dwf_dims_ok(Lx, Ly, Ls) || n_active < 0 || n_active > BATCH_MAX) return refused(QMG_ERR_INVALID);
  if (op != MOP_D && op != MOP_DAGGER) return refused(QMG_ERR_INVALID);
  if (n_active == 0 || pieces == 0) return plan_nothing<MobiusPlan>(MF_NOTHING);
  if ((pieces & ~(unsigned)(QMG_P_SHIFT | QMG_P_ZERO)) != (unsigned)(QMG_P_CLOVER | QMG_P_HOPPING)) return refused(QMG_ERR_UNSUPPORTED);
  if (inplace) return refused(QMG_ERR_INVALID);   // every site is read by its neighbours
  const HalfRowGrid g = half_row_grid(Lx, Ls, 2l * Ly, op == MOP_DAGGER);
  const int f32 = dtype == QMG_C32;
  MobiusPlan pl = {};
  pl.family = op == MOP_D ? MF_LOAD : MF_RESULT;
  pl.lps = Ls;
  pl.block = g.block; pl.gx = g.gx; pl.gy = g.gy;
  pl.flags = ((pieces & QMG_P_ZERO) == (unsigned)QMG_P_ZERO ? DPF_ZERO : 0) | (n_active > 1 ? DPF_BATCH : 0) | (f32 ? DPF_F32 : 0);
  pl.lds = op == MOP_D ? 0 : 2 * DWF_BLOCK_MAX * (f32 ? 16 : 32);
  pl.nk = n_active;
  pl.status = QMG_SUCCESS;
  return pl;
}

// D = A + H B:  A = alpha + kappa L,  B = b5 + c5 L,  alpha = b5 d_w + 1,  kappa = c5 d_w - 1,  d_w = 2 w + M5.  alpha and kappa are formed in
// long double and rounded once; -m kappa (the wall entry of A) is a product of each part of m with the real kappa.
struct MobiusCoef {
  double alpha, kappa;
  double wk[2];   // -m kappa (re, im)
};
// QMG_SUCCESS, or QMG_ERR_INVALID for an argument that is not finite
inline int mobius_coef(double mr, double mi, double w, double M5, double b5, double c5, MobiusCoef* out) {
  const double all[] = {mr, mi, w, M5, b5, c5};
  for (double v : all)
    if (!std::isfinite(v)) return QMG_ERR_INVALID;
  const long double dw = 2.0L * (long double)w + (long double)M5;
  const long double al = (long double)b5 * dw + 1.0L, ka = (long double)c5 * dw - 1.0L;
  MobiusCoef c;
  c.alpha = (double)al; c.kappa = (double)ka;
  c.wk[0] = (double)(-(long double)mr * ka); c.wk[1] = (double)(-(long double)mi * ka);
  *out = c;
  return QMG_SUCCESS;
}

}  // namespace qmg

#endif
