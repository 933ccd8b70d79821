// qmg_mobius_eo_plan.h -- which launch serves a request to the even-odd Moebius entry points (qmg_mobius_inv5, qmg_mobius_hops_inv5,
// qmg_mobius_schur_apply): mobius_eo_plan, which the launches switch on and qmg_mobius_eo_plan() exports, is dw_eo_plan (qmg_dwf_eo_plan.h, with the
// plan, its families and flags) with a fourth kernel and the table / source arguments; and the twisted-circulant tables those kernels take by
// value (mobius_eo_coef).  Host code only, no HIP call.
#ifndef QMG_MOBIUS_EO_PLAN_H
#define QMG_MOBIUS_EO_PLAN_H

#include <cmath>
#include <complex>

#include "qmg_dwf_eo_plan.h"
#include "qmg_mobius_plan.h"

namespace qmg {

// the `kernel` argument of qmg_mobius_eo_plan()
enum MobiusEoKernel {
  MEK_INV5 = 0,           // lhs_p = scale S rhs_p
  MEK_HOPS_INV5 = 1,      // lhs_p (+)= scale S H_{p,1-p} (R rhs_{1-p})
  MEK_SCHUR2 = 2,         // second stage of M:        lhs_p = A_p x_p + H_{p,1-p} (B t_{1-p})
  MEK_SCHUR2_DAGGER = 3   // second stage of M^dagger: lhs_p = Gamma5 [A'_p Gamma5 x_p + B' (H_{p,1-p} t_{1-p})]
};
// the site matrix S applied to the hop sum (or to the own chunk) through LDS, and the matrix R applied to the hop source on the load
enum MobiusEoTable { MET_ONE = 0, MET_AINV = 1, MET_AINV_B = 2 };
enum MobiusEoSource { MES_ONE = 0, MES_B = 1 };

// pieces, n_active, inplace: dw_eo_plan's.  table: MobiusEoTable (kernel 0: not MET_ONE; kernels 2, 3: ignored); source: MobiusEoSource (kernel 1
// only).  A table or source out of range is INVALID like every refusal dw_eo_plan makes before it looks at the pieces, so it is made here.
inline MobiusEoPlan mobius_eo_plan(int dtype, int Lx, int Ly, int Ls, int kernel, unsigned pieces, int table, int source, int n_active, int inplace) {
  const bool bad = (kernel == MEK_INV5 && table != MET_AINV && table != MET_AINV_B) ||
                   (kernel == MEK_HOPS_INV5 && (table < MET_ONE || table > MET_AINV_B || (source != MES_ONE && source != MES_B)));
  if (bad) return plan_refused<MobiusEoPlan>(QMG_ERR_INVALID, MEF_INVALID, MEF_UNSUPPORTED);
  return dw_eo_plan(dtype, Lx, Ly, Ls, kernel, MEK_SCHUR2_DAGGER, pieces, n_active, inplace, source == MES_B, false);
}

// ---- the site-local blocks as twisted circulants ----
// On sigma 0 L^Ls = -m, so f(L) = sum_{k < Ls} f_k L^k with (L^k h)(s) = h(s-k) for s >= k and -m h(s-k+Ls) below; sigma 1 is the mirror under
// s -> Ls-1-s.  With alpha_p = alpha + shift +- eo_shift (+ even, - odd), A_p = alpha_p + kappa L and r = -kappa / alpha_p:
//   A_p^-1    f_k = r^k / (alpha_p (1 + m r^Ls))
//   A_p^-1 B  g_k = b5 f_k + c5 f_{k-1},  g_0 = b5 f_0 - m c5 f_{Ls-1}
// formed in long double and rounded once to double (and once more to the kernel's scalar where that is float).
struct MobiusEoCoef {
  double al[2][2];                    // alpha_p (re, im)
  double kappa, b5, c5;
  double wk[2], wc[2];                // across the wall: -m kappa and -m c5
  double tab[2][DWF_LS_MAX][2];       // the table of S on parity p: f_k
  double tabw[2][DWF_LS_MAX][2];      // -m f_k
};
// dagger: conj(m) and the conjugated shifts (the primed blocks of M^dagger).  table: MobiusEoTable.  need: bit p set when the table of parity
// p is used.  QMG_SUCCESS, or the refusal the entry points document.
inline int mobius_eo_coef(const qmg_stencil_desc* d, int Ls, double mr, double mi, double w, double M5, double b5, double c5, bool dagger, int table, unsigned need,
                          MobiusEoCoef* out) {
  typedef std::complex<long double> C;
  MobiusCoef mc;
  if (int rc = mobius_coef(mr, mi, w, M5, b5, c5, &mc)) return rc;
  const double sh[] = {d->shift[0], d->shift[1], d->eo_shift[0], d->eo_shift[1], d->dof_shift[0], d->dof_shift[1]};
  for (double v : sh)
    if (!std::isfinite(v)) return QMG_ERR_INVALID;
  if (d->dof_shift[0] != 0.0 || d->dof_shift[1] != 0.0) return QMG_ERR_UNSUPPORTED;   // the diagonal is no longer constant along s
  const long double cj = dagger ? -1.0L : 1.0L;
  const long double dw = 2.0L * (long double)w + (long double)M5;
  const long double al0 = (long double)b5 * dw + 1.0L, ka = (long double)c5 * dw - 1.0L;
  const C m((long double)mr, cj * (long double)mi);
  MobiusEoCoef c = {};
  c.kappa = mc.kappa; c.b5 = b5; c.c5 = c5;
  c.wk[0] = (double)(-m * ka).real(); c.wk[1] = (double)(-m * ka).imag();
  c.wc[0] = (double)(-m * (long double)c5).real(); c.wc[1] = (double)(-m * (long double)c5).imag();
  for (int p = 0; p < 2; p++) {
    const long double sg = p ? -1.0L : 1.0L;
    const C ap(al0 + (long double)d->shift[0] + sg * (long double)d->eo_shift[0], cj * ((long double)d->shift[1] + sg * (long double)d->eo_shift[1]));
    c.al[p][0] = (double)ap.real(); c.al[p][1] = (double)ap.imag();
    if (!((need >> p) & 1u)) continue;
    C f[DWF_LS_MAX] = {};
    if (table == MET_ONE) {
      f[0] = C(1.0L, 0.0L);
    } else {
      if (ap == C(0.0L, 0.0L)) return QMG_ERR_INVALID;
      if (!(std::fabs(ka) < std::abs(ap))) return QMG_ERR_UNSUPPORTED;   // |r| >= 1: the powers of r would not decay
      const C r = -ka / ap;
      C rk(1.0L, 0.0L), pw[DWF_LS_MAX + 1];
      for (int k = 0; k <= Ls; k++) { pw[k] = rk; rk *= r; }
      const C den = ap * (C(1.0L, 0.0L) + m * pw[Ls]);
      if (C(1.0L, 0.0L) + m * pw[Ls] == C(0.0L, 0.0L)) return QMG_ERR_INVALID;
      C a[DWF_LS_MAX];
      for (int k = 0; k < Ls; k++) a[k] = pw[k] / den;
      if (table == MET_AINV) {
        for (int k = 0; k < Ls; k++) f[k] = a[k];
      } else {
        f[0] = (long double)b5 * a[0] - m * (long double)c5 * a[Ls - 1];
        for (int k = 1; k < Ls; k++) f[k] = (long double)b5 * a[k] + (long double)c5 * a[k - 1];
      }
    }
    for (int k = 0; k < Ls; k++) {
      const C fw = -m * f[k];
      c.tab[p][k][0] = (double)f[k].real(); c.tab[p][k][1] = (double)f[k].imag();
      c.tabw[p][k][0] = (double)fw.real(); c.tabw[p][k][1] = (double)fw.imag();
      if (!std::isfinite(c.tab[p][k][0]) || !std::isfinite(c.tab[p][k][1]) || !std::isfinite(c.tabw[p][k][0]) || !std::isfinite(c.tabw[p][k][1]))
        return QMG_ERR_INVALID;
    }
  }
  *out = c;
  return QMG_SUCCESS;
}

}  // namespace qmg

#endif
