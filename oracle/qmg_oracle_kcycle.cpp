// qmg_oracle_kcycle.cpp -- CPU ORACLE (test infrastructure) for the K-cycle:
// StatefulMultigridMG::mg_preconditioner (multigrid/stateful_multigrid.h:734-1060) driven by a restarted
// flexible GCR, as tests/n13_wilson_kcycle/wilson_kcycle.cpp:86-122,459-471 and
// tests/n19_wilson_kcycle_precond/wilson_kcycle_precond.cpp:107-318 configure it.  Branches restated:
//   level operator   ORIGINAL, RIGHT_JACOBI or RIGHT_SCHUR (stencil_2d.h:2418-2527), the same on every level
//   smoothers        MR(0.85), or CGNE: MR on A A^dagger, then A^dagger (:845-873, :1023-1056)
//   coarsest solve   restarted GCR on a level operator, or restarted CG on M M^dagger, M^dagger M or their
//                    right-block-Jacobi forms plus normal_shift (:914-1002, shift_function :716-729)
//   hierarchy        n13: Galerkin from the ORIGINAL stencil; n19: Galerkin from the right-block-Jacobi stencil,
//                    each coarse operator with its own right-block-Jacobi variant (coarse.h:120-131)
//
// PARITY UNPINNED for the Krylov drivers: quantum-linalg (minv_vector_gcr_var_precond_restart,
// minv_vector_minres, minv_vector_gcr_restart, minv_vector_cg_restart) is absent and stores no outputs; these are the
// textbook algorithms under the call-site conventions (relative tolerance against ||b||, ops_count = operator
// applications).  What this file pins is the HIP path's K-cycle against an independent CPU statement of
// the same recursion: same hierarchy (the null vectors are INPUTS), same parameters, iteration counts and
// solution compared by tests/test_gpu_kcycle.py.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstring>
#include <vector>

#include "qmg_oracle.h"

typedef std::complex<double> cplx;
typedef std::vector<cplx> cvec;

namespace {

bool is_normal(int t) { return t == QO_MATVEC_M_MDAGGER || t == QO_MATVEC_MDAGGER_M || t == QO_MATVEC_RBJ_M_MDAGGER || t == QO_MATVEC_RBJ_MDAGGER_M; }

struct Level {
  int Lx, Ly, nc;
  long size;
  cvec clover, hopping;          // this level's operator
  cplx shift;
  cvec dclover, dhopping;        // its dagger stencil (build_dagger_stencil, stencil_2d.h:1080-1139)
  cvec cinv, rclover, rhopping;  // its right-block-Jacobi stencil (build_rbjacobi_stencil, :1452-1601)
  cvec rdclover, rdhopping;      // and that stencil's dagger (build_rbj_dagger_stencil, :1989-2060)
  cvec nullv;                    // transfer to the NEXT level: nvec(next nc) x size, block-orthonormalised
  qo_stencil_desc desc(const cvec& cl, const cvec& hop, cplx sh) const {
    qo_stencil_desc d;
    d.Lx = Lx; d.Ly = Ly; d.nc = nc;
    d.clover = cl.empty() ? nullptr : (const double*)cl.data();
    d.hopping = hop.empty() ? nullptr : (const double*)hop.data();
    d.shift[0] = sh.real(); d.shift[1] = sh.imag();
    d.eo_shift[0] = d.eo_shift[1] = d.dof_shift[0] = d.dof_shift[1] = 0.0;
    return d;
  }
  qo_stencil_desc desc() const { return desc(clover, hopping, shift); }
  qo_stencil_desc rb_desc() const { return desc(rclover, rhopping, 0.0); }   // perform_swap_rbjacobi zeroes the shifts (:1604-1639)
  // the stencil of a single-factor operator type
  qo_stencil_desc factor_desc(int t) const {
    switch (t) {
      case QO_MATVEC_DAGGER: return desc(dclover, dhopping, std::conj(shift));
      case QO_MATVEC_RIGHT_JACOBI: return rb_desc();
      case QO_MATVEC_RBJ_DAGGER: return desc(rdclover, rdhopping, 0.0);
      default: return desc();
    }
  }
  long solve_size(int t) const { return t == QO_MATVEC_RIGHT_SCHUR ? size / 2 : size; }
};

struct Params {
  int n_pre, n_post;
  double inner_tol; int inner_max_iter, inner_restart;
  double coarsest_tol; int coarsest_max_iter, coarsest_restart;
  double omega;
  int level_type, coarsest_type, cgne;
  cplx normal_shift;
};

struct MG {
  std::vector<Level> lv;
  Params p;
  std::vector<long> ops;     // operator applications per level
  std::vector<long> iters;   // Krylov iterations per level (as add_iterations_count)
  std::vector<double>* outer_hist = nullptr;     // relative residual after every OUTER (level 0) iteration, if requested
  std::vector<long>* coarsest_hist = nullptr;    // iterations of every coarsest solve, in call order (negative: not converged)
};

double norm2(const cvec& v, long n) { return qo_norm2sq((const double*)v.data(), n); }
cplx cdot(const cvec& a, const cvec& b, long n) { double o[2]; qo_dot((const double*)a.data(), (const double*)b.data(), n, o); return cplx(o[0], o[1]); }
void axpy(cplx a, const cvec& x, cvec& y, long n) { for (long i = 0; i < n; i++) y[i] += a * x[i]; }

void stencil(const qo_stencil_desc& d, cvec& out, const cvec& in, unsigned pieces) { qo_stencil_apply(&d, (double*)out.data(), (const double*)in.data(), pieces); }

// out = A in for an operator type of level l (Stencil2D::apply_M by type, stencil_2d.h:2418-2453); full-length vectors, of which
// the Schur operator reads and writes the even half only.  `shift` is added to a normal operator (shift_function, :724-729).
void apply(MG& mg, int l, int type, cvec& out, const cvec& in, cplx shift = 0.0) {
  const Level& L = mg.lv[l];
  mg.ops[l]++;
  if (type == QO_MATVEC_RIGHT_SCHUR) {   // out_e = in_e - D'_eo D'_oe in_e (apply_M_rbjacobi_schur, :1886-1908)
    const qo_stencil_desc d = L.rb_desc();
    cvec t1(L.size), t2(L.size);
    stencil(d, t1, in, QO_P_OE | QO_P_ZERO);
    stencil(d, t2, t1, QO_P_EO | QO_P_ZERO);
    for (long i = 0; i < L.size / 2; i++) out[i] = in[i] - t2[i];
    return;
  }
  if (is_normal(type)) {   // second (first in): apply_M_M_dagger :1424-1435, _dagger_M :1400-1411, rbjacobi_MMD :2354-2371, _MDM :2282-2299
    const bool rbj = type == QO_MATVEC_RBJ_M_MDAGGER || type == QO_MATVEC_RBJ_MDAGGER_M;
    const int m = rbj ? QO_MATVEC_RIGHT_JACOBI : QO_MATVEC_ORIGINAL, md = rbj ? QO_MATVEC_RBJ_DAGGER : QO_MATVEC_DAGGER;
    const bool mmd = type == QO_MATVEC_M_MDAGGER || type == QO_MATVEC_RBJ_M_MDAGGER;
    cvec t(L.size);
    stencil(L.factor_desc(mmd ? md : m), t, in, QO_P_ALL | QO_P_ZERO);
    stencil(L.factor_desc(mmd ? m : md), out, t, QO_P_ALL | QO_P_ZERO);
    if (shift != 0.0) axpy(shift, in, out, L.size);
    return;
  }
  stencil(L.factor_desc(type), out, in, QO_P_ALL | QO_P_ZERO);
}

void apply_cinv(const Level& L, cvec& out, const cvec& in) {   // apply_M_rbjacobi_cinv (:1848-1866)
  stencil(L.desc(L.cinv, cvec(), 0.0), out, in, QO_P_CLOVER | QO_P_ZERO);
}

// b_prep = prepare_M(b) (:2455-2490)
void prepare(MG& mg, int l, int type, cvec& bp, const cvec& b) {
  const Level& L = mg.lv[l];
  if (type == QO_MATVEC_RIGHT_SCHUR) {   // b_e - D'_eo b_o, zero odd half (prepare_M_rbjacobi_schur, :1912-1928)
    stencil(L.rb_desc(), bp, b, QO_P_EO | QO_P_ZERO);
    for (long i = 0; i < L.size / 2; i++) bp[i] = b[i] - bp[i];
  } else if (type == QO_MATVEC_MDAGGER_M || type == QO_MATVEC_RBJ_MDAGGER_M)   // M^dagger b (:1413-1422, :2301-2318)
    stencil(L.factor_desc(type == QO_MATVEC_MDAGGER_M ? QO_MATVEC_DAGGER : QO_MATVEC_RBJ_DAGGER), bp, b, QO_P_ALL | QO_P_ZERO);
  else bp = b;
}

// x = reconstruct_M(y, b) (:2492-2527)
void reconstruct(MG& mg, int l, int type, cvec& x, const cvec& y, const cvec& b) {
  const Level& L = mg.lv[l];
  const long half = L.size / 2;
  if (type == QO_MATVEC_RIGHT_SCHUR) {   // t_o = b_o - D'_oe y_e ; t_e = y_e ; x = C^-1 t (:1932-1957)
    cvec t(L.size);
    stencil(L.rb_desc(), t, y, QO_P_OE | QO_P_ZERO);
    for (long i = half; i < L.size; i++) t[i] = b[i] - t[i];
    std::copy(y.begin(), y.begin() + half, t.begin());
    apply_cinv(L, x, t);
  } else if (type == QO_MATVEC_RIGHT_JACOBI || type == QO_MATVEC_RBJ_MDAGGER_M) apply_cinv(L, x, y);   // (:1870-1882, :2319-2335)
  else if (type == QO_MATVEC_M_MDAGGER) stencil(L.factor_desc(QO_MATVEC_DAGGER), x, y, QO_P_ALL | QO_P_ZERO);   // (:1437-1446)
  else if (type == QO_MATVEC_RBJ_M_MDAGGER) {   // x = C^-1 M_rbj^dagger y (:2373-2392)
    cvec t(L.size);
    stencil(L.factor_desc(QO_MATVEC_RBJ_DAGGER), t, y, QO_P_ALL | QO_P_ZERO);
    apply_cinv(L, x, t);
  } else x = y;
}

typedef void (*precond_fn)(MG&, int, cvec&, const cvec&);

// minv_vector_minres(x, b, n, iters, tol, omega, op): r = b - A x ; p = A r ; alpha = <p,r>/<p,p> ; x += omega alpha r ; r -= omega alpha p
int minres(MG& mg, int l, int type, cvec& x, const cvec& b, int max_iter, double eps, double omega) {
  const long n = mg.lv[l].solve_size(type);
  cvec r(mg.lv[l].size), p(mg.lv[l].size);
  const double bnorm = std::sqrt(norm2(b, n));
  if (bnorm == 0.0) { std::fill(x.begin(), x.begin() + n, cplx(0.0)); return 0; }   // A x = 0: x = 0 whatever the guess
  apply(mg, l, type, p, x);
  for (long i = 0; i < n; i++) r[i] = b[i] - p[i];
  double rsq = norm2(r, n);
  int k = 0;
  bool conv = (bnorm == 0.0) || (std::sqrt(rsq) < eps * bnorm);
  while (!conv && k < max_iter) {
    apply(mg, l, type, p, r);
    const cplx pr = cdot(p, r, n);
    const double pp = norm2(p, n);
    if (pp == 0.0) break;
    const cplx alpha = omega * pr / pp;
    axpy(alpha, r, x, n);
    axpy(-alpha, p, r, n);
    rsq = norm2(r, n);
    k++;
    if (std::sqrt(rsq) < eps * bnorm) conv = true;
  }
  return k;
}

// restarted flexible GCR (see quantum-mg_amd/include/qmg/krylov.hpp: same algorithm, CPU vectors)
int gcr(MG& mg, int l, int type, cvec& x, const cvec& b, int max_iter, double eps, int restart, precond_fn prec, double* rsq_out) {
  const long n = mg.lv[l].solve_size(type), full = mg.lv[l].size;
  const int basis_max = (restart > 0) ? restart : max_iter;
  cvec r(full), tmp(full);
  std::vector<cvec> Z, W;
  std::vector<double> Wn;
  const double bnorm = std::sqrt(norm2(b, n));
  if (bnorm == 0.0) { std::fill(x.begin(), x.begin() + n, cplx(0.0)); if (rsq_out) *rsq_out = 0.0; return 0; }   // A x = 0: x = 0 whatever the guess
  apply(mg, l, type, tmp, x);
  for (long i = 0; i < n; i++) r[i] = b[i] - tmp[i];
  double rsq = norm2(r, n);
  bool conv = (bnorm == 0.0) || (std::sqrt(rsq) < eps * bnorm);
  int k = 0, kb = 0;
  while (!conv && k < max_iter) {
    if (kb == (int)Z.size()) { Z.push_back(cvec(full)); W.push_back(cvec(full)); Wn.push_back(0.0); }
    cvec& z = Z[kb];
    cvec& w = W[kb];
    if (prec) { std::fill(z.begin(), z.end(), cplx(0.0)); prec(mg, l, z, r); }
    else z = r;
    apply(mg, l, type, w, z);
    if (kb > 0) {
      std::vector<cplx> c(kb);
      for (int i = 0; i < kb; i++) c[i] = cdot(W[i], w, n);       // all dots first (one fused pass on the device)
      for (int i = 0; i < kb; i++) {
        const cplx beta = c[i] / Wn[i];
        axpy(-beta, W[i], w, n);
        axpy(-beta, Z[i], z, n);
      }
    }
    const double ww = norm2(w, n);
    if (ww == 0.0) break;
    Wn[kb] = ww;
    const cplx alpha = cdot(w, r, n) / ww;
    axpy(alpha, z, x, n);
    axpy(-alpha, w, r, n);
    rsq = norm2(r, n);
    k++; kb++;
    if (l == 0 && mg.outer_hist) mg.outer_hist->push_back(std::sqrt(rsq) / bnorm);
    if (std::sqrt(rsq) < eps * bnorm) { conv = true; break; }
    if (kb == basis_max) {
      apply(mg, l, type, tmp, x);
      for (long i = 0; i < n; i++) r[i] = b[i] - tmp[i];
      rsq = norm2(r, n);
      kb = 0;
      if (std::sqrt(rsq) < eps * bnorm) { conv = true; break; }
    }
  }
  if (rsq_out) *rsq_out = rsq;
  return conv ? k : -k - 1;   // negative = not converged
}

// minv_vector_cg_restart: CG cycles of at most `restart` iterations, each from the true residual of the current x; stops on
// success, on a cycle without an iteration or at max_iter.  Hermitian operators only: the normal forms (+ shift).
int cg_restart(MG& mg, int l, int type, cplx shift, cvec& x, const cvec& b, int max_iter, double eps, int restart) {
  const long n = mg.lv[l].solve_size(type), full = mg.lv[l].size;
  cvec r(full), p(full), Ap(full);
  const double bnorm = std::sqrt(norm2(b, n));
  int k = 0;
  bool conv = false;
  if (bnorm == 0.0) { std::fill(x.begin(), x.begin() + n, cplx(0.0)); return 0; }   // A x = 0: x = 0 whatever the guess
  while (k < max_iter) {
    const int chunk = (restart > 0) ? std::min(restart, max_iter - k) : max_iter - k;
    apply(mg, l, type, Ap, x, shift);
    for (long i = 0; i < n; i++) r[i] = b[i] - Ap[i];
    p = r;
    double rsq = norm2(r, n);
    conv = (bnorm == 0.0) || (std::sqrt(rsq) < eps * bnorm);
    int j = 0;
    while (!conv && j < chunk) {
      apply(mg, l, type, Ap, p, shift);
      const double pAp = cdot(p, Ap, n).real();
      if (pAp == 0.0) break;
      const double alpha = rsq / pAp;
      axpy(alpha, p, x, n);
      axpy(-alpha, Ap, r, n);
      const double rn = norm2(r, n);
      j++;
      if (std::sqrt(rn) < eps * bnorm) { conv = true; break; }
      const double beta = rn / rsq;
      rsq = rn;
      for (long i = 0; i < n; i++) p[i] = r[i] + beta * p[i];
    }
    k += j;
    if (conv || j == 0) break;
  }
  return conv ? k : -k - 1;
}

// one smoother application from x = 0: MR on the level operator, or CGNE on ORIGINAL / RIGHT_JACOBI levels: MR on A A^dagger y = b,
// then x = A^dagger y (:847-857, :1032-1042; the reference ignores the CGNE flag on Schur levels)
void smooth(MG& mg, int l, cvec& x, const cvec& b, int iters) {
  const int t = mg.p.level_type;
  if (mg.p.cgne && (t == QO_MATVEC_ORIGINAL || t == QO_MATVEC_RIGHT_JACOBI)) {
    const bool rbj = t == QO_MATVEC_RIGHT_JACOBI;
    cvec y(mg.lv[l].size, cplx(0.0));
    minres(mg, l, rbj ? QO_MATVEC_RBJ_M_MDAGGER : QO_MATVEC_M_MDAGGER, y, b, iters, 1e-15, mg.p.omega);
    apply(mg, l, rbj ? QO_MATVEC_RBJ_DAGGER : QO_MATVEC_DAGGER, x, y);
  } else minres(mg, l, t, x, b, iters, 1e-15, mg.p.omega);
}

// mg_preconditioner (stateful_multigrid.h:734-1060)
void kcycle(MG& mg, int level, cvec& lhs, const cvec& rhs) {
  const int nlev = (int)mg.lv.size();
  Level& F = mg.lv[level];
  const int ft = mg.p.level_type, ct = (level == nlev - 2) ? mg.p.coarsest_type : mg.p.level_type;
  const long fn = F.size, fns = F.solve_size(ft);
  if (nlev == 1) { lhs = rhs; return; }
  Level& Cc = mg.lv[level + 1];
  const long cn = Cc.size;
  cvec Atmp(fn), z1(fn, cplx(0.0)), r1(fn, cplx(0.0));
  // 1. pre-smooth (:845-873)
  if (mg.p.n_pre > 0) {
    smooth(mg, level, z1, rhs, mg.p.n_pre);
    apply(mg, level, ft, Atmp, z1);
    for (long i = 0; i < fns; i++) r1[i] = rhs[i] - Atmp[i];
  } else { std::copy(rhs.begin(), rhs.begin() + fns, r1.begin()); std::copy(rhs.begin(), rhs.begin() + fns, z1.begin()); }
  std::fill(r1.begin() + fns, r1.end(), cplx(0.0));   // (Schur: the odd half of r1 is zero before the restriction)
  // 2. restrict, prepare, coarse solve, reconstruct (:875-1002)
  cvec r_coarse(cn, cplx(0.0)), r_prep(cn, cplx(0.0)), e_coarse(cn, cplx(0.0)), e_rec(cn, cplx(0.0));
  qo_restrict((const double*)F.nullv.data(), Cc.nc, (const double*)r1.data(), (double*)r_coarse.data(), F.Lx, F.Ly, F.nc, Cc.Lx, Cc.Ly, Cc.nc);
  prepare(mg, level + 1, ct, r_prep, r_coarse);
  const double rnorm = std::sqrt(norm2(r_coarse, cn)), rnorm_prep = std::sqrt(norm2(r_prep, cn));
  int it;
  if (level == nlev - 2) {
    const double tol = (rnorm_prep > 0.0) ? mg.p.coarsest_tol * rnorm / rnorm_prep : mg.p.coarsest_tol;
    if (is_normal(ct)) it = cg_restart(mg, level + 1, ct, mg.p.normal_shift, e_coarse, r_prep, mg.p.coarsest_max_iter, tol, mg.p.coarsest_restart);
    else it = gcr(mg, level + 1, ct, e_coarse, r_prep, mg.p.coarsest_max_iter, tol, mg.p.coarsest_restart, nullptr, nullptr);
    if (mg.coarsest_hist) mg.coarsest_hist->push_back(it >= 0 ? it : -(-it - 1));
  } else {
    const double tol = (rnorm_prep > 0.0) ? mg.p.inner_tol * rnorm / rnorm_prep : mg.p.inner_tol;
    it = gcr(mg, level + 1, ct, e_coarse, r_prep, mg.p.inner_max_iter, tol, mg.p.inner_restart, [](MG& m, int l, cvec& o, const cvec& i) { kcycle(m, l, o, i); }, nullptr);
  }
  mg.iters[level + 1] += (it >= 0) ? it : (-it - 1);
  reconstruct(mg, level + 1, ct, e_rec, e_coarse, r_coarse);
  // 3. prolong and correct (:1013-1021)
  cvec z2(fn, cplx(0.0));
  qo_prolong((const double*)F.nullv.data(), Cc.nc, (const double*)e_rec.data(), (double*)z2.data(), F.Lx, F.Ly, F.nc, Cc.Lx, Cc.Ly, Cc.nc);
  if (ct == QO_MATVEC_RIGHT_SCHUR) std::fill(z2.begin() + fn / 2, z2.end(), cplx(0.0));
  for (long i = 0; i < fns; i++) lhs[i] = z1[i] + z2[i];
  // 4. post-smooth (:1023-1056)
  if (mg.p.n_post > 0) {
    apply(mg, level, ft, Atmp, lhs);
    cvec r2(fn, cplx(0.0)), z3(fn, cplx(0.0));
    for (long i = 0; i < fns; i++) r2[i] = rhs[i] - Atmp[i];
    smooth(mg, level, z3, r2, mg.p.n_post);
    for (long i = 0; i < fns; i++) lhs[i] += z3[i];
  }
}

// the variant stencils of a level: dagger on an ORIGINAL hierarchy, right-block-Jacobi (and its dagger) on an n19 one
int build_variants(Level& L, bool rbj) {
  const long cm = (long)L.Lx * L.Ly * L.nc * L.nc;
  if (!rbj) {
    L.dclover.resize(cm); L.dhopping.resize(4 * cm);
    return qo_build_dagger((double*)L.dclover.data(), (double*)L.dhopping.data(), (const double*)L.clover.data(), (const double*)L.hopping.data(), L.Lx, L.Ly, L.nc);
  }
  L.cinv.resize(cm); L.rclover.resize(cm); L.rhopping.resize(4 * cm);
  L.rdclover.resize(cm); L.rdhopping.resize(4 * cm);
  const qo_stencil_desc d = L.desc();
  if (qo_build_rbjacobi((double*)L.cinv.data(), (double*)L.rclover.data(), (double*)L.rhopping.data(), &d)) return -1;
  return qo_build_rbj_dagger(nullptr, (double*)L.rdclover.data(), (double*)L.rdhopping.data(), (const double*)L.cinv.data(),
                             (const double*)L.rclover.data(), (const double*)L.rhopping.data(), L.Lx, L.Ly, L.nc);
}

}  // namespace

extern "C" {

// Wilson K-cycle on an L x L lattice with n_refine 4x4 coarsenings to `coarse_dof` colours per level (see qmg_oracle.h).
// Setup follows the n13 / n19 drivers: TransferMG (two block-ortho passes, transfer.h:160-174), CoarseOperator2D (Galerkin probes of
// the ORIGINAL stencil with its shift copied, or of the right-block-Jacobi stencil, whose shift is 0: coarse.h:120-131); outer restarted
// flexible GCR on the prepared system, reconstructed; true_res = |b - M x| / |b| with the ORIGINAL operator.
int qo_kcycle(const qo_kcycle_params* q, const double* gauge, const double* const* nullvecs, const double* b_, double* x_out_, double* true_res, long* ops,
              long* its, double* hist, int nhist, int* nhist_out, long* chist, int nchist, int* nchist_out) {
  std::vector<double> oh;
  std::vector<long> ch;
  MG mg;
  mg.outer_hist = hist ? &oh : nullptr;
  mg.coarsest_hist = chist ? &ch : nullptr;
  mg.p.n_pre = mg.p.n_post = q->n_smooth;
  mg.p.inner_tol = q->inner_tol; mg.p.inner_max_iter = 1000; mg.p.inner_restart = 32;
  mg.p.coarsest_tol = q->coarsest_tol; mg.p.coarsest_max_iter = 1000; mg.p.coarsest_restart = 32;
  mg.p.omega = 0.85;
  mg.p.level_type = q->level_type; mg.p.coarsest_type = q->coarsest_type; mg.p.cgne = q->cgne;
  mg.p.normal_shift = q->normal_shift;
  if ((q->level_type != QO_MATVEC_ORIGINAL && q->level_type != QO_MATVEC_RIGHT_JACOBI && q->level_type != QO_MATVEC_RIGHT_SCHUR) ||
      !(q->coarsest_type == q->level_type || is_normal(q->coarsest_type)))
    return -100003;
  const bool rbj = q->level_type != QO_MATVEC_ORIGINAL;   // the n19 hierarchy
  if (!rbj && (q->coarsest_type == QO_MATVEC_RBJ_M_MDAGGER || q->coarsest_type == QO_MATVEC_RBJ_MDAGGER_M)) return -100003;
  if (rbj && (q->coarsest_type == QO_MATVEC_M_MDAGGER || q->coarsest_type == QO_MATVEC_MDAGGER_M)) return -100003;
  const int L = q->L, n_refine = q->n_refine, coarse_dof = q->coarse_dof;
  mg.lv.resize(n_refine + 1);
  Level& f = mg.lv[0];
  f.Lx = f.Ly = L; f.nc = 2; f.size = (long)L * L * 2; f.shift = q->mass;
  f.clover.resize((size_t)L * L * 4); f.hopping.resize((size_t)L * L * 16);
  if (qo_wilson_fill((double*)f.clover.data(), (double*)f.hopping.data(), gauge, L, L, 1.0)) return -100000;
  if (build_variants(f, rbj)) return -100004;
  int cl = L;
  for (int i = 1; i <= n_refine; i++) {
    cl /= 4;
    Level& F = mg.lv[i - 1];
    Level& Cc = mg.lv[i];
    Cc.Lx = Cc.Ly = cl; Cc.nc = coarse_dof; Cc.size = (long)cl * cl * coarse_dof; Cc.shift = rbj ? cplx(0.0) : F.shift;
    F.nullv.assign((const cplx*)nullvecs[i - 1], (const cplx*)nullvecs[i - 1] + (size_t)coarse_dof * F.size);
    for (int pass = 0; pass < 2; pass++)
      if (qo_block_orthonormalize((double*)F.nullv.data(), coarse_dof, F.Lx, F.Ly, F.nc, cl, cl, nullptr)) return -100001;
    Cc.clover.resize((size_t)cl * cl * coarse_dof * coarse_dof);
    Cc.hopping.resize(4 * Cc.clover.size());
    const qo_stencil_desc fd = rbj ? F.rb_desc() : F.desc();
    if (qo_coarse_build((double*)Cc.clover.data(), (double*)Cc.hopping.data(), &fd, (const double*)F.nullv.data(), nullptr, cl, cl, coarse_dof)) return -100002;
    if (build_variants(Cc, rbj)) return -100004;
  }
  mg.ops.assign(n_refine + 1, 0);
  mg.iters.assign(n_refine + 1, 0);
  const long n = f.size;
  cvec b((const cplx*)b_, (const cplx*)b_ + n), b_prep(n, cplx(0.0)), y(n, cplx(0.0)), x(n, cplx(0.0));
  prepare(mg, 0, q->level_type, b_prep, b);
  const int it = gcr(mg, 0, q->level_type, y, b_prep, q->max_iter, q->tol, q->restart, [](MG& m, int l, cvec& o, const cvec& i) { kcycle(m, l, o, i); }, nullptr);
  reconstruct(mg, 0, q->level_type, x, y, b);
  cvec Ax(n);
  const qo_stencil_desc d0 = f.desc();
  stencil(d0, Ax, x, QO_P_ALL | QO_P_ZERO);
  *true_res = std::sqrt(qo_diffnorm2sq((const double*)b.data(), (const double*)Ax.data(), n) / norm2(b, n));
  std::memcpy(x_out_, x.data(), sizeof(cplx) * n);
  for (int i = 0; i <= n_refine; i++) { ops[i] = mg.ops[i]; its[i] = mg.iters[i]; }
  int k = 0;
  for (; hist && k < (int)oh.size() && k < nhist; k++) hist[k] = oh[k];
  if (nhist_out) *nhist_out = k;
  k = 0;
  for (; chist && k < (int)ch.size() && k < nchist; k++) chist[k] = ch[k];
  if (nchist_out) *nchist_out = k;
  return it;
}

// the n13 shape: ORIGINAL operator, MR smoothers, restarted-GCR coarsest solve
static qo_kcycle_params n13_params(int L, double mass, int n_refine, int coarse_dof, double tol, int max_iter, int restart, double inner_tol,
                                   double coarsest_tol, int n_smooth) {
  qo_kcycle_params q;
  q.L = L; q.mass = mass; q.n_refine = n_refine; q.coarse_dof = coarse_dof;
  q.tol = tol; q.max_iter = max_iter; q.restart = restart; q.inner_tol = inner_tol; q.coarsest_tol = coarsest_tol; q.n_smooth = n_smooth;
  q.level_type = q.coarsest_type = QO_MATVEC_ORIGINAL; q.cgne = 0; q.normal_shift = 0.0;
  return q;
}

int qo_wilson_kcycle(int L, double mass, int n_refine, int coarse_dof, const double* gauge, const double* const* nullvecs, const double* b_,
                     double tol, int max_iter, int restart, double inner_tol, double coarsest_tol, int n_smooth, double* x_out_,
                     double* true_res, long* ops, long* its) {
  const qo_kcycle_params q = n13_params(L, mass, n_refine, coarse_dof, tol, max_iter, restart, inner_tol, coarsest_tol, n_smooth);
  return qo_kcycle(&q, gauge, nullvecs, b_, x_out_, true_res, ops, its, nullptr, 0, nullptr, nullptr, 0, nullptr);
}

// Same solve, also recording the relative residual after each outer iteration (hist[0..nhist)) and the iteration count of
// each coarsest solve in call order (chist[0..nchist); negative = that solve hit its cap).  Returns as qo_wilson_kcycle;
// *nhist_out / *nchist_out receive the number of entries written.
int qo_wilson_kcycle_history(int L, double mass, int n_refine, int coarse_dof, const double* gauge, const double* const* nullvecs, const double* b_,
                             double tol, int max_iter, int restart, double inner_tol, double coarsest_tol, int n_smooth, double* x_out_,
                             double* true_res, long* ops, long* its, double* hist, int nhist, int* nhist_out, long* chist, int nchist, int* nchist_out) {
  const qo_kcycle_params q = n13_params(L, mass, n_refine, coarse_dof, tol, max_iter, restart, inner_tol, coarsest_tol, n_smooth);
  return qo_kcycle(&q, gauge, nullvecs, b_, x_out_, true_res, ops, its, hist, nhist, nhist_out, chist, nchist, nchist_out);
}

// ---------------------------------------------------------------------------------------------------------------------
// CPU twins of the remaining Krylov drivers the path calls (quantum-linalg, ABSENT: semantics from the call sites, SURVEY
// 2.2; PARITY UNPINNED against the reference, pinned against scipy's independent implementations of the same textbook
// algorithms in tests/test_oracle_krylov.py).  Operator: lhs = M rhs for a stencil descriptor; `op` selects
//   0: M   1: M^dagger M (needs the dagger stencil in `dag`)   -- CG wants a Hermitian positive definite operator.
// Conventions of every solver: x holds the initial guess on entry; stop when sqrt(resSq) < tol * |b|; *iters = iterations
// performed; returns 1 if converged, 0 if not.
//   kind 0: CG                (tests/n02_free_laplace_test/free_laplace.cpp:118; stateful_multigrid.h:915-969)
//   kind 1: BiCGStab-L        (tests/n13_wilson_kcycle/wilson_kcycle.cpp:359), L = param_i; iterations count BiCG steps
//   kind 2: Richardson        (tests/n22_wilson_kcycle_adaptive/wilson_kcycle.cpp:289,664), omega = param_d,
//                             residual checked every param_i iterations
//   kind 3: MR / MinRes       (stateful_multigrid.h:851-860,1037-1046), relaxation omega = param_d
//   kind 4: restarted GCR     (stateful_multigrid.h:915-969), restart = param_i (-1: none)
int qo_krylov_solve(int kind, const qo_stencil_desc* d, const qo_stencil_desc* dag, int op, double* x_, const double* b_, int max_iter, double tol,
                    int param_i, double param_d, int* iters, double* res_sq, double* hist, int nhist) {
  const long n = (long)d->Lx * d->Ly * d->nc;
  cvec x((const cplx*)x_, (const cplx*)x_ + n), b((const cplx*)b_, (const cplx*)b_ + n), tmp(n);
  auto A = [&](cvec& out, const cvec& in) {
    if (op == 0) qo_stencil_apply(d, (double*)out.data(), (const double*)in.data(), QO_P_ALL | QO_P_ZERO);
    else { qo_stencil_apply(d, (double*)tmp.data(), (const double*)in.data(), QO_P_ALL | QO_P_ZERO); qo_stencil_apply(dag, (double*)out.data(), (const double*)tmp.data(), QO_P_ALL | QO_P_ZERO); }
  };
  const double bnorm = std::sqrt(norm2(b, n));
  int k = 0;
  double rsq = 0.0;
  bool conv = false;
  if (bnorm == 0.0) {   // A x = 0: the solution is x = 0 whatever the initial guess was (no iteration, no apply, resSq 0)
    std::memset(x_, 0, sizeof(cplx) * n);
    if (iters) *iters = 0;
    if (res_sq) *res_sq = 0.0;
    return 1;
  }
  auto note = [&](double r2) { if (hist && k - 1 < nhist && k >= 1) hist[k - 1] = std::sqrt(r2) / bnorm; };
  if (kind == 0) {   // CG
    cvec r(n), p(n), Ap(n);
    A(Ap, x);
    for (long i = 0; i < n; i++) r[i] = b[i] - Ap[i];
    p = r;
    rsq = norm2(r, n);
    conv = (bnorm == 0.0) || (std::sqrt(rsq) < tol * bnorm);
    while (!conv && k < max_iter) {
      A(Ap, p);
      const double pAp = cdot(p, Ap, n).real();
      if (pAp == 0.0) break;
      const double alpha = rsq / pAp;
      axpy(alpha, p, x, n);
      axpy(-alpha, Ap, r, n);
      const double rn = norm2(r, n);
      k++;
      note(rn);
      if (std::sqrt(rn) < tol * bnorm) { rsq = rn; conv = true; break; }
      const double beta = rn / rsq;
      rsq = rn;
      for (long i = 0; i < n; i++) p[i] = r[i] + beta * p[i];
    }
  } else if (kind == 1) {   // BiCGStab(L), Sleijpen & Fokkema 1993, Algorithm 3.1
    const int L = param_i;
    std::vector<cvec> r(L + 1, cvec(n)), u(L + 1, cvec(n, cplx(0.0)));
    A(u[0], x);
    for (long i = 0; i < n; i++) r[0][i] = b[i] - u[0][i];
    cvec rt = r[0];
    std::fill(u[0].begin(), u[0].end(), cplx(0.0));
    cplx rho0 = 1.0, alpha = 0.0, omega = 1.0;
    rsq = norm2(r[0], n);
    conv = (bnorm == 0.0) || (std::sqrt(rsq) < tol * bnorm);
    std::vector<cplx> tau((L + 1) * (L + 1)), gam(L + 1), gamp(L + 1), gampp(L + 1);
    std::vector<double> sigma(L + 1);
    bool broke = false;
    while (!conv && k < max_iter && !broke) {
      rho0 = -omega * rho0;
      for (int j = 0; j < L && !broke; j++) {
        const cplx rho1 = cdot(rt, r[j], n);
        if (rho0 == 0.0) { broke = true; break; }
        const cplx beta = alpha * rho1 / rho0;
        rho0 = rho1;
        for (int i = 0; i <= j; i++) for (long q = 0; q < n; q++) u[i][q] = r[i][q] - beta * u[i][q];
        A(u[j + 1], u[j]);
        const cplx g = cdot(rt, u[j + 1], n);
        if (g == 0.0) { broke = true; break; }
        alpha = rho0 / g;
        for (int i = 0; i <= j; i++) axpy(-alpha, u[i + 1], r[i], n);
        A(r[j + 1], r[j]);
        axpy(alpha, u[0], x, n);
        k++;
      }
      if (broke) break;
      for (int j = 1; j <= L && !broke; j++) {
        for (int i = 1; i < j; i++) {
          tau[i * (L + 1) + j] = cdot(r[i], r[j], n) / sigma[i];
          axpy(-tau[i * (L + 1) + j], r[i], r[j], n);
        }
        sigma[j] = norm2(r[j], n);
        if (sigma[j] == 0.0) { broke = true; break; }
        gamp[j] = cdot(r[j], r[0], n) / sigma[j];
      }
      if (broke) break;
      gam[L] = gamp[L];
      omega = gam[L];
      for (int j = L - 1; j >= 1; j--) {
        gam[j] = gamp[j];
        for (int i = j + 1; i <= L; i++) gam[j] -= tau[j * (L + 1) + i] * gam[i];
      }
      for (int j = 1; j < L; j++) {
        gampp[j] = gam[j + 1];
        for (int i = j + 1; i < L; i++) gampp[j] += tau[j * (L + 1) + i] * gam[i + 1];
      }
      axpy(gam[1], r[0], x, n);
      axpy(-gamp[L], r[L], r[0], n);
      axpy(-gam[L], u[L], u[0], n);
      for (int j = 1; j < L; j++) {
        axpy(-gam[j], u[j], u[0], n);
        axpy(gampp[j], r[j], x, n);
        axpy(-gamp[j], r[j], r[0], n);
      }
      rsq = norm2(r[0], n);
      if (hist) for (int q = std::max(0, k - L); q < k && q < nhist; q++) hist[q] = std::sqrt(rsq) / bnorm;
      if (std::sqrt(rsq) < tol * bnorm) conv = true;
    }
  } else if (kind == 2) {   // Richardson: x += omega (b - A x); residual looked at every param_i iterations
    cvec r(n), Ax(n);
    const double omega = param_d;
    const int check = param_i;
    while (k < max_iter) {
      A(Ax, x);
      for (long i = 0; i < n; i++) r[i] = b[i] - Ax[i];
      if (check > 0 && (k % check) == 0) {
        rsq = norm2(r, n);
        if (bnorm == 0.0 || std::sqrt(rsq) < tol * bnorm) { conv = true; break; }
      }
      axpy(omega, r, x, n);
      k++;
    }
    if (!conv) {
      A(Ax, x);
      rsq = qo_diffnorm2sq((const double*)b.data(), (const double*)Ax.data(), n);
      conv = (bnorm == 0.0) || (std::sqrt(rsq) < tol * bnorm);
    }
  } else if (kind == 3) {   // MR(omega)
    cvec r(n), p(n);
    const double omega = param_d;
    A(p, x);
    for (long i = 0; i < n; i++) r[i] = b[i] - p[i];
    rsq = norm2(r, n);
    conv = (bnorm == 0.0) || (std::sqrt(rsq) < tol * bnorm);
    while (!conv && k < max_iter) {
      A(p, r);
      const cplx pr = cdot(p, r, n);
      const double pp = norm2(p, n);
      if (pp == 0.0) break;
      const cplx alpha = omega * pr / pp;
      axpy(alpha, r, x, n);
      axpy(-alpha, p, r, n);
      rsq = norm2(r, n);
      k++;
      note(rsq);
      if (std::sqrt(rsq) < tol * bnorm) conv = true;
    }
  } else if (kind == 4) {   // restarted GCR, unpreconditioned
    const int restart = param_i;
    const int basis_max = (restart > 0) ? restart : max_iter;
    cvec r(n), t(n);
    std::vector<cvec> Z, W;
    std::vector<double> Wn;
    A(t, x);
    for (long i = 0; i < n; i++) r[i] = b[i] - t[i];
    rsq = norm2(r, n);
    conv = (bnorm == 0.0) || (std::sqrt(rsq) < tol * bnorm);
    int kb = 0;
    while (!conv && k < max_iter) {
      if (kb == (int)Z.size()) { Z.push_back(cvec(n)); W.push_back(cvec(n)); Wn.push_back(0.0); }
      Z[kb] = r;
      A(W[kb], Z[kb]);
      for (int i = 0; i < kb; i++) {
        const cplx beta = cdot(W[i], W[kb], n) / Wn[i];
        axpy(-beta, W[i], W[kb], n);
        axpy(-beta, Z[i], Z[kb], n);
      }
      const double ww = norm2(W[kb], n);
      if (ww == 0.0) break;
      Wn[kb] = ww;
      const cplx alpha = cdot(W[kb], r, n) / ww;
      axpy(alpha, Z[kb], x, n);
      axpy(-alpha, W[kb], r, n);
      rsq = norm2(r, n);
      k++; kb++;
      note(rsq);
      if (std::sqrt(rsq) < tol * bnorm) { conv = true; break; }
      if (kb == basis_max) {
        A(t, x);
        for (long i = 0; i < n; i++) r[i] = b[i] - t[i];
        rsq = norm2(r, n);
        kb = 0;
        if (std::sqrt(rsq) < tol * bnorm) { conv = true; break; }
      }
    }
  } else return -1;
  std::memcpy(x_, x.data(), sizeof(cplx) * n);
  if (iters) *iters = k;
  if (res_sq) *res_sq = rsq;
  return conv ? 1 : 0;
}

}  // extern "C"
