// eigen.hpp -- extreme eigenpairs of a Hermitian operator on the device, for coarsest-level deflation
// (StatefulMultigridMG::deflate_coarsest; the reference gets them from ARPACK, stateful_multigrid.h:611-712).
//
//   jacobi_eigh        the dense projected problem: cyclic complex Jacobi on the host (m <= a few hundred), deterministic,
//                      eigenvalues ascending, orthonormal eigenvectors.
//   lanczos_extreme    thick-restart Lanczos (Wu & Simon) with full reorthogonalisation: two classical Gram-Schmidt passes per
//                      step against the whole basis (qmg_basis_dot_t / qmg_basis_update_t: one read of the basis per pass), basis
//                      of m = max(3 nev, nev + 16) vectors (ARPACK's ncv = 3 nev, with a floor for small nev), the Ritz vectors
//                      formed with qmg_basis_update_t.  Converged when |beta_m y_{m-1,i}| = |A x_i - theta_i x_i| <= tol |theta_i|
//                      for every wanted pair (ARPACK's criterion).  The operator is a BatchOp applied to a batch of one, the
//                      apply the coarsest CG uses.
#ifndef QMG_EIGEN_HPP
#define QMG_EIGEN_HPP

#include <algorithm>
#include <cmath>
#include <complex>
#include <iostream>
#include <vector>

namespace qmg {

// A (n x n Hermitian, row-major; only its Hermitian part is used, A is destroyed) = Y diag(w) Y^dagger; w ascending, column j of Y
// (Y[i * n + j]) the eigenvector of w[j].  Returns the number of sweeps.
inline int jacobi_eigh(int n, std::vector<std::complex<double> >& A, std::vector<double>& w, std::vector<std::complex<double> >& Y) {
  typedef std::complex<double> cd;
  for (int i = 0; i < n; i++)
    for (int j = i; j < n; j++) {
      const cd h = 0.5 * (A[(size_t)i * n + j] + std::conj(A[(size_t)j * n + i]));
      A[(size_t)i * n + j] = h; A[(size_t)j * n + i] = std::conj(h);
    }
  for (int i = 0; i < n; i++) A[(size_t)i * n + i] = A[(size_t)i * n + i].real();
  Y.assign((size_t)n * n, 0.0);
  for (int i = 0; i < n; i++) Y[(size_t)i * n + i] = 1.0;
  double total = 0.0;
  for (size_t e = 0; e < (size_t)n * n; e++) total += std::norm(A[e]);
  int sweep = 0;
  for (; sweep < 100; sweep++) {
    double off = 0.0;
    for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) if (i != j) off += std::norm(A[(size_t)i * n + j]);
    if (off <= 1e-32 * total || off == 0.0) break;
    for (int p = 0; p < n - 1; p++)
      for (int q = p + 1; q < n; q++) {
        const cd apq = A[(size_t)p * n + q];
        const double r = std::abs(apq);
        if (r == 0.0) continue;
        // D = diag(1, e^{-i phi}) makes a_pq real (= r); then the real rotation of Numerical Recipes (jacobi, 11.1) zeroes it: U = D R
        const cd ph = apq / r;   // e^{i phi}
        const double app = A[(size_t)p * n + p].real(), aqq = A[(size_t)q * n + q].real();
        const double theta = (aqq - app) / (2.0 * r);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        const cd upp = c, upq = s, uqp = -s * std::conj(ph), uqq = c * std::conj(ph);
        for (int i = 0; i < n; i++) {   // A <- A U (columns p, q)
          const cd aip = A[(size_t)i * n + p], aiq = A[(size_t)i * n + q];
          A[(size_t)i * n + p] = aip * upp + aiq * uqp;
          A[(size_t)i * n + q] = aip * upq + aiq * uqq;
        }
        for (int j = 0; j < n; j++) {   // A <- U^dagger A (rows p, q)
          const cd apj = A[(size_t)p * n + j], aqj = A[(size_t)q * n + j];
          A[(size_t)p * n + j] = std::conj(upp) * apj + std::conj(uqp) * aqj;
          A[(size_t)q * n + j] = std::conj(upq) * apj + std::conj(uqq) * aqj;
        }
        A[(size_t)p * n + q] = 0.0; A[(size_t)q * n + p] = 0.0;
        A[(size_t)p * n + p] = A[(size_t)p * n + p].real(); A[(size_t)q * n + q] = A[(size_t)q * n + q].real();
        for (int i = 0; i < n; i++) {   // Y <- Y U
          const cd yip = Y[(size_t)i * n + p], yiq = Y[(size_t)i * n + q];
          Y[(size_t)i * n + p] = yip * upp + yiq * uqp;
          Y[(size_t)i * n + q] = yip * upq + yiq * uqq;
        }
      }
  }
  std::vector<int> order(n);
  for (int i = 0; i < n; i++) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return A[(size_t)a * n + a].real() < A[(size_t)b * n + b].real(); });
  w.resize(n);
  std::vector<cd> Ys((size_t)n * n);
  for (int j = 0; j < n; j++) {
    w[j] = A[(size_t)order[j] * n + order[j]].real();
    for (int i = 0; i < n; i++) Ys[(size_t)i * n + j] = Y[(size_t)i * n + order[j]];
  }
  Y.swap(Ys);
  return sweep;
}

}  // namespace qmg

#ifndef QMG_EIGEN_HOST_ONLY
#include "batch.hpp"

namespace qmg {

// the basis kernels for any number of basis vectors (the C-ABI takes up to 128 per call)
inline std::vector<complex<double> > basis_dot(const complex<double>* V, int nv, size_t N, const complex<double>* b) {
  std::vector<complex<double> > out(nv);
  for (int j0 = 0; j0 < nv; j0 += 128) {
    const int jj = std::min(128, nv - j0);
    std::vector<double> raw(2 * jj);
    ok(qmg_basis_dot_t(QMG_C64, V + (size_t)j0 * N, jj, N, b, N, 1, N, 1u, raw.data(), 0, current_stream()), "qmg_basis_dot_t");
    for (int j = 0; j < jj; j++) out[j0 + j] = complex<double>(raw[2 * j], raw[2 * j + 1]);
  }
  return out;
}
// B_k += sum_j c[k][j] v_j for nrhs <= 16 vectors B_k = B + k N; c[k * nv + j]
inline void basis_update(const std::vector<complex<double> >& c, const complex<double>* V, int nv, size_t N, complex<double>* B, int nrhs) {
  for (int j0 = 0; j0 < nv; j0 += 128) {
    const int jj = std::min(128, nv - j0);
    std::vector<double> raw((size_t)2 * jj * nrhs);
    for (int k = 0; k < nrhs; k++)
      for (int j = 0; j < jj; j++) { raw[((size_t)k * jj + j) * 2] = c[(size_t)k * nv + j0 + j].real(); raw[((size_t)k * jj + j) * 2 + 1] = c[(size_t)k * nv + j0 + j].imag(); }
    ok(qmg_basis_update_t(QMG_C64, raw.data(), 0, V + (size_t)j0 * N, jj, N, B, N, nrhs, N, full_mask(nrhs), current_stream()), "qmg_basis_update_t");
  }
}

struct LanczosStats { int restarts; int applies; bool converged; };

// The nev smallest (largest = false) or largest eigenpairs of the Hermitian operator `op` on vectors of N elements (a Gaussian start
// vector drawn with `seed` on the lattice Lx x Ly x nc).  evals ascending; evecs: nev contiguous device vectors of N elements, unit norm.
inline LanczosStats lanczos_extreme(BatchOp* op, size_t N, int Lx, int Ly, int nc, int nev, bool largest, double tol, int max_restarts, unsigned long long seed,
                                    std::vector<double>& evals, complex<double>* evecs) {
  typedef complex<double> cd;
  LanczosStats stats = {0, 0, false};
  int m = std::max(3 * nev, nev + 16);
  if ((size_t)m > N) m = (int)N;
  const int keep = std::min(m - 1, nev + (m - nev) / 2);
  complex<double>* V = allocate_vector<cd>((size_t)(m + 1) * N);
  complex<double>* W = allocate_vector<cd>((size_t)(m + 1) * N);
  if (!V || !W) { std::cout << "[QMG-ERROR]: out of device memory for the Lanczos basis\n"; deallocate_vector(&V); deallocate_vector(&W); return stats; }
  std::vector<cd> H((size_t)(m + 1) * m, 0.0);   // H[i * m + j]: A v_j = sum_i H[i][j] v_i
  auto vec = [&](complex<double>* base, int j) { return base + (size_t)j * N; };
  // w -= V[0..j) (V[0..j)^dagger w), twice; returns the summed coefficients
  auto cgs2 = [&](int j, complex<double>* w) {
    std::vector<cd> h = basis_dot(V, j, N, w);
    std::vector<cd> mh(j);
    for (int i = 0; i < j; i++) mh[i] = -h[i];
    basis_update(mh, V, j, N, w, 1);
    const std::vector<cd> h2 = basis_dot(V, j, N, w);
    for (int i = 0; i < j; i++) { mh[i] = -h2[i]; h[i] += h2[i]; }
    basis_update(mh, V, j, N, w, 1);
    return h;
  };
  gaussian_lattice(V, Lx, Ly, nc, seed);
  normalize(V, N);
  int k = 0;   // kept Ritz vectors at the start of the current cycle
  std::vector<double> theta;
  std::vector<cd> Y;
  std::vector<int> sel(m);
  double beta_m = 0.0;
  for (;;) {
    for (int j = k; j < m; j++) {
      complex<double>* w = vec(V, j + 1);
      apply_stencil_typed_batch<double>(Batch(w, N, 1), Batch(vec(V, j), N, 1), 1u, (void*)op);
      stats.applies++;
      const std::vector<cd> h = cgs2(j + 1, w);
      for (int i = 0; i <= j; i++) H[(size_t)i * m + j] = h[i];
      double beta = std::sqrt(norm2sq(w, N));
      double scale = 0.0;
      for (int i = 0; i <= j; i++) scale = std::max(scale, std::abs(h[i]));
      if (!(beta > 1e-12 * scale)) {   // an invariant subspace: continue with a random direction orthogonal to the basis
        gaussian_lattice(w, Lx, Ly, nc, seed + 1000003ull * (unsigned long long)(stats.applies + 1));
        cgs2(j + 1, w);
        normalize(w, N);
        beta = 0.0;
      } else cax(1.0 / beta, w, N);
      H[(size_t)(j + 1) * m + j] = beta;
    }
    beta_m = H[(size_t)m * m + (m - 1)].real();
    std::vector<cd> T((size_t)m * m);
    for (int i = 0; i < m; i++) for (int j = 0; j < m; j++) T[(size_t)i * m + j] = H[(size_t)i * m + j];
    jacobi_eigh(m, T, theta, Y);
    for (int i = 0; i < m; i++) sel[i] = largest ? m - 1 - i : i;
    bool conv = true;
    for (int i = 0; i < nev; i++) conv = conv && std::abs(beta_m * Y[(size_t)(m - 1) * m + sel[i]]) <= tol * std::fabs(theta[sel[i]]);
    if (conv || stats.restarts >= max_restarts) { stats.converged = conv; break; }
    stats.restarts++;
    // thick restart: W[0..keep) = V[0..m) Y[:, sel[0..keep)], W[keep] = v_m
    for (int i0 = 0; i0 < keep; i0 += 16) {
      const int nb = std::min(16, keep - i0);
      std::vector<cd> c((size_t)nb * m);
      for (int q = 0; q < nb; q++) for (int j = 0; j < m; j++) c[(size_t)q * m + j] = Y[(size_t)j * m + sel[i0 + q]];
      zero_vector(vec(W, i0), (size_t)nb * N);
      basis_update(c, V, m, N, vec(W, i0), nb);
    }
    copy_vector(vec(W, keep), vec(V, m), N);
    std::swap(V, W);
    std::fill(H.begin(), H.end(), cd(0.0));
    for (int i = 0; i < keep; i++) {
      H[(size_t)i * m + i] = theta[sel[i]];
      H[(size_t)keep * m + i] = beta_m * Y[(size_t)(m - 1) * m + sel[i]];
      H[(size_t)i * m + keep] = std::conj(H[(size_t)keep * m + i]);   // (column `keep` is recomputed by its own step)
    }
    k = keep;
  }
  // the wanted Ritz vectors, ascending
  std::vector<int> want(sel.begin(), sel.begin() + nev);
  std::sort(want.begin(), want.end());
  evals.resize(nev);
  for (int i0 = 0; i0 < nev; i0 += 16) {
    const int nb = std::min(16, nev - i0);
    std::vector<cd> c((size_t)nb * m);
    for (int q = 0; q < nb; q++) for (int j = 0; j < m; j++) c[(size_t)q * m + j] = Y[(size_t)j * m + want[i0 + q]];
    zero_vector(evecs + (size_t)i0 * N, (size_t)nb * N);
    basis_update(c, V, m, N, evecs + (size_t)i0 * N, nb);
  }
  for (int i = 0; i < nev; i++) { evals[i] = theta[want[i]]; normalize(evecs + (size_t)i * N, N); }
  deallocate_vector(&V);
  deallocate_vector(&W);
  return stats;
}

}  // namespace qmg

// StatefulMultigridMG::deflate_coarsest (declared in multigrid.hpp; stateful_multigrid.h:611-699)
inline void StatefulMultigridMG::deflate_coarsest(int num_low, int num_high, bool print_evals) {
  if (!coarsest_solve->deflate) { std::cout << "[QMG-WARNING]: Coarsest level is not set to deflate. Skipping computing eigenvectors.\n"; return; }
  if (qmg::slab().on) { std::cout << "[QMG-ERROR]: Cannot deflate the coarsest operator of a lattice split into y-slabs.\n"; return; }
  const QMGStencilType ct = coarsest_solve->coarsest_stencil_app;
  if (ct != QMG_MATVEC_M_MDAGGER && ct != QMG_MATVEC_MDAGGER_M && ct != QMG_MATVEC_RBJ_M_MDAGGER && ct != QMG_MATVEC_RBJ_MDAGGER_M) {
    std::cout << "[QMG-ERROR]: Cannot deflate coarsest operator unless it's a normal op solve.\n";
    return;
  }
  if (coarsest_deflated != 0 || coarsest_evals != 0 || coarsest_evecs != 0) { std::cout << "[QMG-WARNING]: Coarsest operator space already deflated.\n"; return; }
  if (num_low < 0 || num_high < 0 || num_low + num_high == 0) return;
  const int nev = num_low + num_high;
  Stencil2D* st = get_stencil(get_num_levels() - 1);
  Lattice2D* lat = get_lattice(get_num_levels() - 1);
  const size_t N = (size_t)lat->get_size_cv_l();
  if (nev > 128) { std::cout << "[QMG-ERROR]: Cannot deflate the coarsest operator with more than 128 eigenvectors (" << nev << " requested).\n"; return; }
  if ((size_t)(3 * std::max(num_low, num_high)) > N) {
    std::cout << "[QMG-ERROR]: Cannot deflate the coarsest operator: a basis of " << 3 * std::max(num_low, num_high) << " vectors exceeds its length " << N << ".\n";
    return;
  }
  BatchOp op(st, ct);   // the unshifted operator (get_apply_function(coarsest_stencil_app) in the reference)
  evec_block = allocate_vector<complex<double> >((size_t)nev * N);
  if (!evec_block) return;
  std::vector<double> ev(nev), part;
  deflate_restarts = deflate_applies = 0;
  for (int side = 0; side < 2; side++) {
    const int cnt = side == 0 ? num_low : num_high;
    if (cnt == 0) continue;
    const int off = side == 0 ? 0 : num_low;
    const qmg::LanczosStats s = qmg::lanczos_extreme(&op, N, lat->get_dim_mu(0), lat->get_dim_mu(1), lat->get_nc(), cnt, side == 1, 1e-5, 1000, 0x5eed0000ull + side,
                                                     part, evec_block + (size_t)off * N);
    if (!s.converged) std::cout << "[QMG-WARNING]: Lanczos for the " << (side == 0 ? "lowest " : "highest ") << cnt << " coarsest eigenpairs did not converge in " << s.restarts << " restarts; keeping the best pairs.\n";
    deflate_restarts += s.restarts; deflate_applies += s.applies;
    for (int i = 0; i < cnt; i++) ev[off + i] = part[i];
  }
  // the two runs' vectors are orthogonal only to (residual / gap) ~ 1e-5 of the high eigenvalues: the high ones are orthogonalised against
  // the low ones (two Gram-Schmidt passes), which moves them by that much
  if (num_low > 0 && num_high > 0)
    for (int i = num_low; i < nev; i++) {
      complex<double>* x = evec_block + (size_t)i * N;
      for (int pass = 0; pass < 2; pass++) {
        std::vector<complex<double> > h = qmg::basis_dot(evec_block, num_low, N, x);
        for (size_t q = 0; q < h.size(); q++) h[q] = -h[q];
        qmg::basis_update(h, evec_block, num_low, N, x, 1);
      }
      normalize(x, N);
    }
  coarsest_deflated = (unsigned)nev;
  coarsest_evals = new complex<double>[nev];
  coarsest_evecs = new complex<double>*[nev];
  std::vector<double> inv(nev);
  for (int i = 0; i < nev; i++) { coarsest_evals[i] = complex<double>(ev[i], 0.0); coarsest_evecs[i] = evec_block + (size_t)i * N; inv[i] = 1.0 / ev[i]; }
  inv_lambda_dev = allocate_vector<double>((size_t)nev);
  if (inv_lambda_dev) qmg::upload(inv_lambda_dev, inv.data(), (size_t)nev);
  if (st->narrow[Stencil2D::QMG_NARROW_SHADOW].on) deflation_basis_f32();   // the fp32 K-cycle's shadow hierarchy already exists
  if (print_evals)
    for (int i = 0; i < nev; i++) std::cout << "[QMG-COARSEST-EVALS]: " << i << " " << ev[i] << "\n";
}

// complex<float> copy of the eigenvectors, for the fp32 K-cycle (made on first use)
inline const void* StatefulMultigridMG::deflation_basis_f32() {
  if (!evec_block32 && evec_block) {
    const size_t n = (size_t)coarsest_deflated * (size_t)get_lattice(get_num_levels() - 1)->get_size_cv_l();
    evec_block32 = allocate_vector<complex<float> >(n);
    if (evec_block32) qmg::ok(qmg_convert(evec_block32, QMG_C32, evec_block, QMG_C64, n, qmg::current_stream()), "qmg_convert");
  }
  return evec_block32;
}

#endif  // QMG_EIGEN_HOST_ONLY
#endif
