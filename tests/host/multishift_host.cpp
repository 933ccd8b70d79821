// Host-only driver of qmg::cgm_coefficients (include/qmg/krylov.hpp), the scalar recurrence of the multi-shift CG, on a dense matrix.
//   ./multishift_host in.bin out.bin
// in.bin: int32 n, ns, max_iter; float64 eps; ns float64 shifts; the n x n Hermitian positive definite matrix A as complex128, row-major; b as
// n complex128.  Runs multi-shift CG for (A + shift_s) x_s = b from x_s = 0, anchored on the smallest shift, with the vector updates of
// bcg_m_core written as plain loops and its freezing rule (shift s stops when zeta_s |r| < eps |b|; the run ends when the smallest has).
// out.bin: int32 iterations; then per iteration: uint32 mask of the shifts iterated in it, ns float64 zeta (after the iteration), r as
// n complex128, the ns iterates x_s as n complex128 each.  No GPU call is made.
#define QMG_KRYLOV_HOST_ONLY
#include <complex>
#include <cstdio>
#include <vector>

#include "../../quantum-mg_amd/include/qmg/krylov.hpp"

typedef std::complex<double> cd;

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: multishift_host in.bin out.bin\n"); return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int hdr[3] = {0, 0, 0};
  double eps = 0.0;
  if (std::fread(hdr, sizeof(int), 3, f) != 3 || std::fread(&eps, sizeof(double), 1, f) != 1) return 2;
  const int n = hdr[0], ns = hdr[1], max_iter = hdr[2];
  if (n < 1 || ns < 1 || ns > 16) return 2;
  std::vector<double> shifts(ns);
  std::vector<cd> A((size_t)n * n), b(n);
  if (std::fread(shifts.data(), sizeof(double), ns, f) != (size_t)ns || std::fread(A.data(), sizeof(cd), A.size(), f) != A.size() ||
      std::fread(b.data(), sizeof(cd), n, f) != (size_t)n) return 2;
  std::fclose(f);

  int base = 0;
  for (int s = 1; s < ns; s++) if (shifts[s] < shifts[base]) base = s;
  std::vector<double> dsigma(ns), zeta(ns, 1.0), zeta_prev(ns, 1.0), a(ns), z(ns), c(ns);
  for (int s = 0; s < ns; s++) dsigma[s] = shifts[s] - shifts[base];
  std::vector<std::vector<cd> > x(ns, std::vector<cd>(n, 0.0)), p(ns, b);
  std::vector<cd> r(b), Ap(n);
  double rsq = 0.0;
  for (int i = 0; i < n; i++) rsq += std::norm(b[i]);
  const double bnorm = std::sqrt(rsq);
  double alpha_prev = 1.0, beta_prev = 0.0;
  unsigned live = (ns >= 32) ? 0xFFFFFFFFu : ((1u << ns) - 1u);

  f = std::fopen(argv[2], "wb");
  if (!f) return 2;
  int iters = 0;
  std::fwrite(&iters, sizeof(int), 1, f);
  while (iters < max_iter && ((live >> base) & 1u) && bnorm > 0.0) {
    double pAp = 0.0;
    for (int i = 0; i < n; i++) {
      cd t = shifts[base] * p[base][i];
      for (int j = 0; j < n; j++) t += A[(size_t)i * n + j] * p[base][j];
      Ap[i] = t;
      pAp += (std::conj(p[base][i]) * t).real();
    }
    if (pAp == 0.0) break;
    const double alpha = rsq / pAp;
    double rn = 0.0;
    for (int i = 0; i < n; i++) { r[i] -= alpha * Ap[i]; rn += std::norm(r[i]); }
    const double beta = rn / rsq;
    const unsigned iterated = live;
    qmg::cgm_coefficients(ns, dsigma.data(), live, alpha, beta, alpha_prev, beta_prev, zeta.data(), zeta_prev.data(), a.data(), z.data(), c.data());
    for (int s = 0; s < ns; s++) {
      if (!((live >> s) & 1u)) continue;
      for (int i = 0; i < n; i++) { x[s][i] += a[s] * p[s][i]; p[s][i] = z[s] * r[i] + c[s] * p[s][i]; }
      if (std::fabs(zeta[s]) * std::sqrt(rn) < eps * bnorm) live &= ~(1u << s);
    }
    alpha_prev = alpha; beta_prev = beta; rsq = rn;
    iters++;
    std::fwrite(&iterated, sizeof(unsigned), 1, f);
    std::fwrite(zeta.data(), sizeof(double), ns, f);
    std::fwrite(r.data(), sizeof(cd), n, f);
    for (int s = 0; s < ns; s++) std::fwrite(x[s].data(), sizeof(cd), n, f);
  }
  std::fseek(f, 0, SEEK_SET);
  std::fwrite(&iters, sizeof(int), 1, f);
  std::fclose(f);
  return 0;
}
