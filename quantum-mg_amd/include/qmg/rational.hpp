// rational.hpp -- Zolotarev's optimal rational approximation of y^(-1/2), the coefficients of one-flavour RHMC (hmc.hpp).  Host arithmetic
// only, no device dependency (tests/host/rhmc_host.cpp compiles this header alone); closed form, no Remez.
//
// For a spectrum in [ra^2, rb^2]: eps = (ra/rb)^2, k^2 = 1 - eps, K = K(k),
//   a_r = cn^2(r K/(2n+1), k) / sn^2(r K/(2n+1), k),  r = 1 .. 2n   (decreasing)
//   r0(y) = A prod_{j=1..n} (y + a_{2j-1}) / (y + a_{2j})  on the scaled variable y in [eps, 1]
// sqrt(y) r0(y) - 1 equioscillates between +-delta at 2n + 2 points of [eps, 1], the first of them eps and the last 1, so the extrema of
// sqrt(y) prod(...) are its two end-point values: A = 2 / (f(eps) + f(1)), delta = |f(1) - f(eps)| / (f(1) + f(eps)).
// Unscaled, with Q^2 the operator:  nu_j^2 = rb^2 a_{2j-1},  mu_j^2 = rb^2 a_{2j},  c0 = A / rb,
//   r(Q^2) = c0 prod_j (Q^2 + nu_j^2)/(Q^2 + mu_j^2) = c0 (1 + sum_j rho_j (Q^2 + mu_j^2)^-1),   rho_j = prod_l (nu_l^2 - mu_j^2) / prod_{l != j} (mu_l^2 - mu_j^2) > 0
// and, for the heatbath (Q Hermitian, so Q^2 + mu^2 = (Q + i mu)(Q - i mu)):
//   prod_j (Q + i mu_j)/(Q + i nu_j) = 1 + sum_j i s_j (Q + i nu_j)^-1,   s_j = prod_l (mu_l - nu_j) / prod_{l != j} (nu_l - nu_j)  (real).
// With the odd and even a_r swapped delta is about 1: the classic mistake.
#ifndef QMG_RATIONAL_HPP
#define QMG_RATIONAL_HPP

#include <cmath>
#include <iostream>
#include <vector>

namespace qmg {

struct ZolotarevInvSqrt {
  int n;
  double ra, rb, c0, delta;
  std::vector<double> mu2, nu2, rho, s;   // poles mu_j^2, zeros nu_j^2, residues rho_j, heatbath residues s_j; j = 0 .. n - 1
  bool ok;
  ZolotarevInvSqrt() : n(0), ra(0.0), rb(0.0), c0(0.0), delta(0.0), ok(false) {}
};

// sn(u, k) and cn(u, k) for the complementary parameter kc2 = 1 - k^2 in (0, 1], and K(k): the arithmetic-geometric mean gives K and the
// scale of the amplitude, the descending Landen recurrence phi_{i-1} = (phi_i + asin(c_i sin(phi_i) / a_i)) / 2 the amplitude itself
// (Abramowitz & Stegun 16.4, 17.6).  u is given as the fraction t of K, u = t K.
inline void jacobi_sn_cn(double t, double kc2, double& sn, double& cn, double& K) {
  const int N = 32;
  double a[N + 1], c[N + 1];
  a[0] = 1.0; c[0] = std::sqrt(1.0 - kc2);
  double b = std::sqrt(kc2);
  int m = 0;
  while (m < N && std::fabs(c[m]) > 1e-17 * a[m]) {
    a[m + 1] = 0.5 * (a[m] + b);
    c[m + 1] = 0.5 * (a[m] - b);
    b = std::sqrt(a[m] * b);
    m++;
  }
  const double pi = 3.14159265358979323846;
  K = pi / (2.0 * a[m]);
  double phi = std::ldexp(a[m] * t * K, m);
  for (int i = m; i > 0; i--) phi = 0.5 * (phi + std::asin(c[i] * std::sin(phi) / a[i]));
  sn = std::sin(phi); cn = std::cos(phi);
}

// The degree-n approximation of y^(-1/2) on [ra^2, rb^2]; n <= 16 (one launch of the pole kernel, one multi-shift CG).  ok = false and a
// [QMG-ERROR] line for ra <= 0, ra >= rb or n outside 1 .. 16.
inline ZolotarevInvSqrt zolotarev_inv_sqrt(int n, double ra, double rb) {
  ZolotarevInvSqrt z;
  if (n < 1 || n > 16 || !(ra > 0.0) || !(ra < rb)) {
    std::cout << "[QMG-ERROR]: zolotarev_inv_sqrt needs 1 <= n <= 16 and 0 < ra < rb (n " << n << ", ra " << ra << ", rb " << rb << ")\n";
    return z;
  }
  z.n = n; z.ra = ra; z.rb = rb;
  const double eps = (ra / rb) * (ra / rb);
  std::vector<double> a(2 * n);
  for (int r = 1; r <= 2 * n; r++) {
    double sn, cn, K;
    jacobi_sn_cn((double)r / (double)(2 * n + 1), eps, sn, cn, K);
    a[r - 1] = (cn * cn) / (sn * sn);
  }
  double f_lo = std::sqrt(eps), f_hi = 1.0;   // sqrt(y) prod_j (y + a_{2j-1}) / (y + a_{2j}) at y = eps and y = 1
  for (int j = 0; j < n; j++) {
    f_lo *= (eps + a[2 * j]) / (eps + a[2 * j + 1]);
    f_hi *= (1.0 + a[2 * j]) / (1.0 + a[2 * j + 1]);
  }
  const double A = 2.0 / (f_lo + f_hi);
  z.delta = std::fabs(f_hi - f_lo) / (f_hi + f_lo);
  z.c0 = A / rb;
  z.mu2.resize(n); z.nu2.resize(n); z.rho.resize(n); z.s.resize(n);
  for (int j = 0; j < n; j++) { z.nu2[j] = rb * rb * a[2 * j]; z.mu2[j] = rb * rb * a[2 * j + 1]; }
  for (int j = 0; j < n; j++) {
    double rho = 1.0, s = 1.0;
    const double nu_j = std::sqrt(z.nu2[j]);
    for (int l = 0; l < n; l++) {
      rho *= z.nu2[l] - z.mu2[j];
      s *= std::sqrt(z.mu2[l]) - nu_j;
      if (l != j) { rho /= z.mu2[l] - z.mu2[j]; s /= std::sqrt(z.nu2[l]) - nu_j; }
    }
    z.rho[j] = rho; z.s[j] = s;
  }
  z.ok = true;
  return z;
}

}  // namespace qmg

#endif
