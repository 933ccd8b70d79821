// stout.hpp -- the stout-smeared links of SchwingerHMC (hmc.hpp) and the chain rule of the fermion force through them (csrc/qmg_stout.hip).
//
//   level k+1:  U^(k+1)_mu(x) = U^(k)_mu(x) exp(-i rho (C^T sin P^(k))_mu(x)),   U^(0) the thin links, V = U^(n) the links of the fermion operator
//   force:      F^(n) = sum_j w_j Ff(X_j, Y_j) on V,   F^(k) = J_k F^(k+1),   J_k = 1 - rho C^T diag(cos P^(k)) C,   pi -= dt (beta C^T sin P^(0) + F^(0))
//
// StoutLinks owns the n levels above the thin links and two force fields.  smear() refreshes the levels from the thin links and returns V;
// kick() is qmg_hmc_fermion_force on V, n - 1 calls of qmg_u1_stout_force_level ping-ponging the two force fields down to level 1, and the
// fused qmg_hmc_momentum_update_stout on the thin links, which applies J_0 and the gauge force in one pass.  kick() uses the levels of the last
// smear(): the caller smears after every change of the thin links (SchwingerHMC does, wherever it hands links to its operator).
#ifndef QMG_STOUT_HPP
#define QMG_STOUT_HPP

#include <cmath>

#include "qmg_device.hpp"

class StoutLinks {
  StoutLinks(StoutLinks const&);
  StoutLinks& operator=(StoutLinks const&);
  complex<double>* lev;   // [n_levels][n_links]: level k + 1 at lev + k n_links
  double* F[2];
  size_t n_links;
  int Lx, Ly;

 public:
  const int n_levels;
  const double rho;

  static const int max_levels = 8;
  static bool valid(int n_levels, double rho) { return n_levels >= 0 && n_levels <= max_levels && std::isfinite(rho) && rho >= 0.0; }

  StoutLinks(int Lx, int Ly, int n_levels, double rho) : lev(0), n_links(2 * (size_t)Lx * Ly), Lx(Lx), Ly(Ly), n_levels(n_levels), rho(rho) {
    F[0] = F[1] = 0;
    if (n_levels > 0 && valid(n_levels, rho)) {
      lev = allocate_vector<complex<double>>(n_links * (size_t)n_levels);
      F[0] = allocate_vector<double>(n_links);
      F[1] = allocate_vector<double>(n_links);
    }
  }
  ~StoutLinks() { deallocate_vector(&lev); deallocate_vector(&F[0]); deallocate_vector(&F[1]); }

  bool on() const { return n_levels > 0; }
  bool ok() const { return valid(n_levels, rho) && (n_levels == 0 || (lev && F[0] && F[1])); }
  // the links of level k, 0 <= k <= n_levels, as of the last smear(); level 0 is `gauge`
  complex<double>* level(complex<double>* gauge, int k) { return k == 0 ? gauge : lev + n_links * (size_t)(k - 1); }
  // the levels from the thin links `gauge`; returns the top level (`gauge` itself without levels)
  complex<double>* smear(complex<double>* gauge) {
    if (!on()) return gauge;
    qmg::ok(qmg_u1_stout_smear(lev, gauge, Lx, Ly, rho, n_levels, qmg::current_stream()), "qmg_u1_stout_smear");
    return level(gauge, n_levels);
  }
  // p -= dt (beta C^T sin P^(0) + J_0 .. J_(n-1) sum_j weights[j] Ff(X[j], Y[j])), the bilinear on the top level of the last smear(gauge)
  void kick(double* p, complex<double>* gauge, const void* const* X, const void* const* Y, const double* weights, int n_poles, double beta, double dt) {
    void* st = qmg::current_stream();
    qmg::ok(qmg_hmc_fermion_force(F[0], level(gauge, n_levels), X, Y, weights, n_poles, Lx, Ly, st), "qmg_hmc_fermion_force");
    int src = 0;
    for (int k = n_levels - 1; k >= 1; k--) {
      qmg::ok(qmg_u1_stout_force_level(F[1 - src], F[src], level(gauge, k), Lx, Ly, rho, st), "qmg_u1_stout_force_level");
      src = 1 - src;
    }
    qmg::ok(qmg_hmc_momentum_update_stout(p, gauge, F[src], Lx, Ly, beta, rho, dt, st), "qmg_hmc_momentum_update_stout");
  }
};

#endif
