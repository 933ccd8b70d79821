// hmc_staggered.hpp -- hybrid Monte Carlo for the Schwinger model with staggered fermions: two tastes (HMC) or one (rooted RHMC), or none,
// with even-odd preconditioned pseudofermions; leapfrog molecular dynamics, everything on the device (csrc/qmg_hmc.hip).  Not in the
// reference.  The surface is SchwingerHMC's (hmc.hpp), the trajectory, the leapfrog and their rules are HmcCore's (hmc_core.hpp); the independent
// statement is tests/stag_hmc_numpy.py.
//
//   D = m + H,  H psi(x) = -1/2 sum_mu eta_mu(x) [U_mu(x) psi(x+mu) - conj(U_mu(x-mu)) psi(x-mu)]   (Staggered2D; eta_x = 1, eta_y = (-1)^x)
// H is anti-Hermitian and connects the parities, so A = D^dag D = m^2 - H^2 is block diagonal, A_ee = m^2 - D_eo D_oe is
// Staggered2D::apply_eo_prec_M, det A_ee = det D (two tastes in two dimensions) and the spectrum of A_ee lies in [m^2, m^2 + 4].
//
// Two tastes:  S_f = phi_e^dag A_ee^-1 phi_e,  phi_e = (D^dag eta)_e = m eta_e - (H eta)_e for a full-lattice eta ~ exp(-eta^dag eta)
//   (Staggered2D::prepare_b);  X_e = A_ee^-1 phi_e by CG over half the volume from a ZERO guess.
// Force:  W = X_e (+) (H X_e)_o (Staggered2D::hop_even_to_odd),  dS_f/dtheta_mu(x) = eta_mu(x) eps(x) Im[U_mu(x) conj(W(x)) W(x+mu)],
//   eps(x) = (-1)^(x+y); the kick is ONE kernel (qmg_hmc_momentum_update_staggered).
// One taste:  S_pf = phi_e^dag r(A_ee) phi_e,  r = zolotarev_inv_sqrt(degree, m, sqrt(m^2 + 4)) -- the interval is known, the caller supplies
//   none.  One multi-shift CG on A_ee with the shifts mu_j^2 gives X_j, W_j = X_j (+) (H X_j)_o, S_pf = c0 (phi^dag phi + sum_j rho_j Re<phi, X_j>),
//   and the kick pi -= dt (Fg + c0 sum_j rho_j F(W_j)) is the same ONE kernel.
// Heatbath of one taste: A_ee has no Hermitian square root on the even sites, so the draw is on the full lattice.  K = i H is Hermitian,
//   A + nu^2 = (K + i nu')(K - i nu'), nu' = sqrt(m^2 + nu^2) (and mu' likewise), and
//   B = c0^(-1/2) prod_j (K + i mu'_j)(K + i nu'_j)^-1 = c0^(-1/2) [1 + sum_j i s'_j (K - i nu'_j)(K^2 + nu'_j^2)^-1],  B B^dag = r(A)^-1,
//   s'_j = (mu'_j - nu'_j) prod_{l != j} (mu'_l - nu'_j) / (nu'_l - nu'_j).  Since A is block diagonal, the even half of B eta is distributed
//   as exp(-phi_e^dag r(A_ee) phi_e).  With Z_j = (-H^2 + nu'_j^2)^-1 eta (one multi-shift CG on Staggered2D::apply_minus_hop_sq):
//   B eta = c0^(-1/2) [eta - H (sum_j s'_j Z_j) + sum_j s'_j nu'_j Z_j].
// There is no reweighting for the rational approximation: the sampled weight is det r(A_ee)^-1, within (1 +- delta)^(Lx Ly / 2) of det D^(1/2).
#ifndef QMG_HMC_STAGGERED_HPP
#define QMG_HMC_STAGGERED_HPP

#include <cmath>

#include "hmc.hpp"

class StaggeredSchwingerHMC : public HmcCore {
  Lattice2D lat_fermion;
  complex<double>*phi, *W, *eta, *tmp1, *tmp2;   // the fermion vectors are full-lattice; phi and the solutions use their even halves
  Staggered2D* op;
  size_t half;
  std::vector<double> nup2, nup, sp;         // one taste, heatbath: nu'_j^2, nu'_j, s'_j (the W_j per pole are HmcCore's sols)

  bool has_fermions() const { return n_tastes != 0; }
  void operator_takes_links() { op->update_links(gauge); }
  // the operator takes the current links; W = X_e (+) (H X_e)_o; returns S_f = Re <phi, X_e>
  double solve_for_force(complex<double>* phi_in, HmcResult& r) {
    if (n_tastes == 1) return solve_poles(phi_in, r);
    op->update_links(gauge);
    zero_vector(W, cv);
    const inversion_info inv = solver(W, phi_in, (int)half, cg_max_iter, cg_eps, apply_eo_staggered_2D_M, (void*)op);
    r.cg_iterations += inv.iter;
    if (!inv.success) r.cg_converged = false;
    op->hop_even_to_odd(W);
    return dot(phi_in, W, half).real();
  }
  // one taste: the operator takes the current links; W_j = X_j (+) (H X_j)_o, X_j = (A_ee + mu_j^2)^-1 phi; returns S_pf
  double solve_poles(complex<double>* phi_in, HmcResult& r) {
    op->update_links(gauge);
    solve_shifts(phi_in, rat.mu2, r);
    double s = norm2sq(phi_in, half);
    for (int j = 0; j < rat.n; j++) {
      s += rat.rho[j] * dot(phi_in, sols[j], half).real();
      op->hop_even_to_odd(sols[j]);
    }
    return rat.c0 * s;
  }
  void kick(double* p, double dt, double beta_g) {
    const void* one[1] = {W};
    const double unit[1] = {1.0};
    const int n = n_tastes == 1 ? rat.n : (n_tastes ? 1 : 0);
    qmg::ok(qmg_hmc_momentum_update_staggered(p, gauge, n_tastes == 1 ? (const void* const*)sols.data() : one, n_tastes == 1 ? pole_weights.data() : unit, n,
                                              lat_gauge.get_dim_mu(0), lat_gauge.get_dim_mu(1), beta_g, dt, n_tastes ? 0u : (unsigned)QMG_HMC_GAUGE_ONLY, qmg::current_stream()),
            "qmg_hmc_momentum_update_staggered");
  }

  // eta on the full lattice: variance 1/2 per real component, from stream 1 of the trajectory
  complex<double>* draw_pseudofermion(unsigned long long traj, HmcResult& hb) {
    gaussian(eta, cv, qmg_hmc_stream_seed(rng.seed, traj, 1));
    cax(std::sqrt(0.5), eta, cv);
    hb = heatbath(phi, eta);
    return phi;
  }

 public:
  double mass;
  int n_tastes;

  // phase_field: DEVICE double[2 Lx Ly], evolved in place.  n_tastes: 0 (pure gauge), 2, or 1 (rooted RHMC, r of degree rhmc_degree in 1 .. 16 on
  // the exact interval [mass^2, mass^2 + 4]).  cg_eps is the tolerance of the CG, for one taste of every shift of the multi-shift CG.
  StaggeredSchwingerHMC(double* phase_field, int Lx, int Ly, double beta, double mass, int n_tastes, double tau, int n_steps, double cg_eps, int cg_max_iter,
                        HeatbathRng& generator, int rhmc_degree = 8)
      : HmcCore("StaggeredSchwingerHMC", "taste", phase_field, Lx, Ly, beta, tau, n_steps, cg_eps, cg_max_iter, generator), lat_fermion(Lx, Ly, 1), phi(0), W(0), eta(0),
        tmp1(0), tmp2(0), op(0), mass(mass), n_tastes(n_tastes) {
    cv = (size_t)lat_fermion.get_size_cv();
    half = cv / 2;
    if (!admit(n_tastes == 0 || n_tastes == 1 || n_tastes == 2)) return;
    if (!(mass > 0.0)) { std::cout << "[QMG-ERROR]: StaggeredSchwingerHMC needs mass > 0.\n"; return; }
    if (n_tastes == 1) {
      rat = qmg::zolotarev_inv_sqrt(rhmc_degree, mass, std::sqrt(mass * mass + 4.0));
      if (!rat.ok) { std::cout << "[QMG-ERROR]: StaggeredSchwingerHMC: one taste needs 1 <= rhmc_degree <= 16.\n"; return; }
      std::vector<double> mup(rat.n);
      nup2.resize(rat.n); nup.resize(rat.n); sp.resize(rat.n);
      for (int j = 0; j < rat.n; j++) {
        pole_weights.push_back(rat.c0 * rat.rho[j]);
        nup2[j] = mass * mass + rat.nu2[j]; nup[j] = std::sqrt(nup2[j]); mup[j] = std::sqrt(mass * mass + rat.mu2[j]);
      }
      for (int j = 0; j < rat.n; j++) {
        double s = 1.0;
        for (int l = 0; l < rat.n; l++) {
          s *= mup[l] - nup[j];
          if (l != j) s /= nup[l] - nup[j];
        }
        sp[j] = s;
      }
    }
    if (allocate_core() && n_tastes) {
      phi = allocate_vector<complex<double>>(cv); W = allocate_vector<complex<double>>(cv); eta = allocate_vector<complex<double>>(cv);
      tmp1 = allocate_vector<complex<double>>(cv); tmp2 = allocate_vector<complex<double>>(cv);
      good = phi && W && eta && tmp1 && tmp2;
      for (int j = 0; j < rat.n; j++) {
        sols.push_back(allocate_vector<complex<double>>(cv));
        good = good && sols.back();
      }
      if (good) {
        polar_vector(theta, gauge, n_links);
        op = new Staggered2D(&lat_fermion, mass, gauge);
        rat_fn = apply_eo_staggered_2D_M; rat_data = (void*)op; rat_size = half;   // r acts on A_ee
      }
    }
    if (!good) std::cout << "[QMG-ERROR]: StaggeredSchwingerHMC: out of device memory.\n";
  }
  ~StaggeredSchwingerHMC() {
    delete op;
    deallocate_vector(&phi); deallocate_vector(&W); deallocate_vector(&eta); deallocate_vector(&tmp1); deallocate_vector(&tmp2);
  }

  // ---- each takes the object's current phases; pseudofermions are even-site vectors of Lx Ly / 2 components ----
  // One taste: phi_e = (B eta)_e, B B^dag = r(A)^-1 on the full lattice: with eta ~ exp(-eta^dag eta), phi_e ~ exp(-phi_e^dag r(A_ee) phi_e).
  // Two tastes: phi_e = (D^dag eta)_e, distributed as exp(-phi_e^dag A_ee^-1 phi_e).
  // phi_even_out: Lx Ly / 2 components; eta_full: Lx Ly components, unchanged.
  HmcResult heatbath(complex<double>* phi_even_out, complex<double>* eta_full) {
    HmcResult r;
    if (refused(good && n_tastes, "heatbath", "needs an object with fermions", r)) return r;
    polar_vector(theta, gauge, n_links);
    op->update_links(gauge);
    if (n_tastes == 2) {   // phi_e = (D^dag eta)_e = m eta_e - (H eta)_e: no solve
      zero_vector(tmp1, cv);
      op->prepare_b(tmp1, eta_full);
      copy_vector(phi_even_out, tmp1, half);
      return r;
    }
    solve_shifts(eta_full, nup2, cv, Staggered2D::apply_minus_hop_sq, (void*)op, r);   // Z_j
    zero_vector(tmp1, cv);                                                       // sum_j s'_j Z_j
    copy_vector(tmp2, eta_full, cv);                                             // eta + sum_j s'_j nu'_j Z_j
    for (int j = 0; j < rat.n; j++) {
      caxpy(sp[j], sols[j], tmp1, cv);
      caxpy(sp[j] * nup[j], sols[j], tmp2, cv);
    }
    op->apply_hopping(sols[0], tmp1);
    caxpy(-1.0, sols[0], tmp2, half);
    caxy(1.0 / std::sqrt(rat.c0), tmp2, phi_even_out, half);
    return r;
  }
  // S_pf = phi_e^dag r(A_ee) phi_e (one taste) or phi_e^dag A_ee^-1 phi_e (two)
  double pseudofermion_action(complex<double>* pseudofermion_even, HmcResult& r) {
    if (refused(good && n_tastes, "pseudofermion_action", "needs an object with fermions", r)) return 0.0;
    polar_vector(theta, gauge, n_links);
    return solve_for_force(pseudofermion_even, r);
  }
};

#endif
