// hmc_staggered.hpp -- hybrid Monte Carlo for the Schwinger model with staggered fermions: two tastes (HMC) or one (rooted RHMC), or none,
// with even-odd preconditioned pseudofermions; leapfrog molecular dynamics, everything on the device (csrc/qmg_hmc.hip).  Not in the
// reference.  The surface and the rules are SchwingerHMC's (hmc.hpp); the independent statement is tests/stag_hmc_numpy.py.
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

class StaggeredSchwingerHMC {
  StaggeredSchwingerHMC(StaggeredSchwingerHMC const&);
  StaggeredSchwingerHMC& operator=(StaggeredSchwingerHMC const&);

  Lattice2D lat_gauge, lat_fermion;
  double* theta;                     // the caller's
  double *theta_saved, *pi;
  complex<double>*gauge, *phi, *W, *eta, *tmp1, *tmp2, *draw;   // the fermion vectors are full-lattice; phi and the solutions use their even halves
  Staggered2D* op;
  HeatbathRng& rng;
  bool good;
  size_t n_links, cv, half;
  qmg::ZolotarevInvSqrt rat;                 // one taste: r(A_ee)
  std::vector<complex<double>*> Ws;          // one taste: W_j per pole
  std::vector<double> pole_weights;          // c0 rho_j
  std::vector<double> nup2, nup, sp;         // one taste, heatbath: nu'_j^2, nu'_j, s'_j

  // the operator takes the current links; W = X_e (+) (H X_e)_o; returns S_f = Re <phi, X_e>
  double solve_W(complex<double>* phi_in, HmcResult& r) {
    if (n_tastes == 1) return solve_poles(phi_in, r);
    op->update_links(gauge);
    zero_vector(W, cv);
    const inversion_info inv = solver(W, phi_in, (int)half, cg_max_iter, cg_eps, apply_eo_staggered_2D_M, (void*)op);
    r.cg_iterations += inv.iter;
    if (!inv.success) r.cg_converged = false;
    op->hop_even_to_odd(W);
    return dot(phi_in, W, half).real();
  }
  // out[j] = (A + shifts[j])^-1 b over `size` components by ONE multi-shift CG from zero, A the operator `fn`; counts into r
  void solve_shifts(std::vector<complex<double>*>& out, complex<double>* b, std::vector<double>& shifts, size_t size, matrix_op_cplx fn, HmcResult& r) {
    for (size_t j = 0; j < out.size(); j++) zero_vector(out[j], cv);
    const std::vector<inversion_info> inv = minv_vector_cg_m(out.data(), b, (int)out.size(), (int)size, 1, cg_max_iter, cg_eps, shifts.data(), fn, (void*)op);
    int iters = 0;
    for (size_t j = 0; j < inv.size(); j++) {
      if (inv[j].iter > iters) iters = inv[j].iter;
      if (!inv[j].success) r.cg_converged = false;
    }
    if (inv.size() != out.size()) r.cg_converged = false;
    r.cg_iterations += iters;
  }
  // one taste: the operator takes the current links; W_j = X_j (+) (H X_j)_o, X_j = (A_ee + mu_j^2)^-1 phi; returns S_pf
  double solve_poles(complex<double>* phi_in, HmcResult& r) {
    op->update_links(gauge);
    solve_shifts(Ws, phi_in, rat.mu2, half, apply_eo_staggered_2D_M, r);
    double s = norm2sq(phi_in, half);
    for (int j = 0; j < rat.n; j++) {
      s += rat.rho[j] * dot(phi_in, Ws[j], half).real();
      op->hop_even_to_odd(Ws[j]);
    }
    return rat.c0 * s;
  }
  // out = r(A_ee) in on the operator's links, even halves (Ws is overwritten)
  void rational_on_links(complex<double>* out, complex<double>* in, HmcResult& r) {
    solve_shifts(Ws, in, rat.mu2, half, apply_eo_staggered_2D_M, r);
    if (out != in) copy_vector(out, in, half);
    for (int j = 0; j < rat.n; j++) caxpy(rat.rho[j], Ws[j], out, half);
    cax(rat.c0, out, half);
  }
  double kinetic(double* p) { return 0.5 * norm2sq((complex<double>*)p, n_links / 2); }
  double gauge_action() { return beta * (double)lat_gauge.get_volume() * (1.0 - std::real(get_plaquette_u1(gauge, &lat_gauge))); }
  void kick(double* p, double dt) {
    const void* one[1] = {W};
    const double unit[1] = {1.0};
    const int n = n_tastes == 1 ? rat.n : (n_tastes ? 1 : 0);
    qmg::ok(qmg_hmc_momentum_update_staggered(p, gauge, n_tastes == 1 ? (const void* const*)Ws.data() : one, n_tastes == 1 ? pole_weights.data() : unit, n,
                                              lat_gauge.get_dim_mu(0), lat_gauge.get_dim_mu(1), beta, dt, n_tastes ? 0u : (unsigned)QMG_HMC_GAUGE_ONLY, qmg::current_stream()),
            "qmg_hmc_momentum_update_staggered");
  }

 public:
  double beta, mass, tau, cg_eps;
  int n_tastes, n_steps, cg_max_iter;
  unsigned long long trajectories_done;
  hmc_solver_fn solver;

  // phase_field: DEVICE double[2 Lx Ly], evolved in place.  n_tastes: 0 (pure gauge), 2, or 1 (rooted RHMC, r of degree rhmc_degree in 1 .. 16 on
  // the exact interval [mass^2, mass^2 + 4]).  cg_eps is the tolerance of the CG, for one taste of every shift of the multi-shift CG.
  StaggeredSchwingerHMC(double* phase_field, int Lx, int Ly, double beta, double mass, int n_tastes, double tau, int n_steps, double cg_eps, int cg_max_iter,
                        HeatbathRng& generator, int rhmc_degree = 8)
      : lat_gauge(Lx, Ly, 1), lat_fermion(Lx, Ly, 1), theta(phase_field), theta_saved(0), pi(0), gauge(0), phi(0), W(0), eta(0), tmp1(0), tmp2(0), draw(0), op(0),
        rng(generator), good(false), beta(beta), mass(mass), tau(tau), cg_eps(cg_eps), n_tastes(n_tastes), n_steps(n_steps), cg_max_iter(cg_max_iter),
        trajectories_done(0), solver(hmc_solve_cg) {
    n_links = (size_t)lat_gauge.get_size_gauge();
    cv = (size_t)lat_fermion.get_size_cv();
    half = cv / 2;
    if (qmg::slab().on) { std::cout << "[QMG-ERROR]: StaggeredSchwingerHMC does not run on y-slabs.\n"; return; }
    if (n_tastes != 0 && n_tastes != 1 && n_tastes != 2) { std::cout << "[QMG-ERROR]: StaggeredSchwingerHMC supports 0, 1 or 2 tastes.\n"; return; }
    if (!phase_field || n_steps < 1 || !(tau > 0.0)) { std::cout << "[QMG-ERROR]: StaggeredSchwingerHMC needs a phase field, n_steps >= 1 and tau > 0.\n"; return; }
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
    theta_saved = allocate_vector<double>(n_links);
    pi = allocate_vector<double>(n_links);
    gauge = allocate_vector<complex<double>>(n_links);
    draw = allocate_vector<complex<double>>(1);
    good = theta_saved && pi && gauge && draw;
    if (good && n_tastes) {
      phi = allocate_vector<complex<double>>(cv); W = allocate_vector<complex<double>>(cv); eta = allocate_vector<complex<double>>(cv);
      tmp1 = allocate_vector<complex<double>>(cv); tmp2 = allocate_vector<complex<double>>(cv);
      good = phi && W && eta && tmp1 && tmp2;
      for (int j = 0; j < rat.n; j++) {
        Ws.push_back(allocate_vector<complex<double>>(cv));
        good = good && Ws.back();
      }
      if (good) {
        polar_vector(theta, gauge, n_links);
        op = new Staggered2D(&lat_fermion, mass, gauge);
      }
    }
    if (!good) std::cout << "[QMG-ERROR]: StaggeredSchwingerHMC: out of device memory.\n";
  }
  ~StaggeredSchwingerHMC() {
    delete op;
    deallocate_vector(&theta_saved); deallocate_vector(&pi); deallocate_vector(&gauge); deallocate_vector(&draw);
    deallocate_vector(&phi); deallocate_vector(&W); deallocate_vector(&eta); deallocate_vector(&tmp1); deallocate_vector(&tmp2);
    for (size_t j = 0; j < Ws.size(); j++) deallocate_vector(&Ws[j]);
  }
  bool ok() const { return good; }
  complex<double>* links() { return gauge; }   // exp(i theta) as of the last call
  Lattice2D* gauge_lattice() { return &lat_gauge; }

  // ---- each takes the object's current phases; pseudofermions are even-site vectors of Lx Ly / 2 components ----
  const qmg::ZolotarevInvSqrt& rational() const { return rat; }
  // out = r(A_ee) in (out may be in).  Returns the multi-shift CG's count and convergence in an HmcResult.
  HmcResult apply_rational(complex<double>* out, complex<double>* in) {
    HmcResult r;
    if (!good || n_tastes != 1) { std::cout << "[QMG-ERROR]: StaggeredSchwingerHMC::apply_rational needs a one-taste object.\n"; r.cg_converged = false; return r; }
    polar_vector(theta, gauge, n_links);
    op->update_links(gauge);
    rational_on_links(out, in, r);
    return r;
  }
  // One taste: phi_e = (B eta)_e, B B^dag = r(A)^-1 on the full lattice: with eta ~ exp(-eta^dag eta), phi_e ~ exp(-phi_e^dag r(A_ee) phi_e).
  // Two tastes: phi_e = (D^dag eta)_e, distributed as exp(-phi_e^dag A_ee^-1 phi_e).
  // phi_even_out: Lx Ly / 2 components; eta_full: Lx Ly components, unchanged.
  HmcResult heatbath(complex<double>* phi_even_out, complex<double>* eta_full) {
    HmcResult r;
    if (!good || !n_tastes) { std::cout << "[QMG-ERROR]: StaggeredSchwingerHMC::heatbath needs an object with fermions.\n"; r.cg_converged = false; return r; }
    polar_vector(theta, gauge, n_links);
    op->update_links(gauge);
    if (n_tastes == 2) {   // phi_e = (D^dag eta)_e = m eta_e - (H eta)_e: no solve
      zero_vector(tmp1, cv);
      op->prepare_b(tmp1, eta_full);
      copy_vector(phi_even_out, tmp1, half);
      return r;
    }
    solve_shifts(Ws, eta_full, nup2, cv, Staggered2D::apply_minus_hop_sq, r);   // Z_j
    zero_vector(tmp1, cv);                                                       // sum_j s'_j Z_j
    copy_vector(tmp2, eta_full, cv);                                             // eta + sum_j s'_j nu'_j Z_j
    for (int j = 0; j < rat.n; j++) {
      caxpy(sp[j], Ws[j], tmp1, cv);
      caxpy(sp[j] * nup[j], Ws[j], tmp2, cv);
    }
    op->apply_hopping(Ws[0], tmp1);
    caxpy(-1.0, Ws[0], tmp2, half);
    caxy(1.0 / std::sqrt(rat.c0), tmp2, phi_even_out, half);
    return r;
  }
  // S_pf = phi_e^dag r(A_ee) phi_e (one taste) or phi_e^dag A_ee^-1 phi_e (two)
  double pseudofermion_action(complex<double>* pseudofermion_even, HmcResult& r) {
    if (!good || !n_tastes) { std::cout << "[QMG-ERROR]: StaggeredSchwingerHMC::pseudofermion_action needs an object with fermions.\n"; r.cg_converged = false; return 0.0; }
    polar_vector(theta, gauge, n_links);
    return solve_W(pseudofermion_even, r);
  }

  // The deterministic part alone: leapfrog over tau from the object's phases with the momenta `momenta` (DEVICE double[2 Lx Ly], evolved in place)
  // and the pseudofermion `pseudofermion_even` (DEVICE, Lx Ly / 2 components; ignored without tastes).  Fills dH, the CG counts and the
  // observables of the end point.
  HmcResult md_evolve(double* momenta, complex<double>* pseudofermion_even) {
    HmcResult r;
    if (!good) { std::cout << "[QMG-ERROR]: StaggeredSchwingerHMC::md_evolve called on an object that was refused.\n"; r.cg_converged = false; return r; }
    const double dt = tau / n_steps;
    polar_vector(theta, gauge, n_links);
    double sf = n_tastes ? solve_W(pseudofermion_even, r) : 0.0;
    const double h0 = kinetic(momenta) + gauge_action() + sf;
    kick(momenta, 0.5 * dt);
    for (int k = 0; k < n_steps; k++) {
      qmg::ok(qmg_hmc_link_update(theta, gauge, momenta, n_links, dt, qmg::current_stream()), "qmg_hmc_link_update");
      if (n_tastes) sf = solve_W(pseudofermion_even, r);
      kick(momenta, k + 1 < n_steps ? dt : 0.5 * dt);
    }
    r.dH = kinetic(momenta) + gauge_action() + sf - h0;
    r.plaquette = std::real(get_plaquette_u1(gauge, &lat_gauge));
    r.topo = get_topo_u1(gauge, &lat_gauge);
    return r;
  }

  // One HMC trajectory with the Metropolis test; on rejection the phases are the ones it started from.
  HmcResult trajectory() {
    HmcResult r;
    if (!good) { std::cout << "[QMG-ERROR]: StaggeredSchwingerHMC::trajectory called on an object that was refused.\n"; r.cg_converged = false; return r; }
    const unsigned long long traj = trajectories_done++;
    int heatbath_iterations = 0; bool heatbath_converged = true;
    void* st = qmg::current_stream();
    qmg::ok(qmg_memcpy_d2d(theta_saved, theta, sizeof(double) * n_links, st), "qmg_memcpy_d2d");
    qmg::ok(qmg_hmc_momentum_refresh(pi, n_links, rng.seed, traj, st), "qmg_hmc_momentum_refresh");
    if (n_tastes) {   // eta on the full lattice: variance 1/2 per real component
      gaussian(eta, cv, qmg_hmc_stream_seed(rng.seed, traj, 1));
      cax(std::sqrt(0.5), eta, cv);
      const HmcResult hb = heatbath(phi, eta);
      heatbath_iterations = hb.cg_iterations; heatbath_converged = hb.cg_converged;
    }
    r = md_evolve(pi, phi);
    r.cg_iterations += heatbath_iterations; r.cg_converged = r.cg_converged && heatbath_converged;
    // a uniform number from the same generator: the Box-Muller radius of a draw is sqrt(-2 log u), so u = exp(-|z|^2 / 2) in (0, 1]
    gaussian(draw, 1, qmg_hmc_stream_seed(rng.seed, traj, 2));
    const complex<double> z = qmg::get_element(draw, 0);
    const double u = std::exp(-0.5 * std::norm(z));
    r.accepted = r.cg_converged && r.dH == r.dH && u < std::exp(-r.dH);
    if (!r.accepted) {
      qmg::ok(qmg_memcpy_d2d(theta, theta_saved, sizeof(double) * n_links, st), "qmg_memcpy_d2d");
      polar_vector(theta, gauge, n_links);
      r.plaquette = std::real(get_plaquette_u1(gauge, &lat_gauge));
      r.topo = get_topo_u1(gauge, &lat_gauge);
    }
    return r;
  }
};

#endif
