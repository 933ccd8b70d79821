// hmc.hpp -- hybrid Monte Carlo for the Schwinger model: compact U(1) in two dimensions with two degenerate Wilson flavours (or none),
// leapfrog molecular dynamics, everything on the device (csrc/qmg_hmc.hip).  Not in the reference, which only generates quenched fields.
//
//   H = 1/2 sum pi^2 + S_g + S_f,   S_g = beta sum_x (1 - cos P(x)),   S_f = phi^dag (D^dag D)^-1 phi,   phi = D^dag eta, eta ~ exp(-eta^dag eta)
//
// The trajectory, the leapfrog and their rules (zero guesses, links before solves, random streams, restoring on rejection) are HmcCore's
// (hmc_core.hpp); this class supplies the fermions.  After every link update the operator takes the new links, X = (D^dag D)^-1 phi is solved
// and Y = D X is applied; the momentum update is ONE kernel (qmg_hmc_momentum_update).
//
// One flavour (n_flavours == 1) is RHMC: the weight det D = det (Q^2)^(1/2), Q = gamma5 D, Q^2 = D^dag D, through the pseudofermion action
//   S_pf = phi^dag r(Q^2) phi,   r(y) = c0 (1 + sum_j rho_j / (y + mu_j^2)) ~ y^(-1/2)  on [spectrum_lo^2, spectrum_hi^2]
// with r Zolotarev's optimal rational function of degree rhmc_degree (rational.hpp).  One multi-shift CG (minv_vector_cg_m on D^dag D with the
// shifts mu_j^2, zero guesses) gives every X_j = (Q^2 + mu_j^2)^-1 phi, Y_j = D X_j, S_pf = c0 (phi^dag phi + sum_j rho_j Re<phi, X_j>), and the
// kick pi -= dt (Fg + c0 sum_j rho_j Ff(X_j, Y_j)) is ONE kernel (qmg_hmc_momentum_update_poles).  The heatbath needs phi^dag r(Q^2) phi =
// eta^dag eta: since Q is Hermitian, Q^2 + mu^2 = (Q + i mu)(Q - i mu), so phi = B eta with
//   B = c0^(-1/2) prod_j (Q + i mu_j)(Q + i nu_j)^-1 = c0^(-1/2) [1 + sum_j i s_j (Q - i nu_j)(Q^2 + nu_j^2)^-1],   B B^dag = r(Q^2)^-1:
// one multi-shift CG for Z_j = (Q^2 + nu_j^2)^-1 eta, then phi = c0^(-1/2) [eta + Q (sum_j i s_j Z_j) + sum_j s_j nu_j Z_j].
// The algorithm samples det r(Q^2)^-1 exactly (the Metropolis test uses the same r); while the spectrum of Q^2 stays inside the interval that
// weight is within (1 +- delta)^(2 Lx Ly) of det D -- there is no reweighting factor here.  range_check() proves it when the spectrum has left.
//
// Stout-smeared fermions (stout_levels > 0; stout.hpp, csrc/qmg_stout.hip): D is D[V], V the stout_levels-fold stout smearing of the links with
// step stout_rho, while S_g stays on the thin links.  Wherever this class hands links to its operator it hands fermion_links(): the thin links
// themselves without levels, otherwise the freshly smeared top level.  The solves and both actions read the same on V; the kick becomes the force
// bilinear on V as a link field, the chain rule down the levels and one fused kernel on the thin links (StoutLinks::kick).  With stout_levels == 0
// none of that code runs.
#ifndef QMG_HMC_HPP
#define QMG_HMC_HPP

#include <cmath>

#include "hmc_core.hpp"
#include "operators.hpp"
#include "stout.hpp"

// SchwingerHMC::range_check: ratio = |xi^dag (r Q^2 r - 1) xi| / xi^dag xi for one Gaussian xi, bound = 2 delta + delta^2.  While the spectrum of
// Q^2 lies in [spectrum_lo^2, spectrum_hi^2] the ratio cannot exceed the bound for ANY xi, so ok == false proves that it has left the interval.
struct RhmcRangeCheck {
  double ratio, bound; bool ok, cg_converged;
  RhmcRangeCheck() : ratio(0.0), bound(0.0), ok(false), cg_converged(false) {}
};

class SchwingerHMC : public HmcCore {
  Lattice2D lat_fermion;
  complex<double>*phi, *X, *Y, *tmp1, *tmp2;
  Wilson2D* op;
  StoutLinks stout;
  std::vector<complex<double>*> Ys;          // one flavour: Y_j per pole (the X_j are HmcCore's sols)

  static void apply_normal(complex<double>* lhs, complex<double>* rhs, void* self) {   // lhs = gamma5 D gamma5 D rhs = D^dag D rhs
    SchwingerHMC* h = (SchwingerHMC*)self;
    h->op->apply_M_overwrite(h->tmp1, rhs);
    h->op->gamma5(h->tmp2, h->tmp1);
    h->op->apply_M_overwrite(h->tmp1, h->tmp2);
    h->op->gamma5(lhs, h->tmp1);
  }
  bool has_fermions() const { return n_flavours != 0; }
  // the links of the fermion operator on the current `gauge`: the thin links, or their freshly smeared top level
  complex<double>* fermion_links() { return stout.smear(gauge); }
  void operator_takes_links() { op->update_links(fermion_links()); }
  // the operator takes the current links; X = (D^dag D)^-1 phi, Y = D X; returns S_f = Re <phi, X>
  double solve_for_force(complex<double>* phi_in, HmcResult& r) {
    if (n_flavours == 1) return solve_poles(phi_in, r);
    op->update_links(fermion_links());
    zero_vector(X, cv);
    const inversion_info inv = solver(X, phi_in, (int)cv, cg_max_iter, cg_eps, apply_normal, (void*)this);
    r.cg_iterations += inv.iter;
    if (!inv.success) r.cg_converged = false;
    op->apply_M_overwrite(Y, X);
    return dot(phi_in, X, cv).real();
  }
  // one flavour: the operator takes the current links; X_j = (D^dag D + mu_j^2)^-1 phi, Y_j = D X_j; returns S_pf
  double solve_poles(complex<double>* phi_in, HmcResult& r) {
    op->update_links(fermion_links());
    solve_shifts(phi_in, rat.mu2, r);
    double s = norm2sq(phi_in, cv);
    for (int j = 0; j < rat.n; j++) {
      op->apply_M_overwrite(Ys[j], sols[j]);
      s += rat.rho[j] * dot(phi_in, sols[j], cv).real();
    }
    return rat.c0 * s;
  }
  void kick(double* p, double dt, double beta_g) {
    if (stout.on() && n_flavours) {   // the levels are those of the last solve_for_force
      const double one = 1.0;
      if (n_flavours == 1) stout.kick(p, gauge, (const void* const*)sols.data(), (const void* const*)Ys.data(), pole_weights.data(), rat.n, beta_g, dt);
      else stout.kick(p, gauge, (const void* const*)&X, (const void* const*)&Y, &one, 1, beta_g, dt);
      return;
    }
    if (n_flavours == 1) {
      qmg::ok(qmg_hmc_momentum_update_poles(p, gauge, (const void* const*)sols.data(), (const void* const*)Ys.data(), pole_weights.data(), rat.n, lat_gauge.get_dim_mu(0),
                                            lat_gauge.get_dim_mu(1), beta_g, dt, 0u, qmg::current_stream()), "qmg_hmc_momentum_update_poles");
      return;
    }
    qmg::ok(qmg_hmc_momentum_update(p, gauge, X, Y, lat_gauge.get_dim_mu(0), lat_gauge.get_dim_mu(1), beta_g, dt, n_flavours ? 0u : (unsigned)QMG_HMC_GAUGE_ONLY,
                                    qmg::current_stream()), "qmg_hmc_momentum_update");
  }
  // eta: variance 1/2 per real component, from stream 1 of the trajectory
  complex<double>* draw_pseudofermion(unsigned long long traj, HmcResult& hb) {
    if (n_flavours == 1) {   // phi = B eta on the current links
      gaussian(tmp1, cv, qmg_hmc_stream_seed(rng.seed, traj, 1));
      cax(std::sqrt(0.5), tmp1, cv);
      copy_vector(Ys[0], tmp1, cv);                          // the solver's operator works in tmp1 and tmp2
      hb = heatbath(phi, Ys[0]);
    } else {   // phi = D^dag eta = gamma5 D gamma5 eta on the current links: no solve, nothing to count
      polar_vector(theta, gauge, n_links);
      op->update_links(fermion_links());
      gaussian(tmp1, cv, qmg_hmc_stream_seed(rng.seed, traj, 1));
      cax(std::sqrt(0.5), tmp1, cv);
      op->gamma5(tmp2, tmp1);
      op->apply_M_overwrite(tmp1, tmp2);
      op->gamma5(phi, tmp1);
    }
    return phi;
  }

 public:
  double mass;
  int n_flavours;

  // phase_field: DEVICE double[2 Lx Ly], evolved in place.  n_flavours: 0 (pure gauge), 2, or 1 (RHMC), which takes three more arguments: the
  // degree of r (1 .. 16) and the interval [spectrum_lo, spectrum_hi] that holds the spectrum of |Q| = (D^dag D)^(1/2).  spectrum_lo is the
  // caller's; spectrum_hi = 0 takes |2 + mass| + 2, an upper bound since the hopping part of D has norm <= 2.  cg_eps is then the tolerance of
  // every shift of the multi-shift CG.  With degree 8 on eps = (lo/hi)^2 = 1e-3, delta = 1.2e-7: det r^-1 is within (1 +- delta)^(2 Lx Ly) of
  // det D, 2.4e-4 at 32^2 and 6e-5 at 16^2.  stout_levels (0 .. 8) and stout_rho (>= 0) put the fermions, of either count, on stout-smeared links; the
  // spectrum is then that of |Q[V]|.  Without fermions the levels are accepted and change nothing.
  SchwingerHMC(double* phase_field, int Lx, int Ly, double beta, double mass, int n_flavours, double tau, int n_steps, double cg_eps, int cg_max_iter, HeatbathRng& generator,
               int rhmc_degree = 8, double spectrum_lo = 0.0, double spectrum_hi = 0.0, int stout_levels = 0, double stout_rho = 0.0)
      : HmcCore("SchwingerHMC", "flavour", phase_field, Lx, Ly, beta, tau, n_steps, cg_eps, cg_max_iter, generator), lat_fermion(Lx, Ly, 2), phi(0), X(0), Y(0), tmp1(0),
        tmp2(0), op(0), stout(Lx, Ly, n_flavours ? stout_levels : 0, stout_rho), mass(mass), n_flavours(n_flavours) {
    cv = (size_t)lat_fermion.get_size_cv();
    rat_fn = apply_normal; rat_data = (void*)this; rat_size = cv;
    if (!admit(n_flavours == 0 || n_flavours == 1 || n_flavours == 2)) return;
    if (!StoutLinks::valid(stout_levels, stout_rho)) {
      std::cout << "[QMG-ERROR]: SchwingerHMC: stout smearing needs 0 <= stout_levels <= " << StoutLinks::max_levels << " and a finite stout_rho >= 0.\n";
      return;
    }
    if (n_flavours == 1) {
      rat = qmg::zolotarev_inv_sqrt(rhmc_degree, spectrum_lo, spectrum_hi != 0.0 ? spectrum_hi : std::fabs(2.0 + mass) + 2.0);
      if (!rat.ok) { std::cout << "[QMG-ERROR]: SchwingerHMC: one flavour needs 1 <= rhmc_degree <= 16 and 0 < spectrum_lo < spectrum_hi.\n"; return; }
      for (int j = 0; j < rat.n; j++) pole_weights.push_back(rat.c0 * rat.rho[j]);
    }
    if (allocate_core() && n_flavours) {
      phi = allocate_vector<complex<double>>(cv); X = allocate_vector<complex<double>>(cv); Y = allocate_vector<complex<double>>(cv);
      tmp1 = allocate_vector<complex<double>>(cv); tmp2 = allocate_vector<complex<double>>(cv);
      good = phi && X && Y && tmp1 && tmp2 && stout.ok();
      for (int j = 0; j < rat.n; j++) {
        sols.push_back(allocate_vector<complex<double>>(cv)); Ys.push_back(allocate_vector<complex<double>>(cv));
        good = good && sols.back() && Ys.back();
      }
      if (good) {
        polar_vector(theta, gauge, n_links);
        op = new Wilson2D(&lat_fermion, mass, fermion_links());
      }
    }
    if (!good) std::cout << "[QMG-ERROR]: SchwingerHMC: out of device memory.\n";
  }
  ~SchwingerHMC() {
    delete op;
    deallocate_vector(&phi); deallocate_vector(&X); deallocate_vector(&Y); deallocate_vector(&tmp1); deallocate_vector(&tmp2);
    for (size_t j = 0; j < Ys.size(); j++) deallocate_vector(&Ys[j]);
  }

  // ---- one flavour only; each takes the object's current phases ----
  // phi = B eta, B B^dag = r(Q^2)^-1 (DEVICE spinors, phi_out must not be eta): with eta ~ exp(-eta^dag eta), phi ~ exp(-phi^dag r(Q^2) phi)
  HmcResult heatbath(complex<double>* phi_out, complex<double>* eta) {
    HmcResult r;
    if (refused(good && n_flavours == 1, "heatbath", one_flavour_object(), r)) return r;
    polar_vector(theta, gauge, n_links);
    op->update_links(fermion_links());
    solve_shifts(eta, rat.nu2, r);                          // Z_j
    zero_vector(Y, cv);                                      // sum_j i s_j Z_j
    copy_vector(phi_out, eta, cv);                           // eta + sum_j s_j nu_j Z_j
    for (int j = 0; j < rat.n; j++) {
      caxpy(complex<double>(0.0, rat.s[j]), sols[j], Y, cv);
      caxpy(rat.s[j] * std::sqrt(rat.nu2[j]), sols[j], phi_out, cv);
    }
    op->apply_M_overwrite(X, Y);
    op->gamma5(Y, X);                                        // Q = gamma5 D
    cxpy(Y, phi_out, cv);
    cax(1.0 / std::sqrt(rat.c0), phi_out, cv);
    return r;
  }
  // S_pf = phi^dag r(Q^2) phi
  double pseudofermion_action(complex<double>* pseudofermion, HmcResult& r) {
    if (refused(good && n_flavours == 1, "pseudofermion_action", one_flavour_object(), r)) return 0.0;
    polar_vector(theta, gauge, n_links);
    return solve_poles(pseudofermion, r);
  }
  // One Gaussian xi (a function of `seed` alone): w = r(Q^2) xi, ratio = | |Q w|^2 - |xi|^2 | / |xi|^2 against 2 delta + delta^2 plus the
  // solver's share, 4 cg_eps spectrum_hi / spectrum_lo: every pole's residual is at most cg_eps |xi|, so w is off by at most cg_eps |xi| r(lo^2)
  // ~ cg_eps |xi| / lo, Q w by hi times that, the quadratic form by twice that times |xi|; and a factor 2 of margin.
  RhmcRangeCheck range_check(unsigned long long seed = 1) {
    RhmcRangeCheck c;
    if (!good || n_flavours != 1) { std::cout << "[QMG-ERROR]: SchwingerHMC::range_check needs a one-flavour object.\n"; return c; }
    HmcResult r;
    polar_vector(theta, gauge, n_links);
    op->update_links(fermion_links());
    gaussian(X, cv, seed);
    const double n2 = norm2sq(X, cv);
    rational_on_links(Y, X, r);
    op->apply_M_overwrite(X, Y);                             // |Q w| = |D w|
    c.ratio = std::fabs(norm2sq(X, cv) - n2) / n2;
    c.bound = 2.0 * rat.delta + rat.delta * rat.delta;
    c.cg_converged = r.cg_converged;
    c.ok = r.cg_converged && c.ratio <= c.bound + 4.0 * cg_eps * rat.rb / rat.ra;
    return c;
  }
};

#endif
