// hmc.hpp -- hybrid Monte Carlo for the Schwinger model: compact U(1) in two dimensions with two degenerate Wilson flavours (or none),
// leapfrog molecular dynamics, everything on the device (csrc/qmg_hmc.hip).  Not in the reference, which only generates quenched fields.
//
//   H = 1/2 sum pi^2 + S_g + S_f,   S_g = beta sum_x (1 - cos P(x)),   S_f = phi^dag (D^dag D)^-1 phi,   phi = D^dag eta, eta ~ exp(-eta^dag eta)
//
// The primary field is the DEVICE phase field theta (double, (mu, eo, y, x) order, U = exp(i theta)) the caller owns; the complex links that
// Wilson2D::update_links and qmg_u1_plaquette consume are kept beside it.  One trajectory: refresh pi, draw phi, leapfrog with half steps of
// the momenta at both ends, dH, Metropolis.  After every link update the operator takes the new links, X = (D^dag D)^-1 phi is solved from a
// ZERO guess (anything else breaks reversibility) and Y = D X is applied; the momentum update is ONE kernel (qmg_hmc_momentum_update).
// Random numbers are functions of (seed, trajectory number) alone (qmg_hmc_stream_seed), whatever was drawn before.
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
#ifndef QMG_HMC_HPP
#define QMG_HMC_HPP

#include <cmath>

#include "krylov.hpp"
#include "operators.hpp"
#include "rational.hpp"
#include "u1.hpp"

struct HmcResult {
  double dH; bool accepted; double plaquette, topo; int cg_iterations; bool cg_converged;
  HmcResult() : dH(0.0), accepted(false), plaquette(0.0), topo(0.0), cg_iterations(0), cg_converged(true) {}
};

// x = A^-1 b for the Hermitian positive definite `op`, x zero on entry.  The molecular dynamics reaches its solver through this pointer
// alone, so that a preconditioned solve can take the place of plain CG.
typedef inversion_info (*hmc_solver_fn)(complex<double>* x, complex<double>* b, int size, int max_iter, double eps, matrix_op_cplx op, void* op_data);
inline inversion_info hmc_solve_cg(complex<double>* x, complex<double>* b, int size, int max_iter, double eps, matrix_op_cplx op, void* op_data) {
  return minv_vector_cg(x, b, size, max_iter, eps, op, op_data);
}

// SchwingerHMC::range_check: ratio = |xi^dag (r Q^2 r - 1) xi| / xi^dag xi for one Gaussian xi, bound = 2 delta + delta^2.  While the spectrum of
// Q^2 lies in [spectrum_lo^2, spectrum_hi^2] the ratio cannot exceed the bound for ANY xi, so ok == false proves that it has left the interval.
struct RhmcRangeCheck {
  double ratio, bound; bool ok, cg_converged;
  RhmcRangeCheck() : ratio(0.0), bound(0.0), ok(false), cg_converged(false) {}
};

class SchwingerHMC {
  SchwingerHMC(SchwingerHMC const&);
  SchwingerHMC& operator=(SchwingerHMC const&);

  Lattice2D lat_gauge, lat_fermion;
  double* theta;                     // the caller's
  double *theta_saved, *pi;
  complex<double>*gauge, *phi, *X, *Y, *tmp1, *tmp2, *draw;
  Wilson2D* op;
  HeatbathRng& rng;
  bool good;
  size_t n_links, cv;
  qmg::ZolotarevInvSqrt rat;                 // one flavour: r(Q^2)
  std::vector<complex<double>*> Xs, Ys;      // one flavour: X_j, Y_j per pole
  std::vector<double> pole_weights;          // c0 rho_j

  static void apply_normal(complex<double>* lhs, complex<double>* rhs, void* self) {   // lhs = gamma5 D gamma5 D rhs = D^dag D rhs
    SchwingerHMC* h = (SchwingerHMC*)self;
    h->op->apply_M_overwrite(h->tmp1, rhs);
    h->op->gamma5(h->tmp2, h->tmp1);
    h->op->apply_M_overwrite(h->tmp1, h->tmp2);
    h->op->gamma5(lhs, h->tmp1);
  }
  // the operator takes the current links; X = (D^dag D)^-1 phi, Y = D X; returns S_f = Re <phi, X>
  double solve_XY(complex<double>* phi_in, HmcResult& r) {
    if (n_flavours == 1) return solve_poles(phi_in, r);
    op->update_links(gauge);
    zero_vector(X, cv);
    const inversion_info inv = solver(X, phi_in, (int)cv, cg_max_iter, cg_eps, apply_normal, (void*)this);
    r.cg_iterations += inv.iter;
    if (!inv.success) r.cg_converged = false;
    op->apply_M_overwrite(Y, X);
    return dot(phi_in, X, cv).real();
  }
  // out[j] = (D^dag D + shifts[j])^-1 b on the operator's links by ONE multi-shift CG from zero; counts into r
  void solve_shifts(std::vector<complex<double>*>& out, complex<double>* b, std::vector<double>& shifts, HmcResult& r) {
    for (size_t j = 0; j < out.size(); j++) zero_vector(out[j], cv);
    const std::vector<inversion_info> inv = minv_vector_cg_m(out.data(), b, (int)out.size(), (int)cv, 1, cg_max_iter, cg_eps, shifts.data(), apply_normal, (void*)this);
    int iters = 0;
    for (size_t j = 0; j < inv.size(); j++) {
      if (inv[j].iter > iters) iters = inv[j].iter;
      if (!inv[j].success) r.cg_converged = false;
    }
    if (inv.size() != out.size()) r.cg_converged = false;
    r.cg_iterations += iters;
  }
  // one flavour: the operator takes the current links; X_j = (D^dag D + mu_j^2)^-1 phi, Y_j = D X_j; returns S_pf
  double solve_poles(complex<double>* phi_in, HmcResult& r) {
    op->update_links(gauge);
    solve_shifts(Xs, phi_in, rat.mu2, r);
    double s = norm2sq(phi_in, cv);
    for (int j = 0; j < rat.n; j++) {
      op->apply_M_overwrite(Ys[j], Xs[j]);
      s += rat.rho[j] * dot(phi_in, Xs[j], cv).real();
    }
    return rat.c0 * s;
  }
  // out = r(Q^2) in on the operator's links (Xs is overwritten)
  void rational_on_links(complex<double>* out, complex<double>* in, HmcResult& r) {
    solve_shifts(Xs, in, rat.mu2, r);
    if (out != in) copy_vector(out, in, cv);
    for (int j = 0; j < rat.n; j++) caxpy(rat.rho[j], Xs[j], out, cv);
    cax(rat.c0, out, cv);
  }
  double kinetic(double* p) { return 0.5 * norm2sq((complex<double>*)p, n_links / 2); }
  double gauge_action() { return beta * (double)lat_gauge.get_volume() * (1.0 - std::real(get_plaquette_u1(gauge, &lat_gauge))); }
  void kick(double* p, double dt) {
    if (n_flavours == 1) {
      qmg::ok(qmg_hmc_momentum_update_poles(p, gauge, (const void* const*)Xs.data(), (const void* const*)Ys.data(), pole_weights.data(), rat.n, lat_gauge.get_dim_mu(0),
                                            lat_gauge.get_dim_mu(1), beta, dt, 0u, qmg::current_stream()), "qmg_hmc_momentum_update_poles");
      return;
    }
    qmg::ok(qmg_hmc_momentum_update(p, gauge, X, Y, lat_gauge.get_dim_mu(0), lat_gauge.get_dim_mu(1), beta, dt, n_flavours ? 0u : (unsigned)QMG_HMC_GAUGE_ONLY,
                                    qmg::current_stream()), "qmg_hmc_momentum_update");
  }

 public:
  double beta, mass, tau, cg_eps;
  int n_flavours, n_steps, cg_max_iter;
  unsigned long long trajectories_done;
  hmc_solver_fn solver;

  // phase_field: DEVICE double[2 Lx Ly], evolved in place.  n_flavours: 0 (pure gauge), 2, or 1 (RHMC), which takes three more arguments: the
  // degree of r (1 .. 16) and the interval [spectrum_lo, spectrum_hi] that holds the spectrum of |Q| = (D^dag D)^(1/2).  spectrum_lo is the
  // caller's; spectrum_hi = 0 takes |2 + mass| + 2, an upper bound since the hopping part of D has norm <= 2.  cg_eps is then the tolerance of
  // every shift of the multi-shift CG.  With degree 8 on eps = (lo/hi)^2 = 1e-3, delta = 1.2e-7: det r^-1 is within (1 +- delta)^(2 Lx Ly) of
  // det D, 2.4e-4 at 32^2 and 6e-5 at 16^2.
  SchwingerHMC(double* phase_field, int Lx, int Ly, double beta, double mass, int n_flavours, double tau, int n_steps, double cg_eps, int cg_max_iter, HeatbathRng& generator,
               int rhmc_degree = 8, double spectrum_lo = 0.0, double spectrum_hi = 0.0)
      : lat_gauge(Lx, Ly, 1), lat_fermion(Lx, Ly, 2), theta(phase_field), theta_saved(0), pi(0), gauge(0), phi(0), X(0), Y(0), tmp1(0), tmp2(0), draw(0), op(0),
        rng(generator), good(false), beta(beta), mass(mass), tau(tau), cg_eps(cg_eps), n_flavours(n_flavours), n_steps(n_steps), cg_max_iter(cg_max_iter),
        trajectories_done(0), solver(hmc_solve_cg) {
    n_links = (size_t)lat_gauge.get_size_gauge();
    cv = (size_t)lat_fermion.get_size_cv();
    if (qmg::slab().on) { std::cout << "[QMG-ERROR]: SchwingerHMC does not run on y-slabs.\n"; return; }
    if (n_flavours != 0 && n_flavours != 1 && n_flavours != 2) { std::cout << "[QMG-ERROR]: SchwingerHMC supports 0, 1 or 2 flavours.\n"; return; }
    if (!phase_field || n_steps < 1 || !(tau > 0.0)) { std::cout << "[QMG-ERROR]: SchwingerHMC needs a phase field, n_steps >= 1 and tau > 0.\n"; return; }
    if (n_flavours == 1) {
      rat = qmg::zolotarev_inv_sqrt(rhmc_degree, spectrum_lo, spectrum_hi != 0.0 ? spectrum_hi : std::fabs(2.0 + mass) + 2.0);
      if (!rat.ok) { std::cout << "[QMG-ERROR]: SchwingerHMC: one flavour needs 1 <= rhmc_degree <= 16 and 0 < spectrum_lo < spectrum_hi.\n"; return; }
      for (int j = 0; j < rat.n; j++) pole_weights.push_back(rat.c0 * rat.rho[j]);
    }
    theta_saved = allocate_vector<double>(n_links);
    pi = allocate_vector<double>(n_links);
    gauge = allocate_vector<complex<double>>(n_links);
    draw = allocate_vector<complex<double>>(1);
    good = theta_saved && pi && gauge && draw;
    if (good && n_flavours) {
      phi = allocate_vector<complex<double>>(cv); X = allocate_vector<complex<double>>(cv); Y = allocate_vector<complex<double>>(cv);
      tmp1 = allocate_vector<complex<double>>(cv); tmp2 = allocate_vector<complex<double>>(cv);
      good = phi && X && Y && tmp1 && tmp2;
      for (int j = 0; j < rat.n; j++) {
        Xs.push_back(allocate_vector<complex<double>>(cv)); Ys.push_back(allocate_vector<complex<double>>(cv));
        good = good && Xs.back() && Ys.back();
      }
      if (good) {
        polar_vector(theta, gauge, n_links);
        op = new Wilson2D(&lat_fermion, mass, gauge);
      }
    }
    if (!good) std::cout << "[QMG-ERROR]: SchwingerHMC: out of device memory.\n";
  }
  ~SchwingerHMC() {
    delete op;
    deallocate_vector(&theta_saved); deallocate_vector(&pi); deallocate_vector(&gauge); deallocate_vector(&draw);
    deallocate_vector(&phi); deallocate_vector(&X); deallocate_vector(&Y); deallocate_vector(&tmp1); deallocate_vector(&tmp2);
    for (size_t j = 0; j < Xs.size(); j++) { deallocate_vector(&Xs[j]); deallocate_vector(&Ys[j]); }
  }
  bool ok() const { return good; }
  complex<double>* links() { return gauge; }   // exp(i theta) as of the last call
  Lattice2D* gauge_lattice() { return &lat_gauge; }

  // ---- one flavour only; each takes the object's current phases ----
  const qmg::ZolotarevInvSqrt& rational() const { return rat; }
  // out = r(Q^2) in (DEVICE spinors; out may be in).  Returns the multi-shift CG's count and convergence in an HmcResult.
  HmcResult apply_rational(complex<double>* out, complex<double>* in) {
    HmcResult r;
    if (!good || n_flavours != 1) { std::cout << "[QMG-ERROR]: SchwingerHMC::apply_rational needs a one-flavour object.\n"; r.cg_converged = false; return r; }
    polar_vector(theta, gauge, n_links);
    op->update_links(gauge);
    rational_on_links(out, in, r);
    return r;
  }
  // phi = B eta, B B^dag = r(Q^2)^-1 (DEVICE spinors, phi_out must not be eta): with eta ~ exp(-eta^dag eta), phi ~ exp(-phi^dag r(Q^2) phi)
  HmcResult heatbath(complex<double>* phi_out, complex<double>* eta) {
    HmcResult r;
    if (!good || n_flavours != 1) { std::cout << "[QMG-ERROR]: SchwingerHMC::heatbath needs a one-flavour object.\n"; r.cg_converged = false; return r; }
    polar_vector(theta, gauge, n_links);
    op->update_links(gauge);
    solve_shifts(Xs, eta, rat.nu2, r);                      // Z_j
    zero_vector(Y, cv);                                      // sum_j i s_j Z_j
    copy_vector(phi_out, eta, cv);                           // eta + sum_j s_j nu_j Z_j
    for (int j = 0; j < rat.n; j++) {
      caxpy(complex<double>(0.0, rat.s[j]), Xs[j], Y, cv);
      caxpy(rat.s[j] * std::sqrt(rat.nu2[j]), Xs[j], phi_out, cv);
    }
    op->apply_M_overwrite(X, Y);
    op->gamma5(Y, X);                                        // Q = gamma5 D
    cxpy(Y, phi_out, cv);
    cax(1.0 / std::sqrt(rat.c0), phi_out, cv);
    return r;
  }
  // S_pf = phi^dag r(Q^2) phi
  double pseudofermion_action(complex<double>* pseudofermion, HmcResult& r) {
    if (!good || n_flavours != 1) { std::cout << "[QMG-ERROR]: SchwingerHMC::pseudofermion_action needs a one-flavour object.\n"; r.cg_converged = false; return 0.0; }
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
    op->update_links(gauge);
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

  // The deterministic part alone: leapfrog over tau from the object's phases with the momenta `momenta` (DEVICE double[2 Lx Ly], evolved in place)
  // and the pseudofermion `pseudofermion` (DEVICE spinor; ignored without flavours).  Fills dH, the CG counts and the observables of the end point.
  HmcResult md_evolve(double* momenta, complex<double>* pseudofermion) {
    HmcResult r;
    if (!good) { std::cout << "[QMG-ERROR]: SchwingerHMC::md_evolve called on an object that was refused.\n"; r.cg_converged = false; return r; }
    const double dt = tau / n_steps;
    polar_vector(theta, gauge, n_links);
    double sf = n_flavours ? solve_XY(pseudofermion, r) : 0.0;
    const double h0 = kinetic(momenta) + gauge_action() + sf;
    kick(momenta, 0.5 * dt);
    for (int k = 0; k < n_steps; k++) {
      qmg::ok(qmg_hmc_link_update(theta, gauge, momenta, n_links, dt, qmg::current_stream()), "qmg_hmc_link_update");
      if (n_flavours) sf = solve_XY(pseudofermion, r);
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
    if (!good) { std::cout << "[QMG-ERROR]: SchwingerHMC::trajectory called on an object that was refused.\n"; r.cg_converged = false; return r; }
    const unsigned long long traj = trajectories_done++;
    int heatbath_iterations = 0; bool heatbath_converged = true;
    void* st = qmg::current_stream();
    qmg::ok(qmg_memcpy_d2d(theta_saved, theta, sizeof(double) * n_links, st), "qmg_memcpy_d2d");
    qmg::ok(qmg_hmc_momentum_refresh(pi, n_links, rng.seed, traj, st), "qmg_hmc_momentum_refresh");
    if (n_flavours == 1) {   // eta: variance 1/2 per real component; phi = B eta on the current links
      gaussian(tmp1, cv, qmg_hmc_stream_seed(rng.seed, traj, 1));
      cax(std::sqrt(0.5), tmp1, cv);
      copy_vector(Ys[0], tmp1, cv);                          // the solver's operator works in tmp1 and tmp2
      const HmcResult hb = heatbath(phi, Ys[0]);
      heatbath_iterations = hb.cg_iterations; heatbath_converged = hb.cg_converged;
    } else if (n_flavours) {   // eta: variance 1/2 per real component; phi = D^dag eta = gamma5 D gamma5 eta on the current links
      polar_vector(theta, gauge, n_links);
      op->update_links(gauge);
      gaussian(tmp1, cv, qmg_hmc_stream_seed(rng.seed, traj, 1));
      cax(std::sqrt(0.5), tmp1, cv);
      op->gamma5(tmp2, tmp1);
      op->apply_M_overwrite(tmp1, tmp2);
      op->gamma5(phi, tmp1);
    }
    r = md_evolve(pi, phi);
    if (n_flavours == 1) { r.cg_iterations += heatbath_iterations; r.cg_converged = r.cg_converged && heatbath_converged; }
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
