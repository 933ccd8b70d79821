// hmc_core.hpp -- the molecular dynamics that every HMC of the Schwinger model here shares: compact U(1) in two dimensions, leapfrog, Metropolis,
// everything on the device (csrc/qmg_hmc.hip).  HmcCore knows the gauge field and nothing of fermions; SchwingerHMC (hmc.hpp, Wilson) and
// StaggeredSchwingerHMC (hmc_staggered.hpp) and DomainWallSchwingerHMC (hmc_dwf.hpp) derive from it and supply the pseudofermion action through
// five hooks.
//
//   H = 1/2 sum pi^2 + S_g + S_f,   S_g = beta sum_x (1 - cos P(x)),   S_f: the derived class's
//
// The primary field is the DEVICE phase field theta (double, (mu, eo, y, x) order, U = exp(i theta)) the caller owns; the complex links that
// the operators' update_links and qmg_u1_plaquette consume are kept beside it.  One trajectory: refresh pi, draw phi, leapfrog with half steps
// of the momenta at both ends, dH, Metropolis.  The rules that make it correct, each stated and kept here alone:
//   * every solve starts from a ZERO guess (anything else breaks reversibility): solve_shifts zeroes its solutions, solve_for_force must;
//   * after every link update the operator takes the new links before anything is solved or applied (the first duty of solve_for_force);
//   * random numbers are functions of (seed, trajectory number, field) alone (qmg_hmc_stream_seed: 0 momenta, 1 pseudofermion noise,
//     2 Metropolis number), whatever was drawn before;
//   * a rejected trajectory restores the phases AND the links, and reports the observables of the restored field;
//   * whenever a hook runs the links are in `gauge`, and that pointer never changes (DwfLinksSchur keeps a copy of it): the inner loop of a
//     two-scale integrator (set_integrator) ping-pongs between `gauge` and a second buffer and always ends in `gauge`.
// A rational pseudofermion action (one flavour, one taste) keeps r, its shifted solutions and the operator r acts on here as well, so that
// the multi-shift solve and its accounting exist once.
#ifndef QMG_HMC_CORE_HPP
#define QMG_HMC_CORE_HPP

#include <cmath>
#include <string>

#include "krylov.hpp"
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

// The molecular-dynamics schemes.  One step of length h, K a kick of the momenta and D a drift of the links:
//   MD_LEAPFROG  K(h/2) D(h) K(h/2)
//   MD_OMELYAN   K(lambda h) D(h/2) K((1 - 2 lambda) h) D(h/2) K(lambda h)      (second-order minimum norm; lambda = 0.1931833275037836)
// Adjacent kicks of consecutive steps are one kick: n steps cost n + 1 force evaluations (leapfrog) or 2 n + 1 (Omelyan).
enum MdScheme { MD_LEAPFROG = 0, MD_OMELYAN = 1 };

// K(first kick) { D K }* of `n` steps of length h with the kicks of consecutive steps merged: calls K(dt) and D(dt) in order.
template <class Kick, class Drift> void md_sequence(MdScheme scheme, double lambda, int n, double h, Kick K, Drift D) {
  if (scheme == MD_LEAPFROG) {
    K(0.5 * h);
    for (int k = 0; k < n; k++) { D(h); K(k + 1 < n ? h : 0.5 * h); }
    return;
  }
  K(lambda * h);
  for (int k = 0; k < n; k++) {
    D(0.5 * h); K((1.0 - 2.0 * lambda) * h);
    D(0.5 * h); K(k + 1 < n ? 2.0 * lambda * h : lambda * h);
  }
}

class HmcCore {
  HmcCore(HmcCore const&);
  HmcCore& operator=(HmcCore const&);

 protected:
  const std::string name, flavour;   // the derived class and what it counts ("flavour", "taste"), for the messages
  Lattice2D lat_gauge;
  double* theta;                     // the caller's
  double *theta_saved, *pi;
  complex<double>*gauge, *draw;
  complex<double>* gauge_other;      // two scales only: the far end of the inner loop's ping-pong; the links are in `gauge` whenever a hook runs
  HeatbathRng& rng;
  bool good;
  size_t n_links, cv;                // cv: components of one of the derived class's fermion vectors
  // a rational action: r, the solutions of its multi-shift solves (cv components each, allocated by the derived class, released here), the
  // weights c0 rho_j of its kick, and the operator r acts on: rat_fn(lhs, rhs, rat_data) on rat_size components
  qmg::ZolotarevInvSqrt rat;
  std::vector<complex<double>*> sols;
  std::vector<double> pole_weights;
  matrix_op_cplx rat_fn;
  void* rat_data;
  size_t rat_size;
  // the integrator (set_integrator): the scheme, the gauge steps inside one drift of the fermion scale (0: one scale) and Omelyan's lambda
  MdScheme md_scheme;
  int md_n_gauge;
  double md_lambda;

  // ---- the hooks of a fermion action ----
  virtual bool has_fermions() const = 0;
  // the operator takes the links in `gauge`
  virtual void operator_takes_links() = 0;
  // the operator takes the current links, the solves run from zero; returns S_f(phi) and leaves the fields that kick() reads
  virtual double solve_for_force(complex<double>* phi, HmcResult& r) = 0;
  // p -= dt (Fg(beta_g) + Ff), Ff from the fields of the last solve_for_force, Fg the gauge force at the coupling beta_g: `beta` on the fused
  // single-scale path, 0.0 for the fermion force alone (every kick kernel multiplies its differences of sin P by the coupling it is given)
  virtual void kick(double* p, double dt, double beta_g) = 0;
  // draws the pseudofermion of trajectory `traj` on the current phases from stream (rng.seed, traj, 1) and returns it; solver counts into hb
  virtual complex<double>* draw_pseudofermion(unsigned long long traj, HmcResult& hb) = 0;

  HmcCore(const char* name, const char* flavour, double* phase_field, int Lx, int Ly, double beta, double tau, int n_steps, double cg_eps, int cg_max_iter, HeatbathRng& generator)
      : name(name), flavour(flavour), lat_gauge(Lx, Ly, 1), theta(phase_field), theta_saved(0), pi(0), gauge(0), draw(0), gauge_other(0), rng(generator), good(false), cv(0), rat_fn(0),
        rat_data(0), rat_size(0), md_scheme(MD_LEAPFROG), md_n_gauge(0), md_lambda(0.1931833275037836), beta(beta), tau(tau), cg_eps(cg_eps), n_steps(n_steps),
        cg_max_iter(cg_max_iter), trajectories_done(0), solver(hmc_solve_cg) {
    n_links = (size_t)lat_gauge.get_size_gauge();
  }
  virtual ~HmcCore() {
    deallocate_vector(&theta_saved); deallocate_vector(&pi); deallocate_vector(&gauge); deallocate_vector(&draw); deallocate_vector(&gauge_other);
    for (size_t j = 0; j < sols.size(); j++) deallocate_vector(&sols[j]);
  }
  // the refusals every action shares, around the derived class's verdict on its flavour count; false (and a line) if the object is refused
  bool admit(bool count_ok) {
    if (qmg::slab().on) { std::cout << "[QMG-ERROR]: " << name << " does not run on y-slabs.\n"; return false; }
    if (!count_ok) { std::cout << "[QMG-ERROR]: " << name << " supports 0, 1 or 2 " << flavour << "s.\n"; return false; }
    if (!theta || n_steps < 1 || !(tau > 0.0)) { std::cout << "[QMG-ERROR]: " << name << " needs a phase field, n_steps >= 1 and tau > 0.\n"; return false; }
    return true;
  }
  bool allocate_core() {
    theta_saved = allocate_vector<double>(n_links);
    pi = allocate_vector<double>(n_links);
    gauge = allocate_vector<complex<double>>(n_links);
    draw = allocate_vector<complex<double>>(1);
    return good = theta_saved && pi && gauge && draw;
  }
  // a method called on an object that cannot serve it: a line, r.cg_converged = false, true
  bool refused(bool is_ok, const char* method, const std::string& needs, HmcResult& r) {
    if (is_ok) return false;
    std::cout << "[QMG-ERROR]: " << name << "::" << method << " " << needs << ".\n";
    r.cg_converged = false;
    return true;
  }
  std::string one_flavour_object() const { return "needs a one-" + flavour + " object"; }

  double kinetic(double* p) { return 0.5 * norm2sq((complex<double>*)p, n_links / 2); }
  double plaquette() { return std::real(get_plaquette_u1(gauge, &lat_gauge)); }
  double gauge_action() { return beta * (double)lat_gauge.get_volume() * (1.0 - plaquette()); }
  void observe(HmcResult& r) { r.plaquette = plaquette(); r.topo = get_topo_u1(gauge, &lat_gauge); }

  // A drift of length e on the fermion scale: md_n_gauge steps of the scheme, of length e / md_n_gauge, under the gauge force alone.  Written
  // as pairs (kick, drift) and a last kick, the pairs go through qmg_hmc_gauge_step from `gauge` to gauge_other and back; an odd count sends its
  // first pair through the two in-place entries, whose bits the fused step has, so that the block ends in `gauge`.  The last kick is the
  // gauge-only kick.
  void gauge_block(double* p, double e) {
    const int Lx = lat_gauge.get_dim_mu(0), Ly = lat_gauge.get_dim_mu(1);
    void* st = qmg::current_stream();
    std::vector<double> kicks, drifts;
    md_sequence(md_scheme, md_lambda, md_n_gauge, e / md_n_gauge, [&](double k) { kicks.push_back(k); }, [&](double d) { drifts.push_back(d); });
    size_t j = 0;
    if (drifts.size() & 1) {
      qmg::ok(qmg_hmc_momentum_update(p, gauge, 0, 0, Lx, Ly, beta, kicks[0], QMG_HMC_GAUGE_ONLY, st), "qmg_hmc_momentum_update");
      qmg::ok(qmg_hmc_link_update(theta, gauge, p, n_links, drifts[0], st), "qmg_hmc_link_update");
      j = 1;
    }
    complex<double>* ends[2] = {gauge, gauge_other};
    for (int src = 0; j < drifts.size(); j++, src ^= 1)
      qmg::ok(qmg_hmc_gauge_step(theta, ends[1 - src], ends[src], p, Lx, Ly, beta, kicks[j], drifts[j], st), "qmg_hmc_gauge_step");
    qmg::ok(qmg_hmc_momentum_update(p, gauge, 0, 0, Lx, Ly, beta, kicks.back(), QMG_HMC_GAUGE_ONLY, st), "qmg_hmc_momentum_update");
  }

  // sols[j] = (A + shifts[j])^-1 b over `size` components by ONE multi-shift CG from zero, A the operator `fn`; counts into r
  void solve_shifts(complex<double>* b, std::vector<double>& shifts, size_t size, matrix_op_cplx fn, void* op_data, HmcResult& r) {
    for (size_t j = 0; j < sols.size(); j++) zero_vector(sols[j], cv);
    const std::vector<inversion_info> inv = minv_vector_cg_m(sols.data(), b, (int)sols.size(), (int)size, 1, cg_max_iter, cg_eps, shifts.data(), fn, op_data);
    int iters = 0;
    for (size_t j = 0; j < inv.size(); j++) {
      if (inv[j].iter > iters) iters = inv[j].iter;
      if (!inv[j].success) r.cg_converged = false;
    }
    if (inv.size() != sols.size()) r.cg_converged = false;
    r.cg_iterations += iters;
  }
  // the same with the operator of the rational action
  void solve_shifts(complex<double>* b, std::vector<double>& shifts, HmcResult& r) { solve_shifts(b, shifts, rat_size, rat_fn, rat_data, r); }
  // out = r(A) in on the operator's links (sols is overwritten)
  void rational_on_links(complex<double>* out, complex<double>* in, HmcResult& r) {
    solve_shifts(in, rat.mu2, r);
    if (out != in) copy_vector(out, in, rat_size);
    for (int j = 0; j < rat.n; j++) caxpy(rat.rho[j], sols[j], out, rat_size);
    cax(rat.c0, out, rat_size);
  }

 public:
  double beta, tau, cg_eps;
  int n_steps, cg_max_iter;
  unsigned long long trajectories_done;
  hmc_solver_fn solver;

  bool ok() const { return good; }
  complex<double>* links() { return gauge; }   // exp(i theta) as of the last call
  Lattice2D* gauge_lattice() { return &lat_gauge; }

  // The integrator of md_evolve and trajectory(); the default is (MD_LEAPFROG, 0).  n_gauge = 0 is one scale: every kick is the fused kick of the
  // gauge and the fermion force.  n_gauge >= 1 is two scales: the kicks of the scheme carry the fermion force alone (none without fermions) and
  // every drift of length e is n_gauge steps of the same scheme, of length e / n_gauge, under the gauge force alone.  lambda is Omelyan's.
  // Refuses n_gauge < 0 and lambda outside (0, 1/2) with a line and false, and leaves the object as it was.
  bool set_integrator(MdScheme scheme, int n_gauge, double lambda = 0.1931833275037836) {
    if ((scheme != MD_LEAPFROG && scheme != MD_OMELYAN) || n_gauge < 0 || !(lambda > 0.0 && lambda < 0.5)) {
      std::cout << "[QMG-ERROR]: " << name << "::set_integrator needs a scheme, n_gauge >= 0 and 0 < lambda < 1/2.\n";
      return false;
    }
    if (n_gauge > 0 && !gauge_other && !(gauge_other = allocate_vector<complex<double>>(n_links))) {
      std::cout << "[QMG-ERROR]: " << name << "::set_integrator: out of device memory.\n";
      return false;
    }
    md_scheme = scheme; md_n_gauge = n_gauge; md_lambda = lambda;
    return true;
  }

  // ---- a rational action only; takes the object's current phases ----
  const qmg::ZolotarevInvSqrt& rational() const { return rat; }
  // out = r(A) in (DEVICE vectors of the pseudofermion's length; out may be in).  Returns the multi-shift CG's count and convergence.
  HmcResult apply_rational(complex<double>* out, complex<double>* in) {
    HmcResult r;
    if (refused(good && rat.ok, "apply_rational", one_flavour_object(), r)) return r;
    polar_vector(theta, gauge, n_links);
    operator_takes_links();
    rational_on_links(out, in, r);
    return r;
  }

  // The deterministic part alone: the integrator (set_integrator; by default leapfrog on one scale) over tau from the object's phases with the momenta `momenta` (DEVICE double[2 Lx Ly], evolved in place)
  // and the pseudofermion `pseudofermion` (DEVICE, the derived class's layout; ignored without fermions).  Fills dH, the CG counts and the
  // observables of the end point.
  HmcResult md_evolve(double* momenta, complex<double>* pseudofermion) {
    HmcResult r;
    if (refused(good, "md_evolve", "called on an object that was refused", r)) return r;
    const bool fermions = has_fermions();
    const double dt = tau / n_steps;
    polar_vector(theta, gauge, n_links);
    double sf = fermions ? solve_for_force(pseudofermion, r) : 0.0;
    const double h0 = kinetic(momenta) + gauge_action() + sf;
    if (md_n_gauge == 0) {   // one scale: the fused kick, and after every drift the solve that the next kick and the last H read
      md_sequence(md_scheme, md_lambda, n_steps, dt,
                  [&](double e) { kick(momenta, e, beta); },
                  [&](double e) {
                    qmg::ok(qmg_hmc_link_update(theta, gauge, momenta, n_links, e, qmg::current_stream()), "qmg_hmc_link_update");
                    if (fermions) sf = solve_for_force(pseudofermion, r);
                  });
    } else {                 // two scales: the fermion force alone outside, every drift a block of gauge steps
      md_sequence(md_scheme, md_lambda, n_steps, dt,
                  [&](double e) { if (fermions) kick(momenta, e, 0.0); },
                  [&](double e) {
                    gauge_block(momenta, e);
                    if (fermions) sf = solve_for_force(pseudofermion, r);
                  });
    }
    r.dH = kinetic(momenta) + gauge_action() + sf - h0;
    observe(r);
    return r;
  }

  // One HMC trajectory with the Metropolis test; on rejection the phases are the ones it started from.
  HmcResult trajectory() {
    HmcResult r, hb;
    if (refused(good, "trajectory", "called on an object that was refused", r)) return r;
    const unsigned long long traj = trajectories_done++;
    void* st = qmg::current_stream();
    qmg::ok(qmg_memcpy_d2d(theta_saved, theta, sizeof(double) * n_links, st), "qmg_memcpy_d2d");
    qmg::ok(qmg_hmc_momentum_refresh(pi, n_links, rng.seed, traj, st), "qmg_hmc_momentum_refresh");
    complex<double>* phi = has_fermions() ? draw_pseudofermion(traj, hb) : 0;
    r = md_evolve(pi, phi);
    r.cg_iterations += hb.cg_iterations; r.cg_converged = r.cg_converged && hb.cg_converged;
    // a uniform number from the same generator: the Box-Muller radius of a draw is sqrt(-2 log u), so u = exp(-|z|^2 / 2) in (0, 1]
    gaussian(draw, 1, qmg_hmc_stream_seed(rng.seed, traj, 2));
    const complex<double> z = qmg::get_element(draw, 0);
    const double u = std::exp(-0.5 * std::norm(z));
    r.accepted = r.cg_converged && r.dH == r.dH && u < std::exp(-r.dH);
    if (!r.accepted) {
      qmg::ok(qmg_memcpy_d2d(theta, theta_saved, sizeof(double) * n_links, st), "qmg_memcpy_d2d");
      polar_vector(theta, gauge, n_links);
      observe(r);
    }
    return r;
  }
};

#endif
