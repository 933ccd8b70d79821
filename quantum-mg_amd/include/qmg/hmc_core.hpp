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
//   * a rejected trajectory restores the phases AND the links, and reports the observables of the restored field.
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

class HmcCore {
  HmcCore(HmcCore const&);
  HmcCore& operator=(HmcCore const&);

 protected:
  const std::string name, flavour;   // the derived class and what it counts ("flavour", "taste"), for the messages
  Lattice2D lat_gauge;
  double* theta;                     // the caller's
  double *theta_saved, *pi;
  complex<double>*gauge, *draw;
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

  // ---- the hooks of a fermion action ----
  virtual bool has_fermions() const = 0;
  // the operator takes the links in `gauge`
  virtual void operator_takes_links() = 0;
  // the operator takes the current links, the solves run from zero; returns S_f(phi) and leaves the fields that kick() reads
  virtual double solve_for_force(complex<double>* phi, HmcResult& r) = 0;
  // p -= dt (Fg + Ff), Ff from the fields of the last solve_for_force
  virtual void kick(double* p, double dt) = 0;
  // draws the pseudofermion of trajectory `traj` on the current phases from stream (rng.seed, traj, 1) and returns it; solver counts into hb
  virtual complex<double>* draw_pseudofermion(unsigned long long traj, HmcResult& hb) = 0;

  HmcCore(const char* name, const char* flavour, double* phase_field, int Lx, int Ly, double beta, double tau, int n_steps, double cg_eps, int cg_max_iter, HeatbathRng& generator)
      : name(name), flavour(flavour), lat_gauge(Lx, Ly, 1), theta(phase_field), theta_saved(0), pi(0), gauge(0), draw(0), rng(generator), good(false), cv(0), rat_fn(0),
        rat_data(0), rat_size(0), beta(beta), tau(tau), cg_eps(cg_eps), n_steps(n_steps), cg_max_iter(cg_max_iter), trajectories_done(0), solver(hmc_solve_cg) {
    n_links = (size_t)lat_gauge.get_size_gauge();
  }
  virtual ~HmcCore() {
    deallocate_vector(&theta_saved); deallocate_vector(&pi); deallocate_vector(&gauge); deallocate_vector(&draw);
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

  // The deterministic part alone: leapfrog over tau from the object's phases with the momenta `momenta` (DEVICE double[2 Lx Ly], evolved in place)
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
    kick(momenta, 0.5 * dt);
    for (int k = 0; k < n_steps; k++) {
      qmg::ok(qmg_hmc_link_update(theta, gauge, momenta, n_links, dt, qmg::current_stream()), "qmg_hmc_link_update");
      if (fermions) sf = solve_for_force(pseudofermion, r);
      kick(momenta, k + 1 < n_steps ? dt : 0.5 * dt);
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
