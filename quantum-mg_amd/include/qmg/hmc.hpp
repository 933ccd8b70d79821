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
#ifndef QMG_HMC_HPP
#define QMG_HMC_HPP

#include <cmath>

#include "krylov.hpp"
#include "operators.hpp"
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

  static void apply_normal(complex<double>* lhs, complex<double>* rhs, void* self) {   // lhs = gamma5 D gamma5 D rhs = D^dag D rhs
    SchwingerHMC* h = (SchwingerHMC*)self;
    h->op->apply_M_overwrite(h->tmp1, rhs);
    h->op->gamma5(h->tmp2, h->tmp1);
    h->op->apply_M_overwrite(h->tmp1, h->tmp2);
    h->op->gamma5(lhs, h->tmp1);
  }
  // the operator takes the current links; X = (D^dag D)^-1 phi, Y = D X; returns S_f = Re <phi, X>
  double solve_XY(complex<double>* phi_in, HmcResult& r) {
    op->update_links(gauge);
    zero_vector(X, cv);
    const inversion_info inv = solver(X, phi_in, (int)cv, cg_max_iter, cg_eps, apply_normal, (void*)this);
    r.cg_iterations += inv.iter;
    if (!inv.success) r.cg_converged = false;
    op->apply_M_overwrite(Y, X);
    return dot(phi_in, X, cv).real();
  }
  double kinetic(double* p) { return 0.5 * norm2sq((complex<double>*)p, n_links / 2); }
  double gauge_action() { return beta * (double)lat_gauge.get_volume() * (1.0 - std::real(get_plaquette_u1(gauge, &lat_gauge))); }
  void kick(double* p, double dt) {
    qmg::ok(qmg_hmc_momentum_update(p, gauge, X, Y, lat_gauge.get_dim_mu(0), lat_gauge.get_dim_mu(1), beta, dt, n_flavours ? 0u : (unsigned)QMG_HMC_GAUGE_ONLY,
                                    qmg::current_stream()), "qmg_hmc_momentum_update");
  }

 public:
  double beta, mass, tau, cg_eps;
  int n_flavours, n_steps, cg_max_iter;
  unsigned long long trajectories_done;
  hmc_solver_fn solver;

  // phase_field: DEVICE double[2 Lx Ly], evolved in place.  n_flavours: 0 (pure gauge) or 2.
  SchwingerHMC(double* phase_field, int Lx, int Ly, double beta, double mass, int n_flavours, double tau, int n_steps, double cg_eps, int cg_max_iter, HeatbathRng& generator)
      : lat_gauge(Lx, Ly, 1), lat_fermion(Lx, Ly, 2), theta(phase_field), theta_saved(0), pi(0), gauge(0), phi(0), X(0), Y(0), tmp1(0), tmp2(0), draw(0), op(0),
        rng(generator), good(false), beta(beta), mass(mass), tau(tau), cg_eps(cg_eps), n_flavours(n_flavours), n_steps(n_steps), cg_max_iter(cg_max_iter),
        trajectories_done(0), solver(hmc_solve_cg) {
    n_links = (size_t)lat_gauge.get_size_gauge();
    cv = (size_t)lat_fermion.get_size_cv();
    if (qmg::slab().on) { std::cout << "[QMG-ERROR]: SchwingerHMC does not run on y-slabs.\n"; return; }
    if (n_flavours != 0 && n_flavours != 2) { std::cout << "[QMG-ERROR]: SchwingerHMC supports 0 or 2 flavours.\n"; return; }
    if (!phase_field || n_steps < 1 || !(tau > 0.0)) { std::cout << "[QMG-ERROR]: SchwingerHMC needs a phase field, n_steps >= 1 and tau > 0.\n"; return; }
    theta_saved = allocate_vector<double>(n_links);
    pi = allocate_vector<double>(n_links);
    gauge = allocate_vector<complex<double>>(n_links);
    draw = allocate_vector<complex<double>>(1);
    good = theta_saved && pi && gauge && draw;
    if (good && n_flavours) {
      phi = allocate_vector<complex<double>>(cv); X = allocate_vector<complex<double>>(cv); Y = allocate_vector<complex<double>>(cv);
      tmp1 = allocate_vector<complex<double>>(cv); tmp2 = allocate_vector<complex<double>>(cv);
      good = phi && X && Y && tmp1 && tmp2;
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
  }
  bool ok() const { return good; }
  complex<double>* links() { return gauge; }   // exp(i theta) as of the last call
  Lattice2D* gauge_lattice() { return &lat_gauge; }

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
    void* st = qmg::current_stream();
    qmg::ok(qmg_memcpy_d2d(theta_saved, theta, sizeof(double) * n_links, st), "qmg_memcpy_d2d");
    qmg::ok(qmg_hmc_momentum_refresh(pi, n_links, rng.seed, traj, st), "qmg_hmc_momentum_refresh");
    if (n_flavours) {   // eta: variance 1/2 per real component; phi = D^dag eta = gamma5 D gamma5 eta on the current links
      polar_vector(theta, gauge, n_links);
      op->update_links(gauge);
      gaussian(tmp1, cv, qmg_hmc_stream_seed(rng.seed, traj, 1));
      cax(std::sqrt(0.5), tmp1, cv);
      op->gamma5(tmp2, tmp1);
      op->apply_M_overwrite(tmp1, tmp2);
      op->gamma5(phi, tmp1);
    }
    r = md_evolve(pi, phi);
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
