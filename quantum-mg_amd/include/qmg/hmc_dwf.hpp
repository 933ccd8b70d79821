// hmc_dwf.hpp -- hybrid Monte Carlo for the Schwinger model with two degenerate flavours of Shamir domain-wall fermions (or none), with
// Pauli-Villars fields, on even-site pseudofermions; leapfrog molecular dynamics, everything on the device.  Not in the reference.  The surface is
// StaggeredSchwingerHMC's (hmc_staggered.hpp), the trajectory, the leapfrog and their rules are HmcCore's (hmc_core.hpp); the independent
// statement is tests/dwf_hmc_numpy.py.
//
//   D(m) = A(m) + H,  A site-local and free of the links, H the hops: diagonal in s, on every slice the Wilson hops (operators.hpp: DwfBase)
//   det D = det A_oo det M,   M(m) = A_ee - H_eo A_oo^-1 H_oe   (qmg_dwf_schur_apply, csrc/qmg_dwf_eo.hip),   Gamma5 M Gamma5 = M^dagger
//
//   S_f = phi^dag P (M^dag M)^-1 P^dag phi,   M = M(mass),  P = M(1) the Pauli-Villars operator;   phi on the even sites, Ls Lx Ly components
// Heatbath: eta ~ exp(-eta^dag eta) on the even sites, phi = P (P^dag P)^-1 M^dag eta (one well-conditioned CG on P^dag P), S_f(phi) = |eta|^2.
// Force:  chi = P^dag phi,  X = (M^dag M)^-1 chi by the solver from a ZERO guess,  Y = M X,  S_f = Re <chi, X>, and on the full lattice, the odd
// halves by kernel K (qmg_dwf_hops_inv5, alpha = -1):
//   X5  = X (+) -A_oo(m)^-1 H_oe X        Y5  = Gamma5 [ G5Y   (+) -A_oo(m)^-1 H_oe G5Y   ],  G5Y   = Gamma5 Y
//   X5' = X (+) -A_oo(1)^-1 H_oe X        Y5' = Gamma5 [ G5phi (+) -A_oo(1)^-1 H_oe G5phi ],  G5phi = Gamma5 phi
//   dS_f/dtheta_mu(x) = sum_s [ Ff_mu(x; X5(s), Y5(s)) - Ff_mu(x; X5'(s), Y5'(s)) ],   Ff the bilinear of the Wilson force;
// the kick is ONE kernel (qmg_hmc_momentum_update_dwf, weights {+1, -1}, QMG_HMC_DWF_G5_Y: the bracketed fields go in as they are).
// M is applied through the C-ABI from the links with a run-time Ls and the wall mass per call (DwfLinksSchur below): the stored nc = 2 Ls
// stencil is neither allocated nor filled.
#ifndef QMG_HMC_DWF_HPP
#define QMG_HMC_DWF_HPP

#include <cmath>

#include "hmc.hpp"

// M(m) and M(m)^dag M(m) on the even half straight from the links, for any 2 <= Ls <= 32: the descriptor names the lattice, nc = 2 Ls and the
// shift M5 and carries no stored field.
struct DwfLinksSchur {
  qmg_stencil_desc d;
  complex<double>* gauge;   // the owner's links
  int Ls;
  double mass;
  complex<double>*tmp, *mid;   // the owner's scratch: full length (stage 1 of M writes its odd half) and half length (M rhs inside M^dag M)

  // lhs_e = Gamma5^out M Gamma5^in rhs_e (flags: QMG_DWF_G5_IN | QMG_DWF_G5_OUT); lhs != rhs
  bool apply(complex<double>* lhs, complex<double>* rhs, unsigned flags) {
    return qmg::ok(qmg_dwf_schur_apply(QMG_C64, &d, gauge, Ls, mass, 0.0, 1.0, lhs, rhs, tmp, 0, flags, 1, 0, 1u, qmg::current_stream()), "qmg_dwf_schur_apply");
  }
  // v_o = -A_oo^-1 H_oe v_e on the full-length v, in place
  bool fill_odd(complex<double>* v) {
    return qmg::ok(qmg_dwf_hops_inv5(QMG_C64, &d, gauge, Ls, mass, 0.0, 1.0, v, v, QMG_P_OE | QMG_P_ZERO_O, -1.0, 0.0, 0, 1, 0, 1u, qmg::current_stream()),
                   "qmg_dwf_hops_inv5");
  }
  static void mdag_m(complex<double>* lhs, complex<double>* rhs, void* self) {
    DwfLinksSchur* op = (DwfLinksSchur*)self;
    if (op->apply(op->mid, rhs, 0)) op->apply(lhs, op->mid, QMG_DWF_G5_IN | QMG_DWF_G5_OUT);
  }
};

class DomainWallSchwingerHMC : public HmcCore {
  complex<double>*phi, *eta, *chi;            // even-site vectors
  complex<double>*X5, *Z5, *X5p, *Z5p;        // full lattice: X5, Gamma5 Y5, X5', Gamma5 Y5'
  complex<double>*tmp, *mid;
  DwfLinksSchur op_m, op_pv;                  // M(mass) and P = M(1)
  size_t half;
  std::vector<double> g5_scale;
  std::vector<int> g5_shuffle;

  bool has_fermions() const { return n_flavours != 0; }
  void operator_takes_links() {}              // M reads `gauge` at every apply: nothing is stored
  void gamma5_even(complex<double>* out, const complex<double>* in) {
    qmg::pattern(g5_scale.data(), g5_shuffle.data(), 2 * Ls, in, out, half / (size_t)(2 * Ls));
  }
  // the solves run from zero on the current links; leaves X5, Z5, X5p, Z5p for kick(); returns S_f = Re <chi, X>
  double solve_for_force(complex<double>* phi_in, HmcResult& r) {
    op_pv.apply(chi, phi_in, QMG_DWF_G5_IN | QMG_DWF_G5_OUT);                      // chi = P^dag phi
    zero_vector(X5, cv);
    const inversion_info inv = solver(X5, chi, (int)half, cg_max_iter, cg_eps, DwfLinksSchur::mdag_m, (void*)&op_m);
    r.cg_iterations += inv.iter;
    if (!inv.success) r.cg_converged = false;
    const double sf = dot(chi, X5, half).real();
    op_m.apply(Z5, X5, QMG_DWF_G5_OUT);                                            // G5Y = Gamma5 M X
    copy_vector(X5p, X5, half);
    gamma5_even(Z5p, phi_in);                                                      // G5phi
    op_m.fill_odd(X5); op_m.fill_odd(Z5);
    op_pv.fill_odd(X5p); op_pv.fill_odd(Z5p);
    return sf;
  }
  void kick(double* p, double dt, double beta_g) {
    const void* xs[2] = {X5, X5p};
    const void* ys[2] = {Z5, Z5p};
    const double w[2] = {1.0, -1.0};
    const unsigned flags = n_flavours ? (unsigned)QMG_HMC_DWF_G5_Y : (unsigned)QMG_HMC_GAUGE_ONLY;
    qmg::ok(qmg_hmc_momentum_update_dwf(p, gauge, xs, ys, w, n_flavours ? 2 : 0, Ls, lat_gauge.get_dim_mu(0), lat_gauge.get_dim_mu(1), beta_g, dt, flags,
                                        qmg::current_stream()), "qmg_hmc_momentum_update_dwf");
  }
  // eta on the even sites: variance 1/2 per real component, from stream 1 of the trajectory
  complex<double>* draw_pseudofermion(unsigned long long traj, HmcResult& hb) {
    gaussian(eta, half, qmg_hmc_stream_seed(rng.seed, traj, 1));
    cax(std::sqrt(0.5), eta, half);
    hb = heatbath(phi, eta);
    return phi;
  }

 public:
  double mass, M5;
  int Ls, n_flavours;

  // phase_field: DEVICE double[2 Lx Ly], evolved in place.  n_flavours: 0 (pure gauge) or 2.  0 < mass <= 1; 3 + M5 > 1.  cg_eps is the
  // tolerance of the CG on M^dag M and of the heatbath's CG on P^dag P.
  DomainWallSchwingerHMC(double* phase_field, int Lx, int Ly, int Ls, double beta, double mass, int n_flavours, double tau, int n_steps, double cg_eps, int cg_max_iter,
                         HeatbathRng& generator, double M5 = -1.0)
      : HmcCore("DomainWallSchwingerHMC", "flavour", phase_field, Lx, Ly, beta, tau, n_steps, cg_eps, cg_max_iter, generator), phi(0), eta(0), chi(0), X5(0), Z5(0), X5p(0),
        Z5p(0), tmp(0), mid(0), half(0), mass(mass), M5(M5), Ls(Ls), n_flavours(n_flavours) {
    if (n_flavours == 1) { std::cout << "[QMG-ERROR]: DomainWallSchwingerHMC supports 0 or 2 flavours (one flavour needs RHMC on M^dag M).\n"; return; }
    if (!admit(n_flavours == 0 || n_flavours == 2)) return;
    if (Ls < 2 || Ls > 32) { std::cout << "[QMG-ERROR]: DomainWallSchwingerHMC needs 2 <= Ls <= 32.\n"; return; }
    if (!(mass > 0.0 && mass <= 1.0)) { std::cout << "[QMG-ERROR]: DomainWallSchwingerHMC needs 0 < mass <= 1.\n"; return; }
    if (!(3.0 + M5 > 1.0)) { std::cout << "[QMG-ERROR]: DomainWallSchwingerHMC needs 3 + M5 > 1.\n"; return; }
    cv = (size_t)2 * Ls * Lx * Ly;
    half = cv / 2;
    for (int s = 0; s < Ls; s++) {
      g5_scale.push_back(1.0); g5_scale.push_back(-1.0);
      g5_shuffle.push_back(2 * (Ls - 1 - s)); g5_shuffle.push_back(2 * (Ls - 1 - s) + 1);
    }
    if (allocate_core() && n_flavours) {
      phi = allocate_vector<complex<double>>(half); eta = allocate_vector<complex<double>>(half); chi = allocate_vector<complex<double>>(half);
      mid = allocate_vector<complex<double>>(half);
      X5 = allocate_vector<complex<double>>(cv); Z5 = allocate_vector<complex<double>>(cv); X5p = allocate_vector<complex<double>>(cv);
      Z5p = allocate_vector<complex<double>>(cv); tmp = allocate_vector<complex<double>>(cv);
      good = phi && eta && chi && mid && X5 && Z5 && X5p && Z5p && tmp;
    }
    if (!good) { std::cout << "[QMG-ERROR]: DomainWallSchwingerHMC: out of device memory.\n"; return; }
    qmg_stencil_desc d = {};
    d.Lx = Lx; d.Ly = Ly; d.nc = 2 * Ls;
    d.shift[0] = M5;
    op_m.d = d; op_m.gauge = gauge; op_m.Ls = Ls; op_m.mass = mass; op_m.tmp = tmp; op_m.mid = mid;
    op_pv = op_m;
    op_pv.mass = 1.0;
    polar_vector(theta, gauge, n_links);
  }
  ~DomainWallSchwingerHMC() {
    deallocate_vector(&phi); deallocate_vector(&eta); deallocate_vector(&chi); deallocate_vector(&mid); deallocate_vector(&X5); deallocate_vector(&Z5);
    deallocate_vector(&X5p); deallocate_vector(&Z5p); deallocate_vector(&tmp);
  }

  // ---- each takes the object's current phases; pseudofermions and eta are even-site vectors of Ls Lx Ly components ----
  // phi = P (P^dag P)^-1 M^dag eta: with eta ~ exp(-eta^dag eta), phi ~ exp(-S_f(phi)) and S_f(phi) = |eta|^2.  eta_even is unchanged.
  HmcResult heatbath(complex<double>* phi_even_out, complex<double>* eta_even) {
    HmcResult r;
    if (refused(good && n_flavours, "heatbath", "needs an object with fermions", r)) return r;
    polar_vector(theta, gauge, n_links);
    op_m.apply(chi, eta_even, QMG_DWF_G5_IN | QMG_DWF_G5_OUT);                     // M^dag eta
    zero_vector(X5, half);
    const inversion_info inv = solver(X5, chi, (int)half, cg_max_iter, cg_eps, DwfLinksSchur::mdag_m, (void*)&op_pv);
    r.cg_iterations += inv.iter;
    if (!inv.success) r.cg_converged = false;
    op_pv.apply(phi_even_out, X5, 0);
    return r;
  }
  // S_f = phi^dag P (M^dag M)^-1 P^dag phi
  double pseudofermion_action(complex<double>* pseudofermion_even, HmcResult& r) {
    if (refused(good && n_flavours, "pseudofermion_action", "needs an object with fermions", r)) return 0.0;
    polar_vector(theta, gauge, n_links);
    return solve_for_force(pseudofermion_even, r);
  }
};

#endif
