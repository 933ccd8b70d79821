// stag_hmc_parity -- the deterministic parts of StaggeredSchwingerHMC (include/qmg/hmc_staggered.hpp) on fields the caller supplies, for
// tests/test_gpu_stag_hmc.py:
//   ./stag_hmc_parity mode L gauge_file dir beta mass tau n_steps cg_eps n_tastes [degree]
// gauge_file: phases in the reference's text format (read_phase_u1).  Files under dir are in the device layout: momenta as 2 L^2 doubles,
// full-lattice vectors as L^2 complex<double>, pseudofermions as the L^2 / 2 complex<double> of the even sites.  One taste prints
//   [RHMC] n <degree> ra <lo> rb <hi> c0 <c0> delta <delta>
// mode md:        reads pi.bin and phi.bin; md_evolve forward (theta_fwd.bin, pi_fwd.bin), momenta negated, md_evolve again (theta_back.bin,
//                 pi_back.bin);  [MD] forward|back dH <dH> cg <CG iterations> converged <0|1> plaq <plaquette>
// mode heatbath:  reads eta.bin (full lattice); phi_e to phi.bin;  [HB] eta2 <eta^dag eta> spf <S_pf(phi_e)> cg <iterations> converged <0|1>
// mode rational:  one taste; reads v.bin; r(A_ee) v to rv.bin and r(A_ee) r(A_ee) v to rrv.bin;  [RAT] cg <iterations> converged <0|1>
// A trailing `integrator <leapfrog|omelyan> <n_gauge>`, behind everything else, sets HmcCore::set_integrator for mode md.
// Exit status 1 if a solve did not converge.
#include "hmc_parity_common.hpp"

using namespace std;
using namespace hmc_parity;

int main(int argc, char** argv) {
  qmg_driver::Guard guard;
  const hmc_run::Integrator integrator = hmc_run::Integrator::peel(argc, argv);   // the trailing `integrator <leapfrog|omelyan> <n_gauge>`, if any
  if (argc < 11) { cout << "usage: ./stag_hmc_parity md|heatbath|rational L gauge_file dir beta mass tau n_steps cg_eps n_tastes [degree]\n"; return -1; }
  if (!qmg::ok(qmg_init(0), "qmg_init")) return 2;
  const string mode = argv[1];
  const int L = stoi(argv[2]);
  const string gauge_file = argv[3], dir = argv[4];
  const double beta = stod(argv[5]), mass = stod(argv[6]), tau = stod(argv[7]);
  const int n_steps = stoi(argv[8]);
  const double cg_eps = stod(argv[9]);
  const int n_tastes = stoi(argv[10]);
  const int degree = argc > 11 ? stoi(argv[11]) : 8;

  Lattice2D lat_gauge(L, L, 1);
  const size_t n_links = (size_t)lat_gauge.get_size_gauge(), cv = (size_t)L * L, half = cv / 2;
  double* phases = allocate_vector<double>(n_links);
  double* pi = allocate_vector<double>(n_links);
  complex<double>* a = allocate_vector<complex<double>>(cv);
  complex<double>* b = allocate_vector<complex<double>>(cv);
  int rc = 0;
  if (!read_phase_u1(phases, &lat_gauge, gauge_file)) rc = 3;
  if (!rc) {
    HeatbathRng generator(1);
    StaggeredSchwingerHMC hmc(phases, L, L, beta, mass, n_tastes, tau, n_steps, cg_eps, 20000, generator, degree);
    cout << setprecision(17);
    if (!hmc.ok() || !integrator.apply(hmc)) rc = 4;
    if (!rc && n_tastes == 1) rhmc_line(hmc);
    if (rc) {   // refused
    } else if (mode == "md") {
      rc = load(dir + "/pi.bin", pi, n_links) && load(dir + "/phi.bin", a, half) ? md_legs(hmc, dir, phases, pi, a, n_links) : 3;
    } else if (mode == "heatbath") {
      rc = heatbath_mode(hmc, dir, a, b, cv, half);
    } else if (mode == "rational") {
      rc = rational_mode(hmc, dir, a, b, half);
    } else {
      rc = unknown_mode(mode);
    }
  }
  deallocate_vector(&phases); deallocate_vector(&pi); deallocate_vector(&a); deallocate_vector(&b);
  qmg::VecPool::release_all();
  return qmg_driver::leave(rc);
}
