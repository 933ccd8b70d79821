// rhmc_parity -- the deterministic parts of one-flavour SchwingerHMC (include/qmg/hmc.hpp) on fields the caller supplies, for
// tests/test_gpu_rhmc.py:
//   ./rhmc_parity mode L gauge_file dir beta mass tau n_steps cg_eps degree spectrum_lo spectrum_hi [stout_levels stout_rho]
// gauge_file: phases in the reference's text format (read_phase_u1).  Files under dir are in the device layout, momenta as 2 L^2 doubles and
// spinors as 2 L^2 complex<double>.  spectrum_hi = 0 takes the facade's default.  stout_levels and stout_rho (default 0 0: thin links) put
// the fermions of every mode on stout-smeared links; the interval is then that of their operator.  Every mode prints the coefficients' line
//   [RHMC] n <degree> ra <lo> rb <hi> c0 <c0> delta <delta>
// mode md:        reads pi.bin and phi.bin; md_evolve forward (theta_fwd.bin, pi_fwd.bin), momenta negated, md_evolve again (theta_back.bin,
//                 pi_back.bin);  [MD] forward|back dH <dH> cg <multi-shift iterations> converged <0|1> plaq <plaquette>
// mode heatbath:  reads eta.bin; phi = B eta to phi.bin;  [HB] eta2 <eta^dag eta> spf <S_pf(phi)> cg <iterations> converged <0|1>
// mode rational:  reads v.bin; r(Q^2) v to rv.bin and r(Q^2) r(Q^2) v to rrv.bin;  [RAT] cg <iterations> converged <0|1>
// mode action:    reads phi.bin;  [SPF] <S_pf(phi)> cg <iterations> converged <0|1>
// mode check:     [RHMC-CHECK] ratio <ratio> bound <bound> ok <0|1>
// A trailing `integrator <leapfrog|omelyan> <n_gauge>`, behind everything else, sets HmcCore::set_integrator for mode md.
// Exit status 1 if a solve did not converge.
#include "hmc_parity_common.hpp"

using namespace std;
using namespace hmc_parity;

int main(int argc, char** argv) {
  qmg_driver::Guard guard;
  const hmc_run::Integrator integrator = hmc_run::Integrator::peel(argc, argv);   // the trailing `integrator <leapfrog|omelyan> <n_gauge>`, if any
  if (argc < 13) { cout << "usage: ./rhmc_parity md|heatbath|rational|action|check L gauge_file dir beta mass tau n_steps cg_eps degree spectrum_lo spectrum_hi [stout_levels stout_rho]\n"; return -1; }
  if (!qmg::ok(qmg_init(0), "qmg_init")) return 2;
  const string mode = argv[1];
  const int L = stoi(argv[2]);
  const string gauge_file = argv[3], dir = argv[4];
  const double beta = stod(argv[5]), mass = stod(argv[6]), tau = stod(argv[7]);
  const int n_steps = stoi(argv[8]);
  const double cg_eps = stod(argv[9]);
  const int degree = stoi(argv[10]);
  const double lo = stod(argv[11]), hi = stod(argv[12]);
  const int stout_levels = argc > 13 ? stoi(argv[13]) : 0;
  const double stout_rho = argc > 14 ? stod(argv[14]) : 0.0;

  Lattice2D lat_gauge(L, L, 1);
  const size_t n_links = (size_t)lat_gauge.get_size_gauge(), cv = 2 * (size_t)L * L;
  double* phases = allocate_vector<double>(n_links);
  double* pi = allocate_vector<double>(n_links);
  complex<double>* a = allocate_vector<complex<double>>(cv);
  complex<double>* b = allocate_vector<complex<double>>(cv);
  int rc = 0;
  if (!read_phase_u1(phases, &lat_gauge, gauge_file)) rc = 3;
  if (!rc) {
    HeatbathRng generator(1);
    SchwingerHMC hmc(phases, L, L, beta, mass, 1, tau, n_steps, cg_eps, 20000, generator, degree, lo, hi, stout_levels, stout_rho);
    cout << setprecision(17);
    if (!hmc.ok() || !integrator.apply(hmc)) rc = 4;
    if (!rc) rhmc_line(hmc);
    if (rc) {   // refused
    } else if (mode == "md") {
      rc = load(dir + "/pi.bin", pi, n_links) && load(dir + "/phi.bin", a, cv) ? md_legs(hmc, dir, phases, pi, a, n_links) : 3;
    } else if (mode == "heatbath") {
      rc = heatbath_mode(hmc, dir, a, b, cv, cv);
    } else if (mode == "rational") {
      rc = rational_mode(hmc, dir, a, b, cv);
    } else if (mode == "action") {
      if (!load(dir + "/phi.bin", a, cv)) rc = 3;
      if (!rc) {
        HmcResult r;
        const double spf = hmc.pseudofermion_action(a, r);
        cout << "[SPF] " << spf << " cg " << r.cg_iterations << " converged " << (r.cg_converged ? 1 : 0) << "\n";
        if (!r.cg_converged) rc = 1;
      }
    } else if (mode == "check") {
      const RhmcRangeCheck c = hmc.range_check();
      cout << "[RHMC-CHECK] ratio " << c.ratio << " bound " << c.bound << " ok " << (c.ok ? 1 : 0) << "\n";
      if (!c.cg_converged) rc = 1;
    } else {
      rc = unknown_mode(mode);
    }
  }
  deallocate_vector(&phases); deallocate_vector(&pi); deallocate_vector(&a); deallocate_vector(&b);
  qmg::VecPool::release_all();
  return qmg_driver::leave(rc);
}
