// hmc_parity -- the deterministic part of SchwingerHMC (include/qmg/hmc.hpp) on fields the caller supplies, for tests/test_gpu_hmc.py:
//   ./hmc_parity L gauge_file dir beta mass n_flavours tau n_steps cg_eps [stout_levels stout_rho]
// gauge_file: phases in the reference's text format (read_phase_u1).  dir/pi.bin: 2 L^2 doubles, dir/phi.bin: 2 L^2 complex<double>, both in
// the device layout.  Runs md_evolve forward, dumps dir/theta_fwd.bin and dir/pi_fwd.bin, negates the momenta, runs md_evolve again and dumps
// dir/theta_back.bin and dir/pi_back.bin.  A trailing `integrator <leapfrog|omelyan> <n_gauge>`, behind everything else, sets HmcCore::set_integrator.  stout_levels and stout_rho (default 0 0: thin links) put the fermions on stout-smeared links.  Prints
//   [MD] forward dH <dH> cg <iterations> converged <0|1> plaq <plaquette>
//   [MD] back    dH <dH> cg <iterations> converged <0|1> plaq <plaquette>
#include "hmc_parity_common.hpp"

using namespace std;
using namespace hmc_parity;

int main(int argc, char** argv) {
  qmg_driver::Guard guard;
  const hmc_run::Integrator integrator = hmc_run::Integrator::peel(argc, argv);   // the trailing `integrator <leapfrog|omelyan> <n_gauge>`, if any
  if (argc < 10) { cout << "usage: ./hmc_parity L gauge_file dir beta mass n_flavours tau n_steps cg_eps [stout_levels stout_rho]\n"; return -1; }
  if (!qmg::ok(qmg_init(0), "qmg_init")) return 2;
  const int L = stoi(argv[1]);
  const string gauge_file = argv[2], dir = argv[3];
  const double beta = stod(argv[4]), mass = stod(argv[5]);
  const int n_flavours = stoi(argv[6]);
  const double tau = stod(argv[7]);
  const int n_steps = stoi(argv[8]);
  const double cg_eps = stod(argv[9]);
  const int stout_levels = argc > 10 ? stoi(argv[10]) : 0;
  const double stout_rho = argc > 11 ? stod(argv[11]) : 0.0;

  Lattice2D lat_gauge(L, L, 1);
  const size_t n_links = (size_t)lat_gauge.get_size_gauge(), cv = 2 * (size_t)L * L;
  double* phases = allocate_vector<double>(n_links);
  double* pi = allocate_vector<double>(n_links);
  complex<double>* phi = allocate_vector<complex<double>>(cv);
  int rc = 0;
  if (!read_phase_u1(phases, &lat_gauge, gauge_file) || !load(dir + "/pi.bin", pi, n_links) || (n_flavours && !load(dir + "/phi.bin", phi, cv))) rc = 3;
  if (!rc) {
    HeatbathRng generator(1);
    SchwingerHMC hmc(phases, L, L, beta, mass, n_flavours, tau, n_steps, cg_eps, 20000, generator, 8, 0.0, 0.0, stout_levels, stout_rho);
    cout << setprecision(17);
    rc = hmc.ok() && integrator.apply(hmc) ? md_legs(hmc, dir, phases, pi, phi, n_links) : 4;
  }
  deallocate_vector(&phases); deallocate_vector(&pi); deallocate_vector(&phi);
  qmg::VecPool::release_all();
  return qmg_driver::leave(rc);
}
