// dwf_hmc_parity -- the deterministic parts of DomainWallSchwingerHMC (include/qmg/hmc_dwf.hpp) on fields the caller supplies, for
// tests/test_gpu_dwf_hmc.py:
//   ./dwf_hmc_parity mode L Ls gauge_file dir beta mass tau n_steps cg_eps n_flavours
// gauge_file: phases in the reference's text format (read_phase_u1).  Files under dir are in the device layout: momenta as 2 L^2 doubles,
// pseudofermions and eta as the Ls L^2 complex<double> of the even sites (nc = 2 Ls, c = 2 s + sigma).
// mode md:        reads pi.bin and phi.bin; md_evolve forward (theta_fwd.bin, pi_fwd.bin), momenta negated, md_evolve again (theta_back.bin,
//                 pi_back.bin);  [MD] forward|back dH <dH> cg <CG iterations> converged <0|1> plaq <plaquette>
// mode heatbath:  reads eta.bin (even sites); phi to phi.bin;  [HB] eta2 <eta^dag eta> spf <S_f(phi)> cg <iterations> converged <0|1>
// A trailing `integrator <leapfrog|omelyan> <n_gauge>`, behind everything else, sets HmcCore::set_integrator for mode md.
// Exit status 1 if a solve did not converge.
#include "hmc_parity_common.hpp"

using namespace std;
using namespace hmc_parity;

int main(int argc, char** argv) {
  qmg_driver::Guard guard;
  const hmc_run::Integrator integrator = hmc_run::Integrator::peel(argc, argv);   // the trailing `integrator <leapfrog|omelyan> <n_gauge>`, if any
  if (argc < 12) { cout << "usage: ./dwf_hmc_parity md|heatbath L Ls gauge_file dir beta mass tau n_steps cg_eps n_flavours\n"; return -1; }
  if (!qmg::ok(qmg_init(0), "qmg_init")) return 2;
  const string mode = argv[1];
  const int L = stoi(argv[2]), Ls = stoi(argv[3]);
  const string gauge_file = argv[4], dir = argv[5];
  const double beta = stod(argv[6]), mass = stod(argv[7]), tau = stod(argv[8]);
  const int n_steps = stoi(argv[9]);
  const double cg_eps = stod(argv[10]);
  const int n_flavours = stoi(argv[11]);

  Lattice2D lat_gauge(L, L, 1);
  const size_t n_links = (size_t)lat_gauge.get_size_gauge(), half = (size_t)Ls * L * L;
  double* phases = allocate_vector<double>(n_links);
  double* pi = allocate_vector<double>(n_links);
  complex<double>* a = allocate_vector<complex<double>>(half);
  complex<double>* b = allocate_vector<complex<double>>(half);
  int rc = 0;
  if (!read_phase_u1(phases, &lat_gauge, gauge_file)) rc = 3;
  if (!rc) {
    HeatbathRng generator(1);
    DomainWallSchwingerHMC hmc(phases, L, L, Ls, beta, mass, n_flavours, tau, n_steps, cg_eps, 20000, generator);
    cout << setprecision(17);
    if (!hmc.ok() || !integrator.apply(hmc)) rc = 4;
    if (rc) {   // refused
    } else if (mode == "md") {
      rc = load(dir + "/pi.bin", pi, n_links) && load(dir + "/phi.bin", a, half) ? md_legs(hmc, dir, phases, pi, a, n_links) : 3;
    } else if (mode == "heatbath") {
      rc = heatbath_mode(hmc, dir, a, b, half, half);
    } else {
      rc = unknown_mode(mode);
    }
  }
  deallocate_vector(&phases); deallocate_vector(&pi); deallocate_vector(&a); deallocate_vector(&b);
  qmg::VecPool::release_all();
  return qmg_driver::leave(rc);
}
