// dwf_hmc -- dynamical Schwinger-model ensembles with two degenerate flavours of Shamir domain-wall fermions (or none) by hybrid Monte Carlo
// (include/qmg/hmc_dwf.hpp: Pauli-Villars pseudofermions on the even sites, leapfrog over tau = 1, Metropolis test, everything on the device).
//   ./dwf_hmc L Ls beta mass n_flavours n_traj n_therm n_steps seed [out.dat [cold|heatbath]]
// n_therm trajectories of thermalisation, then n_traj measured ones.  The start is a non-compact heatbath field at the same beta (100 sweeps)
// unless `cold` is given.  One line per trajectory, as schwinger_hmc prints it:
//   [HMC] <index> dH <dH> acc <0|1> plaq <plaquette> Q <topological charge> cg <CG iterations of the trajectory>
// and at the end the acceptance rate and <exp(-dH)> (which is 1 in equilibrium) with its jackknife error over the measured trajectories:
//   [HMC-FINAL] trajectories <n> acceptance <rate> exp_mdH <mean> +/- <error> plaq <mean> +/- <error> unconverged <count>
// out.dat receives the last configuration through write_gauge_u1 (the format dwf_measure reads) and is read back through read_gauge_u1:
//   [HMC-READBACK] plaq <plaquette> Q <charge>.
// A trailing triple `integrator <leapfrog|omelyan> <n_gauge>` chooses the molecular dynamics (HmcCore::set_integrator) and is echoed before the
// trajectories:  [INTEGRATOR] scheme <leapfrog|omelyan> n_gauge <n_gauge>.  Without it: leapfrog on one scale.
// Exit status 1 if any CG did not converge, 3 if the object was refused.
#include <iostream>
#include <string>

#include "../include/qmg/qmg.hpp"
#include "driver_common.hpp"
#include "hmc_run_common.hpp"

using namespace std;

int main(int argc, char** argv) {
  qmg_driver::Guard guard;
  const hmc_run::Integrator integrator = hmc_run::Integrator::peel(argc, argv);   // the trailing `integrator <leapfrog|omelyan> <n_gauge>`, if any
  if (argc < 10) { cout << "usage: ./dwf_hmc L Ls beta mass n_flavours n_traj n_therm n_steps seed [out.dat [cold|heatbath]]\n"; return -1; }
  if (!qmg::ok(qmg_init(0), "qmg_init")) return 2;
  const int L = stoi(argv[1]), Ls = stoi(argv[2]);
  const double beta = stod(argv[3]), mass = stod(argv[4]);
  const int n_flavours = stoi(argv[5]), n_traj = stoi(argv[6]), n_therm = stoi(argv[7]), n_steps = stoi(argv[8]);
  HeatbathRng generator(stoull(argv[9]));
  const string out_cfg = (argc > 10) ? argv[10] : "";
  const bool cold = (argc > 11) && string(argv[11]) == "cold";
  const double tau = 1.0, cg_eps = 1e-10;
  const int cg_max_iter = 20000;

  Lattice2D lat_gauge(L, L, 1);
  const size_t n_links = (size_t)lat_gauge.get_size_gauge();
  double* phases = allocate_vector<double>(n_links);
  qmg::ok(qmg_memset_zero(phases, sizeof(double) * n_links, qmg::current_stream()), "qmg_memset_zero");
  if (!cold) heatbath_noncompact_update(phases, &lat_gauge, beta, 100, generator);

  int rc = 3;
  {
    DomainWallSchwingerHMC hmc(phases, L, L, Ls, beta, mass, n_flavours, tau, n_steps, cg_eps, cg_max_iter, generator);
    if (hmc.ok() && integrator.apply(hmc)) {
      integrator.line();
      rc = hmc_run::run<DomainWallSchwingerHMC>(hmc, lat_gauge, false, nullptr, 0.0, n_traj, n_therm, out_cfg);
    }
  }
  deallocate_vector(&phases);
  qmg::VecPool::release_all();
  return qmg_driver::leave(rc);
}
