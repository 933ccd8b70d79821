// schwinger_hmc -- dynamical Schwinger-model ensembles: compact U(1) with two degenerate Wilson flavours (or none) by hybrid Monte Carlo
// (include/qmg/hmc.hpp: leapfrog over tau = 1, Metropolis test, everything on the device).
//   ./schwinger_hmc L beta mass n_flavours n_traj n_therm n_steps seed [out.dat [cold|heatbath]]
// n_therm trajectories of thermalisation, then n_traj measured ones.  The start is a non-compact heatbath field at the same beta (100 sweeps)
// unless `cold` is given.  One line per trajectory:
//   [HMC] <index> dH <dH> acc <0|1> plaq <plaquette> Q <topological charge> cg <CG iterations of the trajectory>
// and at the end the acceptance rate and <exp(-dH)> (which is 1 in equilibrium) with its jackknife error over the measured trajectories:
//   [HMC-FINAL] trajectories <n> acceptance <rate> exp_mdH <mean> +/- <error> plaq <mean> +/- <error> unconverged <count>
// out.dat receives the last configuration through write_gauge_u1 (the text format the n13 / n15 / n19 / n22 drivers read) and is read back
// through read_gauge_u1: [HMC-READBACK] plaq <plaquette> Q <charge>.
// Exit status 1 if any CG did not converge.
// n_flavours = 1 is RHMC (include/qmg/hmc.hpp) and takes the degree of the rational function and the interval [lo, hi] of the spectrum of
// (D^dag D)^(1/2) from three more arguments, or from QMG_RHMC_DEGREE (default 8) and QMG_RHMC_LO (required one way or the other); hi = 0 or
// absent is |2 + mass| + 2:
//   ./schwinger_hmc L beta mass 1 n_traj n_therm n_steps seed out.dat cold|heatbath [degree lo [hi]]
// It prints, before the trajectories,
//   [RHMC] n <degree> ra <lo> rb <hi> delta <delta> det_bound <(1 + delta)^(2 L^2) - 1>
// (the sampled weight det r(Q^2)^-1 is within that relative distance of det D while the spectrum stays inside the interval) and, after the
// thermalisation and at the end, SchwingerHMC::range_check on the current field:
//   [RHMC-CHECK] ratio <|xi^dag (r Q^2 r - 1) xi| / xi^dag xi> bound <2 delta + delta^2> ok <0|1>
// ok 0 proves that the spectrum has left the interval; the exit status is then 1 as well.
// One more trailing argument, behind out.dat and cold|heatbath (and the RHMC arguments, if any), chooses the fermions: `wilson` (the default) or
// `staggered` (include/qmg/hmc_staggered.hpp).  With `staggered` n_flavours counts tastes: 2 is HMC on even-odd pseudofermions, 1 the rooted RHMC
// on the exact interval [mass^2, mass^2 + 4] -- it takes the degree alone, prints [RHMC] with det_bound (1 + delta)^(L^2 / 2) - 1 and no
// [RHMC-CHECK]:
//   ./schwinger_hmc L beta mass n_tastes n_traj n_therm n_steps seed out.dat cold|heatbath [degree] staggered
// A trailing triple `stout <n_levels> <rho>`, behind everything else, puts the Wilson fermions on stout-smeared links (include/qmg/stout.hpp): it
// is taken off before the wilson|staggered word is looked at and is refused with `staggered`.  The run then prints, before the trajectories,
//   [STOUT] levels <n_levels> rho <rho>
// and at the end the plaquette of the last configuration's thin links beside that of the links its fermions saw:
//   [STOUT-READBACK] plaq <thin> fat <smeared>
// (stout_smear_u1 on the written links); with an out.dat the smeared links go to out.dat.stout in the same format.
//   ./schwinger_hmc L beta mass n_flavours n_traj n_therm n_steps seed out.dat cold|heatbath [degree lo [hi]] [wilson] stout <n_levels> <rho>
// A trailing triple `integrator <leapfrog|omelyan> <n_gauge>`, behind everything else (the stout triple included), chooses the molecular dynamics
// (HmcCore::set_integrator): the scheme, and with n_gauge >= 1 that many gauge steps inside every drift of the fermion scale.  The run then prints
//   [INTEGRATOR] scheme <leapfrog|omelyan> n_gauge <n_gauge>
// before the trajectories.  Without it: leapfrog on one scale.
#include <cstdlib>
#include <cmath>
#include <iomanip>
#include <iostream>
#include <string>
#include <vector>

#include "../include/qmg/qmg.hpp"
#include "driver_common.hpp"
#include "hmc_run_common.hpp"

using namespace std;

// SchwingerHMC proves with range_check that the spectrum is inside the caller's interval; the staggered interval [m^2, m^2 + 4] is exact and takes no check
static bool range_check_line(SchwingerHMC& hmc) {
  const RhmcRangeCheck c = hmc.range_check();
  cout << "[RHMC-CHECK] ratio " << c.ratio << " bound " << c.bound << " ok " << (c.ok ? 1 : 0) << "\n";
  return c.ok;
}

int main(int argc, char** argv) {
  qmg_driver::Guard guard;
  const hmc_run::Integrator integrator = hmc_run::Integrator::peel(argc, argv);   // the trailing `integrator <leapfrog|omelyan> <n_gauge>`, if any
  // the smearing is the last triple, the discretisation the last argument in front of it, behind out.dat and cold|heatbath
  int stout_levels = 0;
  double stout_rho = 0.0;
  const bool stout = argc > 3 && string(argv[argc - 3]) == "stout";
  if (stout) { stout_levels = atoi(argv[argc - 2]); stout_rho = atof(argv[argc - 1]); argc -= 3; }
  bool staggered = false;
  if (argc > 11 && (string(argv[argc - 1]) == "staggered" || string(argv[argc - 1]) == "wilson")) { staggered = string(argv[argc - 1]) == "staggered"; argc--; }
  if (argc < 9) { cout << "usage: ./schwinger_hmc L beta mass n_flavours n_traj n_therm n_steps seed [out.dat [cold|heatbath]]\n"; return -1; }
  if (stout && staggered) { cout << "[QMG-ERROR]: stout smearing is for the Wilson fermions; `staggered` does not take it.\n"; return -1; }
  if (!qmg::ok(qmg_init(0), "qmg_init")) return 2;
  const int L = stoi(argv[1]);
  const double beta = stod(argv[2]), mass = stod(argv[3]);
  const int n_flavours = stoi(argv[4]), n_traj = stoi(argv[5]), n_therm = stoi(argv[6]), n_steps = stoi(argv[7]);
  HeatbathRng generator(stoull(argv[8]));
  const string out_cfg = (argc > 9) ? argv[9] : "";
  const bool cold = (argc > 10) && string(argv[10]) == "cold";
  const double tau = 1.0, cg_eps = 1e-10;
  const int cg_max_iter = 20000;
  int rhmc_degree = 8;
  double rhmc_lo = 0.0, rhmc_hi = 0.0;
  if (n_flavours == 1) {
    if (getenv("QMG_RHMC_DEGREE")) rhmc_degree = atoi(getenv("QMG_RHMC_DEGREE"));
    if (getenv("QMG_RHMC_LO")) rhmc_lo = atof(getenv("QMG_RHMC_LO"));
    if (argc > 11) rhmc_degree = stoi(argv[11]);
    if (argc > 12) rhmc_lo = stod(argv[12]);
    if (argc > 13) rhmc_hi = stod(argv[13]);
  }

  Lattice2D lat_gauge(L, L, 1);
  const size_t n_links = (size_t)lat_gauge.get_size_gauge();
  double* phases = allocate_vector<double>(n_links);
  qmg::ok(qmg_memset_zero(phases, sizeof(double) * n_links, qmg::current_stream()), "qmg_memset_zero");
  if (!cold) heatbath_noncompact_update(phases, &lat_gauge, beta, 100, generator);

  int rc = 0;
  if (staggered) {
    StaggeredSchwingerHMC hmc(phases, L, L, beta, mass, n_flavours, tau, n_steps, cg_eps, cg_max_iter, generator, rhmc_degree);
    if (!hmc.ok() || !integrator.apply(hmc)) return qmg_driver::leave(3);
    integrator.line();
    rc = hmc_run::run<StaggeredSchwingerHMC>(hmc, lat_gauge, n_flavours == 1, nullptr, 0.5 * L * L, n_traj, n_therm, out_cfg);
  } else {
    SchwingerHMC hmc(phases, L, L, beta, mass, n_flavours, tau, n_steps, cg_eps, cg_max_iter, generator, rhmc_degree, rhmc_lo, rhmc_hi, stout_levels, stout_rho);
    if (!hmc.ok() || !integrator.apply(hmc)) return qmg_driver::leave(3);
    integrator.line();
    if (stout) cout << "[STOUT] levels " << stout_levels << " rho " << stout_rho << "\n";
    rc = hmc_run::run<SchwingerHMC>(hmc, lat_gauge, n_flavours == 1, n_flavours == 1 ? range_check_line : nullptr, 2.0 * L * L, n_traj, n_therm, out_cfg);
    if (stout) {   // the links the fermions of the last configuration saw
      complex<double>* fat = allocate_vector<complex<double>>(n_links);
      stout_smear_u1(fat, hmc.links(), &lat_gauge, stout_rho, stout_levels);
      cout << "[STOUT-READBACK] plaq " << std::real(get_plaquette_u1(hmc.links(), &lat_gauge)) << " fat " << std::real(get_plaquette_u1(fat, &lat_gauge)) << "\n";
      if (!out_cfg.empty()) write_gauge_u1(fat, &lat_gauge, out_cfg + ".stout");
      deallocate_vector(&fat);
    }
  }
  deallocate_vector(&phases);
  qmg::VecPool::release_all();
  return qmg_driver::leave(rc);
}
