// hmc_run_common.hpp -- what schwinger_hmc and dwf_hmc share: the trajectories of an ensemble run, their lines, the final lines and the
// written configuration, for every HMC class on HmcCore.
#ifndef QMG_HMC_RUN_COMMON_HPP
#define QMG_HMC_RUN_COMMON_HPP

#include <cmath>
#include <cstdlib>
#include <iomanip>
#include <iostream>
#include <string>
#include <vector>

#include "../include/qmg/qmg.hpp"

namespace hmc_run {

// The trailing group `integrator <leapfrog|omelyan> <n_gauge>` of a command line (HmcCore::set_integrator), behind everything else: peel()
// takes it off argc before anything else is looked at; apply() sets it on an HMC object.  Without the group nothing is set.
struct Integrator {
  bool given, known;
  MdScheme scheme;
  int n_gauge;
  Integrator() : given(false), known(true), scheme(MD_LEAPFROG), n_gauge(0) {}
  const char* scheme_name() const { return scheme == MD_OMELYAN ? "omelyan" : "leapfrog"; }
  static Integrator peel(int& argc, char** argv) {
    Integrator in;
    if (argc > 3 && std::string(argv[argc - 3]) == "integrator") {
      const std::string word = argv[argc - 2];
      in.given = true;
      in.known = word == "leapfrog" || word == "omelyan";
      in.scheme = word == "omelyan" ? MD_OMELYAN : MD_LEAPFROG;
      in.n_gauge = atoi(argv[argc - 1]);
      argc -= 3;
    }
    return in;
  }
  // false (and a line) if the group names no scheme or the object refuses it
  template <class HMC> bool apply(HMC& hmc) const {
    if (!given) return true;
    if (!known) { std::cout << "[QMG-ERROR]: integrator takes leapfrog or omelyan.\n"; return false; }
    return hmc.set_integrator(scheme, n_gauge);
  }
  void line() const {
    if (given) std::cout << "[INTEGRATOR] scheme " << scheme_name() << " n_gauge " << n_gauge << "\n";
  }
};

// the trajectories, the final lines and the written configuration; returns the exit status.  one_flavour: a rational action, whose [RHMC] line
// is printed first (rhmc_sites: the exponent of its determinant bound).  range_check: null, or what proves after the thermalisation and at
// the end that the spectrum is inside the rational function's interval (false counts as a failure).
template <class HMC>
int run(HMC& hmc, Lattice2D& lat_gauge, bool one_flavour, bool (*range_check)(HMC&), double rhmc_sites, int n_traj, int n_therm, const std::string& out_cfg) {
  using namespace std;
  const size_t n_links = (size_t)lat_gauge.get_size_gauge();
  int unconverged = 0, accepted = 0, range_failures = 0;
  vector<double> w, plaq;
  cout << setprecision(10);
  auto rhmc_check = [&]() {
    if (!range_check(hmc)) range_failures++;
  };
  if (one_flavour) {
    const qmg::ZolotarevInvSqrt& z = hmc.rational();
    cout << "[RHMC] n " << z.n << " ra " << z.ra << " rb " << z.rb << " delta " << z.delta << " det_bound " << expm1(rhmc_sites * log1p(z.delta)) << "\n";
  }
  for (int i = 0; i < n_therm + n_traj; i++) {
    if (range_check && i == n_therm && n_therm > 0) rhmc_check();
    const HmcResult r = hmc.trajectory();
    cout << "[HMC] " << i << " dH " << r.dH << " acc " << (r.accepted ? 1 : 0) << " plaq " << r.plaquette << " Q " << r.topo << " cg " << r.cg_iterations << "\n";
    if (!r.cg_converged) unconverged++;
    if (i >= n_therm) { accepted += r.accepted ? 1 : 0; w.push_back(exp(-r.dH)); plaq.push_back(r.plaquette); }
  }
  // jackknife over single trajectories (for a plain mean: the standard error)
  auto mean_err = [](const vector<double>& v, double& m, double& e) {
    const size_t n = v.size();
    m = 0.0; e = 0.0;
    if (!n) return;
    for (double x : v) m += x;
    m /= (double)n;
    if (n < 2) return;
    double s = 0.0;
    for (double x : v) { const double jk = (m * (double)n - x) / (double)(n - 1); s += (jk - m) * (jk - m); }
    e = sqrt(s * (double)(n - 1) / (double)n);
  };
  double wm, we, pm, pe;
  mean_err(w, wm, we);
  mean_err(plaq, pm, pe);
  cout << "[HMC-FINAL] trajectories " << n_traj << " acceptance " << (n_traj ? (double)accepted / n_traj : 0.0) << " exp_mdH " << wm << " +/- " << we << " plaq " << pm << " +/- " << pe
       << " unconverged " << unconverged << "\n";
  if (range_check) rhmc_check();
  if (!out_cfg.empty()) {   // written, and read back the way the other drivers will read it
    write_gauge_u1(hmc.links(), &lat_gauge, out_cfg);
    complex<double>* check = allocate_vector<complex<double>>(n_links);
    if (read_gauge_u1(check, &lat_gauge, out_cfg)) cout << "[HMC-READBACK] plaq " << std::real(get_plaquette_u1(check, &lat_gauge)) << " Q " << get_topo_u1(check, &lat_gauge) << "\n";
    deallocate_vector(&check);
  }
  return unconverged == 0 && range_failures == 0 ? 0 : 1;
}

}  // namespace hmc_run

#endif
