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
// Exit status 1 if a solve did not converge.
#include <cstdio>
#include <iomanip>
#include <iostream>
#include <string>
#include <vector>

#include "../include/qmg/qmg.hpp"
#include "driver_common.hpp"

using namespace std;

template <typename T> static bool load(const string& path, T* dev, size_t n) {
  vector<T> h(n);
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) { cout << "[QMG-ERROR]: cannot open " << path << "\n"; return false; }
  const size_t got = fread(h.data(), sizeof(T), n, f);
  fclose(f);
  if (got != n) { cout << "[QMG-ERROR]: " << path << " is too short\n"; return false; }
  qmg::upload(dev, h.data(), n);
  return true;
}
template <typename T> static void dump(const string& path, const T* dev, size_t n) {
  vector<T> h = qmg::to_host(dev, n);
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) { cout << "[QMG-ERROR]: cannot open " << path << " for writing\n"; return; }
  fwrite(h.data(), sizeof(T), n, f);
  fclose(f);
}

int main(int argc, char** argv) {
  qmg_driver::Guard guard;
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
    if (!hmc.ok()) rc = 4;
    cout << setprecision(17);
    if (!rc && n_tastes == 1) {
      const qmg::ZolotarevInvSqrt& z = hmc.rational();
      cout << "[RHMC] n " << z.n << " ra " << z.ra << " rb " << z.rb << " c0 " << z.c0 << " delta " << z.delta << "\n";
    }
    if (!rc && mode == "md") {
      if (!load(dir + "/pi.bin", pi, n_links) || !load(dir + "/phi.bin", a, half)) rc = 3;
      for (int leg = 0; leg < 2 && !rc; leg++) {
        const HmcResult r = hmc.md_evolve(pi, a);
        cout << "[MD] " << (leg ? "back" : "forward") << " dH " << r.dH << " cg " << r.cg_iterations << " converged " << (r.cg_converged ? 1 : 0) << " plaq " << r.plaquette << "\n";
        dump(dir + (leg ? "/theta_back.bin" : "/theta_fwd.bin"), phases, n_links);
        dump(dir + (leg ? "/pi_back.bin" : "/pi_fwd.bin"), pi, n_links);
        if (!r.cg_converged) rc = 1;
        cax(-1.0, (complex<double>*)pi, n_links / 2);   // flip the momenta
      }
    } else if (!rc && mode == "heatbath") {
      if (!load(dir + "/eta.bin", a, cv)) rc = 3;
      if (!rc) {
        HmcResult r = hmc.heatbath(b, a);
        const double spf = hmc.pseudofermion_action(b, r);
        cout << "[HB] eta2 " << norm2sq(a, cv) << " spf " << spf << " cg " << r.cg_iterations << " converged " << (r.cg_converged ? 1 : 0) << "\n";
        dump(dir + "/phi.bin", b, half);
        if (!r.cg_converged) rc = 1;
      }
    } else if (!rc && mode == "rational") {
      if (!load(dir + "/v.bin", a, half)) rc = 3;
      if (!rc) {
        HmcResult r = hmc.apply_rational(b, a);
        dump(dir + "/rv.bin", b, half);
        const HmcResult r2 = hmc.apply_rational(a, b);
        dump(dir + "/rrv.bin", a, half);
        const bool conv = r.cg_converged && r2.cg_converged;
        cout << "[RAT] cg " << r.cg_iterations + r2.cg_iterations << " converged " << (conv ? 1 : 0) << "\n";
        if (!conv) rc = 1;
      }
    } else if (!rc) {
      cout << "[QMG-ERROR]: unknown mode " << mode << "\n";
      rc = 5;
    }
  }
  deallocate_vector(&phases); deallocate_vector(&pi); deallocate_vector(&a); deallocate_vector(&b);
  qmg::VecPool::release_all();
  return qmg_driver::leave(rc);
}
