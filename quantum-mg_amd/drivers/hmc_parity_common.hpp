// hmc_parity_common.hpp -- what hmc_parity, rhmc_parity and stag_hmc_parity share: raw files in the device layout to and from device vectors,
// and the modes that read the same on every HMC class (md, heatbath, rational, the [RHMC] line).  Each returns the program's exit status so far:
// 0, 1 if a solve did not converge, 3 if an input file could not be read.
#ifndef QMG_HMC_PARITY_COMMON_HPP
#define QMG_HMC_PARITY_COMMON_HPP

#include <cstdio>
#include <iomanip>
#include <iostream>
#include <string>
#include <vector>

#include "../include/qmg/qmg.hpp"
#include "driver_common.hpp"
#include "hmc_run_common.hpp"   // the trailing `integrator <scheme> <n_gauge>` group

namespace hmc_parity {

template <typename T> bool load(const std::string& path, T* dev, size_t n) {
  std::vector<T> h(n);
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) { std::cout << "[QMG-ERROR]: cannot open " << path << "\n"; return false; }
  const size_t got = fread(h.data(), sizeof(T), n, f);
  fclose(f);
  if (got != n) { std::cout << "[QMG-ERROR]: " << path << " is too short\n"; return false; }
  qmg::upload(dev, h.data(), n);
  return true;
}
template <typename T> void dump(const std::string& path, const T* dev, size_t n) {
  std::vector<T> h = qmg::to_host(dev, n);
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) { std::cout << "[QMG-ERROR]: cannot open " << path << " for writing\n"; return; }
  fwrite(h.data(), sizeof(T), n, f);
  fclose(f);
}

template <class HMC> void rhmc_line(HMC& hmc) {
  const qmg::ZolotarevInvSqrt& z = hmc.rational();
  std::cout << "[RHMC] n " << z.n << " ra " << z.ra << " rb " << z.rb << " c0 " << z.c0 << " delta " << z.delta << "\n";
}

// md_evolve forward from `pi` and `phi` (theta_fwd.bin, pi_fwd.bin), the momenta negated, md_evolve again (theta_back.bin, pi_back.bin)
template <class HMC> int md_legs(HMC& hmc, const std::string& dir, double* phases, double* pi, complex<double>* phi, size_t n_links) {
  int rc = 0;
  for (int leg = 0; leg < 2 && !rc; leg++) {
    const HmcResult r = hmc.md_evolve(pi, phi);
    std::cout << "[MD] " << (leg ? "back" : "forward") << " dH " << r.dH << " cg " << r.cg_iterations << " converged " << (r.cg_converged ? 1 : 0) << " plaq " << r.plaquette << "\n";
    dump(dir + (leg ? "/theta_back.bin" : "/theta_fwd.bin"), phases, n_links);
    dump(dir + (leg ? "/pi_back.bin" : "/pi_fwd.bin"), pi, n_links);
    if (!r.cg_converged) rc = 1;
    cax(-1.0, (complex<double>*)pi, n_links / 2);   // flip the momenta
  }
  return rc;
}

// eta.bin (n_eta components) to `a`, the pseudofermion to `b` and phi.bin (n_phi components)
template <class HMC> int heatbath_mode(HMC& hmc, const std::string& dir, complex<double>* a, complex<double>* b, size_t n_eta, size_t n_phi) {
  if (!load(dir + "/eta.bin", a, n_eta)) return 3;
  HmcResult r = hmc.heatbath(b, a);
  const double spf = hmc.pseudofermion_action(b, r);
  std::cout << "[HB] eta2 " << norm2sq(a, n_eta) << " spf " << spf << " cg " << r.cg_iterations << " converged " << (r.cg_converged ? 1 : 0) << "\n";
  dump(dir + "/phi.bin", b, n_phi);
  return r.cg_converged ? 0 : 1;
}

// v.bin (n components) to `a`; r v to `b` and rv.bin, r r v to `a` and rrv.bin
template <class HMC> int rational_mode(HMC& hmc, const std::string& dir, complex<double>* a, complex<double>* b, size_t n) {
  if (!load(dir + "/v.bin", a, n)) return 3;
  const HmcResult r = hmc.apply_rational(b, a);
  dump(dir + "/rv.bin", b, n);
  const HmcResult r2 = hmc.apply_rational(a, b);
  dump(dir + "/rrv.bin", a, n);
  const bool conv = r.cg_converged && r2.cg_converged;
  std::cout << "[RAT] cg " << r.cg_iterations + r2.cg_iterations << " converged " << (conv ? 1 : 0) << "\n";
  return conv ? 0 : 1;
}

inline int unknown_mode(const std::string& mode) {
  std::cout << "[QMG-ERROR]: unknown mode " << mode << "\n";
  return 5;
}

}  // namespace hmc_parity

#endif
