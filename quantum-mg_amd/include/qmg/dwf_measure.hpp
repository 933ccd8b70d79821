// dwf_measure.hpp -- domain-wall quark propagators and what is measured on them (csrc/qmg_dwf_meas.hip under DwfBase::wall_source /
// wall_project / slice_norms).  Component c = 2 s + sigma, sigma = 0 the P_+ component.
//   wall source      B(x; 0, 0) = eta(x, 0),  B(x; Ls-1, 1) = eta(x, 1)
//   physical quark   q(x, 0) = Psi(x; Ls-1, 0),  q(x, 1) = Psi(x; 0, 1)              Psi = D^-1 B
//   midpoint         q_mp(x, 0) = Psi(x; Ls/2-1, 0),  q_mp(x, 1) = Psi(x; Ls/2, 1)   (even Ls)
//   slice norms      N(y, s, sigma) = sum_x |Psi(x, y; s, sigma)|^2
// For a point source and both source spins, by Gamma5-hermiticity,
//   C_pi(t) = sum_spins N(t, Ls-1, 0) + N(t, 0, 1),   C_mp(t) = sum_spins N(t, Ls/2-1, 0) + N(t, Ls/2, 1),   m_res = sum_t C_mp / sum_t C_pi,
// and sum_{t, sigma} N(t, s, sigma) / sum N is how the propagator is bound to the walls.
// Every solve checks itself against the integrated axial Ward identity, exact on every gauge field for even Ls and real m:
//   m |q|^2 + |q_mp|^2 = Re <eta, q>;    for an approximate Psi~ with r = B - D Psi~:   |lhs - rhs| = |Re <Psi~, Gamma5 E r>| <= |Psi~| |r|
// (E = +1 for s < Ls/2, -1 otherwise), whatever the spectrum of D.
#ifndef QMG_DWF_MEASURE_HPP
#define QMG_DWF_MEASURE_HPP

#include <cmath>
#include <iomanip>
#include <iostream>
#include <limits>
#include <vector>

#include "operators.hpp"

struct dwf_quark_info {
  inversion_info inv;          // of minv_dwf_eo_cg
  double true_residual;        // |B - D Psi|, D from the links
  double psi_norm;             // |Psi|
  double ward_lhs, ward_rhs;   // m |q|^2 + |q_mp|^2 (from the slice norms) and Re <eta, q>; NaN for odd Ls or a complex wall mass
  double ward_defect;          // lhs - rhs
  std::vector<double> norms;   // N[(y Ls + s) 2 + sigma] of Psi
  dwf_quark_info() : true_residual(0.0), psi_norm(0.0), ward_lhs(0.0), ward_rhs(0.0), ward_defect(0.0) {}
};

// q4 = the physical quark field of D^-1 (wall source of eta4): source, minv_dwf_eo_cg from a zero guess, projection.  q4, eta4: 4D (nc = 2)
// vectors on lat4, the lattice of dwf with nc = 2; psi5: where the 5D solution goes (overwritten), or null.  eps as in minv_dwf_eo_cg.
inline dwf_quark_info minv_dwf_quark(complex<double>* q4, complex<double>* eta4, complex<double>* psi5, int max_iter, double eps, DwfBase* dwf, Lattice2D* lat4) {
  dwf_quark_info info;
  Lattice2D* lat5 = dwf->lat;
  const int Ls = dwf->get_Ls(), Ly = lat5->get_dim_mu(1);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  if (lat4->get_nc() != 2 || lat4->get_dim_mu(0) != lat5->get_dim_mu(0) || lat4->get_dim_mu(1) != Ly) {
    std::cout << "[QMG-ERROR]: minv_dwf_quark needs the operator's lattice with nc = 2 for the 4D fields.\n";
    info.ward_lhs = info.ward_rhs = info.ward_defect = nan;
    return info;
  }
  const size_t n5 = (size_t)lat5->get_size_cv_l(), n4 = (size_t)lat4->get_size_cv_l();
  complex<double>* b = allocate_vector<complex<double>>(n5);
  complex<double>* psi = psi5 ? psi5 : allocate_vector<complex<double>>(n5);
  dwf->wall_source(b, eta4);
  zero_vector(psi, n5);
  info.inv = minv_dwf_eo_cg(psi, b, max_iter, eps, dwf);
  dwf->wall_project(q4, psi, false);
  // the true residual on the full operator from the links
  complex<double>* dpsi = allocate_vector<complex<double>>(n5);
  const qmg_stencil_desc d = dwf->desc();
  qmg::ok(qmg_dwf_apply_direct(QMG_C64, &d, dwf->direct.gauge, Ls, dwf->get_mass().real(), dwf->get_mass().imag(), dwf->direct.w, dpsi, psi, QMG_P_ALL | QMG_P_ZERO, 1, 0,
                               1u, qmg::current_stream()), "qmg_dwf_apply_direct");
  info.true_residual = std::sqrt(diffnorm2sq(dpsi, b, n5));
  info.psi_norm = std::sqrt(norm2sq(psi, n5));
  info.norms.assign((size_t)2 * Ls * Ly, 0.0);
  dwf->slice_norms(info.norms.data(), psi);
  if ((Ls & 1) || dwf->get_mass().imag() != 0.0) {
    std::cout << "[QMG-INFO]: minv_dwf_quark: the axial Ward identity needs an even Ls and a real wall mass; its fields are NaN.\n";
    info.ward_lhs = info.ward_rhs = info.ward_defect = nan;
  } else {
    double q2 = 0.0, mp2 = 0.0;
    for (int y = 0; y < Ly; y++) {
      const double* N = info.norms.data() + (size_t)y * 2 * Ls;
      q2 += N[2 * (Ls - 1)] + N[1];
      mp2 += N[2 * (Ls / 2 - 1)] + N[2 * (Ls / 2) + 1];
    }
    info.ward_lhs = dwf->get_mass().real() * q2 + mp2;
    info.ward_rhs = dot(eta4, q4, n4).real();
    info.ward_defect = info.ward_lhs - info.ward_rhs;
  }
  deallocate_vector(&dpsi); deallocate_vector(&b);
  if (!psi5) deallocate_vector(&psi);
  return info;
}

// C_pi(t), C_mp(t) and the fifth-dimension profile N(s), accumulated over source spins and configurations from the slice norms of the solves
struct DwfCorrelators {
  int Ly, Ls, count;                      // count: the add() calls
  std::vector<double> pion, mid, prof;    // sums over what was added; mid is NaN for odd Ls
  DwfCorrelators(int Ly, int Ls) : Ly(Ly), Ls(Ls), count(0), pion(Ly, 0.0), mid(Ly, (Ls & 1) ? std::numeric_limits<double>::quiet_NaN() : 0.0), prof(Ls, 0.0) {}
  void add(const std::vector<double>& norms) {
    for (int y = 0; y < Ly; y++) {
      const double* N = norms.data() + (size_t)y * 2 * Ls;
      pion[y] += N[2 * (Ls - 1)] + N[1];
      if (!(Ls & 1)) mid[y] += N[2 * (Ls / 2 - 1)] + N[2 * (Ls / 2) + 1];
      for (int s = 0; s < Ls; s++) prof[s] += N[2 * s] + N[2 * s + 1];
    }
    count++;
  }
  void add(const dwf_quark_info& info) { add(info.norms); }
  double m_res() const {
    double p = 0.0, m = 0.0;
    for (int y = 0; y < Ly; y++) { p += pion[y]; m += mid[y]; }
    return m / p;
  }
  // the blocks of drivers/dwf_measure; configs: the correlators are printed per configuration (two source spins each)
  void print(std::ostream& os, int configs = 1) const {
    const std::ios::fmtflags f = os.flags();
    const std::streamsize pr = os.precision();
    os << std::scientific << std::setprecision(16);
    os << "[QMG-BEGIN-PION]\n";
    for (int y = 0; y < Ly; y++) os << y << " " << pion[y] / configs << "\n";
    os << "[QMG-END-PION]\n[QMG-BEGIN-MIDPOINT]\n";
    for (int y = 0; y < Ly; y++) os << y << " " << mid[y] / configs << "\n";
    os << "[QMG-END-MIDPOINT]\n[QMG-BEGIN-MRES]\n";
    for (int y = 0; y < Ly; y++) os << y << " " << mid[y] / pion[y] << "\n";
    os << "[QMG-END-MRES]\n[QMG-BEGIN-SPROFILE]\n";
    double total = 0.0;
    for (int s = 0; s < Ls; s++) total += prof[s];
    for (int s = 0; s < Ls; s++) os << s << " " << prof[s] / total << "\n";
    os << "[QMG-END-SPROFILE]\n[QMG-BEGIN-PION-EFFMASS]\n";
    for (int y = 1; y < Ly - 1; y++) os << y << " " << std::acosh((pion[y + 1] + pion[y - 1]) / (2.0 * pion[y])) << "\n";
    os << "[QMG-END-PION-EFFMASS]\n";
    os << "[QMG-MRES]: " << m_res() << "\n";
    os.flags(f);
    os.precision(pr);
  }
};

#endif
