// dwf_measure -- domain-wall quark propagators on one U(1) configuration: pion and midpoint correlators, the residual mass, the
// fifth-dimension profile, and the integrated axial Ward identity of every solve (include/qmg/dwf_measure.hpp).
//   ./dwf_measure L cfg_file mass Ls [M5 eps max_iter]
// cfg_file: one gauge field in the reference's text format (read_gauge_u1).  Point source at the origin, both source spins, each through
// minv_dwf_quark (wall source, CG on the even-odd Schur complement from the links, wall projection).  Defaults: M5 -1, eps 1e-10, max_iter 20000.
// Output (17 significant digits):
//   [QMG-WARD]: spin iterations true_residual psi_norm lhs rhs defect      one line per solve: m |q|^2 + |q_mp|^2 against Re <eta, q>
//   [QMG-BEGIN-PION] / [QMG-BEGIN-MIDPOINT] / [QMG-BEGIN-MRES] / [QMG-BEGIN-SPROFILE] / [QMG-BEGIN-PION-EFFMASS] blocks, `index value` lines,
//   each closed by its [QMG-END-...]; C_pi(t) and C_mp(t) are not folded;   [QMG-MRES]: sum_t C_mp / sum_t C_pi
// The exit status is nonzero if a solve does not converge.  An ensemble is one run per file (u1_make_config or schwinger_hmc write them).
#include <cmath>
#include <iomanip>
#include <iostream>
#include <string>

#include "../include/qmg/qmg.hpp"
#include "driver_common.hpp"

using namespace std;

int main(int argc, char** argv) {
  qmg_driver::Guard guard;
  if (argc < 5) { cout << "usage: ./dwf_measure L cfg_file mass Ls [M5 eps max_iter]\n"; return -1; }
  if (!qmg::ok(qmg_init(0), "qmg_init")) return 2;
  const int L = stoi(argv[1]);
  const string cfg = argv[2];
  const double mass = stod(argv[3]);
  const int Ls = stoi(argv[4]);
  const double M5 = argc > 5 ? stod(argv[5]) : -1.0;
  const double eps = argc > 6 ? stod(argv[6]) : 1e-10;
  const int max_iter = argc > 7 ? stoi(argv[7]) : 20000;
  if (L < 2 || (L & 1) || Ls < 2 || Ls > 32) { cout << "[QMG-ERROR]: L must be even and Ls in 2 .. 32.\n"; return 3; }

  Lattice2D lat_g(L, L, 1), lat4(L, L, 2), lat5(L, L, 2 * Ls);
  complex<double>* gauge = allocate_vector<complex<double>>(lat_g.get_size_gauge());
  if (!read_gauge_u1(gauge, &lat_g, cfg)) return 3;
  // Ls = 32 (nc = 64) is beyond the stored-stencil apply, so createDwfLs declines it; the links route and the Schur methods do not need it
  Stencil2D* made = Ls == 32 ? new Dwf2D<32>(&lat5, mass, gauge, M5) : createDwfLs(&lat5, mass, gauge, Ls, M5);
  DwfBase* dwf = dynamic_cast<DwfBase*>(made);
  if (!dwf || !dwf->generated) { cout << "[QMG-ERROR]: no domain-wall operator for Ls = " << Ls << ".\n"; return 4; }

  const size_t n4 = (size_t)lat4.get_size_cv_l();
  complex<double>* eta = allocate_vector<complex<double>>(n4);
  complex<double>* q = allocate_vector<complex<double>>(n4);
  DwfCorrelators corr(L, Ls);
  int unconverged = 0;
  cout << scientific << setprecision(16);
  for (int spin = 0; spin < 2; spin++) {
    zero_vector(eta, n4);
    qmg::set_element(eta, (size_t)lat4.cv_coord_to_index(0, 0, spin), complex<double>(1.0, 0.0));
    const dwf_quark_info info = minv_dwf_quark(q, eta, 0, max_iter, eps, dwf, &lat4);
    if (!info.inv.success) unconverged++;
    corr.add(info);
    cout << "[QMG-WARD]: " << spin << " " << info.inv.iter << " " << info.true_residual << " " << info.psi_norm << " " << info.ward_lhs << " " << info.ward_rhs << " "
         << info.ward_defect << "\n";
  }
  corr.print(cout);
  if (unconverged) cout << "[QMG-ERROR]: " << unconverged << " of 2 solves did not converge in " << max_iter << " iterations.\n";

  delete made;
  deallocate_vector(&eta); deallocate_vector(&q); deallocate_vector(&gauge);
  qmg::VecPool::release_all();
  return qmg_driver::leave(unconverged == 0 ? 0 : 1);
}
