// dwf_eo_selftest -- the even-odd Schur complement of the domain-wall operator (DwfBase, include/qmg/operators.hpp; csrc/qmg_dwf_eo.hip) held to
// the full operator from the links on one Gaussian U(1) configuration, and the solve on it held to the solve on D^dagger D.
//   ./dwf_eo_selftest L Ls mass seed [rounds]
// One line per check, `[QMG-DWF-EO] name value PASS|FAIL`; the exit status is nonzero on any FAIL.
//   (a) schur_vs_D_odd, schur_vs_D   for Gaussian x_e, v = [x_e; -A^-1 H_oe x_e] (qmg_dwf_hops_inv5) through apply_M from the links:
//                          |(D v)_o| / |H_oe x_e| and the relative l2 difference of (D v)_e to apply_M_schur5(x_e), both < 1e-13.  v_o is the same
//                          kernel-K result on both sides; on top of it either side sums the <= 3 fifth-dimension terms of A and 8 hop
//                          terms per element in fp64 (the odd half: 2 Ls + 10 terms of A A^-1 H cancelling against 8 of H), so the difference
//                          is rounding of O(Ls) terms: a few 1e-16 relative to the norms.
//   (b) schur_gamma5_hermiticity   |<y, M^dagger x> - <M y, x>| / (|y| |M^dagger x|) on the even half (real mass): < 1e-12.
//   (c) eo_iterations, eo_true_residual   minv_dwf_eo_cg to 1e-10; |b - D x| / |b| with the full D from the links <= 1e-8 (the stopping test
//                          is on the normal equations of M, hence the slack).
//   (d) full_iterations, full_true_residual, eo_vs_full_solution   CG on D^dagger D (apply_stencil_2D_M_dagger_M, the stored dagger stencil) on the
//                          same b, its tolerance tightened until its true residual on D is at or below (c)'s (aiming at [1/2, 1] of it):
//                          eo_iterations < full_iterations, and the two solutions differ by <= 1e-7 in relative l2.  full_true_residual
//                          is reported, not gated.  Where the stored nc = 2 Ls apply does not exist (Ls = 32) there is no such solve
//                          and (d) is not printed.
// With `rounds` the two solves of (c) and (d) are then timed alternately, wall clock around each (tools/dwf_eo_bench.py): one line
// `[QMG-DWF-EO-BENCH] round r eo_ms t full_ms t` per round.  The dagger stencil and D^dagger b are made before the clock starts.
#include <iomanip>
#include <string>

#include "dw_selftest_common.hpp"

using namespace std;

static dw_selftest::Lines line("[QMG-DWF-EO]");

int main(int argc, char** argv) {
  qmg_driver::Guard guard;
  if (argc < 5) { cout << "usage: ./dwf_eo_selftest L Ls mass seed [rounds]\n"; return -1; }
  const int rounds = argc > 5 ? stoi(argv[5]) : 0;
  cout << setprecision(17);
  if (!qmg::ok(qmg_init(0), "qmg_init")) return 2;
  const int L = stoi(argv[1]), Ls = stoi(argv[2]);
  const double mass = stod(argv[3]);
  const unsigned long long seed = stoull(argv[4]);
  Lattice2D lat_g(L, L, 1), lat(L, L, 2 * Ls);
  dw_selftest::Vectors vec;
  complex<double>* gauge = vec.make(lat_g.get_size_gauge());
  // link phases N(0, 0.4^2)
  if (!qmg::ok(qmg_u1_gauss_gauge(gauge, L, L, 1.0 / (0.4 * 0.4), seed, qmg::current_stream()), "qmg_u1_gauss_gauge")) return 3;
  // Ls = 32 (nc = 64) is beyond the stored-stencil apply, so createDwfLs declines it; the links route and the Schur methods do not need it
  const bool stored = Ls != 32;
  Stencil2D* made = stored ? createDwfLs(&lat, mass, gauge, Ls) : new Dwf2D<32>(&lat, mass, gauge);
  DwfBase* dwf = dynamic_cast<DwfBase*>(made);
  if (!dwf || !dwf->generated) { cout << "[QMG-DWF-EO] create 0 FAIL\n"; return 4; }
  const int n = (int)lat.get_size_cv_l(), half = n / 2;
  complex<double>*x = vec.make(n), *y = vec.make(n), *v = vec.make(n), *t1 = vec.make(n), *t2 = vec.make(n), *b = vec.make(n), *xe = vec.make(n), *xf = vec.make(n);
  gaussian(x, n, seed + 101);
  gaussian(y, n, seed + 102);
  gaussian(b, n, seed + 200);
  const bool direct_on = dwf->direct.on && dwf->direct.kind == Stencil2D::QMG_DIRECT_DWF;
  const qmg_stencil_desc d = dwf->desc();

  qmg_driver::phase("schur vs D");
  copy_vector(v, x, n);
  qmg::ok(qmg_dwf_hops_inv5(QMG_C64, &d, dwf->direct.gauge, Ls, mass, 0.0, dwf->direct.w, v, v, QMG_P_OE | QMG_P_ZERO_O, -1.0, 0.0, 0, 1, 0, 1u, qmg::current_stream()),
          "qmg_dwf_hops_inv5");
  dwf->apply_M_overwrite(t1, v);                                     // D v: the odd half vanishes, the even half is M x_e
  qmg::ok(qmg_dwf_apply_direct(QMG_C64, &d, dwf->direct.gauge, Ls, mass, 0.0, dwf->direct.w, t2, x, QMG_P_OE | QMG_P_ZERO_O, 1, 0, 1u, qmg::current_stream()),
          "qmg_dwf_apply_direct");
  const double odd = sqrt(norm2sq(t1 + half, half) / norm2sq(t2 + half, half));
  zero_vector(t2, n);
  dwf->apply_M_schur5(t2, x);
  const double even = sqrt(diffnorm2sq(t1, t2, half) / norm2sq(t2, half));

  qmg_driver::phase("gamma5");
  zero_vector(t1, n);
  dwf->apply_M_schur5_dagger(t1, x);
  dwf->apply_M_schur5(t2, y);
  const complex<double> lhs = dot(y, t1, half), rhs = dot(t2, x, half);
  const double herm = abs(lhs - rhs) / sqrt(norm2sq(y, half) * norm2sq(t1, half));

  qmg_driver::phase("eo cg");
  const int max_iter = 5000;
  const double eps = 1e-10;
  zero_vector(xe, n);
  const inversion_info eo = minv_dwf_eo_cg(xe, b, max_iter, eps, dwf);
  const double bnorm = norm2sq(b, n);
  const double eo_res = dw_selftest::true_residual(dwf, t1, xe, b, n, bnorm);

  inversion_info full = eo;
  double full_res = 0.0, sol_diff = 0.0, eps_full = eps;
  const auto full_solve = [&](complex<double>* sol, double tol) { return minv_vector_cg(sol, t2, n, max_iter, tol, apply_stencil_2D_M_dagger_M, (void*)dwf); };
  if (stored) {
    qmg_driver::phase("full cg");
    dwf->build_dagger_stencil();
    zero_vector(t2, n);
    dwf->apply_M_dagger(t2, b);                                      // the right-hand side of the normal equations
    full = dw_selftest::tightened_solve(dwf, xf, t1, b, n, bnorm, eo_res, eps_full, full_res, full_solve);
    sol_diff = sqrt(diffnorm2sq(xe, xf, n) / norm2sq(xf, n));
  }

  line("direct_route_on", direct_on ? 1.0 : 0.0, direct_on);
  line("schur_vs_D_odd", odd, odd < 1e-13);
  line("schur_vs_D", even, even < 1e-13);
  line("schur_gamma5_hermiticity", herm, herm < 1e-12);
  line("eo_iterations", (double)eo.iter, eo.success && eo.iter < max_iter && (!stored || eo.iter < full.iter));
  line("eo_true_residual", eo_res, eo_res <= 1e-8);
  if (stored) {
    line("full_iterations", (double)full.iter, full.success && full.iter < max_iter);
    line("full_true_residual", full_res, true);   // a figure: how closely the comparison solve was matched to (c)
    line("eo_vs_full_solution", sol_diff, sol_diff <= 1e-7);
  }

  if (stored && rounds > 0)
    dw_selftest::timing_rounds("[QMG-DWF-EO-BENCH]", rounds, n, xe, xf, [&](complex<double>* sol) { minv_dwf_eo_cg(sol, b, max_iter, eps, dwf); },
                               [&](complex<double>* sol) { full_solve(sol, eps_full); });

  delete made;
  vec.release();
  qmg::VecPool::release_all();
  return qmg_driver::leave(line.all_pass ? 0 : 1);
}
