// mobius_eo_selftest -- the even-odd Schur complement of the Moebius domain-wall operator (MobiusBase, include/qmg/operators.hpp;
// csrc/qmg_mobius_eo.hip) held to the full operator from the links on one Gaussian U(1) configuration, and the solve on it held to the solve on
// D^dagger D, after dwf_eo_selftest.  b5 = 1.5, c5 = 0.5, M5 = -1.
//   ./mobius_eo_selftest L Ls mass seed [rounds [solution_file]]
// One line per check, `[QMG-MOBIUS-EO] name value PASS|FAIL`; the exit status is nonzero on any FAIL.
//   (a) links_route_on; schur_vs_D   for Gaussian x_e: b = [M x_e; 0] (apply_M_schur5), x = reconstruct_M_schur5(x_e, b), then D x from the links
//                          against b: |D x - b| / |b| < 1e-13.  The odd half of D x is A A^-1 H B x_e cancelling against H B x_e, the even half
//                          repeats the sums of M: rounding of O(Ls) terms per element.
//   (b) schur_adjointness  |<y, M x> - <M^dagger y, x>| / (|y| |M x|) on the even half: < 1e-12.
//   (c) eo_iterations, eo_true_residual   minv_mobius_eo_cg to 1e-10; |b - D x| / |b| with the full D from the links <= 1e-8 (the stopping test
//                          is on the normal equations of M, hence the slack).
//   (d) full_iterations, full_true_residual, eo_vs_full_solution   minv_mobius_cg (CG on D^dagger D, both applies from the links) on the same
//                          b, its tolerance tightened until its true residual on D is at or below (c)'s (aiming at [1/2, 1] of it):
//                          eo_iterations < full_iterations, and the two solutions differ by <= 1e-7 in relative l2.  full_true_residual is
//                          reported, not gated.
// With `rounds` > 0 the two solves of (c) and (d) are then timed alternately, wall clock around each (tools/mobius_eo_bench.py): one line
// `[QMG-MOBIUS-EO-BENCH] round r eo_ms t full_ms t` per round.  With a solution_file the links, b and the even-odd solution are written there
// as raw complex<double> (2 L^2, then twice 2 Ls L^2 numbers in the device layout), for a dense solve elsewhere.
#include <iomanip>
#include <string>

#include "dw_selftest_common.hpp"

using namespace std;

static dw_selftest::Lines line("[QMG-MOBIUS-EO]");

int main(int argc, char** argv) {
  qmg_driver::Guard guard;
  if (argc < 5) { cout << "usage: ./mobius_eo_selftest L Ls mass seed [rounds [solution_file]]\n"; return -1; }
  const int rounds = argc > 5 ? stoi(argv[5]) : 0;
  cout << setprecision(17);
  if (!qmg::ok(qmg_init(0), "qmg_init")) return 2;
  const int L = stoi(argv[1]), Ls = stoi(argv[2]);
  const double mass = stod(argv[3]), b5 = 1.5, c5 = 0.5;
  const unsigned long long seed = stoull(argv[4]);
  Lattice2D lat_g(L, L, 1), lat(L, L, 2 * Ls);
  dw_selftest::Vectors vec;
  complex<double>* gauge = vec.make(lat_g.get_size_gauge());
  // link phases N(0, 0.4^2)
  if (!qmg::ok(qmg_u1_gauss_gauge(gauge, L, L, 1.0 / (0.4 * 0.4), seed, qmg::current_stream()), "qmg_u1_gauss_gauge")) return 3;
  MobiusBase* mob = createMobiusLs(&lat, mass, gauge, Ls, b5, c5);
  if (!mob || !mob->generated) { cout << "[QMG-MOBIUS-EO] create 0 FAIL\n"; return 4; }
  const int n = (int)lat.get_size_cv_l(), half = n / 2;
  complex<double>*x = vec.make(n), *y = vec.make(n), *v = vec.make(n), *t1 = vec.make(n), *t2 = vec.make(n), *b = vec.make(n), *xe = vec.make(n), *xf = vec.make(n);
  gaussian(x, n, seed + 101);
  gaussian(y, n, seed + 102);
  gaussian(b, n, seed + 200);
  const bool links_on = mob->links_ready();

  qmg_driver::phase("schur vs D");
  zero_vector(t2, n);
  mob->apply_M_schur5(t2, x);                                        // b = [M x_e; 0]
  zero_vector(v, n);
  mob->reconstruct_M_schur5(v, x, t2);                               // v = [x_e; -A^-1 H_oe B x_e]
  mob->apply_M_overwrite(t1, v);                                     // D v
  const double vs_D = sqrt(diffnorm2sq(t1, t2, n) / norm2sq(t2, n));

  qmg_driver::phase("adjointness");
  zero_vector(t1, n);
  mob->apply_M_schur5(t1, x);
  mob->apply_M_schur5_dagger(t2, y);
  const complex<double> lhs = dot(y, t1, half), rhs = dot(t2, x, half);
  const double adj = abs(lhs - rhs) / sqrt(norm2sq(y, half) * norm2sq(t1, half));

  qmg_driver::phase("eo cg");
  const int max_iter = 5000;
  const double eps = 1e-10;
  zero_vector(xe, n);
  const inversion_info eo = minv_mobius_eo_cg(xe, b, max_iter, eps, mob);
  const double bnorm = norm2sq(b, n);
  const double eo_res = dw_selftest::true_residual(mob, t1, xe, b, n, bnorm);
  if (argc > 6) {
    const complex<double>* parts[3] = {gauge, b, xe};
    const size_t lens[3] = {(size_t)lat_g.get_size_gauge(), (size_t)n, (size_t)n};
    if (!dw_selftest::write_raw(argv[6], parts, lens, 3)) line("solution_file", 0.0, false);
  }

  qmg_driver::phase("full cg");
  double full_res = 0.0, eps_full = eps;
  const auto full_solve = [&](complex<double>* sol, double tol) { return minv_mobius_cg(sol, b, max_iter, tol, mob); };
  const inversion_info full = dw_selftest::tightened_solve(mob, xf, t1, b, n, bnorm, eo_res, eps_full, full_res, full_solve);
  const double sol_diff = sqrt(diffnorm2sq(xe, xf, n) / norm2sq(xf, n));

  line("links_route_on", links_on ? 1.0 : 0.0, links_on);
  line("schur_vs_D", vs_D, vs_D < 1e-13);
  line("schur_adjointness", adj, adj < 1e-12);
  line("eo_iterations", (double)eo.iter, eo.success && eo.iter < max_iter && eo.iter < full.iter);
  line("eo_true_residual", eo_res, eo_res <= 1e-8);
  line("full_iterations", (double)full.iter, full.success && full.iter < max_iter);
  line("full_true_residual", full_res, true);   // a figure: how closely the comparison solve was matched to (c)
  line("eo_vs_full_solution", sol_diff, sol_diff <= 1e-7);

  if (rounds > 0)
    dw_selftest::timing_rounds("[QMG-MOBIUS-EO-BENCH]", rounds, n, xe, xf, [&](complex<double>* sol) { minv_mobius_eo_cg(sol, b, max_iter, eps, mob); },
                               [&](complex<double>* sol) { full_solve(sol, eps_full); });

  delete mob;
  vec.release();
  qmg::VecPool::release_all();
  return qmg_driver::leave(line.all_pass ? 0 : 1);
}
