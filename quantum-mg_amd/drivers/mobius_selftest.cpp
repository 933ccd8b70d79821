// mobius_selftest -- the Moebius domain-wall operator of the facade (Mobius2D / createMobiusLs, include/qmg/operators.hpp) held to itself on
// one Gaussian U(1) configuration, after dwf_selftest.
//   ./mobius_selftest L Ls m b5 c5 [seed [solution_file]]
// One line per check, `[QMG-MOBIUS] name value PASS|FAIL`, then `[MOBIUS-SELFTEST] PASS` or `FAIL`; the exit status is nonzero on any FAIL.
//   (a) links_route_on; links_vs_stored, dagger_links_vs_stored   apply_M / apply_M_dagger with the links route on against the same calls after
//       drop_direct_links() (the stored fields, and the dagger stencil built from them): relative l2 difference < 1e-13.  Only where the
//       stored-stencil apply serves nc = 2 Ls (qmg_stencil_plan is asked); at Ls = 32 the two lines are absent.
//   (b) adjointness          |<y, D x> - <D^dagger y, x>| / (|x| |y|), both applies from the links: < 1e-12.
//   (c) gamma5_violation     |Gamma5 D Gamma5 x - D^dagger x| / |x|: reported, not gated (it is not zero for c5 != 0: B and H do not commute).
//   (d) shamir_limit         a second operator with b5 = 1, c5 = 0 against Dwf2D<Ls> with shift = M5: relative l2 difference < 1e-13.
//   (e) cg_iterations, cg_true_residual   minv_mobius_cg to 1e-10; the recomputed |b - D x| / |b| <= 1e-8.  With a solution_file the links, b and
//       x of this solve are written there as raw complex<double> (2 L^2, then twice 2 Ls L^2 numbers in the device layout), for a dense solve elsewhere.
#include <iomanip>
#include <string>

#include "dw_selftest_common.hpp"

using namespace std;

static dw_selftest::Lines line("[QMG-MOBIUS]");

// Dwf2D of run-time Ls for the Shamir limit: createDwfLs, and at Ls = 32 (which it declines: no stored apply at nc = 64) the class itself
static Stencil2D* shamir(Lattice2D* lat, double mass, complex<double>* gauge, int Ls, bool stored) {
  if (stored) return createDwfLs(lat, mass, gauge, Ls);
  return Ls == 32 ? new Dwf2D<32>(lat, mass, gauge) : nullptr;
}

int main(int argc, char** argv) {
  qmg_driver::Guard guard;
  if (argc < 6) { cout << "usage: ./mobius_selftest L Ls m b5 c5 [seed [solution_file]]\n"; return -1; }
  cout << setprecision(17);
  if (!qmg::ok(qmg_init(0), "qmg_init")) return 2;
  const int L = stoi(argv[1]), Ls = stoi(argv[2]);
  const double mass = stod(argv[3]), b5 = stod(argv[4]), c5 = stod(argv[5]);
  const unsigned long long seed = argc > 6 ? stoull(argv[6]) : 7ull;
  Lattice2D lat_g(L, L, 1), lat(L, L, 2 * Ls);
  dw_selftest::Vectors vec;
  complex<double>* gauge = vec.make(lat_g.get_size_gauge());
  // link phases N(0, 0.4^2)
  if (!qmg::ok(qmg_u1_gauss_gauge(gauge, L, L, 1.0 / (0.4 * 0.4), seed, qmg::current_stream()), "qmg_u1_gauss_gauge")) return 3;
  int plan[12];
  const bool stored = qmg_stencil_plan(QMG_SE_APPLY, 0, 0, L, L, 2 * Ls, QMG_P_ALL | QMG_P_ZERO, 1, 0, 0, 1, 1, 0, 0, plan, 12) == QMG_SUCCESS && plan[0] != 0 && plan[0] != 9;
  MobiusBase* mob = createMobiusLs(&lat, mass, gauge, Ls, b5, c5);
  if (!mob || !mob->generated) { cout << "[QMG-MOBIUS] create 0 FAIL\n[MOBIUS-SELFTEST] FAIL\n"; return 4; }
  const int n = (int)lat.get_size_cv_l();
  complex<double>*x = vec.make(n), *y = vec.make(n), *Dx = vec.make(n), *Ddy = vec.make(n), *Ddx = vec.make(n), *t1 = vec.make(n), *t2 = vec.make(n), *b = vec.make(n);
  gaussian(x, n, seed + 101);
  gaussian(y, n, seed + 102);
  gaussian(b, n, seed + 200);

  qmg_driver::phase("apply");
  const bool links_on = mob->links_ready();
  zero_vector(Dx, n);  mob->apply_M(Dx, x);
  zero_vector(Ddy, n); mob->apply_M_dagger(Ddy, y);        // no dagger stencil has been built: this is the links route or nothing
  zero_vector(Ddx, n); mob->apply_M_dagger(Ddx, x);
  const double adj = abs(dot(y, Dx, n) - dot(Ddy, x, n)) / sqrt(norm2sq(x, n) * norm2sq(y, n));

  qmg_driver::phase("gamma5");
  mob->gamma5(t1, x);
  mob->apply_M_overwrite(t2, t1);
  mob->gamma5(t2);
  const double g5v = sqrt(diffnorm2sq(t2, Ddx, n) / norm2sq(x, n));

  qmg_driver::phase("shamir");
  double sham = -1.0;
  {
    MobiusBase* lim = createMobiusLs(&lat, mass, gauge, Ls, 1.0, 0.0);
    Stencil2D* dwf = shamir(&lat, mass, gauge, Ls, stored);
    if (lim && dwf && lim->generated && dwf->generated) {
      lim->apply_M_overwrite(t1, x);
      dwf->apply_M_overwrite(t2, x);
      sham = sqrt(diffnorm2sq(t1, t2, n) / norm2sq(t2, n));
    }
    delete lim;
    delete dwf;
  }

  qmg_driver::phase("cg");
  const int max_iter = 5000;
  const double eps = 1e-10;
  zero_vector(t1, n);
  const inversion_info info = minv_mobius_cg(t1, b, max_iter, eps, mob);
  const double true_res = dw_selftest::true_residual(mob, t2, t1, b, n, norm2sq(b, n));
  if (argc > 7) {
    const complex<double>* parts[3] = {gauge, b, t1};
    const size_t lens[3] = {(size_t)lat_g.get_size_gauge(), (size_t)n, (size_t)n};
    if (!dw_selftest::write_raw(argv[7], parts, lens, 3)) line("solution_file", 0.0, false);
  }

  double dvs = -1.0, ddvs = -1.0;
  if (stored) {
    qmg_driver::phase("stored");
    mob->drop_direct_links();
    mob->build_dagger_stencil();
    zero_vector(t1, n); mob->apply_M(t1, x);
    dvs = sqrt(diffnorm2sq(Dx, t1, n) / norm2sq(t1, n));
    zero_vector(t2, n); mob->apply_M_dagger(t2, x);
    ddvs = sqrt(diffnorm2sq(Ddx, t2, n) / norm2sq(t2, n));
  }

  line("links_route_on", links_on ? 1.0 : 0.0, links_on);
  if (stored) {
    line("links_vs_stored", dvs, dvs >= 0.0 && dvs < 1e-13);
    line("dagger_links_vs_stored", ddvs, ddvs >= 0.0 && ddvs < 1e-13);
  }
  line("adjointness", adj, adj < 1e-12);
  line("gamma5_violation", g5v, true);
  line("shamir_limit", sham, sham >= 0.0 && sham < 1e-13);
  line("cg_iterations", (double)info.iter, info.success && info.iter < max_iter);
  line("cg_true_residual", true_res, true_res <= 1e-8);
  cout << "[MOBIUS-SELFTEST] " << (line.all_pass ? "PASS" : "FAIL") << "\n";

  delete mob;
  vec.release();
  qmg::VecPool::release_all();
  return qmg_driver::leave(line.all_pass ? 0 : 1);
}
