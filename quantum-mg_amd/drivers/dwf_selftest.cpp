// dwf_selftest -- the Shamir domain-wall operator of the facade (Dwf2D / createDwfLs, include/qmg/operators.hpp) held to itself on one
// Gaussian U(1) configuration: the apply from the links against the stored stencil, Gamma5-hermiticity, the dagger stencil, and a CG solve
// of the normal equations alone and as a lock-step batch.
//   ./dwf_selftest L Ls mass seed
// One line per check, `[QMG-DWF] name value PASS|FAIL`; the exit status is nonzero on any FAIL.
//   (a) direct_vs_stored   apply_M with the links route on against the same call after drop_direct_links(): relative l2 difference.
//                          Both routes sum the same <= 14 terms per element in fp64, so the difference is rounding alone: < 1e-13.
//   (b) gamma5_hermiticity |<y, G5 D G5 x> - <D y, x>| / (|y| |G5 D G5 x|) with the facade's gamma5 and dot (real mass): < 1e-12.
//   (c) dagger_vs_gamma5   build_dagger_stencil + apply_M_dagger against G5 D G5: relative l2 difference < 1e-13.
//   (d) cg_iterations, cg_true_residual   CG on M^dagger M (apply_stencil_2D_M_dagger_M) to 1e-10; the recomputed |b - D^dag D x| / |b| <= 1e-9.
//   (e) batch_iterations, batch_residual  the same solve as a batch of 3 through the batch engine: every system takes the iterations and
//                          reaches the residual of its single solve (the batch kernels' per-system arithmetic is the single-vector one).
#include <iomanip>
#include <string>

#include "dw_selftest_common.hpp"

using namespace std;

static dw_selftest::Lines line("[QMG-DWF]");

int main(int argc, char** argv) {
  qmg_driver::Guard guard;
  if (argc < 5) { cout << "usage: ./dwf_selftest L Ls mass seed\n"; return -1; }
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
  Stencil2D* dwf = createDwfLs(&lat, mass, gauge, Ls);
  if (!dwf || !dwf->generated) { cout << "[QMG-DWF] create 0 FAIL\n"; return 4; }
  const int n = (int)lat.get_size_cv_l();
  const int nsys = 3;
  complex<double>*x = vec.make(n), *y = vec.make(n), *t1 = vec.make(n), *t2 = vec.make(n), *g5dg5x = vec.make(n), *Dx_direct = vec.make(n);
  complex<double>*B = vec.make((size_t)nsys * n), *X = vec.make((size_t)nsys * n), *X1 = vec.make(n);
  gaussian(x, n, seed + 101);
  gaussian(y, n, seed + 102);

  qmg_driver::phase("apply");
  const bool direct_on = dwf->direct.on && dwf->direct.kind == Stencil2D::QMG_DIRECT_DWF;
  zero_vector(Dx_direct, n);
  dwf->apply_M(Dx_direct, x);

  qmg_driver::phase("gamma5");
  dwf->gamma5(t1, x);
  dwf->apply_M_overwrite(t2, t1);
  copy_vector(g5dg5x, t2, n);
  dwf->gamma5(g5dg5x);                 // the in-place form
  dwf->apply_M_overwrite(t2, y);
  const complex<double> lhs = dot(y, g5dg5x, n), rhs = dot(t2, x, n);
  const double herm = abs(lhs - rhs) / sqrt(norm2sq(y, n) * norm2sq(g5dg5x, n));

  qmg_driver::phase("dagger");
  dwf->build_dagger_stencil();
  zero_vector(t1, n);
  dwf->apply_M_dagger(t1, x);
  const double dag = sqrt(diffnorm2sq(t1, g5dg5x, n) / norm2sq(g5dg5x, n));

  qmg_driver::phase("cg");
  const int max_iter = 5000;
  const double eps = 1e-10;
  vector<inversion_info> single(nsys);
  vector<double> true_res(nsys, 0.0);
  for (int k = 0; k < nsys; k++) {
    complex<double>* b = B + (size_t)k * n;
    gaussian(b, n, seed + 200 + k);
    zero_vector(X1, n);
    single[k] = minv_vector_cg(X1, b, n, max_iter, eps, apply_stencil_2D_M_dagger_M, (void*)dwf);
    apply_stencil_2D_M_dagger_M(t1, X1, (void*)dwf);
    true_res[k] = sqrt(diffnorm2sq(t1, b, n) / norm2sq(b, n));
  }

  qmg_driver::phase("batch cg");
  zero_vector(X, (size_t)nsys * n);
  BatchOp op(dwf, QMG_MATVEC_MDAGGER_M);
  const vector<inversion_info> batch = bcg_core<double>(qmg::Batch(X, n, nsys), qmg::Batch(B, n, nsys), n, max_iter, eps, -1, apply_stencil_typed_batch<double>, &op,
                                                        qmg::full_mask(nsys), false, 0, "CG");
  int iter_diff = 0;
  double res_diff = 0.0, batch_true = 0.0;
  bool batch_ok = true;
  for (int k = 0; k < nsys; k++) {
    iter_diff = max(iter_diff, abs(batch[k].iter - single[k].iter));
    res_diff = max(res_diff, abs(batch[k].resSq - single[k].resSq) / single[k].resSq);
    apply_stencil_2D_M_dagger_M(t1, X + (size_t)k * n, (void*)dwf);
    batch_true = max(batch_true, sqrt(diffnorm2sq(t1, B + (size_t)k * n, n) / norm2sq(B + (size_t)k * n, n)));
    batch_ok = batch_ok && batch[k].success && single[k].success;
  }

  qmg_driver::phase("stored");
  dwf->drop_direct_links();
  zero_vector(t1, n);
  dwf->apply_M(t1, x);
  const double dvs = sqrt(diffnorm2sq(Dx_direct, t1, n) / norm2sq(t1, n));

  line("direct_route_on", direct_on ? 1.0 : 0.0, direct_on);
  line("direct_vs_stored", dvs, dvs < 1e-13);
  line("gamma5_hermiticity", herm, herm < 1e-12);
  line("dagger_vs_gamma5", dag, dag < 1e-13);
  line("cg_iterations", (double)single[0].iter, single[0].success && single[0].iter < max_iter);
  line("cg_true_residual", true_res[0], true_res[0] <= 1e-9);
  line("batch_iterations", (double)iter_diff, batch_ok && iter_diff == 0);
  line("batch_residual", res_diff, res_diff == 0.0 && batch_true <= 1e-9);

  delete dwf;
  vec.release();
  qmg::VecPool::release_all();
  return qmg_driver::leave(line.all_pass ? 0 : 1);
}
