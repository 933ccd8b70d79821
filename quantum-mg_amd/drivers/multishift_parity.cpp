// multishift_parity -- runs the multi-shift CG of include/qmg/krylov.hpp (bcg_m_core / minv_vector_cg_m) through the mass-scan helpers of
// include/qmg/operators.hpp on ONE fixed gauge field and dumps right-hand sides and per-shift solutions, so that
// tests/test_gpu_multishift.py can hold them to numpy (tests/coordspace.py) and to the single-shift CG that is already pinned
// (minv_vector_cg, tests/test_gpu_krylov.py).
//   ./multishift_parity L gauge_file dump_dir staggered m1,m2,...      Staggered2D::solve_masses: x_i = D(m_i)^-1 b
//   ./multishift_parity L gauge_file dump_dir laplace   msq1,msq2,...  GaugedLaplace2D::solve_masses: x_i = (Laplace + msq_i)^-1 b
// b is gaussian on both parities (dumped as b.bin), eps = 1e-10.  Per shift i:
//   [KRYLOV] cgm_<i>   the multi-shift solve's inversion_info for that shift       x_<i>.bin
//   [KRYLOV] solo_<i>  minv_vector_cg alone on A + sigma_i to the same eps         xsolo_<i>.bin (staggered: m_i y - H y of its solution y)
// [TIMING]: both repeated once more with warm scratch pools: operator applies and wall seconds of the one multi-shift solve and of the S solo solves.
// [STATE]: the operator's shift and its apply_M output before and after solve_masses (bitwise).
// `laplace` adds the lock-step batch: three right-hand sides x every shift through bcg_m_core against three batches of one
// ([BATCH] rows), the same batch with the middle right-hand side zero ([BATCH0] rows), and a non-zero initial guess ([GUESS]).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <iomanip>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../include/qmg/qmg.hpp"
#include "driver_common.hpp"

using namespace std;

static void dump(const string& dir, const string& name, complex<double>* dev, size_t n) {
  vector<complex<double>> h = qmg::to_host(dev, n);
  FILE* f = fopen((dir + "/" + name + ".bin").c_str(), "wb");
  fwrite(h.data(), sizeof(complex<double>), n, f);
  fclose(f);
}
static void report(const string& name, const inversion_info& i, double bnorm) {
  cout << "[KRYLOV] " << name << " success " << (i.success ? 1 : 0) << " iter " << i.iter << " ops " << i.ops_count << " rel_res " << sqrt(i.resSq) / bnorm << "\n";
}

// A + sigma for the solo runs
struct Shifted { matrix_op_cplx f; void* data; double sigma; int n; };
static void apply_shifted(complex<double>* lhs, complex<double>* rhs, void* extra) {
  Shifted* s = (Shifted*)extra;
  s->f(lhs, rhs, s->data);
  caxpy(s->sigma, rhs, lhs, s->n);
}

int main(int argc, char** argv) {
  qmg_driver::Guard guard;
  if (argc < 6) { cout << "usage: ./multishift_parity L gauge_file dump_dir staggered|laplace v1,v2,...\n"; return -1; }
  cout << setprecision(17);
  if (!qmg::ok(qmg_init(0), "qmg_init")) return 2;
  const int L = stoi(argv[1]);
  const string gauge_file = argv[2], dir = argv[3], kind = argv[4];
  vector<double> vals;
  { stringstream list(argv[5]); string item; while (getline(list, item, ',')) vals.push_back(stod(item)); }
  const int S = (int)vals.size();
  const bool stag = kind == "staggered";
  if (!stag && kind != "laplace") return -1;
  const double eps = 1e-10;
  const int max_iter = 5000;

  Lattice2D lat(L, L, 1);
  complex<double>* gauge = allocate_vector<complex<double>>(lat.get_size_gauge());
  if (!read_gauge_u1(gauge, &lat, gauge_file)) return 3;
  const int n = (int)lat.get_size_cv_l();
  Staggered2D staggered(&lat, 0.0625, gauge), hop(&lat, 0.0, gauge);   // `hop`: D(0) = H, for the solo runs' reconstruction
  GaugedLaplace2D laplace(&lat, 0.0625, gauge), laplace0(&lat, 0.0, gauge);
  Stencil2D* op = stag ? (Stencil2D*)&staggered : (Stencil2D*)&laplace;

  complex<double>* b = allocate_vector<complex<double>>(n);
  complex<double>* before = allocate_vector<complex<double>>(n);
  complex<double>* after = allocate_vector<complex<double>>(n);
  complex<double>* y = allocate_vector<complex<double>>(n);
  complex<double>* t = allocate_vector<complex<double>>(n);
  vector<complex<double>*> xs(S);
  for (int s = 0; s < S; s++) xs[s] = allocate_vector<complex<double>>(n);
  gaussian(b, n, 5151ull);
  dump(dir, "b", b, n);
  const double bn = sqrt(norm2sq(b, n));

  // ---- every shift at once
  const complex<double> shift_before = op->get_shift();
  zero_vector(before, n); op->apply_M(before, b);
  const vector<inversion_info> inv = stag ? staggered.solve_masses(xs.data(), b, vals.data(), S, max_iter, eps) : laplace.solve_masses(xs.data(), b, vals.data(), S, max_iter, eps);
  zero_vector(after, n); op->apply_M(after, b);
  const vector<complex<double>> hb = qmg::to_host(before, n), ha = qmg::to_host(after, n);
  cout << "[STATE] shift_unchanged " << (op->get_shift() == shift_before ? 1 : 0) << " apply_unchanged " << (memcmp(hb.data(), ha.data(), sizeof(complex<double>) * n) == 0 ? 1 : 0) << "\n";
  for (int s = 0; s < S && s < (int)inv.size(); s++) { report("cgm_" + to_string(s), inv[s], bn); dump(dir, "x_" + to_string(s), xs[s], n); }

  // ---- each shift alone: the single-shift CG on A + sigma_s
  for (int s = 0; s < S; s++) {
    Shifted sh = {stag ? Staggered2D::apply_minus_hop_sq : GaugedLaplace2D::apply_massless, stag ? (void*)&staggered : (void*)&laplace, stag ? vals[s] * vals[s] : vals[s], n};
    zero_vector(y, n);
    const inversion_info si = minv_vector_cg(y, b, n, max_iter, eps, apply_shifted, (void*)&sh);
    report("solo_" + to_string(s), si, bn);
    if (stag) { zero_vector(t, n); hop.apply_M(t, y); caxpby(-1.0, t, vals[s], y, n); }   // x = m y - H y
    dump(dir, "xsolo_" + to_string(s), y, n);
  }

  // ---- the same work again, timed (the pools are warm now): one multi-shift solve against the S single-shift solves
  {
    qmg::ok(qmg_stream_sync(qmg::current_stream()), "sync");
    double t0 = qmg::wall_now();
    const vector<inversion_info> again = stag ? staggered.solve_masses(xs.data(), b, vals.data(), S, max_iter, eps) : laplace.solve_masses(xs.data(), b, vals.data(), S, max_iter, eps);
    qmg::ok(qmg_stream_sync(qmg::current_stream()), "sync");
    const double t_multi = qmg::wall_now() - t0;
    int solo_ops = 0;
    t0 = qmg::wall_now();
    for (int s = 0; s < S; s++) {
      Shifted sh = {stag ? Staggered2D::apply_minus_hop_sq : GaugedLaplace2D::apply_massless, stag ? (void*)&staggered : (void*)&laplace, stag ? vals[s] * vals[s] : vals[s], n};
      zero_vector(y, n);
      solo_ops += minv_vector_cg(y, b, n, max_iter, eps, apply_shifted, (void*)&sh).ops_count;
      if (stag) { zero_vector(t, n); hop.apply_M(t, y); caxpby(-1.0, t, vals[s], y, n); }
    }
    qmg::ok(qmg_stream_sync(qmg::current_stream()), "sync");
    cout << "[TIMING] multishift_ops " << (again.empty() ? 0 : again[0].ops_count) << " multishift_seconds " << t_multi << " solo_ops " << solo_ops << " solo_seconds " << qmg::wall_now() - t0 << "\n";
  }

  // ---- lock-step batch: three right-hand sides x S shifts (gauged Laplace at m^2 = 0 through the batch apply)
  if (!stag) {
    const int K = 3;
    const unsigned all = qmg::full_mask(K);
    qmg::BatchPool pool((size_t)n, K);
    qmg::Batch bb = pool.get();
    vector<qmg::Batch> xb(S), xr(S);
    for (int s = 0; s < S; s++) { xb[s] = pool.get(); xr[s] = pool.get(); }
    for (int pass = 0; pass < 2; pass++) {   // pass 1: the middle right-hand side is zero
      for (int k = 0; k < K; k++) gaussian(bb.vec(k), n, 6000ull + k);
      if (pass == 1) zero_vector(bb.vec(1), n);
      for (int s = 0; s < S; s++) { qmg::bzero(xb[s], n, all); qmg::bzero(xr[s], n, all); }
      const vector<inversion_info> bi = bcg_m_core<double>(xb, bb, n, max_iter, eps, vals, apply_stencil_2D_M_batch, (void*)&laplace0, all, 0);
      for (int k = 0; k < K; k++) {
        vector<qmg::Batch> x1(S);
        for (int s = 0; s < S; s++) x1[s] = qmg::Batch(xr[s].vec(k), n, 1);
        const vector<inversion_info> si = bcg_m_core<double>(x1, qmg::Batch(bb.vec(k), n, 1), n, max_iter, eps, vals, apply_stencil_2D_M_batch, (void*)&laplace0, 1u, 0);
        for (int s = 0; s < S; s++) {
          const double ref = norm2sq(xr[s].vec(k), n);
          cout << (pass == 0 ? "[BATCH]" : "[BATCH0]") << " rhs " << k << " shift " << s << " success " << (bi[(size_t)k * S + s].success ? 1 : 0) << " iter " << bi[(size_t)k * S + s].iter
               << " alone_success " << (si[s].success ? 1 : 0) << " alone_iter " << si[s].iter << " x_norm " << sqrt(norm2sq(xb[s].vec(k), n)) << " rel_diff "
               << (ref > 0 ? sqrt(diffnorm2sq(xb[s].vec(k), xr[s].vec(k), n) / ref) : sqrt(diffnorm2sq(xb[s].vec(k), xr[s].vec(k), n))) << "\n";
        }
      }
    }
    // a non-zero initial guess is refused: nothing is iterated, nothing converges
    for (int k = 0; k < K; k++) gaussian(bb.vec(k), n, 6000ull + k);
    for (int s = 0; s < S; s++) qmg::bzero(xb[s], n, all);
    gaussian(xb[S - 1].vec(2), n, 7000ull);
    const double g0 = norm2sq(xb[S - 1].vec(2), n);
    const vector<inversion_info> gi = bcg_m_core<double>(xb, bb, n, max_iter, eps, vals, apply_stencil_2D_M_batch, (void*)&laplace0, all, 0);
    bool any = false;
    for (size_t i = 0; i < gi.size(); i++) any = any || gi[i].success || gi[i].iter != 0 || gi[i].ops_count != 0;
    cout << "[GUESS] refused " << (!any && norm2sq(xb[S - 1].vec(2), n) == g0 && norm2sq(xb[0].vec(0), n) == 0.0 ? 1 : 0) << "\n";
  }

  for (int s = 0; s < S; s++) deallocate_vector(&xs[s]);
  deallocate_vector(&b); deallocate_vector(&before); deallocate_vector(&after); deallocate_vector(&y); deallocate_vector(&t); deallocate_vector(&gauge);
  qmg::VecPool::release_all();
  return qmg_driver::leave(0);
}
