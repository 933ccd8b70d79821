// krylov_batch_parity -- runs the lock-step batch cores of include/qmg/krylov.hpp (bmr_core, bbicgstab_l_core, bgcr_core, bcg_core) on
// UNEVEN batches: six systems that stop at very different iterations, one of them with a zero right-hand side, one converged at
// iteration 0, one a 2^-40 copy of another, one slow; under the full mask and with a slot masked out and filled with NaN; in
// T = double and T = float (the fp32 shadow of the operators); with the systems n and n + 37 complex numbers apart.
// tests/test_gpu_krylov_batch.py writes the inputs (tests/krylov_batch_numpy.py) and holds the output to dense numpy solves.
//   ./krylov_batch_parity case_dir
// case_dir holds
//   cases.txt          line 1: `masses <wilson16> <wilson16h> <laplace34x10 m^2>`; then one case per line:
//                      name core(mr|bicg|gcr|cg) op(wilson16|wilson16f|wilson16h|normal16|laplace34x10; wilson16f is wilson16 with other guesses) guess max_iter_f64 max_iter_f32 pi pre eps_ps fixed converging
//                      (pi: L of BiCGStab(L), restart of GCR / CG, -1 none; pre: flexible GCR with 4 bmr_core steps as preconditioner;
//                      eps_ps: eps_per_system = eps * {1, 1, 1, 1e2, 1, 1e-2}; fixed: eps = 1e-30; eps = 1e-9 in double, 1e-3 in float)
//   links_16x16.dat, links_34x10.dat      U(1) phases in the format of tests/golden/*.dat (read_gauge_u1)
//   rhs0_<op>.bin, rhsg_<op>.bin, guess_<op>.bin     6 x n complex<double>: right-hand sides of the zero-guess runs, of the guess runs, guesses
// and receives, per run `tag` = <case>_<f64|f32>_s<0|1>_<mask in hex> (a batch) or <case>_<f64|f32>_a<k> (system k alone, a batch of one):
//   x_<tag>.bin        the WHOLE solution allocation in complex<T>, padding and masked-out slots included
//   rhs_<op>_<0|g>_<f64|f32>.bin   the six right-hand sides as the cores saw them (rounded to T)
// and prints
//   [SYS] tag k slot success iter ops resSq       one line per system (slot: which right-hand side system k holds, -1 none)
//   [OPS] tag m m m ...                           the mask of every operator call the core made, in order (hex)
//   [PRE] tag m m m ...                           the same for the applies inside the preconditioner
//   [RHS] tag unchanged 0|1                       the right-hand-side allocation, NaN padding included, byte for byte after the solve
// The operator goes to the cores through a recording wrapper around apply_stencil_typed_batch<T>.  Padding between the systems, and every
// slot outside the mask (rhs, x and guess), is NaN before each solve.  include/qmg_hip.h states no alignment RULE for vec_stride (fp32
// arrays "should" be 16-byte aligned with even strides, else the kernels fall back to 8-byte accesses): n + 37 is odd, so the float systems sit on
// 8-byte boundaries.  One more run puts bgcr_core on 16 systems (BATCH_MAX) under mask 0xA5A5, the six right-hand sides repeating in the
// active slots.  The converging CG cases also carry the check that lived in facade_selftest: a batch equals its systems solved alone.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <limits>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../include/qmg/qmg.hpp"
#include "driver_common.hpp"

using namespace std;

struct Case { string name, core, op; int guess, max_iter[2], pi, pre, eps_ps, fixed, converging; };
struct Op { BatchOp* bop; size_t n; vector<complex<double> > rhs0, rhsg, guess; };
struct Rec { BatchOp* op; vector<unsigned>* log; };
static const double EPS_FACTOR[6] = {1.0, 1.0, 1.0, 1e2, 1.0, 1e-2};
static int failures = 0;

template <typename T>
static void rec_apply(qmg::BatchT<T> lhs, qmg::BatchT<T> rhs, unsigned mask, void* extra) {
  Rec* r = (Rec*)extra;
  r->log->push_back(mask);
  apply_stencil_typed_batch<T>(lhs, rhs, mask, (void*)r->op);
}
// 4 MR steps from zero on the mask the solver hands over (the smoother form of batch.hpp), recorded in the preconditioner's own list
template <typename T>
static void rec_precond(qmg::BatchT<T> lhs, qmg::BatchT<T> rhs, int size, unsigned mask, void* extra, inversion_verbose_struct*) {
  bmr_core<T>(lhs, rhs, size, 4, 1e-15, 0.85, rec_apply<T>, extra, mask, true);
}

static bool read_bin(const string& path, vector<complex<double> >& v, size_t count) {
  v.resize(count);
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) { cout << "[QMG-ERROR]: cannot open " << path << "\n"; return false; }
  const size_t got = fread(v.data(), sizeof(complex<double>), count, f);
  fclose(f);
  if (got != count) { cout << "[QMG-ERROR]: " << path << " is too short\n"; return false; }
  return true;
}
template <typename T>
static void write_bin(const string& path, const vector<complex<T> >& v) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) { cout << "[QMG-ERROR]: cannot write " << path << "\n"; return; }
  fwrite(v.data(), sizeof(complex<T>), v.size(), f);
  fclose(f);
}
template <typename T> static const char* prec_name() { return sizeof(T) == sizeof(double) ? "f64" : "f32"; }

// a batch allocation on the host: NaN everywhere, then system k = rows[slot_of[k]] rounded to T (slot_of[k] < 0: left NaN)
template <typename T>
static vector<complex<T> > layout(const vector<complex<double> >* rows, size_t n, size_t stride, const vector<int>& slot_of, bool zero) {
  const T nan = numeric_limits<T>::quiet_NaN();
  vector<complex<T> > h(stride * slot_of.size(), complex<T>(nan, nan));
  for (size_t k = 0; k < slot_of.size(); k++) {
    if (slot_of[k] < 0) continue;
    for (size_t i = 0; i < n; i++) h[k * stride + i] = zero ? complex<T>(0, 0) : complex<T>((T)(*rows)[slot_of[k] * n + i].real(), (T)(*rows)[slot_of[k] * n + i].imag());
  }
  return h;
}

// one solve: system k of `nrhs` holds right-hand side slot_of[k]; returns the per-system results and leaves the solution on the host in *x_out
template <typename T>
static vector<inversion_info> solve(const Case& c, Op& op, size_t stride, const vector<int>& slot_of, unsigned mask, const string& dir, const string& tag,
                                    vector<complex<T> >* x_out) {
  const int nrhs = (int)slot_of.size(), pi = sizeof(T) == sizeof(double) ? 0 : 1;
  const size_t n = op.n, total = stride * nrhs;
  const vector<complex<T> > hb = layout<T>(c.guess ? &op.rhsg : &op.rhs0, n, stride, slot_of, false);
  const vector<complex<T> > hx = layout<T>(&op.guess, n, stride, slot_of, !c.guess);
  complex<T>* db = allocate_vector<complex<T> >(total);
  complex<T>* dx = allocate_vector<complex<T> >(total);
  qmg::upload(db, hb.data(), total);
  qmg::upload(dx, hx.data(), total);
  qmg::BatchT<T> b(db, stride, nrhs), x(dx, stride, nrhs);
  const double eps = c.fixed ? 1e-30 : (pi == 0 ? 1e-9 : 1e-3);
  vector<double> epsv(nrhs, eps);
  for (int k = 0; k < nrhs; k++) if (slot_of[k] >= 0) epsv[k] = eps * EPS_FACTOR[slot_of[k]];
  const vector<double>* eps_ps = c.eps_ps ? &epsv : 0;
  vector<unsigned> ops_log, pre_log;
  Rec rec = {op.bop, &ops_log}, prec = {op.bop, &pre_log};
  const int max_iter = c.max_iter[pi], size = (int)n;
  const bool zero_guess = !c.guess;
  vector<inversion_info> inv;
  if (c.core == "mr") inv = bmr_core<T>(x, b, size, max_iter, eps, 0.85, rec_apply<T>, (void*)&rec, mask, zero_guess);
  else if (c.core == "bicg") inv = bbicgstab_l_core<T>(x, b, size, max_iter, eps, c.pi, rec_apply<T>, (void*)&rec, mask, zero_guess);
  else if (c.core == "gcr") inv = bgcr_core<T>(x, b, size, max_iter, eps, c.pi, rec_apply<T>, (void*)&rec, c.pre ? rec_precond<T> : (batch_precond_op_t<T>)0, (void*)&prec, mask, zero_guess, 0, "GCR", eps_ps);
  else inv = bcg_core<T>(x, b, size, max_iter, eps, c.pi, rec_apply<T>, (void*)&rec, mask, zero_guess, 0, "CG", eps_ps);
  *x_out = qmg::to_host(dx, total);
  const vector<complex<T> > b_after = qmg::to_host(db, total);
  write_bin<T>(dir + "/x_" + tag + ".bin", *x_out);
  for (int k = 0; k < nrhs; k++)
    cout << "[SYS] " << tag << " " << k << " " << slot_of[k] << " " << (inv[k].success ? 1 : 0) << " " << inv[k].iter << " " << inv[k].ops_count << " " << inv[k].resSq << "\n";
  cout << "[OPS] " << tag << hex;
  for (size_t i = 0; i < ops_log.size(); i++) cout << " " << ops_log[i];
  cout << "\n[PRE] " << tag;
  for (size_t i = 0; i < pre_log.size(); i++) cout << " " << pre_log[i];
  cout << dec << "\n[RHS] " << tag << " unchanged " << (memcmp(hb.data(), b_after.data(), total * sizeof(complex<T>)) == 0 ? 1 : 0) << "\n";
  deallocate_vector(&db); deallocate_vector(&dx);
  return inv;
}

template <typename T>
static void run_case(const Case& c, Op& op, const string& dir) {
  const string pn = prec_name<T>();
  const size_t n = op.n;
  vector<vector<complex<T> > > alone(6);
  vector<inversion_info> alone_inv(6);
  for (int pass = 0; pass < 2; pass++) {
    const size_t stride = pass == 0 ? n : n + 37;
    for (int m = 0; m < 2; m++) {
      const unsigned mask = m == 0 ? 0x3Fu : 0x3Bu;
      vector<int> slot_of(6);
      for (int k = 0; k < 6; k++) slot_of[k] = ((mask >> k) & 1u) ? k : -1;
      ostringstream tag;
      tag << c.name << "_" << pn << "_s" << pass << "_" << hex << mask;
      vector<complex<T> > xb;
      const vector<inversion_info> bi = solve<T>(c, op, stride, slot_of, mask, dir, tag.str(), &xb);
      if (!c.converging || pass != 0 || m != 0) continue;
      // every system alone, as a batch of one
      for (int k = 0; k < 6; k++) {
        ostringstream at;
        at << c.name << "_" << pn << "_a" << k;
        alone_inv[k] = solve<T>(c, op, n, vector<int>(1, k), 1u, dir, at.str(), &alone[k])[0];
      }
      if (c.core != "cg" || sizeof(T) != sizeof(double)) continue;
      // masking and freezing reproduce a system solved alone: same iteration counts (+-1), the same solutions (an apply of several systems
      // may sum in another order)
      bool all_ok = true;
      int worst_it = 0;
      double worst_x = 0.0;
      for (int k = 0; k < 6; k++) {
        all_ok = all_ok && alone_inv[k].success && bi[k].success;
        worst_it = max(worst_it, abs(alone_inv[k].iter - bi[k].iter));
        double d2 = 0.0, r2 = 0.0;
        for (size_t i = 0; i < n; i++) { d2 += norm(complex<double>(xb[k * stride + i]) - complex<double>(alone[k][i])); r2 += norm(complex<double>(alone[k][i])); }
        if (r2 > 0.0) worst_x = max(worst_x, sqrt(d2 / r2));
        else all_ok = all_ok && d2 == 0.0;
      }
      const bool good = all_ok && worst_it <= 1 && worst_x < 1e-7;
      if (!good) failures++;
      cout << (good ? "[ OK ] " : "[FAIL] ") << "bcg_core " << c.name << ", 6 uneven systems == each system alone : " << worst_x << "\n";
    }
  }
}

// bgcr_core on BATCH_MAX systems under 0xA5A5: the six right-hand sides repeat in the active slots, NaN in the others
template <typename T>
static void run_sixteen(const Case& c, Op& op, const string& dir) {
  const unsigned mask = 0xA5A5u;
  vector<int> slot_of(qmg::BATCH_MAX, -1);
  int j = 0;
  for (int k = 0; k < qmg::BATCH_MAX; k++) if ((mask >> k) & 1u) slot_of[k] = (j++) % 6;
  vector<complex<T> > xb;
  solve<T>(c, op, op.n + 37, slot_of, mask, dir, c.name + "_" + prec_name<T>() + "_s1_a5a5", &xb);
}

template <typename T>
static void dump_rhs(Op& op, const string& name, const string& dir) {
  vector<int> ident(6);
  for (int k = 0; k < 6; k++) ident[k] = k;
  write_bin<T>(dir + "/rhs_" + name + "_0_" + prec_name<T>() + ".bin", layout<T>(&op.rhs0, op.n, op.n, ident, false));
  write_bin<T>(dir + "/rhs_" + name + "_g_" + prec_name<T>() + ".bin", layout<T>(&op.rhsg, op.n, op.n, ident, false));
}

int main(int argc, char** argv) {
  qmg_driver::Guard guard;
  if (argc < 2) { cout << "usage: ./krylov_batch_parity case_dir\n"; return -1; }
  cout << setprecision(17);
  if (!qmg::ok(qmg_init(0), "qmg_init")) return 2;
  const string dir = argv[1];
  ifstream in((dir + "/cases.txt").c_str());
  string word;
  double mass = 0.0, heavy = 0.0, msq = 0.0;
  if (!(in >> word >> mass >> heavy >> msq) || word != "masses") { cout << "[QMG-ERROR]: cases.txt does not start with the masses\n"; return 3; }
  vector<Case> cases;
  Case c;
  while (in >> c.name >> c.core >> c.op >> c.guess >> c.max_iter[0] >> c.max_iter[1] >> c.pi >> c.pre >> c.eps_ps >> c.fixed >> c.converging) cases.push_back(c);

  Lattice2D lat_g(16, 16, 1), lat_w(16, 16, 2), lat_l(34, 10, 1);
  complex<double>* gauge_w = allocate_vector<complex<double> >(lat_g.get_size_gauge());
  complex<double>* gauge_l = allocate_vector<complex<double> >(lat_l.get_size_gauge());
  if (!read_gauge_u1(gauge_w, &lat_g, dir + "/links_16x16.dat") || !read_gauge_u1(gauge_l, &lat_l, dir + "/links_34x10.dat")) return 3;
  Wilson2D wilson(&lat_w, mass, gauge_w), wilson_heavy(&lat_w, heavy, gauge_w);
  wilson.build_dagger_stencil();
  GaugedLaplace2D laplace(&lat_l, msq, gauge_l);
  if (!wilson.enable_f32_shadow() || !wilson_heavy.enable_f32_shadow() || !laplace.enable_f32_shadow()) { cout << "[QMG-ERROR]: no fp32 shadow\n"; return 4; }
  BatchOp bw(&wilson, QMG_MATVEC_ORIGINAL), bh(&wilson_heavy, QMG_MATVEC_ORIGINAL), bn(&wilson, QMG_MATVEC_MDAGGER_M), bl(&laplace, QMG_MATVEC_ORIGINAL);
  map<string, Op> ops;
  ops["wilson16"].bop = &bw; ops["wilson16f"].bop = &bw; ops["wilson16h"].bop = &bh; ops["normal16"].bop = &bn; ops["laplace34x10"].bop = &bl;
  for (map<string, Op>::iterator it = ops.begin(); it != ops.end(); ++it) {
    Op& o = it->second;
    o.n = (size_t)o.bop->st->get_lattice()->get_size_cv_l();
    if (!read_bin(dir + "/rhs0_" + it->first + ".bin", o.rhs0, 6 * o.n) || !read_bin(dir + "/rhsg_" + it->first + ".bin", o.rhsg, 6 * o.n) ||
        !read_bin(dir + "/guess_" + it->first + ".bin", o.guess, 6 * o.n)) return 3;
    dump_rhs<double>(o, it->first, dir);
    dump_rhs<float>(o, it->first, dir);
  }
  const double t0 = qmg::wall_now();
  bool sixteen_done = false;
  for (size_t i = 0; i < cases.size(); i++) {
    if (!ops.count(cases[i].op)) { cout << "[QMG-ERROR]: unknown operator " << cases[i].op << "\n"; return 3; }
    Op& o = ops[cases[i].op];
    qmg_driver::phase(cases[i].name.c_str(), false);
    run_case<double>(cases[i], o, dir);
    run_case<float>(cases[i], o, dir);
    if (!sixteen_done && cases[i].core == "gcr" && cases[i].pi > 0 && cases[i].converging && !cases[i].pre) {
      run_sixteen<double>(cases[i], o, dir);
      run_sixteen<float>(cases[i], o, dir);
      sixteen_done = true;
    }
  }
  qmg::ok(qmg_stream_sync(qmg::current_stream()), "sync");
  cout << "[TIMING] cases " << cases.size() << " seconds " << qmg::wall_now() - t0 << "\n";
  deallocate_vector(&gauge_w); deallocate_vector(&gauge_l);
  qmg::VecPool::release_all();
  return qmg_driver::leave(failures ? 1 : 0);
}
