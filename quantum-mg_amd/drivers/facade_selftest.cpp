// facade_selftest -- device-side checks of the C++ facade against the identities the reference's own
// tests print (they store no numbers): every check recomputes a quantity two ways on the GPU
// through the facade's reference-named methods and compares.  Exit code = number of failed checks.
//   n00  cshift round trip                                   (tests/n00_cshift)
//   n04  staggered even-odd preconditioned solve             (tests/n04_staggered_test, staggered.h:190-240)
//   n03  gauged Laplace even-odd preconditioned solve        (tests/n03_gauge_laplace_test, gaugedlaplace.h:154-204)
//   n08  Galerkin: built coarse op == emulated R A P         (tests/n08_distance1_build_test:117-147, multigrid.h:465-512)
//   n17  <y, M x> = <M^dag y, x>, M^dag M / M M^dag          (tests/n17_dagger_stencil_test:85-96)
//   n18  right-block-Jacobi and Schur solves reconstruct the ORIGINAL system   (tests/n18_rbjacobi_stencil_test:153-231)
//   n21  rbj-dagger normal equations (CGNE / CGNR)           (tests/n21_rbj_dagger_stencil_test:138-209)
//   storage / lattice / multigrid bookkeeping
//   the route of an apply: in each live state the facade gives, bit for bit, what the entry point named by the policy table gives
//   the narrow copies of the matrices: which of them exist, and which uses are on, after each enable_* / disable_* / build_* / update_links call
#include <cmath>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <iostream>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include <unistd.h>

#include "../include/qmg/qmg.hpp"
#include "driver_common.hpp"

using namespace std;

static int failures = 0;
static void check(bool okv, const string& what, double val) {
  cout << (okv ? "[ OK ] " : "[FAIL] ") << what << " : " << val << "\n";
  if (!okv) failures++;
}
static double rel_resid(Stencil2D* op, complex<double>* x, complex<double>* b, long n) {   // ||b - A x|| / ||b|| with the ORIGINAL operator
  complex<double>* Ax = allocate_vector<complex<double>>(n);
  zero_vector(Ax, n);
  op->apply_M(Ax, x);
  const double r = sqrt(diffnorm2sq(b, Ax, n) / norm2sq(b, n));
  deallocate_vector(&Ax);
  return r;
}

// The route of an apply (Stencil2D::resolve_route / run_route): the facade's result against the entry point that the policy table of DESIGN 6b names for
// the state, called directly with desc() and the arrays the table names.  Both launch the same kernel with the same arguments, so the bytes must agree:
// `got` and `want` start from the same contents (systems a mask leaves out and a parity no piece writes must stay as they were), three systems of n.
struct RouteCheck {
  size_t n;
  complex<double>*in, *other, *init, *got, *want;
  complex<float>* in32;
  explicit RouteCheck(size_t n_) : n(n_) {
    complex<double>** all[] = {&in, &other, &init, &got, &want};
    for (auto p : all) *p = allocate_vector<complex<double>>(3 * n);
    gaussian(in, 3 * n, 3100); gaussian(other, 3 * n, 3101); gaussian(init, 3 * n, 3102);
    void* f = 0;
    qmg::ok(qmg_malloc(&f, 3 * n * sizeof(complex<float>)), "qmg_malloc");
    in32 = (complex<float>*)f;
    qmg::ok(qmg_convert(in32, QMG_C32, in, QMG_C64, 3 * n, qmg::current_stream()), "qmg_convert");
  }
  ~RouteCheck() {
    complex<double>** all[] = {&in, &other, &init, &got, &want};
    for (auto p : all) deallocate_vector(p);
    qmg_free(in32);
  }
  // state_ok: the operator is in the state the row is about; facade: false where it declined
  void operator()(const string& what, bool state_ok, const std::function<bool(void*)>& facade, const std::function<int(void*)>& entry) {
    copy_vector(got, init, 3 * n); copy_vector(want, init, 3 * n);
    const bool served = facade(got);
    const int rc = entry(want);
    const std::vector<complex<double>> g = qmg::to_host(got, 3 * n), w = qmg::to_host(want, 3 * n), i0 = qmg::to_host(init, 3 * n);
    const bool same = memcmp(g.data(), w.data(), 3 * n * sizeof(complex<double>)) == 0, wrote = memcmp(g.data(), i0.data(), 3 * n * sizeof(complex<double>)) != 0;
    check(state_ok && served && rc == QMG_SUCCESS && same && wrote, "route: " + what, rc);
  }
};

// Which narrow matrix copies an operator holds, as "S<bits>:<copies> F<on>:<copies> H<on>:<copies> <g>".  S: the storage under fp64 vectors
// (enable_f32_matrices), with its width 32 / 16 or - while off; F: the complex<float> shadow and H: its complex<half> copies (enable_f32_shadow), + on, - off.
// One letter per copy that is there: c clover, h hopping, r right-block-Jacobi hops, i cinv, C / H the dagger stencil's clover / hops, R the rbj-dagger hops.
// g: direct.gauge32 is there, -: it is not.
typedef Stencil2D S;
enum { STORAGE = S::QMG_NARROW_STORAGE, SHADOW = S::QMG_NARROW_SHADOW, HALF = S::QMG_NARROW_SHADOW_HALF };
static void* clover_copy(const Stencil2D& s, int use, S::QMGArraySet set = S::QMG_ARR_ORIGINAL) { return s.narrow[use].copy[set][S::QMG_SLOT_CLOVER]; }
static void* hopping_copy(const Stencil2D& s, int use, S::QMGArraySet set = S::QMG_ARR_ORIGINAL) { return s.narrow[use].copy[set][S::QMG_SLOT_HOPPING]; }
static string narrow_census(const Stencil2D& s) {
  auto there = [](std::initializer_list<std::pair<const void*, char>> copies) { string o; for (const auto& c : copies) if (c.first) o += c.second; return o; };
  const S::NarrowCopies &st = s.narrow[STORAGE], &f = s.narrow[SHADOW], &h = s.narrow[HALF];
  return "S" + (st.on ? to_string(st.bits) : string("-")) + ":" +
         there({{clover_copy(s, STORAGE), 'c'}, {hopping_copy(s, STORAGE), 'h'}, {hopping_copy(s, STORAGE, S::QMG_ARR_RBJ_HOPPING), 'r'}, {clover_copy(s, STORAGE, S::QMG_ARR_RBJ_CINV), 'i'}}) +
         " F" + (f.on ? "+:" : "-:") + there({{clover_copy(s, SHADOW), 'c'}, {hopping_copy(s, SHADOW), 'h'}, {hopping_copy(s, SHADOW, S::QMG_ARR_RBJ_HOPPING), 'r'}, {clover_copy(s, SHADOW, S::QMG_ARR_RBJ_CINV), 'i'},
                                              {clover_copy(s, SHADOW, S::QMG_ARR_DAGGER), 'C'}, {hopping_copy(s, SHADOW, S::QMG_ARR_DAGGER), 'H'}, {hopping_copy(s, SHADOW, S::QMG_ARR_RBJ_DAGGER), 'R'}}) +
         " H" + (h.on ? "+:" : "-:") + there({{clover_copy(s, HALF), 'c'}, {hopping_copy(s, HALF), 'h'}, {hopping_copy(s, HALF, S::QMG_ARR_RBJ_HOPPING), 'r'}}) + (s.direct.gauge32 ? " g" : " -");
}
// what a call prints is kept out of the program's output (the drivers' tests take a [QMG-WARNING] / [QMG-ERROR] line for a failure) and handed to the check
struct Captured {
  std::ostringstream text;
  std::streambuf* old;
  Captured() : old(cout.rdbuf(text.rdbuf())) {}
  ~Captured() { cout.rdbuf(old); }
};
// a fresh Galerkin operator of `fine` on (L / 4)^2 with nc = nvec
struct Galerkin {
  Lattice2D lat;
  std::vector<complex<double>*> nv;
  TransferMG* transfer;
  CoarseOperator2D* op;
  Galerkin(Lattice2D* fine_lat, Stencil2D* fine, int L, int nvec, CoarseOperator2D::QMGCoarseBuildStencil extra) : lat(L / 4, L / 4, nvec), nv(nvec) {
    for (int j = 0; j < nvec; j++) { nv[j] = allocate_vector<complex<double>>(fine_lat->get_size_cv_l()); gaussian(nv[j], fine_lat->get_size_cv_l(), 1300ull + j); }
    transfer = new TransferMG(fine_lat, &lat, nv.data(), true, false, QMG_DOUBLE_NONE);
    op = new CoarseOperator2D(&lat, fine, fine_lat, transfer, false, false, extra);
  }
  ~Galerkin() {
    delete op; delete transfer;
    for (auto& v : nv) deallocate_vector(&v);
  }
};

int main(int argc, char** argv) {
  qmg_driver::Guard guard;
  const string gauge_file = (argc > 1) ? argv[1] : "../../tests/golden/l32t32b60_heatbath.dat";
  if (!qmg::ok(qmg_init(0), "qmg_init")) return 100;
  const int L = 32;
  Lattice2D lat1(L, L, 1), lat2(L, L, 2);
  complex<double>* gauge = allocate_vector<complex<double>>(lat1.get_size_gauge());
  if (!read_gauge_u1(gauge, &lat1, gauge_file)) return 101;
  const long n1 = lat1.get_size_cv_l(), n2 = lat2.get_size_cv_l();
  inversion_verbose_struct quiet(VERB_NONE, "");

  // ---- lattice / storage bookkeeping
  {
    int bad = 0;
    for (int x = 0; x < L; x++) for (int y = 0; y < L; y++) { int xx, yy; lat2.index_to_coord(lat2.coord_to_index(x, y), xx, yy); if (xx != x || yy != y) bad++; }
    check(bad == 0, "Lattice2D coord<->index round trip", bad);
    ArrayStorageMG<complex<double>> pool(n1, 2);
    complex<double>*a = pool.check_out(), *b = pool.check_out(), *c = pool.check_out();
    bool okp = pool.get_number_allocated() == 3 && pool.get_number_checked() == 3 && a != b && b != c;
    pool.check_in(b); pool.check_in(c);
    okp = okp && pool.get_number_checked() == 1 && pool.check_out() == b;
    pool.check_in(b); pool.check_in(a);
    pool.consolidate(1);
    check(okp && pool.get_number_allocated() >= 1 && pool.get_number_checked() == 0, "ArrayStorageMG check_out/check_in/consolidate", pool.get_number_allocated());
  }

  // ---- n00: cshift there and back is the identity
  {
    complex<double>*v = allocate_vector<complex<double>>(n2), *s = allocate_vector<complex<double>>(n2), *t = allocate_vector<complex<double>>(n2);
    gaussian(v, n2, 5);
    cshift(s, v, QMG_CSHIFT_FROM_XP1, QMG_EO_FROM_EVENODD, 2, &lat2);
    cshift(t, s, QMG_CSHIFT_FROM_XM1, QMG_EO_FROM_EVENODD, 2, &lat2);
    double d = diffnorm2sq(t, v, n2);
    cshift(s, v, QMG_CSHIFT_FROM_YM1, QMG_EO_FROM_EVENODD, 2, &lat2);
    cshift(t, s, QMG_CSHIFT_FROM_YP1, QMG_EO_FROM_EVENODD, 2, &lat2);
    d += diffnorm2sq(t, v, n2);
    check(d == 0.0, "n00 cshift round trips", d);
    deallocate_vector(&v); deallocate_vector(&s); deallocate_vector(&t);
  }

  // ---- n04 / n03: even-odd preconditioned CG for staggered and gauged Laplace
  {
    Staggered2D stag(&lat1, 0.1, gauge);
    complex<double>*b = allocate_vector<complex<double>>(n1), *bp = allocate_vector<complex<double>>(n1), *x = allocate_vector<complex<double>>(n1);
    gaussian(b, n1, 11);
    zero_vector(bp, n1); zero_vector(x, n1);
    stag.prepare_b(bp, b);
    inversion_info inv = minv_vector_cg(x, bp, (int)(n1 / 2), 4000, 1e-10, apply_eo_staggered_2D_M, (void*)&stag, &quiet);
    stag.reconstruct_x(x, b);
    check(inv.success && rel_resid(&stag, x, b, n1) < 1e-8, "n04 staggered eo-preconditioned CG solves the full system", rel_resid(&stag, x, b, n1));
    GaugedLaplace2D lap(&lat1, 0.01, gauge);
    zero_vector(bp, n1); zero_vector(x, n1);
    lap.prepare_b(bp, b);
    inv = minv_vector_cg(x, bp, (int)(n1 / 2), 4000, 1e-10, apply_eo_gauge_laplace_2D_M, (void*)&lap, &quiet);
    lap.reconstruct_x(x, b);
    check(inv.success && rel_resid(&lap, x, b, n1) < 1e-8, "n03 gauged-Laplace eo-preconditioned CG solves the full system", rel_resid(&lap, x, b, n1));
    deallocate_vector(&b); deallocate_vector(&bp); deallocate_vector(&x);
  }

  // ---- Wilson: dagger, normal equations, rbjacobi, Schur, rbj-dagger
  Wilson2D wilson(&lat2, complex<double>(0.05, 0.0), gauge);
  {
    complex<double>*x = allocate_vector<complex<double>>(n2), *y = allocate_vector<complex<double>>(n2), *t = allocate_vector<complex<double>>(n2),
                   *u = allocate_vector<complex<double>>(n2), *b = allocate_vector<complex<double>>(n2), *bp = allocate_vector<complex<double>>(n2);
    gaussian(x, n2, 21); gaussian(y, n2, 22); gaussian(b, n2, 23);
    wilson.build_dagger_stencil();
    zero_vector(t, n2); wilson.apply_M(t, x);
    zero_vector(u, n2); wilson.apply_M_dagger(u, y);
    const complex<double> lhs = dot(y, t, n2), rhs = dot(u, x, n2);
    check(abs(lhs - rhs) / abs(lhs) < 1e-12, "n17 <y, M x> = <M^dag y, x>", abs(lhs - rhs) / abs(lhs));
    // gamma5-hermiticity: M^dag = g5 M g5
    wilson.gamma5(t, y); zero_vector(bp, n2); wilson.apply_M(bp, t); wilson.gamma5(bp);
    check(sqrt(diffnorm2sq(bp, u, n2) / norm2sq(u, n2)) < 1e-13, "Wilson gamma5-hermiticity M^dag = g5 M g5", sqrt(diffnorm2sq(bp, u, n2) / norm2sq(u, n2)));
    // CGNR: M^dag M x = M^dag b through the type dispatch (prepare / apply function / reconstruct)
    zero_vector(bp, n2); wilson.prepare_M(bp, b, QMG_MATVEC_MDAGGER_M);
    zero_vector(t, n2);
    inversion_info inv = minv_vector_cg(t, bp, (int)n2, 4000, 1e-11, Stencil2D::get_apply_function(QMG_MATVEC_MDAGGER_M), (void*)&wilson, &quiet);
    zero_vector(u, n2); wilson.reconstruct_M(u, t, b, QMG_MATVEC_MDAGGER_M);
    check(inv.success && rel_resid(&wilson, u, b, n2) < 1e-8, "n17 CGNR (M^dag M) solves the original system", rel_resid(&wilson, u, b, n2));
    // CGNE: M M^dag y = b, x = M^dag y
    zero_vector(bp, n2); wilson.prepare_M(bp, b, QMG_MATVEC_M_MDAGGER);
    zero_vector(t, n2);
    inv = minv_vector_cg(t, bp, (int)n2, 4000, 1e-11, Stencil2D::get_apply_function(QMG_MATVEC_M_MDAGGER), (void*)&wilson, &quiet);
    zero_vector(u, n2); wilson.reconstruct_M(u, t, b, QMG_MATVEC_M_MDAGGER);
    check(inv.success && rel_resid(&wilson, u, b, n2) < 1e-8, "n17 CGNE (M M^dag) solves the original system", rel_resid(&wilson, u, b, n2));

    // n18: right block Jacobi  (A C^-1) y = b, x = C^-1 y
    wilson.build_rbjacobi_stencil();
    zero_vector(bp, n2); wilson.prepare_M(bp, b, QMG_MATVEC_RIGHT_JACOBI);
    zero_vector(t, n2);
    inv = minv_vector_gcr_restart(t, bp, (int)n2, 4000, 1e-10, 32, Stencil2D::get_apply_function(QMG_MATVEC_RIGHT_JACOBI), (void*)&wilson, &quiet);
    zero_vector(u, n2); wilson.reconstruct_M(u, t, b, QMG_MATVEC_RIGHT_JACOBI);
    check(inv.success && rel_resid(&wilson, u, b, n2) < 1e-8, "n18 right-block-Jacobi GCR reconstructs the original solution", rel_resid(&wilson, u, b, n2));
    // n18/n19: Schur system on the even half
    zero_vector(bp, n2); wilson.prepare_M(bp, b, QMG_MATVEC_RIGHT_SCHUR);
    zero_vector(t, n2);
    inv = minv_vector_gcr_restart(t, bp, (int)(n2 / 2), 4000, 1e-10, 32, Stencil2D::get_apply_function(QMG_MATVEC_RIGHT_SCHUR), (void*)&wilson, &quiet);
    zero_vector(u, n2); wilson.reconstruct_M(u, t, b, QMG_MATVEC_RIGHT_SCHUR);
    check(inv.success && rel_resid(&wilson, u, b, n2) < 1e-8, "n18 Schur (even-odd) GCR reconstructs the original solution", rel_resid(&wilson, u, b, n2));
    const int schur_iters = inv.iter;
    // rbjacobi apply == original apply composed with cinv
    zero_vector(t, n2); wilson.apply_M_rbjacobi_cinv(t, x);
    zero_vector(u, n2); wilson.apply_M(u, t);
    zero_vector(bp, n2); wilson.apply_M_rbjacobi(bp, x);
    check(sqrt(diffnorm2sq(bp, u, n2) / norm2sq(u, n2)) < 1e-12, "rbjacobi apply == M . C^-1", sqrt(diffnorm2sq(bp, u, n2) / norm2sq(u, n2)));

    // n21: rbj-dagger and the two right-Jacobi normal operators
    wilson.build_rbj_dagger_stencil();
    zero_vector(t, n2); wilson.apply_M_rbjacobi(t, x);
    zero_vector(u, n2); wilson.apply_M_rbj_dagger(u, y);
    const complex<double> l2 = dot(y, t, n2), r2 = dot(u, x, n2);
    check(abs(l2 - r2) / abs(l2) < 1e-12, "n21 <y, M_rbj x> = <M_rbj^dag y, x>", abs(l2 - r2) / abs(l2));
    zero_vector(bp, n2); wilson.prepare_M(bp, b, QMG_MATVEC_RBJ_MDAGGER_M);
    zero_vector(t, n2);
    inv = minv_vector_cg(t, bp, (int)n2, 4000, 1e-11, Stencil2D::get_apply_function(QMG_MATVEC_RBJ_MDAGGER_M), (void*)&wilson, &quiet);
    zero_vector(u, n2); wilson.reconstruct_M(u, t, b, QMG_MATVEC_RBJ_MDAGGER_M);
    check(inv.success && rel_resid(&wilson, u, b, n2) < 1e-8, "n21 rbj CGNR (M^dag M) reconstructs the original solution", rel_resid(&wilson, u, b, n2));
    zero_vector(bp, n2); wilson.prepare_M(bp, b, QMG_MATVEC_RBJ_M_MDAGGER);
    zero_vector(t, n2);
    inv = minv_vector_cg(t, bp, (int)n2, 4000, 1e-11, Stencil2D::get_apply_function(QMG_MATVEC_RBJ_M_MDAGGER), (void*)&wilson, &quiet);
    zero_vector(u, n2); wilson.reconstruct_M(u, t, b, QMG_MATVEC_RBJ_M_MDAGGER);
    check(inv.success && rel_resid(&wilson, u, b, n2) < 1e-8, "n21 rbj CGNE (M M^dag) reconstructs the original solution", rel_resid(&wilson, u, b, n2));
    cout << "       (Schur GCR iterations: " << schur_iters << ")\n";
    for (complex<double>** p : {&x, &y, &t, &u, &b, &bp}) deallocate_vector(p);
  }

  // ---- n08: Galerkin through MultigridMG: built coarse stencil vs the emulated level (R A P)
  {
    const int nvec = 4;
    Lattice2D clat(L / 4, L / 4, nvec);
    complex<double>** nv = new complex<double>*[nvec];
    for (int j = 0; j < nvec; j++) { nv[j] = allocate_vector<complex<double>>(n2); gaussian(nv[j], n2, 40 + j); }
    TransferMG transfer(&lat2, &clat, nv, true, false, QMG_DOUBLE_NONE);
    // P^dag P = 1 (n05)
    const long nc_ = clat.get_size_cv_l();
    complex<double>*vc = allocate_vector<complex<double>>(nc_), *vf = allocate_vector<complex<double>>(n2), *vc2 = allocate_vector<complex<double>>(nc_);
    gaussian(vc, nc_, 50); zero_vector(vf, n2); zero_vector(vc2, nc_);
    transfer.prolong_c2f(vc, vf); transfer.restrict_f2c(vf, vc2);
    check(sqrt(diffnorm2sq(vc, vc2, nc_) / norm2sq(vc, nc_)) < 1e-13, "n05 P^dag P = 1 on the coarse space", sqrt(diffnorm2sq(vc, vc2, nc_) / norm2sq(vc, nc_)));
    MultigridMG built(&lat2, &wilson), emulated(&lat2, &wilson);
    built.push_level(&clat, &transfer, true, false, MultigridMG::QMG_MULTIGRID_PRECOND_ORIGINAL, nv);
    emulated.push_level(&clat, &transfer, false, false, MultigridMG::QMG_MULTIGRID_PRECOND_ORIGINAL, (complex<double>**)0);
    complex<double>*o1 = allocate_vector<complex<double>>(nc_), *o2 = allocate_vector<complex<double>>(nc_);
    zero_vector(o1, nc_); zero_vector(o2, nc_);
    built.apply_stencil(o1, vc, 1);
    emulated.apply_stencil(o2, vc, 1);
    check(sqrt(diffnorm2sq(o1, o2, nc_) / norm2sq(o2, nc_)) < 1e-12, "n08 Galerkin: built coarse apply == emulated R A P", sqrt(diffnorm2sq(o1, o2, nc_) / norm2sq(o2, nc_)));
    check(built.get_num_levels() == 2 && built.get_global_null_vectors(0) != 0 && emulated.get_stencil(1) == 0, "MultigridMG level bookkeeping", built.get_num_levels());
    built.pop_level();
    check(built.get_num_levels() == 1, "MultigridMG pop_level", built.get_num_levels());
    for (complex<double>** p : {&vc, &vf, &vc2, &o1, &o2}) deallocate_vector(p);
    for (int j = 0; j < nvec; j++) deallocate_vector(&nv[j]);
    delete[] nv;
  }

  // ---- n01 / n14: U(1) utilities (u1/u1_utils.h): write_gauge_u1 -> read_gauge_u1 round trip in the reference's text format,
  //      plaquette / topology of the stored configuration, a non-compact heatbath step, coarse-shift bookkeeping
  {
    const string tmp_cfg = string(getenv("TMPDIR") ? getenv("TMPDIR") : "/tmp") + "/qmg_selftest_cfg." + to_string((long)getpid()) + ".dat";
    write_gauge_u1(gauge, &lat1, tmp_cfg);
    complex<double>* g2 = allocate_vector<complex<double>>(lat1.get_size_gauge());
    const bool rd = read_gauge_u1(g2, &lat1, tmp_cfg);
    std::remove(tmp_cfg.c_str());
    check(rd && sqrt(diffnorm2sq(gauge, g2, lat1.get_size_gauge()) / norm2sq(gauge, lat1.get_size_gauge())) < 1e-15, "write_gauge_u1 -> read_gauge_u1 round trip",
          sqrt(diffnorm2sq(gauge, g2, lat1.get_size_gauge())));
    const complex<double> plaq = get_plaquette_u1(gauge, &lat1);
    const double topo = get_topo_u1(gauge, &lat1);
    check(plaq.real() > 0.85 && plaq.real() < 0.97 && fabs(topo - std::round(topo)) < 1e-9, "plaquette of the beta = 6.0 fixture in (0.85, 0.97), integer topological charge", plaq.real());
    double* ph = allocate_vector<double>(lat1.get_size_gauge());
    qmg::ok(qmg_u1_gauge_to_phase(ph, gauge, (size_t)lat1.get_size_gauge(), 0), "qmg_u1_gauge_to_phase");
    const double s0 = get_noncompact_action_u1(ph, 6.0, &lat1);
    HeatbathRng rng(99ull);
    heatbath_noncompact_update(ph, &lat1, 6.0, 50, rng);
    polar_vector(ph, g2, (size_t)lat1.get_size_gauge());
    const double p1 = get_plaquette_u1(g2, &lat1).real(), s1 = get_noncompact_action_u1(ph, 6.0, &lat1) / (L * L);
    check(rng.sweeps_done == 50 && p1 > 0.88 && p1 < 0.96 && s1 > 0.4 && s1 < 0.6 && s0 > 0.0, "heatbath at beta = 6.0 keeps the plaquette near exp(-1/12), action per plaquette near 1/2", p1);
    deallocate_vector(&ph); deallocate_vector(&g2);
  }
  // ---- coarse shift after a variant swap (deliberate deviation from coarse.h:131, which leaves shift_backup at 0)
  {
    const int nvec = 8;
    Lattice2D latc(L / 4, L / 4, nvec);
    Wilson2D wm(&lat2, complex<double>(0.13, 0.0), gauge);
    complex<double>** nv = new complex<double>*[nvec];
    for (int j = 0; j < nvec; j++) { nv[j] = allocate_vector<complex<double>>(n2); gaussian(nv[j], n2, 500ull + j); }
    TransferMG tr(&lat2, &latc, nv, true, false, QMG_DOUBLE_NONE);
    CoarseOperator2D co(&latc, &wm, &lat2, &tr, false, false, CoarseOperator2D::QMG_COARSE_BUILD_DAGGER);
    const long ncv = latc.get_size_cv_l();
    complex<double>*v = allocate_vector<complex<double>>(ncv), *a1 = allocate_vector<complex<double>>(ncv), *a2 = allocate_vector<complex<double>>(ncv);
    gaussian(v, ncv, 600ull);
    zero_vector(a1, ncv); co.apply_M(a1, v);
    zero_vector(a2, ncv); co.apply_M_dagger(a2, v);   // swaps the dagger stencil in and out again
    zero_vector(a2, ncv); co.apply_M(a2, v);
    check(co.get_shift() == complex<double>(0.13, 0.0) && diffnorm2sq(a1, a2, ncv) == 0.0, "coarse operator keeps its (non-zero) shift across a dagger swap", co.get_shift().real());
    // the complex<float> copies of enable_f32_matrices mirror the ORIGINAL arrays: while the dagger stencil is swapped in they must not be applied
    zero_vector(a1, ncv); co.apply_M_dagger(a1, v);
    const bool f32on = co.enable_f32_matrices();
    zero_vector(a2, ncv); co.apply_M_dagger(a2, v);
    check(f32on && diffnorm2sq(a1, a2, ncv) == 0.0, "apply_M_dagger is untouched by fp32-stored ORIGINAL matrices", sqrt(diffnorm2sq(a1, a2, ncv) / norm2sq(a1, ncv)));
    zero_vector(a1, ncv); co.apply_M(a1, v);
    co.disable_f32_matrices();
    zero_vector(a2, ncv); co.apply_M(a2, v);
    const double d32 = sqrt(diffnorm2sq(a1, a2, ncv) / norm2sq(a2, ncv));
    check(d32 > 0.0 && d32 < 1e-6, "apply_M with fp32-stored matrices is the fp64 apply to fp32 rounding", d32);
    // complex<half> storage (opt-in): nc = 8 qualifies (a multiple of 4, entries inside half range); the apply is the fp64 apply to half rounding
    const bool f16on = co.enable_f32_matrices(16);
    zero_vector(a1, ncv); co.apply_M(a1, v);
    const double d16 = sqrt(diffnorm2sq(a1, a2, ncv) / norm2sq(a2, ncv));
    check(f16on && co.narrow[STORAGE].bits == 16 && d16 > 1e-6 && d16 < 2e-3, "apply_M with 16-bit-stored matrices is the fp64 apply to half rounding", d16);
    co.disable_f32_matrices();
    for (complex<double>** p : {&v, &a1, &a2}) deallocate_vector(p);
    for (int j = 0; j < nvec; j++) deallocate_vector(&nv[j]);
    delete[] nv;
  }

  // ---- the batch engine's operators by type (include/qmg/batch.hpp: apply_stencil_typed_batch / prepare_M_batch / reconstruct_M_batch) against the
  // single-vector type dispatch (Stencil2D::apply_M / prepare_M / reconstruct_M, stencil_2d.h:2418-2527): all nine types, three systems, on the Wilson
  // operator (nc = 2 kernels) and on a Galerkin operator with every variant built (nc = 8 kernels)
  {
    const int nvec = 8, nb = 3;
    Lattice2D latc(L / 4, L / 4, nvec);
    complex<double>** nv = new complex<double>*[nvec];
    for (int j = 0; j < nvec; j++) { nv[j] = allocate_vector<complex<double>>(n2); gaussian(nv[j], n2, 900ull + j); }
    TransferMG tr(&lat2, &latc, nv, true, false, QMG_DOUBLE_NONE);
    CoarseOperator2D co(&latc, &wilson, &lat2, &tr, false, false, CoarseOperator2D::QMG_COARSE_BUILD_ALL);
    co.disable_f32_matrices();
    const QMGStencilType types[9] = {QMG_MATVEC_ORIGINAL, QMG_MATVEC_DAGGER, QMG_MATVEC_RIGHT_JACOBI, QMG_MATVEC_RIGHT_SCHUR, QMG_MATVEC_M_MDAGGER,
                                     QMG_MATVEC_MDAGGER_M, QMG_MATVEC_RBJ_DAGGER, QMG_MATVEC_RBJ_M_MDAGGER, QMG_MATVEC_RBJ_MDAGGER_M};
    Stencil2D* ops[2] = {&wilson, &co};
    for (int o = 0; o < 2; o++) {
      Stencil2D* st = ops[o];
      const size_t n = (size_t)st->get_lattice()->get_size_cv_l();
      qmg::BatchPool pool(n, nb);
      qmg::Batch in = pool.get(), rhs2 = pool.get(), out = pool.get(), ref = pool.get();
      const unsigned all = qmg::full_mask(nb);
      for (int k = 0; k < nb; k++) { gaussian(in.vec(k), (long)n, 950ull + 10 * o + k); gaussian(rhs2.vec(k), (long)n, 980ull + 10 * o + k); }
      double worst_apply = 0.0, worst_prep = 0.0, worst_rec = 0.0;
      for (int t = 0; t < 9; t++) {
        const size_t nsolve = (types[t] == QMG_MATVEC_RIGHT_SCHUR) ? n / 2 : n;
        BatchOp bop(st, types[t]);
        qmg::bzero(out, n, all); qmg::bzero(ref, n, all);
        apply_stencil_typed_batch<double>(out, in, all, (void*)&bop);
        for (int k = 0; k < nb; k++) Stencil2D::get_apply_function(types[t])(ref.vec(k), in.vec(k), (void*)st);
        for (int k = 0; k < nb; k++) worst_apply = std::max(worst_apply, sqrt(diffnorm2sq(out.vec(k), ref.vec(k), (long)nsolve) / norm2sq(ref.vec(k), (long)nsolve)));
        qmg::bzero(out, n, all); qmg::bzero(ref, n, all);
        prepare_M_batch<double>(st, types[t], out, in, all);
        for (int k = 0; k < nb; k++) st->prepare_M(ref.vec(k), in.vec(k), types[t]);
        for (int k = 0; k < nb; k++) worst_prep = std::max(worst_prep, sqrt(diffnorm2sq(out.vec(k), ref.vec(k), (long)n) / norm2sq(ref.vec(k), (long)n)));
        qmg::bzero(out, n, all); qmg::bzero(ref, n, all);
        reconstruct_M_batch<double>(st, types[t], out, in, rhs2, all);
        for (int k = 0; k < nb; k++) st->reconstruct_M(ref.vec(k), in.vec(k), rhs2.vec(k), types[t]);
        for (int k = 0; k < nb; k++) worst_rec = std::max(worst_rec, sqrt(diffnorm2sq(out.vec(k), ref.vec(k), (long)n) / norm2sq(ref.vec(k), (long)n)));
      }
      check(worst_apply < 1e-13, o == 0 ? "batch applies by type == Stencil2D::apply_M by type (Wilson, 9 types x 3 systems)" : "batch applies by type == apply_M by type (Galerkin nc = 8, 9 types x 3 systems)", worst_apply);
      check(worst_prep < 1e-13, o == 0 ? "prepare_M_batch == prepare_M (Wilson)" : "prepare_M_batch == prepare_M (Galerkin nc = 8)", worst_prep);
      check(worst_rec < 1e-13, o == 0 ? "reconstruct_M_batch == reconstruct_M (Wilson)" : "reconstruct_M_batch == reconstruct_M (Galerkin nc = 8)", worst_rec);
      // (bcg_core on a batch against each system solved alone: drivers/krylov_batch_parity.cpp, on six systems that stop at different iterations)
      // a normal operator with CoarsestSolveMG::normal_shift (stateful_multigrid.h:724-729)
      BatchOp sh(st, QMG_MATVEC_RBJ_MDAGGER_M);
      sh.normal_shift = complex<double>(0.37, 0.0); sh.shift_length = n;
      apply_stencil_typed_batch<double>(out, in, all, (void*)&sh);
      Stencil2D::get_apply_function(QMG_MATVEC_RBJ_MDAGGER_M)(ref.vec(1), in.vec(1), (void*)st);
      caxpy(complex<double>(0.37, 0.0), in.vec(1), ref.vec(1), (long)n);
      const double dsh = sqrt(diffnorm2sq(out.vec(1), ref.vec(1), (long)n) / norm2sq(ref.vec(1), (long)n));
      check(dsh < 1e-13, o == 0 ? "shifted normal operator (Wilson)" : "shifted normal operator (Galerkin nc = 8)", dsh);
    }
    // the route of an apply on the Galerkin operator (nc = 8, no links): the stored arrays in fp64, their narrow copies, one epilogue
    {
      RouteCheck route((size_t)latc.get_size_cv_l());
      const size_t n = route.n;
      void* st = qmg::current_stream();
      const unsigned M0 = QMG_P_ALL | QMG_P_ZERO, OE0 = QMG_P_OE | QMG_P_ZERO_O, C0 = QMG_P_CLOVER | QMG_P_ZERO;
      const qmg_apply_epilogue e = {route.other, 1.0, -1.0, 0};
      qmg_stencil_desc d = co.desc(), d0 = co.desc();   // d0: arrays by hand, no shifts (the right-block-Jacobi pieces)
      for (int i = 0; i < 2; i++) d0.shift[i] = d0.eo_shift[i] = d0.dof_shift[i] = 0.0;
      route("Galerkin nc = 8, fp64 == qmg_stencil_apply_batch", !co.narrow[STORAGE].on, [&](void* o) { co.apply_M_overwrite((complex<double>*)o, route.in); return true; },
            [&](void* o) { return qmg_stencil_apply_batch(&d, o, route.in, M0, 1, 0, 1u, st); });
      route("Galerkin nc = 8, epilogue on system 1 of 2 == qmg_stencil_apply_epi_t", true,
            [&](void* o) { return co.launch_set_epi<double>(M0, (complex<double>*)o, route.in, Stencil2D::QMG_ARR_ORIGINAL, co.shift, co.eo_shift, co.dof_shift, n, 1, e); },
            [&](void* o) { return qmg_stencil_apply_epi_t(QMG_C64, 0, &d, o, route.in, M0, n, 1, &e, st); });
      bool on = co.enable_f32_matrices(32);
      d.clover = clover_copy(co, STORAGE); d.hopping = hopping_copy(co, STORAGE);
      route("Galerkin nc = 8, enable_f32_matrices(32) == qmg_stencil_apply_mat32", on && co.narrow[STORAGE].bits == 32 && d.clover && d.hopping,
            [&](void* o) { co.apply_M_overwrite((complex<double>*)o, route.in); return true; }, [&](void* o) { return qmg_stencil_apply_mat32(&d, o, route.in, M0, 1, 0, 1u, st); });
      d0.clover = 0; d0.hopping = hopping_copy(co, STORAGE, S::QMG_ARR_RBJ_HOPPING);
      route("Galerkin nc = 8, rbj hops alone == qmg_stencil_apply_mat32 on rbj_hopping32", d0.hopping != 0,
            [&](void* o) { co.launch_set_batch<double>(OE0, (complex<double>*)o, route.in, Stencil2D::QMG_ARR_RBJ_HOPPING, 0.0, 0.0, 0.0, 2, n, 0b10u); return true; },
            [&](void* o) { return qmg_stencil_apply_mat32(&d0, o, route.in, OE0, 2, n, 0b10u, st); });
      d0.clover = clover_copy(co, STORAGE, S::QMG_ARR_RBJ_CINV); d0.hopping = 0;
      route("Galerkin nc = 8, cinv alone == qmg_stencil_apply_mat32 on rbj_cinv32", d0.clover != 0,
            [&](void* o) { co.launch_set_batch<double>(C0, (complex<double>*)o, route.in, Stencil2D::QMG_ARR_RBJ_CINV, 0.0, 0.0, 0.0, 2, n, 0b11u); return true; },
            [&](void* o) { return qmg_stencil_apply_mat32(&d0, o, route.in, C0, 2, n, 0b11u, st); });
      on = co.enable_f32_matrices(16);
      d.clover = clover_copy(co, STORAGE); d.hopping = hopping_copy(co, STORAGE);
      route("Galerkin nc = 8, enable_f32_matrices(16) == qmg_stencil_apply_mat16_t", on && co.narrow[STORAGE].bits == 16 && d.clover && d.hopping,
            [&](void* o) { co.apply_M_overwrite((complex<double>*)o, route.in); return true; },
            [&](void* o) { return qmg_stencil_apply_mat16_t(QMG_C64, &d, o, route.in, M0, 1, 0, 1u, st); });
      co.disable_f32_matrices();
    }
    for (int j = 0; j < nvec; j++) deallocate_vector(&nv[j]);
    delete[] nv;
  }

  // ---- clear_stencils / prune_stencils on an operator that applies straight from the links: the cached link copy must
  // not outlive the stored arrays.  Reference semantics (stencil_2d.h:339-404): after clear_stencils the matrices are zero, so
  // apply_M adds shift * rhs and nothing else; after pruning the hopping term only clover + shift act.
  {
    const double m = 0.21;
    complex<double>*v = allocate_vector<complex<double>>(n2), *a = allocate_vector<complex<double>>(n2), *w = allocate_vector<complex<double>>(n2);
    gaussian(v, n2, 77);
    {
      Wilson2D wil(&lat2, m, gauge);
      wil.clear_stencils();
      zero_vector(a, n2); wil.apply_M(a, v);
      caxy(m, v, w, n2);
      check(diffnorm2sq(a, w, n2) <= 1e-28 * norm2sq(w, n2), "after clear_stencils apply_M is the shift term alone", sqrt(diffnorm2sq(a, w, n2) / norm2sq(w, n2)));
      zero_vector(a, n2); apply_stencil_2D_M(a, v, (void*)&wil);
      check(diffnorm2sq(a, w, n2) <= 1e-28 * norm2sq(w, n2), "after clear_stencils apply_stencil_2D_M is the shift term alone", sqrt(diffnorm2sq(a, w, n2) / norm2sq(w, n2)));
    }
    {
      Wilson2D wil(&lat2, m, gauge);
      wil.prune_stencils(QMG_PIECE_HOPPING);
      zero_vector(a, n2); wil.apply_M(a, v);
      caxy(2.0 + m, v, w, n2);   // Wilson clover = 2 w 1 (wilson.h:167-170), w = 1
      check(diffnorm2sq(a, w, n2) <= 1e-28 * norm2sq(w, n2), "after pruning the hopping term apply_M is clover + shift", sqrt(diffnorm2sq(a, w, n2) / norm2sq(w, n2)));
    }
    for (complex<double>** p : {&v, &a, &w}) deallocate_vector(p);
  }

  // ---- the route of an apply on the Wilson operator (nc = 2): from the links, from the stored arrays, from the fp32 shadows
  {
    Wilson2D w(&lat2, complex<double>(0.05, 0.0), gauge);
    RouteCheck route((size_t)n2);
    const size_t n = route.n;
    void* st = qmg::current_stream();
    const unsigned M0 = QMG_P_ALL | QMG_P_ZERO, OE0 = QMG_P_OE | QMG_P_ZERO_O;
    const qmg_apply_epilogue e = {route.other, 1.0, -1.0, 0};
    const int Ly = lat2.get_dim_mu(1);
    qmg_stencil_desc d = w.desc();
    auto apply_M = [&](void* o) { w.apply_M_overwrite((complex<double>*)o, route.in); return true; };
    auto batch32 = [&](void* o) {
      w.launch_set_batch<float>(M0, (complex<float>*)o, route.in32, Stencil2D::QMG_ARR_ORIGINAL, w.shift, w.eo_shift, w.dof_shift, 3, n, 0b101u);
      return true;
    };
    route("Wilson, plain == qmg_wilson_apply_direct", w.direct.on && w.direct.kind == Stencil2D::QMG_DIRECT_WILSON, apply_M,
          [&](void* o) { return qmg_wilson_apply_direct(QMG_C64, &d, w.direct.gauge, Ly, 0, w.direct.w, o, route.in, 0, 0, M0, 1, 0, 0, 1u, 0, st); });
    route("Wilson, epilogue on system 1 of 2 == qmg_wilson_apply_direct_epi", w.direct.on,
          [&](void* o) { return w.launch_set_epi<double>(M0, (complex<double>*)o, route.in, Stencil2D::QMG_ARR_ORIGINAL, w.shift, w.eo_shift, w.dof_shift, n, 1, e); },
          [&](void* o) { return qmg_wilson_apply_direct_epi(QMG_C64, &d, w.direct.gauge, Ly, 0, w.direct.w, o, route.in, 0, 0, M0, 2, n, 0, 0b10u, &e, st); });
    w.build_rbjacobi_stencil();
    qmg_stencil_desc dh = w.desc();
    dh.clover = 0; dh.hopping = w.rbjacobi_hopping;
    for (int i = 0; i < 2; i++) dh.shift[i] = dh.eo_shift[i] = dh.dof_shift[i] = 0.0;
    route("Wilson, rbj hops == qmg_wilson_hops_direct", w.direct.on && w.direct.rbj_scale != 0.0,
          [&](void* o) { w.launch_set_batch<double>(OE0, (complex<double>*)o, route.in, Stencil2D::QMG_ARR_RBJ_HOPPING, 0.0, 0.0, 0.0, 1, 0, 1u); return true; },
          [&](void* o) { return qmg_wilson_hops_direct(QMG_C64, &dh, w.direct.gauge, Ly, 0, w.direct.w, w.direct.rbj_scale, o, route.in, 0, 0, OE0, 1, 0, 0, 1u, 0, st); });
    bool on = w.enable_f32_shadow(false);
    route("Wilson, fp32 batch of 3, mask 0b101, links == qmg_wilson_apply_direct on gauge32", on && w.direct.gauge32 != 0, batch32,
          [&](void* o) { return qmg_wilson_apply_direct(QMG_C32, &d, w.direct.gauge32, Ly, 0, w.direct.w, o, route.in32, 0, 0, M0, 3, n, 0, 0b101u, 0, st); });
    w.build_dagger_stencil();
    w.perform_swap_dagger();
    qmg_stencil_desc dd = w.desc();
    route("Wilson, dagger swapped in == qmg_stencil_apply_batch on the swapped arrays", dd.clover != d.clover && dd.hopping != d.hopping, apply_M,
          [&](void* o) { return qmg_stencil_apply_batch(&dd, o, route.in, M0, 1, 0, 1u, st); });
    w.perform_swap_dagger();
    w.drop_direct_links();
    route("Wilson, links dropped == qmg_stencil_apply_batch", !w.direct.on, apply_M, [&](void* o) { return qmg_stencil_apply_batch(&d, o, route.in, M0, 1, 0, 1u, st); });
    qmg_stencil_desc dn = d;
    dn.clover = clover_copy(w, SHADOW); dn.hopping = hopping_copy(w, SHADOW);
    route("Wilson, fp32 batch of 3, mask 0b101, shadow == qmg_stencil_apply_t", w.narrow[SHADOW].on && !w.narrow[HALF].on, batch32,
          [&](void* o) { return qmg_stencil_apply_t(QMG_C32, &dn, o, route.in32, M0, 3, n, 0b101u, st); });
    on = w.enable_f32_shadow(true);
    dn.clover = clover_copy(w, HALF); dn.hopping = hopping_copy(w, HALF);
    route("Wilson, fp32 batch of 3, mask 0b101, half shadow == qmg_stencil_apply_h16", on && w.narrow[HALF].on, batch32,
          [&](void* o) { return qmg_stencil_apply_h16(&dn, o, route.in32, M0, 3, n, 0b101u, st); });
  }

  // ---- which narrow copies of the matrices exist after which call (narrow_census): the answers are written out by hand from the rules of
  // enable_f32_matrices / narrow_rbjacobi_copies / enable_f32_shadow and their disable_* (include/qmg/stencil2d.hpp)
  {
    typedef CoarseOperator2D C;
    auto copies = [&](const string& what, Stencil2D& op, bool as_expected, const string& want) {
      const string got = narrow_census(op);
      check(as_expected && got == want, "copies: " + what + " -> " + want + (got == want ? "" : " (got " + got + ")"), 0);
    };
    auto said = [](const Captured& c, const char* line) { return c.text.str().find(line) != string::npos; };
    {   // storage under fp64 vectors, Galerkin nc = 8, the right-block-Jacobi stencil built AFTER the copies
      Galerkin g(&lat2, &wilson, L, 8, C::QMG_COARSE_BUILD_ORIGINAL);
      Stencil2D& op = *g.op;
      copies("Galerkin nc = 8, fresh", op, true, "S-: F-: H-: -");
      bool on = op.enable_f32_matrices(32);
      copies("enable_f32_matrices(32)", op, on, "S32:ch F-: H-: -");
      on = op.enable_f32_matrices(16);
      copies("enable_f32_matrices(16) over it", op, on, "S16:ch F-: H-: -");
      op.build_rbjacobi_stencil();
      copies("build_rbjacobi_stencil after it: its copies in the level's width", op, op.built_rbjacobi, "S16:chri F-: H-: -");
      op.disable_f32_matrices();
      copies("disable_f32_matrices", op, true, "S-: F-: H-: -");
      on = op.enable_f32_matrices(32);
      copies("enable_f32_matrices(32) after build_rbjacobi_stencil", op, on, "S32:chri F-: H-: -");
      on = op.enable_f32_matrices(16);
      copies("enable_f32_matrices(16) after build_rbjacobi_stencil", op, on, "S16:chri F-: H-: -");
      on = op.enable_f32_shadow(true);
      copies("enable_f32_shadow(true) beside the storage", op, on, "S16:chri F+:chri H+:chr -");
      op.disable_f32_shadow();
      copies("disable_f32_shadow leaves the storage", op, true, "S16:chri F-: H-: -");
      on = op.enable_f32_shadow(false);
      op.disable_f32_matrices();
      copies("disable_f32_matrices leaves the shadow", op, on, "S-: F+:chri H-: -");
    }
    {   // the shadows of a Galerkin operator with every variant built; no links, so no gauge32
      Galerkin g(&lat2, &wilson, L, 8, C::QMG_COARSE_BUILD_ALL);
      Stencil2D& op = *g.op;
      bool on = op.enable_f32_shadow(false);
      copies("Galerkin nc = 8, every variant built, enable_f32_shadow(false)", op, on, "S-: F+:chriCHR H-: -");
      on = op.enable_f32_shadow(true);
      copies("... enable_f32_shadow(true)", op, on, "S-: F+:chriCHR H+:chr -");
      op.disable_f32_shadow();
      copies("... disable_f32_shadow", op, true, "S-: F-: H-: -");
    }
    {   // nc = 4: no storage, no half shadow
      Galerkin g(&lat2, &wilson, L, 4, C::QMG_COARSE_BUILD_ORIGINAL);
      Stencil2D& op = *g.op;
      bool on;
      { Captured c; on = op.enable_f32_matrices(32); on = on || !said(c, "fp32 matrix storage is not available for nc = 4."); }
      copies("Galerkin nc = 4, enable_f32_matrices(32) refuses", op, !on, "S-: F-: H-: -");
      on = op.enable_f32_shadow(true);
      copies("Galerkin nc = 4, enable_f32_shadow(true): complex<float> only", op, on, "S-: F+:ch H-: -");
    }
    {   // the Wilson operator (nc = 2, applied from its links): no storage; the shadow with each variant built and not; gauge32 outlives the shadow
      Wilson2D w(&lat2, complex<double>(0.05, 0.0), gauge);
      copies("Wilson, fresh", w, w.direct.on, "S-: F-: H-: -");
      bool on;
      { Captured c; on = w.enable_f32_matrices(32); on = on || !said(c, "fp32 matrix storage is not available for nc = 2."); }
      copies("Wilson, enable_f32_matrices(32) refuses", w, !on, "S-: F-: H-: -");
      { Captured c; on = w.enable_f32_matrices(16); on = on || !said(c, "fp32 matrix storage is not available for nc = 2."); }
      copies("Wilson, enable_f32_matrices(16) refuses", w, !on, "S-: F-: H-: -");
      on = w.enable_f32_shadow(false);
      copies("Wilson, no variant, enable_f32_shadow(false)", w, on, "S-: F+:ch H-: g");
      on = w.enable_f32_shadow(true);
      copies("Wilson, no variant, enable_f32_shadow(true)", w, on, "S-: F+:ch H+:ch g");
      w.disable_f32_shadow();
      copies("Wilson, disable_f32_shadow leaves gauge32", w, w.direct.gauge32 != 0, "S-: F-: H-: g");
      w.build_rbjacobi_stencil();
      on = w.enable_f32_shadow(false);
      copies("Wilson, rbjacobi built, enable_f32_shadow(false)", w, on, "S-: F+:chri H-: g");
      on = w.enable_f32_shadow(true);
      copies("Wilson, rbjacobi built, enable_f32_shadow(true)", w, on, "S-: F+:chri H+:chr g");
      w.build_rbj_dagger_stencil();
      on = w.enable_f32_shadow(false);
      copies("Wilson, rbjacobi and rbj-dagger built, enable_f32_shadow(false)", w, on, "S-: F+:chriR H-: g");
      on = w.enable_f32_shadow(true);
      copies("Wilson, rbjacobi and rbj-dagger built, enable_f32_shadow(true)", w, on, "S-: F+:chriR H+:chr g");
      w.build_dagger_stencil();
      on = w.enable_f32_shadow(false);
      copies("Wilson, every variant built, enable_f32_shadow(false)", w, on, "S-: F+:chriCHR H-: g");
      on = w.enable_f32_shadow(true);
      copies("Wilson, every variant built, enable_f32_shadow(true)", w, on, "S-: F+:chriCHR H+:chr g");
      // while a variant is swapped in: refused, and the shadow that was on is gone
      bool (Stencil2D::*const swaps[3])() = {&Stencil2D::perform_swap_dagger, &Stencil2D::perform_swap_rbjacobi, &Stencil2D::perform_swap_rbj_dagger};
      const char* const names[3] = {"the dagger stencil", "the rbjacobi stencil", "the rbj-dagger stencil"};
      for (int v = 0; v < 3; v++) {
        on = w.enable_f32_shadow(v == 1);
        const bool in = (w.*swaps[v])();
        bool refused;
        { Captured c; refused = !w.enable_f32_shadow(v != 1) && said(c, "enable_f32_shadow called while a stencil variant is swapped in."); }
        const bool out = !(w.*swaps[v])();
        copies(string("Wilson, enable_f32_shadow with ") + names[v] + " swapped in refuses", w, on && in && refused && out, "S-: F-: H-: g");
      }
      // update_links with a shadow on: the variants go, the copies stay as they were (stale: "call again after changing the matrices")
      on = w.enable_f32_shadow(true);
      const void* const before = clover_copy(w, SHADOW);
      w.update_links(gauge);
      copies("Wilson, update_links under a shadow: variants dropped, copies kept", w,
             on && !w.built_dagger && !w.built_rbjacobi && !w.built_rbj_dagger && before != 0 && clover_copy(w, SHADOW) == before, "S-: F+:chriCHR H+:chr g");
      on = w.enable_f32_shadow(true);
      copies("Wilson, enable_f32_shadow(true) again after update_links", w, on, "S-: F+:ch H+:ch g");
    }
    {   // the dagger stencil alone
      Wilson2D w(&lat2, complex<double>(0.05, 0.0), gauge);
      w.build_dagger_stencil();
      bool on = w.enable_f32_shadow(false);
      copies("Wilson, dagger built alone, enable_f32_shadow(false)", w, on, "S-: F+:chCH H-: g");
      on = w.enable_f32_shadow(true);
      copies("Wilson, dagger built alone, enable_f32_shadow(true)", w, on, "S-: F+:chCH H+:ch g");
    }
  }

  deallocate_vector(&gauge);
  qmg::VecPool::release_all();
  cout << (failures ? "[SELFTEST FAILED] " : "[SELFTEST PASSED] ") << failures << " failure(s)\n";
  return qmg_driver::leave(failures);
}
