// operators.hpp -- the concrete stencils of the reference on device arrays:
//   Wilson2D (operators/wilson.h), Staggered2D (operators/staggered.h), GaugedLaplace2D
//   (operators/gaugedlaplace.h), FreeLaplace2D (tests/n02_free_laplace_test/free_laplace.h), DwfBase / Dwf2D<Ls> / createDwfLs (operators/dwf.h).
//   Not in the reference: MobiusBase / Mobius2D<Ls> / createMobiusLs, the Moebius domain-wall operator on the layout of Dwf2D, and
//   DomainWallBase, the host layer DwfBase and MobiusBase share.
// CoarseOperator2D lives in coarse.hpp (it needs TransferMG).
#ifndef QMG_OPERATORS_HPP
#define QMG_OPERATORS_HPP

#include "krylov.hpp"
#include "stencil2d.hpp"

namespace qmg {
inline void pattern(const double* scale, const int* shuffle, int nc, const complex<double>* x, complex<double>* y, size_t nsite) {
  ok(qmg_caxy_pattern(scale, shuffle, nc, x, y, nsite, current_stream()), "qmg_caxy_pattern");
}
}  // namespace qmg

// ---------------- Wilson (nc = 2: two spin components over U(1)) ----------------
struct Wilson2D : public Stencil2D {
 protected:
  Wilson2D(Wilson2D const&);
  Wilson2D& operator=(Wilson2D const&);
  double wilson_coeff;
  complex<double>* scratch;   // for in-place per-site permutations

  void per_site(const double s0, const double s1, int p0, int p1, complex<double>* out, complex<double>* in) {
    const double sc[2] = {s0, s1};
    const int sh[2] = {p0, p1};
    const size_t vol = (size_t)lat->get_volume();
    if (out == in) {
      if (!scratch) scratch = allocate_vector<complex<double>>(lat->get_size_cv_l());
      qmg::pattern(sc, sh, 2, in, scratch, vol);
      copy_vector(out, scratch, lat->get_size_cv_l());
    } else {
      qmg::pattern(sc, sh, 2, in, out, vol);
    }
  }

 public:
  void update_links(complex<double>* gauge_links) {   // wilson.h:153-226; gauge_links: DEVICE nc=1 LatticeGauge (y-slab mode: of the WHOLE lattice)
    if (qmg::slab().on)
      qmg::ok(qmg_wilson_fill_slab(clover, hopping, gauge_links, lat->get_dim_mu(0), lat->get_dim_mu(1) * qmg::slab().world, qmg::slab().rank * lat->get_dim_mu(1),
                                   lat->get_dim_mu(1), wilson_coeff, qmg::current_stream()), "qmg_wilson_fill_slab");
    else
      qmg::ok(qmg_wilson_fill(clover, hopping, gauge_links, lat->get_dim_mu(0), lat->get_dim_mu(1), wilson_coeff, qmg::current_stream()), "qmg_wilson_fill");
    drop_variant_stencils();   // (the reference leaves a built rbj_dagger stencil dangling here, wilson.h:211-225; it is dropped too)
    set_direct_links(gauge_links, wilson_coeff);   // the ORIGINAL-operator applies go straight from the links (qmg_wilson.hip)
    generated = true;
  }

  Wilson2D(Lattice2D* in_lat, complex<double> mass, complex<double>* gauge_links, double wilson_coeff = 1.0)
      : Stencil2D(in_lat, QMG_PIECE_CLOVER_HOPPING, mass, 0.0, 0.0), wilson_coeff(wilson_coeff), scratch(0) {
    if (lat->get_nc() != 2) { std::cout << "[QMG-ERROR]: Wilson2D only supports Nc = 2.\n"; return; }
    update_links(gauge_links);
  }
  ~Wilson2D() { if (scratch) deallocate_vector(&scratch); }

  static int get_dof(int i = 0) { return 2; }
  static chirality_state has_chirality() { return QMG_CHIRAL_YES; }

  virtual void gamma5(complex<double>* vec) { per_site(1.0, -1.0, 0, 1, vec, vec); }                                   // :74-81
  virtual void gamma5(complex<double>* g5_vec, complex<double>* vec) { per_site(1.0, -1.0, 0, 1, g5_vec, vec); }        // :83-93
  virtual void chiral_projection(complex<double>* v, bool is_up) { is_up ? per_site(1.0, 0.0, 0, 1, v, v) : per_site(0.0, 1.0, 0, 1, v, v); }   // :96-102
  virtual void chiral_projection_copy(complex<double>* orig, complex<double>* dest, bool is_up) {                        // :105-117
    is_up ? per_site(1.0, 0.0, 0, 1, dest, orig) : per_site(0.0, 1.0, 0, 1, dest, orig);
  }
  virtual void chiral_projection_both(complex<double>* orig_to_up, complex<double>* down) {                              // :120-125
    per_site(0.0, 1.0, 0, 1, down, orig_to_up);
    per_site(1.0, 0.0, 0, 1, orig_to_up, orig_to_up);
  }
  virtual void sigma1(complex<double>* vec) { per_site(1.0, 1.0, 1, 0, vec, vec); }                                      // :128-135
  virtual void sigma1(complex<double>* s1_vec, complex<double>* vec) { per_site(1.0, 1.0, 1, 0, s1_vec, vec); }          // :138-143
  virtual QMGDefaultChirality get_default_chirality() { return QMG_CHIRALITY_GAMMA_5; }
};

// ---------------- domain wall: what the Shamir and the Moebius operator share (nc = 2 Ls) ----------------
// Component c = 2 s + sigma: Ls copies of the Wilson spin blocks coupled along the fifth dimension.  The stored arrays (the full nc x nc
// matrices) serve the dagger / right-block-Jacobi / Galerkin builds and every piece set the links entries decline; the ORIGINAL-operator
// applies go straight from the links.  Whole lattice only: y-slabs are not served.
// DomainWallBase holds what does not depend on which operator it is: the wall mass, M5, Ls, Gamma5, the measurements on a five-dimensional
// field, and the skeleton of the 4D even-odd Schur complement M from the links, in the reference's Schur convention (stencil_2d.h:1886-1957):
// the arrays are addressed as full-length vectors of which the even half is the system -- a solver hands over half-length arrays --,
// eo_cvector is the scratch.  There is no stored fallback, so the Schur methods also serve Ls = 32.  An operator fills in
//   schur5_ready    whether the Schur methods can run, saying why not;
//   schur5_stages   the two launches of M or M^dagger;
//   prepare_M_schur5 / reconstruct_M_schur5   its own launch sequence around A_o^-1.
enum { QMG_DW_LS_MAX = 32 };
#define QMG_DW_LS_LIST(X) X(2) X(4) X(6) X(8) X(12) X(16) X(24) X(32)   // the reference's list of Ls values (dwf.h:261-293), for both factories

struct DomainWallBase : public Stencil2D {
 protected:
  complex<double> mass;
  double M5;
  int dw_Ls;
  double g5_scale[2 * QMG_DW_LS_MAX];   // gamma5 as a scale / shuffle pattern (dwf.h:36-37, 62-67), filled for Ls
  int g5_shuffle[2 * QMG_DW_LS_MAX];
  complex<double>* scratch;         // for the in-place gamma5
  complex<double>* schur5_vector;   // M rhs inside apply_M_schur5_dagger_M, allocated on demand

  DomainWallBase(Lattice2D* in_lat, complex<double> shift, complex<double> mass, double M5, int Ls)
      : Stencil2D(in_lat, QMG_PIECE_CLOVER_HOPPING, shift, 0.0, 0.0), mass(mass), M5(M5), dw_Ls(Ls), scratch(0), schur5_vector(0) {
    for (int i = 0; i < Ls && i < QMG_DW_LS_MAX; i++) {
      g5_scale[2 * i] = 1.0; g5_scale[2 * i + 1] = -1.0;
      g5_shuffle[2 * i] = 2 * (Ls - 1 - i); g5_shuffle[2 * i + 1] = 2 * (Ls - 1 - i) + 1;
    }
  }
  // what a constructor refuses, by the name of its class: a lattice that is not nc = 2 Ls, and y-slabs
  bool served(const char* cls) const {
    if (lat->get_nc() != 2 * dw_Ls) { std::cout << "[QMG-ERROR]: " << cls << " only supports Nc = 2 Ls.\n"; return false; }
    if (qmg::slab().on) { std::cout << "[QMG-ERROR]: " << cls << " is not decomposed into y-slabs.\n"; return false; }
    return true;
  }
  // whether the ORIGINAL-operator applies come from the links of `kind`
  bool links_route(int kind) const { return direct.on && direct.kind == kind && !swap_dagger && !swap_rbjacobi && !swap_rbj_dagger; }
  bool schur5_scratch() {
    if (eo_cvector == 0) eo_cvector = allocate_vector<complex<double>>(lat->get_size_cv_l());
    return eo_cvector != 0;
  }
  // lhs_e = M rhs_e or M^dagger rhs_e: the operator's two launches
  virtual bool schur5_stages(const char* who, complex<double>* lhs, complex<double>* rhs, bool dagger) = 0;

 public:
  virtual ~DomainWallBase() {
    if (scratch) deallocate_vector(&scratch);
    if (schur5_vector) deallocate_vector(&schur5_vector);
  }
  int get_Ls() const { return dw_Ls; }
  complex<double> get_mass() const { return mass; }
  double get_M5() const { return M5; }

  // (Gamma5 psi)(s, sigma) = (-1)^sigma psi(Ls-1-s, sigma)
  virtual void gamma5(complex<double>* vec) {                                                                            // dwf.h:104-108
    if (!scratch) scratch = allocate_vector<complex<double>>(lat->get_size_cv_l());
    qmg::pattern(g5_scale, g5_shuffle, 2 * dw_Ls, vec, scratch, (size_t)lat->get_volume());
    copy_vector(vec, scratch, lat->get_size_cv_l());
  }
  virtual void gamma5(complex<double>* g5_vec, complex<double>* vec) {                                                   // :110-114
    if (g5_vec == vec) { gamma5(vec); return; }
    qmg::pattern(g5_scale, g5_shuffle, 2 * dw_Ls, vec, g5_vec, (size_t)lat->get_volume());
  }
  virtual void chiral_projection(complex<double>*, bool) { return; }                                                     // empty in the reference (:117-146)
  virtual void chiral_projection_copy(complex<double>*, complex<double>*, bool) { return; }
  virtual void chiral_projection_both(complex<double>*, complex<double>*) { return; }
  virtual QMGDefaultChirality get_default_chirality() { return QMG_CHIRALITY_GAMMA_5; }

  // whether the Schur methods can run (the links route is on, and what the operator's dagger form asks); says why not, makes the scratch
  virtual bool schur5_ready(const char* who, bool dagger = false) = 0;
  // lhs_e = M rhs_e, overwriting; lhs != rhs
  void apply_M_schur5(complex<double>* lhs, complex<double>* rhs) {
    if (schur5_ready("apply_M_schur5")) schur5_stages("apply_M_schur5", lhs, rhs, false);
  }
  // lhs_e = M^dagger rhs_e: two launches, as M
  void apply_M_schur5_dagger(complex<double>* lhs, complex<double>* rhs) {
    if (schur5_ready("apply_M_schur5_dagger", true)) schur5_stages("apply_M_schur5_dagger", lhs, rhs, true);
  }
  void apply_M_schur5_dagger_M(complex<double>* lhs, complex<double>* rhs) {
    if (!schur5_ready("apply_M_schur5_dagger_M", true)) return;
    if (!schur5_vector) schur5_vector = allocate_vector<complex<double>>(lat->get_size_cv_l() / 2);
    if (schur5_stages("apply_M_schur5_dagger_M", schur5_vector, rhs, false)) schur5_stages("apply_M_schur5_dagger_M", lhs, schur5_vector, true);
  }
  // b_r,e = b_e - (hops A_o^-1 b)_e, odd half zero (full-length arrays; b_r != b)
  virtual void prepare_M_schur5(complex<double>* b_r, complex<double>* b) = 0;
  // x_e = y_e, x_o = A_o^-1 (b_o - (hops y)_o)   (x and b full-length; of y_e the even half is read)
  virtual void reconstruct_M_schur5(complex<double>* x, complex<double>* y_e, complex<double>* b) = 0;

  // ---- measurements (csrc/qmg_dwf_meas.hip; include/qmg/dwf_measure.hpp builds the propagator and the correlators on these) ----
  // psi5 = the wall source of the 4D (nc = 2) field eta4: eta4(x, 0) on (s, sigma) = (0, 0), eta4(x, 1) on (Ls-1, 1), zero elsewhere
  bool wall_source(complex<double>* psi5, complex<double>* eta4) {
    return qmg::ok(qmg_dwf_wall_source(QMG_C64, lat->get_dim_mu(0), lat->get_dim_mu(1), dw_Ls, psi5, eta4, 1, 0, 0, qmg::current_stream()), "qmg_dwf_wall_source");
  }
  // q4 = the physical quark field (Ls-1, 0), (0, 1) of psi5, or its midpoint field (Ls/2-1, 0), (Ls/2, 1) (even Ls only: false otherwise)
  bool wall_project(complex<double>* q4, complex<double>* psi5, bool midpoint) {
    if (midpoint && (dw_Ls & 1)) { std::cout << "[QMG-ERROR]: wall_project: an odd Ls has no midpoint between the walls.\n"; return false; }
    return qmg::ok(qmg_dwf_wall_project(QMG_C64, lat->get_dim_mu(0), lat->get_dim_mu(1), dw_Ls, q4, psi5, midpoint ? 1 : 0, 1, 0, 0, qmg::current_stream()),
                   "qmg_dwf_wall_project");
  }
  // sum[(y Ls + s) 2 + sigma] = sum_x |psi5(x, y; s, sigma)|^2 on the host: 2 Ls Ly doubles
  bool slice_norms(double* sum, complex<double>* psi5) {
    return qmg::ok(qmg_dwf_slice_norms(QMG_C64, lat->get_dim_mu(0), lat->get_dim_mu(1), dw_Ls, psi5, 1, 0, nullptr, sum, qmg::current_stream()), "qmg_dwf_slice_norms");
  }
};

// The Schur complement with the matrix_op_cplx signature (extra_data: a DomainWallBase*), for the Krylov solvers on the even half.
inline void apply_domain_wall_schur5_Mdagger_M(complex<double>* lhs, complex<double>* rhs, void* extra_data) {
  ((DomainWallBase*)extra_data)->apply_M_schur5_dagger_M(lhs, rhs);
}
// D x = b by CG on the normal equations of the even-odd Schur complement: prepare, M^dagger b', minv_vector_cg over the half length from the
// even half of x as the initial guess, reconstruct.  x and b are full-length; eps is the relative residual of M^dagger M y = M^dagger b'.
// Where the Schur methods cannot run (schur5_ready) nothing is solved, x is untouched, success is false and the name is `not_run`.
inline inversion_info minv_domain_wall_eo_cg(complex<double>* x, complex<double>* b, int max_iter, double eps, DomainWallBase* op, const char* who, const char* not_run,
                                             inversion_verbose_struct* verb) {
  const size_t n = op->lat->get_size_cv_l(), half = n / 2;
  if (!op->schur5_ready(who, true)) {
    inversion_info none;
    none.name = not_run;
    return none;
  }
  complex<double>* b_r = allocate_vector<complex<double>>(n);
  complex<double>* rhs = allocate_vector<complex<double>>(half);
  op->prepare_M_schur5(b_r, b);
  op->apply_M_schur5_dagger(rhs, b_r);
  const inversion_info info = minv_vector_cg(x, rhs, (int)half, max_iter, eps, apply_domain_wall_schur5_Mdagger_M, (void*)op, verb);
  op->reconstruct_M_schur5(x, x, b);
  deallocate_vector(&b_r); deallocate_vector(&rhs);
  return info;
}

// ---------------- Shamir domain wall (operators/dwf.h) ----------------
// The domain-wall height M5 is the stencil's identity shift, the wall mass couples slice Ls-1 to slice 0.  D = A + H with A = clover + shift
// site-local and constant (qmg_dwf_fill / qmg_dwf_apply_direct, csrc/qmg_dwf.hip; qmg_dwf_inv5 / qmg_dwf_hops_inv5 / qmg_dwf_schur_apply,
// csrc/qmg_dwf_eo.hip):
//   M = A_ee - H_eo A_oo^-1 H_oe,   Gamma5 M Gamma5 = M^dagger for real m and shifts (no dagger stencil, the launches and bytes of M).
struct DwfBase : public DomainWallBase {
 protected:
  DwfBase(Lattice2D* in_lat, complex<double> mass, double M5, int Ls) : DomainWallBase(in_lat, M5, mass, M5, Ls) {}

  virtual bool schur5_stages(const char* who, complex<double>* lhs, complex<double>* rhs, bool dagger) {
    const qmg_stencil_desc d = desc();
    return qmg::ok(qmg_dwf_schur_apply(QMG_C64, &d, direct.gauge, dw_Ls, mass.real(), mass.imag(), direct.w, lhs, rhs, eo_cvector, 0,
                                       dagger ? QMG_DWF_G5_IN | QMG_DWF_G5_OUT : 0u, 1, 0, 1u, qmg::current_stream()), who);
  }

 public:
  virtual bool schur5_ready(const char* who, bool dagger = false) {
    if (!links_route(QMG_DIRECT_DWF)) {
      std::cout << "[QMG-ERROR]: " << who << " needs the domain-wall links route (direct.on, no variant swapped in); there is no stored fallback.\n";
      return false;
    }
    if (dagger && (mass.imag() != 0.0 || shift.imag() != 0.0 || eo_shift.imag() != 0.0)) {
      std::cout << "[QMG-ERROR]: " << who << " uses Gamma5 M Gamma5 = M^dagger, which holds for a real wall mass and real shifts only.\n";
      return false;
    }
    return schur5_scratch();
  }
  // b_r,e = b_e - H_eo A_oo^-1 b_o
  virtual void prepare_M_schur5(complex<double>* b_r, complex<double>* b) {
    if (!schur5_ready("prepare_M_schur5")) return;
    const qmg_stencil_desc d = desc();
    const long half = lat->get_size_cv_l() / 2;
    qmg::ok(qmg_dwf_inv5(QMG_C64, &d, dw_Ls, mass.real(), mass.imag(), direct.w, eo_cvector, b, QMG_P_CLOVER_O, 1.0, 0.0, 1, 0, 1u, qmg::current_stream()), "qmg_dwf_inv5");
    qmg::ok(qmg_dwf_apply_direct(QMG_C64, &d, direct.gauge, dw_Ls, mass.real(), mass.imag(), direct.w, b_r, eo_cvector, QMG_P_EO | QMG_P_ZERO_E, 1, 0, 1u,
                                 qmg::current_stream()), "qmg_dwf_apply_direct");
    cxpay(b, -1.0, b_r, half);
    zero_vector(b_r + half, half);
  }
  // x_o = A_oo^-1 (b_o - H_oe y_e)
  virtual void reconstruct_M_schur5(complex<double>* x, complex<double>* y_e, complex<double>* b) {
    if (!schur5_ready("reconstruct_M_schur5")) return;
    const qmg_stencil_desc d = desc();
    const long half = lat->get_size_cv_l() / 2;
    if (x != y_e) copy_vector(x, y_e, half);
    qmg::ok(qmg_dwf_inv5(QMG_C64, &d, dw_Ls, mass.real(), mass.imag(), direct.w, x, b, QMG_P_CLOVER_O, 1.0, 0.0, 1, 0, 1u, qmg::current_stream()), "qmg_dwf_inv5");
    qmg::ok(qmg_dwf_hops_inv5(QMG_C64, &d, direct.gauge, dw_Ls, mass.real(), mass.imag(), direct.w, x, x, QMG_P_OE, -1.0, 0.0, 0, 1, 0, 1u, qmg::current_stream()),
            "qmg_dwf_hops_inv5");
  }
};

template <int Ls>
struct Dwf2D : public DwfBase {
 protected:
  Dwf2D(Dwf2D const&);
  Dwf2D& operator=(Dwf2D const&);

 public:
  void update_links(complex<double>* gauge_links) {   // dwf.h:154-255; gauge_links: DEVICE nc=1 LatticeGauge
    qmg::ok(qmg_dwf_fill(clover, hopping, gauge_links, lat->get_dim_mu(0), lat->get_dim_mu(1), Ls, mass.real(), mass.imag(), 1.0, qmg::current_stream()), "qmg_dwf_fill");
    drop_variant_stencils();
    set_direct_links(gauge_links, 1.0, QMG_DIRECT_DWF, Ls, mass);   // the ORIGINAL-operator applies go straight from the links
    generated = true;
  }

  Dwf2D(Lattice2D* in_lat, complex<double> mass, complex<double>* gauge_links, double M5 = -1.0) : DwfBase(in_lat, mass, M5, Ls) {
    if (served("Dwf2D")) update_links(gauge_links);
  }

  static int get_dof(int i = 0) { return 2 * Ls; }
  static chirality_state has_chirality() { return QMG_CHIRAL_YES; }
};

// A domain-wall operator of run-time Ls (dwf.h:261-293): the reference's list of Ls values, of which those are served whose nc = 2 Ls the
// stored-stencil apply serves (the variants and every piece set the links kernel declines go through it): qmg_stencil_plan is asked.
inline Stencil2D* createDwfLs(Lattice2D* in_lat, complex<double> mass, complex<double>* gauge_links, int Ls, double M5 = -1.0) {
  int plan[12];
#define QMG_DW_LS_IS(N) || Ls == N
  const bool listed = false QMG_DW_LS_LIST(QMG_DW_LS_IS);
#undef QMG_DW_LS_IS
  const bool stored = listed && qmg_stencil_plan(QMG_SE_APPLY, 0, 0, in_lat->get_dim_mu(0), in_lat->get_dim_mu(1), 2 * Ls, QMG_P_ALL | QMG_P_ZERO, 1, 0, 0, 1, 1, 0, 0,
                                                 plan, 12) == QMG_SUCCESS && plan[0] != 0 && plan[0] != 9;
  if (stored) {   // (Ls = 32, nc = 64: not served by the stored-stencil apply today)
    switch (Ls) {
#define QMG_DW_LS_CASE(N) case N: return new Dwf2D<N>(in_lat, mass, gauge_links, M5);
      QMG_DW_LS_LIST(QMG_DW_LS_CASE)
#undef QMG_DW_LS_CASE
      default: break;
    }
  }
  std::cout << "[QMG-ERROR]: Unsupported Ls " << Ls << " for domain wall operator. Add a template to dwf.h.\n";
  return nullptr;
}

// The Schur complement with the matrix_op_cplx signature (extra_data: a DwfBase*), for the Krylov solvers on the even half.
inline void apply_dwf_schur5_M(complex<double>* lhs, complex<double>* rhs, void* extra_data) { ((DwfBase*)extra_data)->apply_M_schur5(lhs, rhs); }
inline void apply_dwf_schur5_Mdagger_M(complex<double>* lhs, complex<double>* rhs, void* extra_data) { ((DwfBase*)extra_data)->apply_M_schur5_dagger_M(lhs, rhs); }

// minv_domain_wall_eo_cg on the Shamir operator
inline inversion_info minv_dwf_eo_cg(complex<double>* x, complex<double>* b, int max_iter, double eps, DwfBase* dwf, inversion_verbose_struct* verb = 0) {
  return minv_domain_wall_eo_cg(x, b, max_iter, eps, dwf, "minv_dwf_eo_cg", "CG (even-odd domain wall): not run", verb);
}

// ---------------- Moebius domain wall (nc = 2 Ls, the layout of Dwf2D; not in the reference) ----------------
// D = D_W (b5 + c5 L) + (1 - L) = A + H B with D_W = 2 w + M5 + H (include/qmg_hip.h has L, A, B); b5 = 1, c5 = 0 is Dwf2D with shift = M5.  M5 sits
// inside D_W and is multiplied by B, so it is a parameter of the operator and the stencil's three shifts are zero.  In the stored arrays
// (qmg_mobius_fill) the hopping blocks are no longer diagonal in s; apply_M and apply_M_dagger on the whole lattice go straight from the links
// (qmg_mobius_apply_direct, op 0 / op 1, csrc/qmg_mobius.hip).  Gamma5 D Gamma5 is NOT D^dagger here (B and H do not commute): the dagger is the
// entry's op 1, and it needs no stored dagger stencil while the links route is on.  The Schur complement (qmg_mobius_inv5 /
// qmg_mobius_hops_inv5 / qmg_mobius_schur_apply, csrc/qmg_mobius_eo.hip):
//   M = A_e - H_eo B A_o^-1 H_oe B,   M^dagger = Gamma5 [A'_e - B' H_eo A'_o^-1 B' H_oe] Gamma5   (the entry's op 1)
// serves any complex wall mass and shifts: the dagger has kernels of its own.
struct MobiusBase : public DomainWallBase {
 protected:
  double b5, c5;
  MobiusBase(Lattice2D* in_lat, complex<double> mass, double M5, double b5, double c5, int Ls) : DomainWallBase(in_lat, 0, mass, M5, Ls), b5(b5), c5(c5) {}

  virtual bool schur5_stages(const char* who, complex<double>* lhs, complex<double>* rhs, bool dagger) {
    const qmg_stencil_desc d = desc();
    return qmg::ok(qmg_mobius_schur_apply(QMG_C64, &d, direct.gauge, dw_Ls, mass.real(), mass.imag(), direct.w, M5, b5, c5, lhs, rhs, eo_cvector, 0, dagger ? 1 : 0, 1, 0,
                                          1u, qmg::current_stream()), who);
  }

 public:
  double get_b5() const { return b5; }
  double get_c5() const { return c5; }
  // whether both applies come from the links (the normal-equation solve below works on that: no stored fallback at Ls = 32)
  bool links_ready() const { return links_route(QMG_DIRECT_MOBIUS); }
  // lhs = D^dagger D rhs, both applies from the links; extra_cvector holds D rhs
  void apply_M_dagger_M_links(complex<double>* lhs, complex<double>* rhs) {
    apply_M_overwrite(extra_cvector, rhs);
    zero_vector(lhs, lat->get_size_cv_l());
    apply_M_dagger(lhs, extra_cvector);
  }

  virtual bool schur5_ready(const char* who, bool dagger = false) {
    if (!links_ready()) {
      std::cout << "[QMG-ERROR]: " << who << " needs the Moebius links route (direct.on, no variant swapped in); there is no stored fallback.\n";
      return false;
    }
    return schur5_scratch();
  }
  // b_r,e = b_e - H_eo B A_o^-1 b_o
  virtual void prepare_M_schur5(complex<double>* b_r, complex<double>* b) {
    if (!schur5_ready("prepare_M_schur5")) return;
    const qmg_stencil_desc d = desc();
    const long half = lat->get_size_cv_l() / 2;
    const double mr = mass.real(), mi = mass.imag();
    qmg::ok(qmg_mobius_inv5(QMG_C64, &d, dw_Ls, mr, mi, direct.w, M5, b5, c5, eo_cvector, b, QMG_P_CLOVER_O, QMG_MOBIUS_S_AINV, 1.0, 0.0, 1, 0, 1u,
                            qmg::current_stream()), "qmg_mobius_inv5");
    copy_vector(b_r, b, half);
    qmg::ok(qmg_mobius_hops_inv5(QMG_C64, &d, direct.gauge, dw_Ls, mr, mi, direct.w, M5, b5, c5, b_r, eo_cvector, QMG_P_EO, QMG_MOBIUS_S_ONE, QMG_MOBIUS_R_B,
                                 -1.0, 0.0, 0, 1, 0, 1u, qmg::current_stream()), "qmg_mobius_hops_inv5");
    zero_vector(b_r + half, half);
  }
  // x_o = A_o^-1 (b_o - H_oe B y_e)
  virtual void reconstruct_M_schur5(complex<double>* x, complex<double>* y_e, complex<double>* b) {
    if (!schur5_ready("reconstruct_M_schur5")) return;
    const qmg_stencil_desc d = desc();
    const long half = lat->get_size_cv_l() / 2;
    const double mr = mass.real(), mi = mass.imag();
    if (x != y_e) copy_vector(x, y_e, half);
    qmg::ok(qmg_mobius_inv5(QMG_C64, &d, dw_Ls, mr, mi, direct.w, M5, b5, c5, x, b, QMG_P_CLOVER_O, QMG_MOBIUS_S_AINV, 1.0, 0.0, 1, 0, 1u,
                            qmg::current_stream()), "qmg_mobius_inv5");
    qmg::ok(qmg_mobius_hops_inv5(QMG_C64, &d, direct.gauge, dw_Ls, mr, mi, direct.w, M5, b5, c5, x, x, QMG_P_OE, QMG_MOBIUS_S_AINV, QMG_MOBIUS_R_B, -1.0, 0.0,
                                 0, 1, 0, 1u, qmg::current_stream()), "qmg_mobius_hops_inv5");
  }
};

template <int Ls>
struct Mobius2D : public MobiusBase {
 protected:
  Mobius2D(Mobius2D const&);
  Mobius2D& operator=(Mobius2D const&);

 public:
  void update_links(complex<double>* gauge_links) {   // gauge_links: DEVICE nc=1 LatticeGauge
    qmg::ok(qmg_mobius_fill(clover, hopping, gauge_links, lat->get_dim_mu(0), lat->get_dim_mu(1), Ls, mass.real(), mass.imag(), 1.0, M5, b5, c5, qmg::current_stream()),
            "qmg_mobius_fill");
    drop_variant_stencils();
    set_direct_links(gauge_links, 1.0, QMG_DIRECT_MOBIUS, Ls, mass, M5, b5, c5);   // apply_M and apply_M_dagger go straight from the links
    generated = true;
  }

  Mobius2D(Lattice2D* in_lat, complex<double> mass, complex<double>* gauge_links, double b5, double c5, double M5 = -1.0)
      : MobiusBase(in_lat, mass, M5, b5, c5, Ls) {
    if (served("Mobius2D")) update_links(gauge_links);
  }

  static int get_dof(int i = 0) { return 2 * Ls; }
  static chirality_state has_chirality() { return QMG_CHIRAL_YES; }
};

// A Moebius operator of run-time Ls: createDwfLs's list of Ls values.  Where the stored-stencil apply does not serve nc = 2 Ls (Ls = 32 today)
// the operator is made all the same: both applies and the solves below come from the links, and only what needs the stored arrays is missing.
inline MobiusBase* createMobiusLs(Lattice2D* in_lat, complex<double> mass, complex<double>* gauge_links, int Ls, double b5, double c5, double M5 = -1.0) {
  switch (Ls) {
#define QMG_DW_LS_CASE(N) case N: return new Mobius2D<N>(in_lat, mass, gauge_links, b5, c5, M5);
    QMG_DW_LS_LIST(QMG_DW_LS_CASE)
#undef QMG_DW_LS_CASE
    default: break;
  }
  std::cout << "[QMG-ERROR]: Unsupported Ls " << Ls << " for the Moebius domain wall operator.\n";
  return nullptr;
}

inline void apply_mobius_Mdagger_M(complex<double>* lhs, complex<double>* rhs, void* extra_data) { ((MobiusBase*)extra_data)->apply_M_dagger_M_links(lhs, rhs); }

// D x = b by CG on the normal equations: minv_vector_cg on D^dagger D with D^dagger b as the right-hand side, from x as the initial guess; eps is
// the relative residual of D^dagger D x = D^dagger b.  Both applies come from the links, so this works at Ls = 32; where the links route is off
// nothing is solved and success is false.
inline inversion_info minv_mobius_cg(complex<double>* x, complex<double>* b, int max_iter, double eps, MobiusBase* mobius, inversion_verbose_struct* verb = 0) {
  const size_t n = mobius->lat->get_size_cv_l();
  if (!mobius->links_ready()) {
    std::cout << "[QMG-ERROR]: minv_mobius_cg needs the Moebius links route (direct.on, no variant swapped in).\n";
    inversion_info none;
    none.name = "CG (Moebius domain wall): not run";
    return none;
  }
  complex<double>* rhs = allocate_vector<complex<double>>(n);
  zero_vector(rhs, n);
  mobius->apply_M_dagger(rhs, b);
  const inversion_info info = minv_vector_cg(x, rhs, (int)n, max_iter, eps, apply_mobius_Mdagger_M, (void*)mobius, verb);
  deallocate_vector(&rhs);
  return info;
}

// The Schur complement with the matrix_op_cplx signature (extra_data: a MobiusBase*), for the Krylov solvers on the even half.
inline void apply_mobius_schur5_M(complex<double>* lhs, complex<double>* rhs, void* extra_data) { ((MobiusBase*)extra_data)->apply_M_schur5(lhs, rhs); }
inline void apply_mobius_schur5_Mdagger_M(complex<double>* lhs, complex<double>* rhs, void* extra_data) {
  ((MobiusBase*)extra_data)->apply_M_schur5_dagger_M(lhs, rhs);
}

// minv_domain_wall_eo_cg on the Moebius operator (everything comes from the links, so this works at Ls = 32)
inline inversion_info minv_mobius_eo_cg(complex<double>* x, complex<double>* b, int max_iter, double eps, MobiusBase* mobius, inversion_verbose_struct* verb = 0) {
  return minv_domain_wall_eo_cg(x, b, max_iter, eps, mobius, "minv_mobius_eo_cg", "CG (even-odd Moebius domain wall): not run", verb);
}

// ---------------- shared by the two nc = 1 operators: hand-rolled even-odd normal operator ----------------
struct EoPrecNc1 : public Stencil2D {
 protected:
  complex<double>* tmp_eo_space;
  EoPrecNc1(Lattice2D* l, int pieces, complex<double> s) : Stencil2D(l, pieces, s, 0.0, 0.0), tmp_eo_space(0) {}
  ~EoPrecNc1() { if (tmp_eo_space) deallocate_vector(&tmp_eo_space); }
  void drop_variants() {
    if (built_dagger) { if (dagger_clover) deallocate_vector(&dagger_clover); deallocate_vector(&dagger_hopping); built_dagger = false; }
    if (built_rbjacobi) { deallocate_vector(&rbjacobi_cinv); if (rbjacobi_clover) deallocate_vector(&rbjacobi_clover); deallocate_vector(&rbjacobi_hopping); built_rbjacobi = false; }
  }
  // b_new_e = diag b_e - D_eo b_o
  void prepare_b_impl(complex<double>* b_new, complex<double>* b, complex<double> diag) {
    const long half = lat->get_size_cv_l() / 2;
    launch(QMG_P_EO | QMG_P_ZERO_E, b_new, b, 0, hopping, 0.0, 0.0, 0.0);
    caxpby(diag, b, complex<double>(-1.0), b_new, half);
  }
  // lhs_e = diag^2 rhs_e - D_eo D_oe rhs_e
  void apply_eo_prec_impl(complex<double>* lhs, complex<double>* rhs, complex<double> diag) {
    const long cv = lat->get_size_cv_l();
    if (!tmp_eo_space) tmp_eo_space = allocate_vector<complex<double>>(cv);
    launch(QMG_P_OE | QMG_P_ZERO_O, tmp_eo_space, rhs, 0, hopping, 0.0, 0.0, 0.0);
    launch(QMG_P_EO | QMG_P_ZERO_E, tmp_eo_space, tmp_eo_space, 0, hopping, 0.0, 0.0, 0.0);
    caxpbyz(diag * diag, rhs, complex<double>(-1.0), tmp_eo_space, lhs, cv / 2);
  }
  // x_o = (b_o - D_oe x_e) / diag
  void reconstruct_x_impl(complex<double>* x, complex<double>* b, complex<double> diag) {
    const long half = lat->get_size_cv_l() / 2;
    launch(QMG_P_OE | QMG_P_ZERO_O, x, x, 0, hopping, 0.0, 0.0, 0.0);
    caxpby(1.0 / diag, b + half, -1.0 / diag, x + half, half);
  }
};

// ---------------- Staggered (staggered.h) ----------------
struct Staggered2D : public EoPrecNc1 {
  void update_links(complex<double>* gauge_links) {   // :81-123
    if (qmg::slab().on)   // y-slab mode: gauge_links is the gauge field of the WHOLE lattice, this rank fills its rows
      qmg::ok(qmg_staggered_fill_slab(hopping, gauge_links, lat->get_dim_mu(0), lat->get_dim_mu(1) * qmg::slab().world, qmg::slab().rank * lat->get_dim_mu(1),
                                      lat->get_dim_mu(1), qmg::current_stream()), "qmg_staggered_fill_slab");
    else
    qmg::ok(qmg_staggered_fill(hopping, gauge_links, lat->get_dim_mu(0), lat->get_dim_mu(1), qmg::current_stream()), "qmg_staggered_fill");
    drop_variants();
    generated = true;
  }
  Staggered2D(Lattice2D* in_lat, complex<double> mass, complex<double>* gauge_links) : EoPrecNc1(in_lat, QMG_PIECE_HOPPING, mass) {
    if (lat->get_nc() != 1) { std::cout << "[QMG-ERROR]: Staggered2D only supports Nc = 1.\n"; return; }
    update_links(gauge_links);
  }
  static int get_dof(int i = 0) { return 1; }
  static chirality_state has_chirality() { return QMG_CHIRAL_YES; }
  virtual void gamma5(complex<double>* vec) { const long h = lat->get_size_cv_l() / 2; cax(-1.0, vec + h, h); }                      // :140-143
  virtual void gamma5(complex<double>* g5_vec, complex<double>* vec) { const long h = lat->get_size_cv_l() / 2; copy_vector(g5_vec, vec, h); caxy(-1.0, vec + h, g5_vec + h, h); }
  virtual void chiral_projection(complex<double>* v, bool is_up) { const long h = lat->get_size_cv_l() / 2; zero_vector(is_up ? v + h : v, h); }   // :152-158
  virtual void chiral_projection_copy(complex<double>* orig, complex<double>* dest, bool is_up) {
    const long h = lat->get_size_cv_l() / 2;
    if (is_up) { zero_vector(dest + h, h); copy_vector(dest, orig, h); } else { zero_vector(dest, h); copy_vector(dest + h, orig + h, h); }
  }
  virtual void chiral_projection_both(complex<double>* orig_to_up, complex<double>* down) {
    const long h = lat->get_size_cv_l() / 2;
    zero_vector(down, h); copy_vector(down + h, orig_to_up + h, h); zero_vector(orig_to_up + h, h);
  }
  virtual QMGDefaultChirality get_default_chirality() { return QMG_CHIRALITY_GAMMA_5; }
  void prepare_b(complex<double>* b_new, complex<double>* b) { prepare_b_impl(b_new, b, shift); }                 // :190-202
  void apply_eo_prec_M(complex<double>* lhs, complex<double>* rhs) { apply_eo_prec_impl(lhs, rhs, shift); }       // m^2 - D_eo D_oe (:206-224)
  void reconstruct_x(complex<double>* x, complex<double>* b) { reconstruct_x_impl(x, b, shift); }                 // :228-240

  // Every mass of a scan at once (not in the reference, whose drivers solve mass by mass): xs[i] = D(masses[i])^-1 b on the full lattice,
  // b general (both parities).  With H = D(0), the anti-Hermitian hopping part, D(m)^-1 = (m - H) (m^2 - H^2)^-1 and -H^2 is Hermitian
  // positive semi-definite and independent of the mass (block diagonal in parity: -D_eo D_oe on the even sites, -D_oe D_eo on the odd
  // ones, the operator of apply_eo_prec_M for both parities).  So ONE multi-shift CG (minv_vector_cg_m) on A = -H^2 with the shifts
  // m_i^2 gives every y_i = (m_i^2 - H^2)^-1 b for the operator applies of the lightest mass, and x_i = m_i y_i - H y_i costs one
  // more hopping apply per mass.  Real masses > 0; xs[i] distinct device vectors, overwritten.  The object's shift, its built
  // variants and every other method are untouched.  Returns one inversion_info per mass (iter: when that mass froze).
  std::vector<inversion_info> solve_masses(complex<double>** xs, complex<double>* b, const double* masses, int n_mass, int max_iter, double eps,
                                           inversion_verbose_struct* verb = 0) {
    if (qmg::slab().on) { std::cout << "[QMG-ERROR]: Staggered2D::solve_masses does not run on y-slabs.\n"; return std::vector<inversion_info>((size_t)(n_mass > 0 ? n_mass : 0)); }
    const long cv = lat->get_size_cv_l();
    std::vector<double> sigma((size_t)(n_mass > 0 ? n_mass : 0));
    for (int i = 0; i < n_mass; i++) { sigma[i] = masses[i] * masses[i]; zero_vector(xs[i], cv); }
    std::vector<inversion_info> inv = minv_vector_cg_m(xs, b, n_mass, (int)cv, 1, max_iter, eps, sigma.data(), apply_minus_hop_sq, (void*)this, false, verb);
    for (int i = 0; i < n_mass && i < (int)inv.size(); i++) {
      if (!tmp_eo_space) tmp_eo_space = allocate_vector<complex<double>>(cv);
      launch(QMG_P_HOPPING | QMG_P_ZERO, tmp_eo_space, xs[i], 0, hopping, 0.0, 0.0, 0.0);
      caxpby(-1.0, tmp_eo_space, masses[i], xs[i], cv);
    }
    return inv;
  }
  // H = D(0), the hopping part alone, for the staggered molecular dynamics (hmc_staggered.hpp):
  void apply_hopping(complex<double>* lhs, complex<double>* rhs) { launch(QMG_P_HOPPING | QMG_P_ZERO, lhs, rhs, 0, hopping, 0.0, 0.0, 0.0); }   // lhs = H rhs, lhs != rhs
  void hop_even_to_odd(complex<double>* w) { launch(QMG_P_OE | QMG_P_ZERO_O, w, w, 0, hopping, 0.0, 0.0, 0.0); }   // w_o = (H w_e)_o in place, w_e kept
  static void apply_minus_hop_sq(complex<double>* lhs, complex<double>* rhs, void* self) {   // lhs = -H^2 rhs
    Staggered2D* st = (Staggered2D*)self;
    const long cv = st->lat->get_size_cv_l();
    if (!st->tmp_eo_space) st->tmp_eo_space = allocate_vector<complex<double>>(cv);
    st->launch(QMG_P_HOPPING | QMG_P_ZERO, st->tmp_eo_space, rhs, 0, st->hopping, 0.0, 0.0, 0.0);
    st->launch(QMG_P_HOPPING | QMG_P_ZERO, lhs, st->tmp_eo_space, 0, st->hopping, 0.0, 0.0, 0.0);
    cax(-1.0, lhs, cv);
  }
};
inline void apply_eo_staggered_2D_M(complex<double>* lhs, complex<double>* rhs, void* extra_data) { ((Staggered2D*)extra_data)->apply_eo_prec_M(lhs, rhs); }

// ---------------- Gauged Laplace (gaugedlaplace.h) ----------------
struct GaugedLaplace2D : public EoPrecNc1 {
  void update_links(complex<double>* gauge_links) {   // :77-115
    if (qmg::slab().on)   // y-slab mode: gauge_links is the gauge field of the WHOLE lattice
      qmg::ok(qmg_laplace_fill_slab(clover, hopping, gauge_links, lat->get_dim_mu(0), lat->get_dim_mu(1) * qmg::slab().world, qmg::slab().rank * lat->get_dim_mu(1),
                                    lat->get_dim_mu(1), qmg::current_stream()), "qmg_laplace_fill_slab");
    else
    qmg::ok(qmg_laplace_fill(clover, hopping, gauge_links, lat->get_dim_mu(0), lat->get_dim_mu(1), qmg::current_stream()), "qmg_laplace_fill");
    drop_variants();
    generated = true;
  }
  GaugedLaplace2D(Lattice2D* in_lat, complex<double> mass_sq, complex<double>* gauge_links) : EoPrecNc1(in_lat, QMG_PIECE_CLOVER_HOPPING, mass_sq) {
    if (lat->get_nc() != 1) { std::cout << "[QMG-ERROR]: GaugedLaplace2D only supports Nc = 1.\n"; return; }
    update_links(gauge_links);
  }
  static int get_dof(int i = 0) { return 1; }
  static chirality_state has_chirality() { return QMG_CHIRAL_NO; }
  virtual void chiral_projection(complex<double>*, bool) { return; }
  virtual void chiral_projection_copy(complex<double>*, complex<double>*, bool) { return; }
  virtual void chiral_projection_both(complex<double>*, complex<double>*) { return; }
  virtual QMGDefaultChirality get_default_chirality() { return QMG_CHIRALITY_NONE; }
  void prepare_b(complex<double>* b_new, complex<double>* b) { prepare_b_impl(b_new, b, 4.0 + shift); }             // :154-166
  void apply_eo_prec_M(complex<double>* lhs, complex<double>* rhs) { apply_eo_prec_impl(lhs, rhs, 4.0 + shift); }   // :170-188
  void reconstruct_x(complex<double>* x, complex<double>* b) { reconstruct_x_impl(x, b, 4.0 + shift); }             // :192-204

  // Every m^2 of a scan at once: xs[i] = (Laplace + mass_sqs[i])^-1 b from ONE multi-shift CG (minv_vector_cg_m).  The operator at m^2 = 0
  // is Hermitian positive (semi-)definite and m^2 is a multiple of the identity, so nothing is reconstructed.  mass_sqs[i] > 0, real.
  // The object's shift, its built variants and every other method are untouched.
  std::vector<inversion_info> solve_masses(complex<double>** xs, complex<double>* b, const double* mass_sqs, int n_mass, int max_iter, double eps,
                                           inversion_verbose_struct* verb = 0) {
    if (qmg::slab().on) { std::cout << "[QMG-ERROR]: GaugedLaplace2D::solve_masses does not run on y-slabs.\n"; return std::vector<inversion_info>((size_t)(n_mass > 0 ? n_mass : 0)); }
    const long cv = lat->get_size_cv_l();
    std::vector<double> sigma(mass_sqs, mass_sqs + (n_mass > 0 ? n_mass : 0));
    for (int i = 0; i < n_mass; i++) zero_vector(xs[i], cv);
    return minv_vector_cg_m(xs, b, n_mass, (int)cv, 1, max_iter, eps, sigma.data(), apply_massless, (void*)this, false, verb);
  }
  static void apply_massless(complex<double>* lhs, complex<double>* rhs, void* self) {   // lhs = (4 + hopping) rhs: the operator at m^2 = 0
    GaugedLaplace2D* gl = (GaugedLaplace2D*)self;
    gl->launch(QMG_P_CLOVER | QMG_P_HOPPING | QMG_P_ZERO, lhs, rhs, gl->clover, gl->hopping, 0.0, 0.0, 0.0);
  }
};
inline void apply_eo_gauge_laplace_2D_M(complex<double>* lhs, complex<double>* rhs, void* extra_data) { ((GaugedLaplace2D*)extra_data)->apply_eo_prec_M(lhs, rhs); }

// ---------------- Free Laplace (tests/n02_free_laplace_test/free_laplace.h:18-42) ----------------
struct FreeLaplace2D : public Stencil2D {
  FreeLaplace2D(Lattice2D* in_lat, complex<double> mass_sq) : Stencil2D(in_lat, QMG_PIECE_CLOVER_HOPPING, mass_sq, 0.0, 0.0) {
    if (lat->get_nc() != 1) { std::cout << "[QMG-ERROR]: FreeLaplace2D only supports Nc = 1.\n"; return; }
    // 4 on the clover, -1 on the hopping: fill = constant -> zero then shift-by-constant via caxy on a ones vector is overkill; upload.
    std::vector<complex<double>> c((size_t)lat->get_size_cm_l(), 4.0), h((size_t)lat->get_size_hopping_l(), -1.0);
    qmg::upload(clover, c.data(), c.size());
    qmg::upload(hopping, h.data(), h.size());
    generated = true;
  }
  virtual void chiral_projection(complex<double>*, bool) { return; }
  virtual void chiral_projection_copy(complex<double>*, complex<double>*, bool) { return; }
  virtual void chiral_projection_both(complex<double>*, complex<double>*) { return; }
  virtual QMGDefaultChirality get_default_chirality() { return QMG_CHIRALITY_NONE; }
};

#endif
