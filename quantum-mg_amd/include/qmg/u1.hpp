// u1.hpp -- U(1) gauge utilities on device fields (reference: u1/u1_utils.h): text I/O in the reference's format
// (read_gauge_u1 :38-67, write_gauge_u1 :105-168), unit field (:172-181), polar_vector, non-compact heatbath (:607-757; here
// a four-colour parallel heatbath on the device, csrc/qmg_u1.hip), plaquette / topology / non-compact action (:386-508).
// Field preparation on the device as well: hot and Gaussian starts and random gauge transforms (:183-237), apply_gauge_trans_u1
// (:241-272), APE smearing (:276-383) and the two instantons (:545-603); read_phase_u1 (:70-102) is host text I/O like read_gauge_u1.
// lorentz_gauge_fix_u1 (:511-542) is an unfinished stub in the reference (its loop never ends) and has no counterpart.
// `gauge_field` is a DEVICE nc=1 LatticeGauge (mu, eo, y, x) of complex links; `phases` a DEVICE double field in the same order.
#ifndef QMG_U1_HPP
#define QMG_U1_HPP

#include <cstdio>
#include <string>
#include <vector>

#include "lattice2d.hpp"
#include "qmg_device.hpp"

// One phase per line; loop order x outer, y, mu inner (u1_utils.h:53-63).
inline bool read_gauge_u1(complex<double>* gauge_field, Lattice2D* lat, std::string input_file) {
  if (lat->get_nc() != 1) { std::cout << "[QMG-ERROR]: U1 gauge functions require Nc = 1 lattice.\n"; return false; }
  const int x_len = lat->get_dim_mu(0), y_len = lat->get_dim_mu(1);
  std::FILE* f = std::fopen(input_file.c_str(), "r");
  if (!f) { std::cout << "[QMG-ERROR]: cannot open gauge file " << input_file << "\n"; return false; }
  std::vector<complex<double>> host((size_t)lat->get_size_gauge());
  bool good = true;
  for (int x = 0; x < x_len && good; x++)
    for (int y = 0; y < y_len && good; y++)
      for (int mu = 0; mu < 2; mu++) {
        double phase;
        if (std::fscanf(f, "%lf", &phase) != 1) { good = false; break; }
        host[lat->gauge_coord_to_index(x, y, 0, 0, mu)] = std::polar(1.0, phase);
      }
  std::fclose(f);
  if (!good) { std::cout << "[QMG-ERROR]: gauge file " << input_file << " is too short for this lattice.\n"; return false; }
  qmg::upload(gauge_field, host.data(), host.size());
  return true;
}

// Periodic tiling of a small (t_len x t_len) configuration file onto a larger lattice: the same U(1)
// config as an L x L field (valid because the configuration is periodic).  Not in the reference; used by the
// benchmark drivers to reach 2048^2 / 4096^2 from the committed 64^2 fixture.
inline bool read_gauge_u1_tiled(complex<double>* gauge_field, Lattice2D* lat, std::string input_file, int t_len) {
  if (lat->get_nc() != 1) { std::cout << "[QMG-ERROR]: U1 gauge functions require Nc = 1 lattice.\n"; return false; }
  const int x_len = lat->get_dim_mu(0), y_len = lat->get_dim_mu(1);
  if (x_len % t_len || y_len % t_len) { std::cout << "[QMG-ERROR]: lattice is not a multiple of the tile.\n"; return false; }
  std::FILE* f = std::fopen(input_file.c_str(), "r");
  if (!f) { std::cout << "[QMG-ERROR]: cannot open gauge file " << input_file << "\n"; return false; }
  std::vector<double> ph((size_t)2 * t_len * t_len);
  for (size_t k = 0; k < ph.size(); k++)
    if (std::fscanf(f, "%lf", &ph[k]) != 1) { std::fclose(f); std::cout << "[QMG-ERROR]: gauge file too short.\n"; return false; }
  std::fclose(f);
  std::vector<complex<double>> host((size_t)lat->get_size_gauge());
  for (int x = 0; x < x_len; x++)
    for (int y = 0; y < y_len; y++)
      for (int mu = 0; mu < 2; mu++)
        host[lat->gauge_coord_to_index(x, y, 0, 0, mu)] = std::polar(1.0, ph[((size_t)(x % t_len) * t_len + (y % t_len)) * 2 + mu]);
  qmg::upload(gauge_field, host.data(), host.size());
  return true;
}

inline void unit_gauge_u1(complex<double>* gauge_field, Lattice2D* lat) {   // u1_utils.h:172-181
  if (lat->get_nc() != 1) { std::cout << "[QMG-ERROR]: U1 gauge functions require Nc = 1 lattice.\n"; return; }
  std::vector<complex<double>> host((size_t)lat->get_size_gauge(), complex<double>(1.0, 0.0));
  qmg::upload(gauge_field, host.data(), host.size());
}


// write_gauge_u1 (u1_utils.h:105-135): one phase arg(U) per line, fixed notation with 20 digits, loop order x outer, y, mu inner
inline void write_gauge_u1(complex<double>* gauge_field, Lattice2D* lat, std::string output_file) {
  if (lat->get_nc() != 1) { std::cout << "[QMG-ERROR]: U1 gauge functions require Nc = 1 lattice.\n"; return; }
  const int x_len = lat->get_dim_mu(0), y_len = lat->get_dim_mu(1);
  std::vector<complex<double>> host = qmg::to_host(gauge_field, (size_t)lat->get_size_gauge());
  std::FILE* f = std::fopen(output_file.c_str(), "w");
  if (!f) { std::cout << "[QMG-ERROR]: cannot open " << output_file << " for writing\n"; return; }
  for (int x = 0; x < x_len; x++)
    for (int y = 0; y < y_len; y++)
      for (int mu = 0; mu < 2; mu++) std::fprintf(f, "%.20f\n", std::arg(host[lat->gauge_coord_to_index(x, y, 0, 0, mu)]));
  std::fclose(f);
}
// the phase-field overload (:138-168): the non-compact phases themselves, not reduced to (-pi, pi]
inline void write_gauge_u1(double* phase_field, Lattice2D* lat, std::string output_file) {
  if (lat->get_nc() != 1) { std::cout << "[QMG-ERROR]: U1 gauge functions require Nc = 1 lattice.\n"; return; }
  const int x_len = lat->get_dim_mu(0), y_len = lat->get_dim_mu(1);
  std::vector<double> host = qmg::to_host(phase_field, (size_t)lat->get_size_gauge());
  std::FILE* f = std::fopen(output_file.c_str(), "w");
  if (!f) { std::cout << "[QMG-ERROR]: cannot open " << output_file << " for writing\n"; return; }
  for (int x = 0; x < x_len; x++)
    for (int y = 0; y < y_len; y++)
      for (int mu = 0; mu < 2; mu++) std::fprintf(f, "%.20f\n", host[lat->gauge_coord_to_index(x, y, 0, 0, mu)]);
  std::fclose(f);
}

// polar_vector(phases, gauge_field, n): U = exp(i A)
inline void polar_vector(double* phases, complex<double>* gauge_field, size_t n) { qmg::ok(qmg_u1_phase_to_gauge(gauge_field, phases, n, qmg::current_stream()), "qmg_u1_phase_to_gauge"); }

// Non-compact heatbath (u1_utils.h:607-757).  The reference threads a std::mt19937 through; here the generator state is a
// (seed, sweeps done) pair so that successive calls continue one stream (and a count of the random fields drawn, see rand_gauge_u1).
struct HeatbathRng { unsigned long long seed, sweeps_done, fields_drawn; explicit HeatbathRng(unsigned long long s = 1337ull) : seed(s), sweeps_done(0), fields_drawn(0) {} };
inline void heatbath_noncompact_update(double* phase_field, Lattice2D* lat, double beta, int n_update, HeatbathRng& generator) {
  if (lat->get_nc() != 1) { std::cout << "[QMG-ERROR]: U1 gauge functions require Nc = 1 lattice.\n"; return; }
  qmg::ok(qmg_u1_heatbath_noncompact(phase_field, lat->get_dim_mu(0), lat->get_dim_mu(1), beta, n_update, generator.seed, generator.sweeps_done, qmg::current_stream()),
          "qmg_u1_heatbath_noncompact");
  generator.sweeps_done += (unsigned long long)n_update;
}

// Just the phases, not compactified (u1_utils.h:70-99): `phase_field` a DEVICE double field, same file order as read_gauge_u1
inline bool read_phase_u1(double* phase_field, Lattice2D* lat, std::string input_file) {
  if (lat->get_nc() != 1) { std::cout << "[QMG-ERROR]: U1 gauge functions require Nc = 1 lattice.\n"; return false; }
  const int x_len = lat->get_dim_mu(0), y_len = lat->get_dim_mu(1);
  std::FILE* f = std::fopen(input_file.c_str(), "r");
  if (!f) { std::cout << "[QMG-ERROR]: cannot open gauge file " << input_file << "\n"; return false; }
  std::vector<double> host((size_t)lat->get_size_gauge());
  bool good = true;
  for (int x = 0; x < x_len && good; x++)
    for (int y = 0; y < y_len && good; y++)
      for (int mu = 0; mu < 2; mu++)
        if (std::fscanf(f, "%lf", &host[lat->gauge_coord_to_index(x, y, 0, 0, mu)]) != 1) { good = false; break; }
  std::fclose(f);
  if (!good) { std::cout << "[QMG-ERROR]: gauge file " << input_file << " is too short for this lattice.\n"; return false; }
  qmg::upload(phase_field, host.data(), host.size());
  return true;
}

// Random fields (u1_utils.h:183-237).  Where the reference threads a std::mt19937 through, the HeatbathRng stands in: every call
// draws its field from a seed derived from (seed, calls made) and counts itself, so consecutive calls give different fields and a
// program that makes the same calls in the same order gets the same fields.  The distributions are the reference's, the streams not.
inline unsigned long long u1_next_field_seed(HeatbathRng& generator) {
  return generator.seed * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull * (++generator.fields_drawn);
}
inline void rand_gauge_u1(complex<double>* gauge_field, Lattice2D* lat, HeatbathRng& generator) {   // :185-195
  if (lat->get_nc() != 1) { std::cout << "[QMG-ERROR]: U1 gauge functions require Nc = 1 lattice.\n"; return; }
  qmg::ok(qmg_u1_hot_gauge(gauge_field, lat->get_dim_mu(0), lat->get_dim_mu(1), u1_next_field_seed(generator), qmg::current_stream()), "qmg_u1_hot_gauge");
}
inline void gauss_gauge_u1(complex<double>* gauge_field, Lattice2D* lat, HeatbathRng& generator, double beta) {   // :200-223
  if (lat->get_nc() != 1) { std::cout << "[QMG-ERROR]: U1 gauge functions require Nc = 1 lattice.\n"; return; }
  qmg::ok(qmg_u1_gauss_gauge(gauge_field, lat->get_dim_mu(0), lat->get_dim_mu(1), beta, u1_next_field_seed(generator), qmg::current_stream()), "qmg_u1_gauss_gauge");
}
inline void rand_trans_u1(complex<double>* gauge_trans, Lattice2D* lat, HeatbathRng& generator) {   // :227-237
  if (lat->get_nc() != 1) { std::cout << "[QMG-ERROR]: U1 gauge functions require Nc = 1 lattice.\n"; return; }
  qmg::ok(qmg_u1_random_trans(gauge_trans, lat->get_dim_mu(0), lat->get_dim_mu(1), u1_next_field_seed(generator), qmg::current_stream()), "qmg_u1_random_trans");
}

// u_i(x) = g(x) u_i(x) g^dag(x + i) (:241-272); `gauge_trans` a DEVICE nc = 1 colour vector
inline void apply_gauge_trans_u1(complex<double>* gauge_field, complex<double>* gauge_trans, Lattice2D* lat) {
  if (lat->get_nc() != 1) { std::cout << "[QMG-ERROR]: U1 gauge functions require Nc = 1 lattice.\n"; return; }
  qmg::ok(qmg_u1_gauge_transform(gauge_field, gauge_trans, lat->get_dim_mu(0), lat->get_dim_mu(1), qmg::current_stream()), "qmg_u1_gauge_transform");
}

// APE smearing with parameter alpha, n_iter times (:276-383); smeared_field == gauge_field is allowed
inline void apply_ape_smear_u1(complex<double>* smeared_field, complex<double>* gauge_field, Lattice2D* lat, double alpha, int n_iter) {
  if (lat->get_nc() != 1) { std::cout << "[QMG-ERROR]: U1 gauge functions require Nc = 1 lattice.\n"; return; }
  qmg::ok(qmg_u1_ape_smear(smeared_field, gauge_field, lat->get_dim_mu(0), lat->get_dim_mu(1), alpha, n_iter, qmg::current_stream()), "qmg_u1_ape_smear");
}

// Stout smearing (not in the reference; csrc/qmg_stout.hip): n_levels times U_mu(x) <- U_mu(x) exp(-i rho dS_w/dtheta_mu(x)), S_w = sum_x (1 - cos P(x)).
// smeared_field receives the top level alone -- the links an ensemble generated by SchwingerHMC with (stout_levels, stout_rho) = (n_levels, rho)
// has its fermions on.  smeared_field must not be gauge_field; n_levels == 0 copies.  The lower levels live in a buffer of the call's own.
inline void stout_smear_u1(complex<double>* smeared_field, complex<double>* gauge_field, Lattice2D* lat, double rho, int n_levels) {
  if (lat->get_nc() != 1) { std::cout << "[QMG-ERROR]: U1 gauge functions require Nc = 1 lattice.\n"; return; }
  if (n_levels < 0 || smeared_field == gauge_field) { std::cout << "[QMG-ERROR]: stout_smear_u1 needs n_levels >= 0 and smeared_field != gauge_field.\n"; return; }
  const int Lx = lat->get_dim_mu(0), Ly = lat->get_dim_mu(1);
  const size_t n = (size_t)lat->get_size_gauge();
  if (n_levels == 0) { copy_vector(smeared_field, gauge_field, n); return; }
  if (n_levels == 1) { qmg::ok(qmg_u1_stout_smear(smeared_field, gauge_field, Lx, Ly, rho, 1, qmg::current_stream()), "qmg_u1_stout_smear"); return; }
  complex<double>* lower = allocate_vector<complex<double>>(n * (size_t)(n_levels - 1));
  if (!lower) { std::cout << "[QMG-ERROR]: stout_smear_u1: out of device memory.\n"; return; }
  qmg::ok(qmg_u1_stout_smear(lower, gauge_field, Lx, Ly, rho, n_levels - 1, qmg::current_stream()), "qmg_u1_stout_smear");
  qmg::ok(qmg_u1_stout_smear(smeared_field, lower + n * (size_t)(n_levels - 2), Lx, Ly, rho, 1, qmg::current_stream()), "qmg_u1_stout_smear");
  deallocate_vector(&lower);
}

inline void create_instanton_u1(complex<double>* gauge_field, Lattice2D* lat, double Q, const int x0, const int y0) {   // :545-572
  if (lat->get_nc() != 1) { std::cout << "[QMG-ERROR]: U1 gauge functions require Nc = 1 lattice.\n"; return; }
  qmg::ok(qmg_u1_instanton(gauge_field, lat->get_dim_mu(0), lat->get_dim_mu(1), Q, x0, y0, qmg::current_stream()), "qmg_u1_instanton");
}
inline void create_noncompact_instanton_u1(double* phase_field, Lattice2D* lat, double Q) {   // :575-603
  if (lat->get_nc() != 1) { std::cout << "[QMG-ERROR]: U1 gauge functions require Nc = 1 lattice.\n"; return; }
  qmg::ok(qmg_u1_noncompact_instanton(phase_field, lat->get_dim_mu(0), lat->get_dim_mu(1), Q, qmg::current_stream()), "qmg_u1_noncompact_instanton");
}

inline complex<double> get_plaquette_u1(complex<double>* gauge_field, Lattice2D* lat) {   // :424-462
  if (lat->get_nc() != 1) { std::cout << "[QMG-ERROR]: U1 gauge functions require Nc = 1 lattice.\n"; return -50; }
  double o[3] = {0, 0, 0};
  qmg::ok(qmg_u1_plaquette(gauge_field, lat->get_dim_mu(0), lat->get_dim_mu(1), o, qmg::current_stream()), "qmg_u1_plaquette");
  return complex<double>(o[0], o[1]);
}
inline double get_topo_u1(complex<double>* gauge_field, Lattice2D* lat) {   // :465-508
  if (lat->get_nc() != 1) { std::cout << "[QMG-ERROR]: U1 gauge functions require Nc = 1 lattice.\n"; return -50.1; }
  double o[3] = {0, 0, 0};
  qmg::ok(qmg_u1_plaquette(gauge_field, lat->get_dim_mu(0), lat->get_dim_mu(1), o, qmg::current_stream()), "qmg_u1_plaquette");
  return o[2];
}
inline double get_noncompact_action_u1(double* phase_field, double beta, Lattice2D* lat) {   // :386-421
  if (lat->get_nc() != 1) { std::cout << "[QMG-ERROR]: U1 gauge functions require Nc = 1 lattice.\n"; return -50; }
  double o = 0.0;
  qmg::ok(qmg_u1_noncompact_action(phase_field, lat->get_dim_mu(0), lat->get_dim_mu(1), beta, &o, qmg::current_stream()), "qmg_u1_noncompact_action");
  return o;
}

// ---- Wilson flow and Wilson / Polyakov loops (csrc/qmg_flow.hip; not in the reference).  fp64, single domain: y-slabs are refused. ----
inline bool u1_flow_refused(Lattice2D* lat, const char* who) {
  if (lat->get_nc() != 1) { std::cout << "[QMG-ERROR]: U1 gauge functions require Nc = 1 lattice.\n"; return true; }
  if (qmg::slab().on) { std::cout << "[QMG-ERROR]: " << who << " does not run on y-slabs.\n"; return true; }
  return false;
}

// Flows a link field and keeps the phases theta (U = exp(i theta)) across calls, so that "flow k steps, measure, flow k steps, ..." never
// goes back through arg.  `gauge_field` is the caller's and is flowed in place; t is the flow time reached.
class WilsonFlowU1 {
  WilsonFlowU1(WilsonFlowU1 const&);
  WilsonFlowU1& operator=(WilsonFlowU1 const&);
  Lattice2D* lat;
  complex<double>* gauge;
  double* theta;
  double t;

 public:
  WilsonFlowU1(complex<double>* gauge_field, Lattice2D* lattice) : lat(lattice), gauge(gauge_field), theta(0), t(0.0) {
    if (u1_flow_refused(lat, "WilsonFlowU1")) return;
    theta = allocate_vector<double>((size_t)lat->get_size_gauge());
    if (!theta) { std::cout << "[QMG-ERROR]: WilsonFlowU1: out of device memory.\n"; return; }
    reset();
  }
  ~WilsonFlowU1() { deallocate_vector(&theta); }
  bool ok() const { return theta != 0; }
  // take the phases from the links again (after the caller changed them) and restart the clock
  void reset() {
    if (!theta) return;
    qmg::ok(qmg_u1_gauge_to_phase(theta, gauge, (size_t)lat->get_size_gauge(), qmg::current_stream()), "qmg_u1_gauge_to_phase");
    t = 0.0;
  }
  // n_steps third-order Runge-Kutta steps of size eps
  void flow(double eps, int n_steps) {
    if (!theta) { std::cout << "[QMG-ERROR]: WilsonFlowU1::flow called on an object that was refused.\n"; return; }
    if (qmg::ok(qmg_u1_flow(theta, gauge, lat->get_dim_mu(0), lat->get_dim_mu(1), eps, n_steps, qmg::current_stream()), "qmg_u1_flow")) t += eps * n_steps;
  }
  double time() const { return t; }
  double* phases() { return theta; }
  complex<double>* links() { return gauge; }
  double energy() { return 1.0 - std::real(get_plaquette_u1(gauge, lat)); }   // E(t) = S_w / V
};

// n_steps steps of size eps on a link field, in place
inline void wilson_flow_u1(complex<double>* gauge_field, Lattice2D* lat, double eps, int n_steps) {
  WilsonFlowU1 f(gauge_field, lat);
  if (f.ok()) f.flow(eps, n_steps);
}

// out[(R - 1) t_max + (T - 1)] = lattice average of the R x T Wilson loop in the x-y plane, 1 <= R <= r_max <= Lx/2, 1 <= T <= t_max <= Ly/2; `out` is a HOST array
inline bool get_wilson_loops_u1(complex<double>* gauge_field, Lattice2D* lat, int r_max, int t_max, complex<double>* out) {
  if (u1_flow_refused(lat, "get_wilson_loops_u1")) return false;
  return qmg::ok(qmg_u1_wilson_loops(gauge_field, lat->get_dim_mu(0), lat->get_dim_mu(1), r_max, t_max, reinterpret_cast<double*>(out), qmg::current_stream()), "qmg_u1_wilson_loops");
}
// out[0]: the Polyakov loop in x averaged over y, out[1]: in y averaged over x; `out` is a HOST array
inline bool get_polyakov_u1(complex<double>* gauge_field, Lattice2D* lat, complex<double>* out) {
  if (u1_flow_refused(lat, "get_polyakov_u1")) return false;
  return qmg::ok(qmg_u1_polyakov(gauge_field, lat->get_dim_mu(0), lat->get_dim_mu(1), reinterpret_cast<double*>(out), qmg::current_stream()), "qmg_u1_polyakov");
}

#endif
