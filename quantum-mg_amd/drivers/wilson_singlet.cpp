// wilson_singlet -- flavour-singlet loops of the two-flavour Wilson Schwinger model on one U(1) configuration, from diluted Z4 noise on
// lock-step batch solves (include/qmg/singlet.hpp): the chiral condensate, m Tr(gamma5 D^-1) beside the geometric charge, the disconnected
// pseudoscalar correlator and, with nt = L, the one-end-trick pion and the flavour-singlet correlator C_eta = C_pi - 2 D_disc.
//   ./wilson_singlet L mass beta n_refine coarse_dof gauge_file tile n_noise nt spin eo seed [bicgstab|kcycle|kcycle_f32] [dump_dir]
// The first seven arguments are n13's (n13_setup.hpp builds the operator and, for the K-cycle routes, the hierarchy; with `bicgstab`, the
// default, n_refine is ignored and no hierarchy is built).  Noise a has seed `seed + a`; its nt ncs neo dilution classes are solved in
// batches of at most 16.  Output (17 significant digits):
//   [QMG-CLASS]: noise class iterations true_residual source_norm       one line per solve (the residual is relative to the source norm)
//   [QMG-LOOPS]: noise condensate q5 mass*q5 topo iterations worst_true_residual
//   [QMG-CONDENSATE]: mean +/- standard error over the noises
//   [QMG-BEGIN-DISC] (n_noise >= 2), and with nt == L [QMG-BEGIN-PION], [QMG-BEGIN-ETA] and their -EFFMASS blocks: `t value` lines, each
//   block closed by its [QMG-END-...]; nothing is folded
//   [QMG-TIMING]: setup ; solves ; dilution + loops kernels ; aggregate iterations/s
// dump_dir: loops_noise<a>.txt (`class y ReS ImS ReP ImP N` per line) and psi_noise<a>.bin (the solutions, raw complex128, class by class).
// The exit status is nonzero if a solve missed 20 * tol.  An ensemble is one run per file.
#include <cstdio>

#include "n13_setup.hpp"

static void effmass_block(const char* tag, const std::vector<double>& c) {
  const int n = (int)c.size();
  cout << "[QMG-BEGIN-" << tag << "-EFFMASS]\n";
  for (int j = 1; j < n - 1; j++) cout << j << " " << std::acosh((c[j + 1] + c[j - 1]) / (2.0 * c[j])) << "\n";
  cout << "[QMG-END-" << tag << "-EFFMASS]\n";
}
static void table_block(const char* tag, const std::vector<double>& c) {
  cout << "[QMG-BEGIN-" << tag << "]\n";
  for (size_t j = 0; j < c.size(); j++) cout << j << " " << c[j] << "\n";
  cout << "[QMG-END-" << tag << "]\n";
}

int main(int argc, char** argv) {
  qmg_driver::Guard guard;
  if (argc < 13) {
    std::cout << "usage: ./wilson_singlet L mass beta n_refine coarse_dof gauge_file tile n_noise nt spin eo seed [bicgstab|kcycle|kcycle_f32] [dump_dir]\n";
    return -1;
  }
  const std::string route = argc > 13 ? argv[13] : "bicgstab";
  if (route != "bicgstab" && route != "kcycle" && route != "kcycle_f32") { std::cout << "[QMG-ERROR]: the solver is bicgstab, kcycle or kcycle_f32.\n"; return -1; }
  const std::string dump = argc > 14 ? argv[14] : "";
  const int n_noise = stoi(argv[8]);
  const qmg::Dilution dil(stoi(argv[9]), stoi(argv[10]), stoi(argv[11]));
  const unsigned long long seed0 = stoull(argv[12]);
  if (n_noise < 1) { std::cout << "[QMG-ERROR]: n_noise must be positive.\n"; return -1; }

  char zero_levels[] = "0";
  std::vector<char*> args(argv, argv + argc);
  if (route == "bicgstab") args[4] = zero_levels;   // no hierarchy
  N13 s;
  const int rc = s.build(8, args.data());
  if (rc) return rc;
  if (qmg::slab().on) { std::cout << "[QMG-ERROR]: wilson_singlet does not run in y-slab mode.\n"; return 4; }
  Lattice2D* lat = s.lats[0];
  Stencil2D* op = s.mg_object->get_stencil(0);
  Lattice2D lat_gauge(s.x_len, s.y_len, 1);
  const double topo = get_topo_u1(s.gauge_field, &lat_gauge);

  inversion_verbose_struct quiet(VERB_NONE, "");
  qmg::SingletBicgstab bi(op, s.tol, 4000, 6);
  qmg::SingletKcycle kc(s.mg_object, s.tol, s.max_iter, s.restart_freq, route == "kcycle_f32", &quiet);
  if (route != "bicgstab" && !kc.prepare()) return 5;
  qmg::SingletLoops loops(lat, dil, 0, route == "bicgstab" ? qmg::singlet_solve_bicgstab : qmg::singlet_solve_kcycle, route == "bicgstab" ? (void*)&bi : (void*)&kc, op);
  loops.keep_solutions = !dump.empty();
  if (route != "bicgstab") loops.max_batch = qmg::batch_systems_that_fit(s.mg_object, std::min(s.restart_freq, 48), qmg::BATCH_MAX);
  const int n_classes = dil.classes(lat->get_nc());
  cout << "[QMG-INFO]: " << n_noise << " noises x " << n_classes << " dilution classes (nt " << dil.nt << " spin " << dil.spin << " eo " << dil.eo << ") by " << route
       << " in lock-step batches of at most " << std::min(loops.max_batch, n_classes) << "\n";

  std::vector<qmg::LoopSet> noises(n_noise);
  qmg::SingletResult res;
  bool ok_ = true;
  double solve_s = 0.0, kernel_s = 0.0;
  long iters = 0;
  cout << scientific << setprecision(16);
  for (int a = 0; a < n_noise; a++) {
    if (!loops.measure(seed0 + (unsigned long long)a, noises[a])) { s.destroy(); return qmg_driver::leave(6); }
    const qmg::LoopSet& m = noises[a];
    for (int d = 0; d < n_classes; d++) {
      cout << "[QMG-CLASS]: " << a << " " << d << " " << m.iters[d] << " " << m.true_res[d] << " " << m.src_norm[d] << "\n";
      ok_ = ok_ && m.converged[d] && m.true_res[d] < 20 * s.tol;
    }
    std::vector<qmg::LoopSet> one(1, m);
    one[0].psi.clear();
    qmg::SingletLoops::combine(one, res);
    cout << "[QMG-LOOPS]: " << a << " " << res.condensate << " " << res.q5[0] << " " << s.mass * res.q5[0] << " " << topo << " " << m.total_iters() << " " << m.worst_residual() << "\n";
    solve_s += m.solve_s; kernel_s += m.kernel_s; iters += m.total_iters();
    if (!dump.empty()) {
      FILE* f = fopen((dump + "/loops_noise" + std::to_string(a) + ".txt").c_str(), "w");
      FILE* g = fopen((dump + "/psi_noise" + std::to_string(a) + ".bin").c_str(), "wb");
      if (!f || !g) { std::cout << "[QMG-ERROR]: cannot write into " << dump << "\n"; s.destroy(); return qmg_driver::leave(7); }
      for (int d = 0; d < n_classes; d++) {
        for (int y = 0; y < m.Ly; y++)
          fprintf(f, "%d %d %.17e %.17e %.17e %.17e %.17e\n", d, y, m.S[d][y].real(), m.S[d][y].imag(), m.P[d][y].real(), m.P[d][y].imag(), m.N[d][y]);
        fwrite(m.psi[d].data(), sizeof(complex<double>), m.psi[d].size(), g);
      }
      fclose(f); fclose(g);
      noises[a].psi.clear();
    }
  }
  qmg::SingletLoops::combine(noises, res);
  cout << "[QMG-CONDENSATE]: " << res.condensate << " +/- " << res.condensate_err << "\n";
  if (res.has_disc) table_block("DISC", res.Ddisc);
  if (res.has_pion) { table_block("PION", res.Cpi); effmass_block("PION", res.Cpi); }
  if (res.has_pion && res.has_disc) { table_block("ETA", res.Ceta); effmass_block("ETA", res.Ceta); }
  cout << setprecision(6) << "[QMG-TIMING]: setup " << s.setup_s << " s ; solves " << solve_s << " s ; dilution + loops kernels " << kernel_s << " s ; aggregate iterations/s "
       << iters / solve_s << "\n";
  if (!ok_) cout << "[QMG-ERROR]: a solve missed 20 * tol = " << 20 * s.tol << ".\n";
  s.destroy();
  return qmg_driver::leave(ok_ ? 0 : 1);
}
