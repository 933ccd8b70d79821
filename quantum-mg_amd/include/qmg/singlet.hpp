// singlet.hpp -- flavour-singlet loops from diluted Z4 noise on lock-step batch solves (csrc/qmg_singlet.hip).
//
// The noise is a function of (seed, element): eta_i = i^(h >> 62), h the first hash the Gaussian generator takes for element i.  A dilution
// (nt, spin, eo) splits it into D = nt ncs neo sources with disjoint supports, class d(i) = ((y mod nt) ncs + (spin ? c : 0)) neo + (eo ? p : 0)
// (ncs = spin ? nc : 1, neo = eo ? 2 : 1, p the parity half).  With psi^(d) = D^-1 eta^(d) and g(i) the sign of gamma5, per class and row y
//   S_d(y) = sum_{i in row y, d(i) = d} conj(eta_i) psi^(d)_i        P_d(y) = the same sum of conj(eta_i) g(i) psi^(d)_i
//   N_d(y) = sum_{i in row y} |psi^(d)_i|^2                          (over the WHOLE row)
// SingletLoops::measure walks the classes in batches of at most 16: one launch dilutes a batch of sources, the solve hook advances them in
// lock step, one launch takes the loops of the batch.  Signs and normalisation of what `combine` forms of them, stated once (Nn noises,
// S(y) = sum_d S_d(y) and P(y) = sum_d P_d(y) per noise; tests/singlet_numpy.py is the independent statement):
//   condensate = Re sum_y S(y) / (Lx Ly), its mean over the noises and the standard error of that mean
//   q5         = sum_y Re P(y)                                        (m q5 sits beside the geometric charge of get_topo_u1)
//   Ddisc(t)   = 1 / (Nn (Nn - 1) Ly) sum_{a != b} sum_{y0} Re P_a(y0) Re P_b((y0 + t) mod Ly)            (Nn >= 2: no noise meets itself)
//   Cpi(t)     = 1 / (Nn Ly) sum_a sum_{t0} sum_{d: row of class d = t0} N_d((t0 + t) mod Ly)              (nt == Ly: the one-end trick)
//   Ceta(t)    = Cpi(t) - N_f Ddisc(t)
#ifndef QMG_SINGLET_HPP
#define QMG_SINGLET_HPP

#include <algorithm>
#include <chrono>
#include <cmath>
#include <iostream>
#include <vector>

#include "batch.hpp"

namespace qmg {

struct Dilution {
  int nt, spin, eo;
  Dilution(int nt_ = 1, int spin_ = 0, int eo_ = 0) : nt(nt_), spin(spin_), eo(eo_) {}
  int classes(int nc) const { return nt * (spin ? nc : 1) * (eo ? 2 : 1); }
  int row_of(int d, int nc) const { return d / ((spin ? nc : 1) * (eo ? 2 : 1)); }   // y mod nt of class d
};

// x = D^-1 b for the active systems of a batch, from zero; info: one entry per system of the batch.  false: the solve could not run.
typedef bool (*singlet_solve_t)(Batch x, Batch b, unsigned mask, void* data, std::vector<inversion_info>* info);

// hook (a): BiCGStab-L on the ORIGINAL operator, no hierarchy
struct SingletBicgstab {
  Stencil2D* st;
  double tol;
  int max_iter, L;
  SingletBicgstab(Stencil2D* st_, double tol_ = 1e-10, int max_iter_ = 4000, int L_ = 6) : st(st_), tol(tol_), max_iter(max_iter_), L(L_) {}
};
inline bool singlet_solve_bicgstab(Batch x, Batch b, unsigned mask, void* data, std::vector<inversion_info>* info) {
  SingletBicgstab* s = (SingletBicgstab*)data;
  const size_t n = (size_t)s->st->lat->get_size_cv_l();
  BatchOp op(s->st, QMG_MATVEC_ORIGINAL);
  bzero(x, n, mask);
  *info = bbicgstab_l_core<double>(x, b, (int)n, s->max_iter, s->tol, s->L, apply_stencil_typed_batch<double>, (void*)&op, mask, true);
  return true;
}

// hook (b): the outer VPGCR with the batch K-cycle as its preconditioner (drivers/mrhs_solve.hpp); f32: the K-cycle runs in complex<float>
// on the fp32 shadow of the hierarchy, the outer solve and its tolerance stay fp64
struct SingletKcycle {
  StatefulMultigridMG* mg;
  double tol;
  int max_iter, restart_freq;
  bool f32;
  inversion_verbose_struct* verb;
  SingletKcycle(StatefulMultigridMG* mg_, double tol_ = 1e-10, int max_iter_ = 1000, int restart_freq_ = 32, bool f32_ = false, inversion_verbose_struct* verb_ = 0)
      : mg(mg_), tol(tol_), max_iter(max_iter_), restart_freq(restart_freq_), f32(f32_), verb(verb_) {}
  // once, before the first solve: the hierarchy is one the batch K-cycle runs, and its fp32 shadow exists where asked for
  bool prepare() {
    BatchKcycle probe(mg, 1);
    if (!probe.supported()) { std::cout << "[QMG-ERROR]: the batched K-cycle does not implement this hierarchy's level / coarsest operator types.\n"; return false; }
    if (f32 && !probe.enable_f32_hierarchy()) { std::cout << "[QMG-ERROR]: could not build the fp32 shadow of the hierarchy\n"; return false; }
    return true;
  }
};
inline bool singlet_solve_kcycle(Batch x, Batch b, unsigned mask, void* data, std::vector<inversion_info>* info) {
  SingletKcycle* s = (SingletKcycle*)data;
  const size_t n = (size_t)s->mg->get_lattice(0)->get_size_cv_l();
  BatchKcycle bk(s->mg, x.nrhs);
  BatchOp op0(s->mg->get_stencil(0), QMG_MATVEC_ORIGINAL);
  qmg_reserve_kcycle_scratch(s->mg, n, std::min(s->restart_freq > 0 ? s->restart_freq : s->max_iter, 64), x.nrhs);
  bzero(x, n, mask);
  *info = bgcr_core<double>(x, b, (int)n, s->max_iter, s->tol, s->restart_freq, apply_stencil_typed_batch<double>, (void*)&op0,
                            s->f32 ? mg_preconditioner_batch_mixed : mg_preconditioner_batch<double>, (void*)&bk, mask, true, s->verb, "VPGCR-restart");
  return true;
}

// what one noise gives: [class][row]
struct LoopSet {
  int Lx, Ly, nc;
  Dilution dil;
  unsigned long long seed;
  std::vector<std::vector<complex<double> > > S, P;
  std::vector<std::vector<double> > N;
  std::vector<int> iters;              // per class
  std::vector<char> converged;
  std::vector<double> true_res;        // |eta^(d) - D psi^(d)| / |eta^(d)| against the ORIGINAL operator
  std::vector<double> src_norm;        // |eta^(d)|: the square root of the size of the class's support
  long n_applies;                      // operator applies of all solves, the residual checks included
  double solve_s, kernel_s;            // wall time of the solves; of the dilution and loops launches
  std::vector<std::vector<complex<double> > > psi;   // the solutions, where SingletLoops::keep_solutions asks for them
  LoopSet() : Lx(0), Ly(0), nc(0), seed(0), n_applies(0), solve_s(0.0), kernel_s(0.0) {}
  double worst_residual() const { double w = 0.0; for (size_t d = 0; d < true_res.size(); d++) w = std::max(w, true_res[d]); return w; }
  long total_iters() const { long t = 0; for (size_t d = 0; d < iters.size(); d++) t += iters[d]; return t; }
};

struct SingletResult {
  int n_f;                                                // flavours in Ceta; set before combine (2)
  std::vector<std::vector<complex<double> > > S, P;       // [noise][y]
  std::vector<double> condensate_per_noise, q5;           // [noise]
  double condensate, condensate_err;
  bool has_disc, has_pion;                                // Nn >= 2; nt == Ly
  std::vector<double> Ddisc, Cpi, Ceta;                   // [t]; Ceta needs both
  SingletResult() : n_f(2), condensate(0.0), condensate_err(0.0), has_disc(false), has_pion(false) {}
};

class SingletLoops {
 public:
  bool keep_solutions;   // LoopSet::psi is filled (tests)
  int max_batch;         // systems per batch at most (what the solver's own storage leaves room for); 16

  SingletLoops(Lattice2D* lat_, Dilution dil_, int g5_mode_, singlet_solve_t solve_, void* data_, Stencil2D* op_)
      : keep_solutions(false), max_batch(BATCH_MAX), lat(lat_), dil(dil_), g5_mode(g5_mode_), solve(solve_), data(data_), op(op_) {}

  // the D classes of one noise; false (with a [QMG-ERROR] line) where the measurement cannot run -- a solve that misses its tolerance is
  // reported in out.converged / out.true_res, not here
  bool measure(unsigned long long seed, LoopSet& out) {
    if (slab().on) { std::cout << "[QMG-ERROR]: SingletLoops is not available in y-slab mode (a timeslice is one row of ONE rank's slab).\n"; return false; }
    const int Lx = lat->get_dim_mu(0), Ly = lat->get_dim_mu(1), nc = lat->get_nc();
    if (dil.nt < 1 || Ly % dil.nt || (dil.spin != 0 && dil.spin != 1) || (dil.eo != 0 && dil.eo != 1) || (g5_mode == 0 && (nc & 1))) {
      std::cout << "[QMG-ERROR]: SingletLoops needs nt >= 1 that divides Ly, spin and eo in {0, 1}, and an even nc for the Wilson gamma5.\n";
      return false;
    }
    const size_t n = (size_t)lat->get_size_cv_l();
    const int D = dil.classes(nc);
    out = LoopSet();
    out.Lx = Lx; out.Ly = Ly; out.nc = nc; out.dil = dil; out.seed = seed;
    out.S.assign(D, std::vector<complex<double> >(Ly)); out.P = out.S;
    out.N.assign(D, std::vector<double>(Ly, 0.0));
    out.iters.assign(D, 0); out.converged.assign(D, 0); out.true_res.assign(D, 0.0); out.src_norm.assign(D, 0.0);
    if (keep_solutions) out.psi.assign(D, std::vector<complex<double> >());
    const int per_batch = std::max(1, std::min(std::min(D, max_batch), std::min((int)BATCH_MAX, systems_that_fit(n))));
    std::vector<double> loops((size_t)per_batch * Ly * 5);
    for (int d0 = 0; d0 < D; d0 += per_batch) {
      const int nb = std::min(per_batch, D - d0);
      const unsigned all = full_mask(nb);
      BatchPool pool(n, nb);
      Batch b = pool.get(), x = pool.get(), Ax = pool.get();
      if (b.p == 0 || x.p == 0 || Ax.p == 0) { std::cout << "[QMG-ERROR]: out of device memory for a batch of " << nb << " systems\n"; return false; }
      qmg_stream_sync(current_stream());
      std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
      if (!ok(qmg_noise_dilute_batch(QMG_C64, b.p, Lx, Ly, nc, dil.nt, dil.spin, dil.eo, d0, seed, nb, b.stride, all, current_stream()), "qmg_noise_dilute_batch")) return false;
      qmg_stream_sync(current_stream());
      std::chrono::steady_clock::time_point t1 = std::chrono::steady_clock::now();
      std::vector<inversion_info> inv;
      if (!solve(x, b, all, data, &inv) || (int)inv.size() != nb) { std::cout << "[QMG-ERROR]: the batch solve of classes " << d0 << " .. " << d0 + nb - 1 << " did not run\n"; return false; }
      qmg_stream_sync(current_stream());
      std::chrono::steady_clock::time_point t2 = std::chrono::steady_clock::now();
      op->apply_M_overwrite_batch(Ax.p, x.p, nb, x.stride, all);   // the true residual against the ORIGINAL operator
      const std::vector<double> rsq = bdiffnorm2sq(b, Ax, n, all), bsq = bnorm2sq(b, n, all);
      qmg_stream_sync(current_stream());
      std::chrono::steady_clock::time_point t3 = std::chrono::steady_clock::now();
      if (!ok(qmg_loops_timeslice_batch(QMG_C64, x.p, Lx, Ly, nc, dil.nt, dil.spin, dil.eo, d0, seed, g5_mode, nb, x.stride, all, 0, loops.data(), current_stream()),
              "qmg_loops_timeslice_batch")) return false;
      std::chrono::steady_clock::time_point t4 = std::chrono::steady_clock::now();
      out.kernel_s += secs(t0, t1) + secs(t3, t4);
      out.solve_s += secs(t1, t2);
      for (int k = 0; k < nb; k++) {
        const int d = d0 + k;
        for (int y = 0; y < Ly; y++) {
          const double* v = &loops[((size_t)k * Ly + y) * 5];
          out.S[d][y] = complex<double>(v[0], v[1]);
          out.P[d][y] = complex<double>(v[2], v[3]);
          out.N[d][y] = v[4];
        }
        out.iters[d] = inv[k].iter;
        out.converged[d] = inv[k].success ? 1 : 0;
        out.true_res[d] = std::sqrt(rsq[k] / bsq[k]);
        out.src_norm[d] = std::sqrt(bsq[k]);
        out.n_applies += inv[k].ops_count + 1;
        if (keep_solutions) out.psi[d] = to_host(x.vec(k), n);
      }
    }
    return true;
  }

  // the observables of Nn noises of one lattice and dilution (the header's formulas); host arithmetic only
  static void combine(const std::vector<LoopSet>& noises, SingletResult& r) {
    const int n_f = r.n_f;
    r = SingletResult();
    r.n_f = n_f;
    const int nn = (int)noises.size();
    if (nn == 0) return;
    const int Lx = noises[0].Lx, Ly = noises[0].Ly, nc = noises[0].nc;
    const Dilution dil = noises[0].dil;
    r.S.assign(nn, std::vector<complex<double> >(Ly)); r.P = r.S;
    r.condensate_per_noise.assign(nn, 0.0); r.q5.assign(nn, 0.0);
    for (int a = 0; a < nn; a++) {
      for (size_t d = 0; d < noises[a].S.size(); d++)
        for (int y = 0; y < Ly; y++) { r.S[a][y] += noises[a].S[d][y]; r.P[a][y] += noises[a].P[d][y]; }
      double s = 0.0, p = 0.0;
      for (int y = 0; y < Ly; y++) { s += r.S[a][y].real(); p += r.P[a][y].real(); }
      r.condensate_per_noise[a] = s / ((double)Lx * Ly);
      r.q5[a] = p;
      r.condensate += r.condensate_per_noise[a] / nn;
    }
    if (nn > 1) {
      double var = 0.0;
      for (int a = 0; a < nn; a++) var += (r.condensate_per_noise[a] - r.condensate) * (r.condensate_per_noise[a] - r.condensate);
      r.condensate_err = std::sqrt(var / (nn - 1) / nn);
    }
    r.has_disc = nn >= 2;
    if (r.has_disc) {
      r.Ddisc.assign(Ly, 0.0);
      for (int t = 0; t < Ly; t++) {
        double acc = 0.0;
        for (int a = 0; a < nn; a++)
          for (int b = 0; b < nn; b++)
            if (a != b)
              for (int y0 = 0; y0 < Ly; y0++) acc += r.P[a][y0].real() * r.P[b][(y0 + t) % Ly].real();
        r.Ddisc[t] = acc / ((double)nn * (nn - 1) * Ly);
      }
    }
    r.has_pion = dil.nt == Ly;
    if (r.has_pion) {
      r.Cpi.assign(Ly, 0.0);
      for (int a = 0; a < nn; a++)
        for (size_t d = 0; d < noises[a].N.size(); d++) {
          const int t0 = dil.row_of((int)d, nc);
          for (int t = 0; t < Ly; t++) r.Cpi[t] += noises[a].N[d][(t0 + t) % Ly];
        }
      for (int t = 0; t < Ly; t++) r.Cpi[t] /= (double)nn * Ly;
      if (r.has_disc) {
        r.Ceta.assign(Ly, 0.0);
        for (int t = 0; t < Ly; t++) r.Ceta[t] = r.Cpi[t] - r.n_f * r.Ddisc[t];
      }
    }
  }

 private:
  Lattice2D* lat;
  Dilution dil;
  int g5_mode;
  singlet_solve_t solve;
  void* data;
  Stencil2D* op;

  static double secs(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }
  // source, solution, residual and some twenty Krylov vectors per system in the HBM that is free now, 15 % head-room
  static int systems_that_fit(size_t n) {
    size_t free_b = 0, total_b = 0;
    if (qmg_mem_info(&free_b, &total_b) != QMG_SUCCESS) return 1;
    free_b += VecPool::cached_bytes();
    const double fit = 0.85 * (double)free_b / (24.0 * (double)n * 16.0);
    return fit < 1.0 ? 1 : fit > (double)BATCH_MAX ? (int)BATCH_MAX : (int)fit;
  }
};

}  // namespace qmg

#endif
