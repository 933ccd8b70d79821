// dw_selftest_common.hpp -- what dwf_selftest, mobius_selftest, dwf_eo_selftest and mobius_eo_selftest share: the `[TAG] name value PASS|FAIL`
// line, the device vectors of a run, the raw solution file, and for the two even-odd drivers the comparison solve tightened to the even-odd
// solve's true residual and the alternating timing rounds, which take the two solves as callables.
#ifndef QMG_DW_SELFTEST_COMMON_HPP
#define QMG_DW_SELFTEST_COMMON_HPP

#include <chrono>
#include <cmath>
#include <cstdio>
#include <iostream>
#include <vector>

#include "../include/qmg/qmg.hpp"
#include "driver_common.hpp"

namespace dw_selftest {

// one line per check under the driver's tag; all_pass is the exit status
struct Lines {
  const char* tag;
  bool all_pass;
  explicit Lines(const char* tag) : tag(tag), all_pass(true) {}
  void operator()(const char* name, double value, bool pass) {
    std::cout << tag << " " << name << " " << value << " " << (pass ? "PASS" : "FAIL") << "\n";
    if (!pass) all_pass = false;
  }
};

// the device vectors of a run, freed together
struct Vectors {
  std::vector<complex<double>*> all;
  complex<double>* make(size_t n) { all.push_back(allocate_vector<complex<double>>(n)); return all.back(); }
  void release() { for (complex<double>*& p : all) deallocate_vector(&p); all.clear(); }
};

// `count` device vectors as raw complex<double>, one after the other; false where the file cannot be written whole
inline bool write_raw(const char* path, const complex<double>* const* parts, const size_t* lens, int count) {
  FILE* f = fopen(path, "wb");
  bool written = f != nullptr;
  for (int i = 0; written && i < count; i++) {
    const std::vector<complex<double>> h = qmg::to_host(parts[i], lens[i]);
    written = fwrite(h.data(), sizeof(complex<double>), lens[i], f) == lens[i];
  }
  if (f) fclose(f);
  return written;
}

// |b - D x| / |b| with the operator's apply_M; t is overwritten with D x, bnorm = |b|^2
inline double true_residual(Stencil2D* op, complex<double>* t, complex<double>* x, complex<double>* b, int n, double bnorm) {
  op->apply_M_overwrite(t, x);
  return std::sqrt(diffnorm2sq(t, b, n) / bnorm);
}

// The comparison solve of an even-odd selftest: solve(xf, eps_full) from xf = 0, its tolerance tightened (at most 10 attempts) until its true
// residual on D is at or below eo_res, aiming at [1/2, 1] of it.  eps_full and full_res are left as the last attempt had them.
template <class Solve>
inline inversion_info tightened_solve(Stencil2D* op, complex<double>* xf, complex<double>* t, complex<double>* b, int n, double bnorm, double eo_res, double& eps_full,
                                      double& full_res, Solve solve) {
  inversion_info full;
  for (int attempt = 0; attempt < 10; attempt++) {
    zero_vector(xf, n);
    full = solve(xf, eps_full);
    full_res = true_residual(op, t, xf, b, n, bnorm);
    if (full_res <= eo_res && full_res >= 0.5 * eo_res) break;
    eps_full *= 0.75 * eo_res / full_res;
  }
  return full;
}

// wall clock around one solve from sol = 0, the stream drained on either side
template <class Solve>
inline double wall_ms(complex<double>* sol, int n, Solve solve) {
  zero_vector(sol, n);
  qmg_stream_sync(qmg::current_stream());
  const auto t0 = std::chrono::steady_clock::now();
  solve(sol);
  qmg_stream_sync(qmg::current_stream());
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
// the two solves timed alternately: one line `<tag> round r eo_ms t full_ms t` per round
template <class Eo, class Full>
inline void timing_rounds(const char* tag, int rounds, int n, complex<double>* xe, complex<double>* xf, Eo eo_solve, Full full_solve) {
  qmg_driver::phase("timing");
  for (int r = 0; r < rounds; r++) {
    const double te = wall_ms(xe, n, eo_solve), tf = wall_ms(xf, n, full_solve);
    std::cout << tag << " round " << r << " eo_ms " << te << " full_ms " << tf << "\n";
  }
}

}  // namespace dw_selftest

#endif
