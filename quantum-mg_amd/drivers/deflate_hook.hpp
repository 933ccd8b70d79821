// deflate_hook.hpp -- the drivers' coarsest-level deflation switch (StatefulMultigridMG::deflate_coarsest, include/qmg/eigen.hpp).
//   QMG_DEFLATE=n_low[,n_high]   after the hierarchy is built: deflate_coarsest(n_low, n_high, true), which prints the eigenvalues as
//                                [QMG-COARSEST-EVALS] lines; its cost goes on a line of its own,
//                                [QMG-DEFLATION-TIMING]: <s> s, <restarts> restarts, <applies> applies
//                                and the caller counts the seconds as setup
//   QMG_DEFLATE_USE=0            the pairs are computed, then CoarsestSolveMG::deflate is switched off (test hook)
//   QMG_DUMP_DIR                 also coarsest_evals.bin (nev complex128), coarsest_evecs.bin (nev vectors back to back) and, for a coarsest
//                                vector length N <= 1024, coarsest_op.bin: the dense coarsest operator, column j = A e_j, columns back to back
// Without QMG_DEFLATE nothing happens and nothing is printed.
#ifndef QMG_DEFLATE_HOOK_HPP
#define QMG_DEFLATE_HOOK_HPP

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <iomanip>
#include <iostream>
#include <string>
#include <vector>

#include "../include/qmg/qmg.hpp"

inline bool deflate_hook_on() { return getenv("QMG_DEFLATE") != 0; }

// returns the seconds deflate_coarsest took (0 without the hook)
inline double deflate_from_env(StatefulMultigridMG* mg, const char* dump_dir, bool root) {
  const char* env = getenv("QMG_DEFLATE");
  if (!env) return 0.0;
  const std::string spec(env);
  const size_t comma = spec.find(',');
  const int n_low = atoi(spec.substr(0, comma).c_str());
  const int n_high = (comma == std::string::npos) ? 0 : atoi(spec.substr(comma + 1).c_str());
  qmg_stream_sync(qmg::current_stream());
  const auto t0 = std::chrono::steady_clock::now();
  mg->deflate_coarsest(n_low, n_high, root);
  qmg_stream_sync(qmg::current_stream());
  const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  const unsigned nev = mg->get_coarsest_deflated();
  if (nev == 0) return s;
  if (root)
    std::cout << std::setprecision(6) << "[QMG-DEFLATION-TIMING]: " << s << " s, " << mg->get_deflation_restarts() << " restarts, " << mg->get_deflation_applies()
              << " applies\n" << std::setprecision(20);
  if (getenv("QMG_DEFLATE_USE") && atoi(getenv("QMG_DEFLATE_USE")) == 0) mg->get_coarsest_solve()->deflate = false;
  if (dump_dir) {
    const int nl = mg->get_num_levels();
    const size_t N = (size_t)mg->get_lattice(nl - 1)->get_size_cv_l();
    FILE* f = fopen((std::string(dump_dir) + "/coarsest_evals.bin").c_str(), "wb");
    if (f) { fwrite(mg->get_coarsest_evals(), sizeof(complex<double>), nev, f); fclose(f); }
    f = fopen((std::string(dump_dir) + "/coarsest_evecs.bin").c_str(), "wb");
    for (unsigned i = 0; i < nev && f; i++) {
      const std::vector<complex<double> > h = qmg::to_host(mg->get_coarsest_evecs()[i], N);
      fwrite(h.data(), sizeof(complex<double>), N, f);
    }
    if (f) fclose(f);
    if (N <= 1024) {
      BatchOp op(mg->get_stencil(nl - 1), mg->get_coarsest_solve()->coarsest_stencil_app);   // unshifted, as the eigensolver sees it
      complex<double>* e = allocate_vector<complex<double> >(N);
      complex<double>* a = allocate_vector<complex<double> >(N);
      f = fopen((std::string(dump_dir) + "/coarsest_op.bin").c_str(), "wb");
      for (size_t j = 0; j < N && f && e && a; j++) {
        zero_vector(e, N);
        qmg::set_element(e, j, complex<double>(1.0, 0.0));
        apply_stencil_typed_batch<double>(qmg::Batch(a, N, 1), qmg::Batch(e, N, 1), 1u, (void*)&op);
        const std::vector<complex<double> > h = qmg::to_host(a, N);
        fwrite(h.data(), sizeof(complex<double>), N, f);
      }
      if (f) fclose(f);
      deallocate_vector(&e);
      deallocate_vector(&a);
    }
  }
  return s;
}

#endif
