// krylov.hpp -- the Krylov solvers, on device-resident vectors: MR(omega), CG (restarted or not), multi-shift CG, flexible GCR and BiCGStab(L).
//
// The reference takes these from quantum-linalg (`inverters/generic_*.h`, absent; only the call sites
// are known: stateful_multigrid.h:851-990,1037-1046, tests/n13_wilson_kcycle/wilson_kcycle.cpp:459-466,
// tests/n02_free_laplace_test/free_laplace.cpp:118).  Names, argument order and the inversion_info /
// inversion_verbose_struct conventions follow those call sites; the algorithms are the textbook ones
// (PARITY UNPINNED: there is no stored output of the reference's solvers anywhere).
//   * tolerance is relative:  stop when sqrt(resSq) < tol * ||b||
//   * resSq is the (recursive) residual norm squared at exit; iter counts iterations; ops_count counts
//     operator applications (used by DslashTrackerMG, stateful_multigrid.h:854-865)
// All vectors are device pointers; every reduction is a two-stage device reduction whose result comes back
// to the host because the control flow depends on it.
//
// Each method has ONE implementation, for a LOCK-STEP BATCH of up to 16 independent systems (bmr_core, bcg_core, bcg_m_core,
// bgcr_core, bbicgstab_l_core): one launch per step for the whole batch, every scalar and every decision per system, and a system that
// converges is FROZEN (its bit leaves the active mask: no kernel reads or writes it) while the rest continue.  The reference-
// named single-vector entry points (minv_vector_minres, minv_vector_cg, ..., minv_vector_bicgstab_l) run these cores on a
// batch of one; only Richardson is single-vector code.  Every type and function of the batch layer is a template on the
// storage scalar T of the vectors (double | float); all scalars, inner products and convergence decisions stay fp64.
// The operators, the K-cycle and the mixed-precision preconditioner of a batch are in batch.hpp.
//
// THE PER-SYSTEM RULES are stated once, in qmg::SolveLedger (host arithmetic, below); a core holds its algorithm and asks the ledger.
//   * |b_k| = 0: A x = 0 has the solution x = 0 whatever the guess was, so x_k is zeroed (one bzero), the system reports success at
//     iter 0 with resSq 0 and ops_count 0, and it is in no mask that reaches an apply, the opening residual included.
//   * Opening: r = b - A x costs one counted apply per system; under zero_guess the caller has zeroed phi, r0 = b and nothing is applied.
//     A system whose opening |r| < eps_k |b| has converged at its guess and never becomes active; max_iter <= 0 makes none active.
//   * ops_count: every apply handed to a mask counts once for each system of that mask.
//   * The active mask: a bit leaves on convergence (sqrt(rsq) < eps_k |b|, success), on breakdown (a zero denominator: no success, iter as
//     it stood) or at the cap (iter >= max_iter, no success), and never returns.  Frozen systems are neither read nor written.
//   * MR and GCR carry |r|^2 as a recurrence, rsq -= delta, which loses absolute accuracy ~1e-16 rsq_ref: a true norm re-anchors it
//     (rsq = rsq_ref = |r|^2) after every 8 orders of magnitude and whenever it announces sqrt(rsq) < c eps_k |b| (MR c = 4, GCR c = 1: a
//     convergence is always confirmed by a true norm).  GCR restarts (a counted true residual) BEFORE it looks at the cap; CG opens every
//     cycle like a solve, from the true residual of the current x; BiCGStab(L) takes a true norm at the end of each L-block.
//   * eps_k is eps, or eps_per_system[k] where a core takes it (GCR, CG).  Closing: (success, iter, resSq, ops_count) per system; a
//     system outside `mask` keeps inversion_info's defaults; the closing line's RelTol is sqrt(resSq) / |b|, 0 when |b| = 0.
#ifndef QMG_KRYLOV_HPP
#define QMG_KRYLOV_HPP

#include <cmath>
#include <complex>
#include <string>
#include <vector>

namespace qmg {

inline unsigned full_mask(int nrhs) { return (nrhs >= 32) ? 0xFFFFFFFFu : ((1u << nrhs) - 1u); }
inline bool is_active(unsigned mask, int k) { return (mask >> k) & 1u; }

// The book-keeping of one lock-step solve: which systems run, stop, re-anchor and report (the rules of the header comment).  Host arithmetic
// only, like cgm_coefficients below: tests/host/krylov_ledger_host.cpp drives it with QMG_KRYLOV_HOST_ONLY and no device code.
struct SolveLedger {
  int nrhs, max_iter;
  unsigned mask, zero_b, run, act;   // the caller's systems; those with b = 0; those that take an opening residual; those still iterating
  std::vector<double> bsq, bnorm, rsq, rsq_ref, eps;
  std::vector<int> its, ops;
  std::vector<bool> conv;
  struct Row { bool success; int iter; double resSq; int ops_count; };
  SolveLedger(const std::vector<double>& bsq_, unsigned mask_, int max_iter_, double eps_, const std::vector<double>* eps_per_system = 0)
      : nrhs((int)bsq_.size()), max_iter(max_iter_), mask(mask_), zero_b(0), act(0), bsq(bsq_), bnorm(nrhs, 0.0), eps(nrhs, eps_), its(nrhs, 0), ops(nrhs, 0),
        conv(nrhs, false) {
    if (eps_per_system) eps = *eps_per_system;
    for (int k = 0; k < nrhs; k++) {
      if (!is_active(mask, k)) bsq[k] = 0.0;
      bnorm[k] = std::sqrt(bsq[k]);
      if (is_active(mask, k) && bsq[k] == 0.0) { zero_b |= 1u << k; conv[k] = true; }
    }
    run = mask & ~zero_b;
    rsq = rsq_ref = bsq;
  }
  bool below(int k, double c) const { return std::sqrt(rsq[k]) < c * eps[k] * bnorm[k]; }
  // the systems of m open (a solve, or a CG cycle) with |r_k|^2 = r0[k]; returns the active mask
  unsigned open(unsigned m, const std::vector<double>& r0) {
    act = 0;
    for (int k = 0; k < nrhs; k++) {
      if (!is_active(m, k)) continue;
      anchor(k, r0[k]);
      conv[k] = below(k, 1.0);
      if (!conv[k] && max_iter > 0) act |= 1u << k;
    }
    return act;
  }
  void count(unsigned m) { for (int k = 0; k < nrhs; k++) if (is_active(m, k)) ops[k]++; }
  // rsq -= delta; true when the recurrence wants a true norm (anchor)
  bool recur(int k, double delta, double c) { rsq[k] -= delta; return !(rsq[k] > 1e-8 * rsq_ref[k]) || below(k, c); }
  void anchor(int k, double true_rsq) { rsq[k] = rsq_ref[k] = true_rsq; }
  void breakdown(int k) { act &= ~(1u << k); }
  bool settle(int k) {   // the convergence test on rsq: a converged system is frozen
    if (below(k, 1.0)) { conv[k] = true; act &= ~(1u << k); }
    return conv[k];
  }
  bool step(int k) { its[k]++; return settle(k); }
  void cap() { for (int k = 0; k < nrhs; k++) if (is_active(act, k) && its[k] >= max_iter) act &= ~(1u << k); }
  Row row(int k) const { Row o = {conv[k], its[k], rsq[k], ops[k]}; return o; }
  double rel(int k) const { return bnorm[k] > 0 ? std::sqrt(rsq[k]) / bnorm[k] : 0.0; }
};

// GCR with raw search directions: y_j such that sum_k alpha_k z'_k = sum_j y_j z_j, z'_k = z_k + sum_{i<k} c[k][i] z'_i
inline std::vector<std::complex<double> > gcr_direction_weights(const std::vector<std::complex<double> >& alpha,
                                                                const std::vector<std::vector<std::complex<double> > >& c, int K) {
  std::vector<std::complex<double> > beta(alpha.begin(), alpha.begin() + K);
  for (int k = K - 1; k >= 0; k--)
    for (int i = 0; i < k; i++) beta[i] += beta[k] * c[k][i];
  return beta;
}

// ---------------------------------------------------------------------------------------------
// The scalar recurrence of multi-shift CG (B. Jegerlehner, hep-lat/9612014), in CG's own notation.  CG on the base system
// A0 = A + sigma_0 takes, in iteration n,  alpha_n = |r_n|^2 / <p_n, A0 p_n>,  x += alpha_n p_n,  r_{n+1} = r_n - alpha_n A0 p_n,
// beta_n = |r_{n+1}|^2 / |r_n|^2,  p_{n+1} = r_{n+1} + beta_n p_n.  The residual of the system shifted by dsigma_s = sigma_s - sigma_0
// stays collinear with the base residual, r^s_n = zeta^s_n r_n, as long as every x^s starts from zero, with
//   zeta_{n+1} = zeta_n zeta_{n-1} alpha_{n-1} / ( alpha_n beta_{n-1} (zeta_{n-1} - zeta_n) + zeta_{n-1} alpha_{n-1} (1 + dsigma alpha_n) )
//   alpha^s_n  = alpha_n zeta_{n+1} / zeta_n ,      beta^s_n = beta_n (zeta_{n+1} / zeta_n)^2
// from zeta_{-1} = zeta_0 = 1, alpha_{-1} = 1, beta_{-1} = 0 (so zeta_1 = 1 / (1 + dsigma alpha_0), and the base shift keeps zeta = 1).
// One call advances every shift of `active` (bit s) by one iteration and hands back the three coefficients of the fused vector update
//   x^s += a[s] p^s ;  p^s = z[s] r_{n+1} + c[s] p^s        (a = alpha^s_n, z = zeta_{n+1}, c = beta^s_n)
// zeta[s] / zeta_prev[s] hold zeta_n / zeta_{n-1} on entry and zeta_{n+1} / zeta_n on return.  A shift outside `active` is left alone:
// its zeta keeps the value it froze at and its coefficients come back 0.  dsigma >= 0 makes 0 < zeta_{n+1} <= zeta_n: zeta only decays,
// the faster the larger the shift, which is why a converged shift has to be frozen instead of iterated into underflow.
// Host arithmetic only (tests/host/multishift_host.cpp compiles this header with QMG_KRYLOV_HOST_ONLY and no device code).
// ---------------------------------------------------------------------------------------------
inline void cgm_coefficients(int ns, const double* dsigma, unsigned active, double alpha, double beta, double alpha_prev, double beta_prev,
                             double* zeta, double* zeta_prev, double* a, double* z, double* c) {
  for (int s = 0; s < ns; s++) {
    a[s] = z[s] = c[s] = 0.0;
    if (!((active >> s) & 1u)) continue;
    const double zn = zeta[s], zo = zeta_prev[s];
    const double ratio = zo * alpha_prev / (alpha * beta_prev * (zo - zn) + zo * alpha_prev * (1.0 + dsigma[s] * alpha));   // zeta_{n+1} / zeta_n
    zeta_prev[s] = zn;
    zeta[s] = zn * ratio;
    a[s] = alpha * ratio;
    z[s] = zeta[s];
    c[s] = beta * ratio * ratio;
  }
}

}  // namespace qmg

#ifndef QMG_KRYLOV_HOST_ONLY
#include <algorithm>
#include <iostream>
#include <map>

#include "qmg_device.hpp"

namespace qmg {

// Scratch vectors for one solve.  Returned to a free list on scope exit instead of hipFree (which synchronises the device): the smoothers run
// thousands of times per solve.  The free list is kept BY CAPACITY: a request for n elements takes the smallest cached block that holds
// n and is not more than twice as large (so the complex<double> scratch of one solve serves the complex<float> batch of the next, and a
// Schur system's half-length vectors fit a full-length block) -- a K-cycle solve that follows another one in the same process then runs
// without a single hipMalloc in its timed region (GB-sized hipMalloc / hipFree calls cost milliseconds each and synchronise).
struct VecPool {
  std::vector<complex<double>*> v;
  size_t n;
  // per host thread (a thread = one stream = one rank when ranks are emulated by threads: qmg_comm_emulate_*)
  struct Shared {
    std::map<size_t, std::vector<complex<double>*>> free_by_cap;   // capacity (elements) -> cached blocks
    std::map<complex<double>*, size_t> cap;                         // every block this pool system has allocated and not yet freed
    size_t cached_elems;
    Shared() : cached_elems(0) {}
  };
  static Shared& shared() { static thread_local Shared s; return s; }
  explicit VecPool(size_t n_) : n(n_) {}
  complex<double>* get() {
    Shared& sh = shared();
    complex<double>* p = 0;
    for (auto it = sh.free_by_cap.lower_bound(n); it != sh.free_by_cap.end() && it->first <= 2 * n; ++it)
      if (!it->second.empty()) { p = it->second.back(); it->second.pop_back(); sh.cached_elems -= it->first; break; }
    // "malloc_poison": a recycled block leaves the pool as a fresh one does, 0xFF in every byte, on the stream its user launches on (the key off:
    // one branch inside the call, no launch) -- the previous solve's plausible numbers would hide a vector that is read before it is written
    if (p) ok(qmg_poison_scratch(p, n * sizeof(complex<double>), current_stream()), "qmg_poison_scratch");
    if (!p) {
      // nothing cached serves the request.  If the HBM that is left cannot either, the cached blocks of OTHER capacities are given back first (a
      // batch of 3 systems after single-system solves found 36 GB of single-system scratch on the free list that no request of its own could
      // take, and ran out of memory at basis vector 56 of 128: batch_systems_that_fit counts cached scratch as free, so it has to be)
      size_t free_b = 0, total_b = 0;
      const size_t need = n * sizeof(complex<double>);
      if (sh.cached_elems > 0 && qmg_mem_info(&free_b, &total_b) == QMG_SUCCESS && free_b < need + ((size_t)1 << 30)) release_all();
      p = allocate_vector<complex<double>>(n);
      if (p) sh.cap[p] = n;
    }
    v.push_back(p);
    return p;
  }
  ~VecPool() {
    Shared& sh = shared();
    for (auto p : v) {
      if (!p) continue;
      const size_t c = sh.cap[p];
      sh.free_by_cap[c].push_back(p);
      sh.cached_elems += c;
    }
  }
  static size_t cached_bytes() { return shared().cached_elems * sizeof(complex<double>); }
  // make sure the free list holds `count` blocks that serve a request for n elements: a solver's scratch allocated BEFORE its timed region (the device allocator's
  // cost for GB-sized blocks is erratic on this platform: 134 calls took 3 ms in one run and 0.66 s in the next, drivers' `[QMG-TIMING]` lines)
  static bool reserve(size_t n, int count) {
    Shared& sh = shared();
    int have = 0;   // blocks on the free list that a request for n elements would take
    for (auto it = sh.free_by_cap.lower_bound(n); it != sh.free_by_cap.end() && it->first <= 2 * n; ++it) have += (int)it->second.size();
    for (int i = have; i < count; i++) {
      // best effort: leave a quarter of the HBM alone (what the solve cannot find here it allocates on demand, and says so)
      size_t free_b = 0, total_b = 0;
      if (qmg_mem_info(&free_b, &total_b) != QMG_SUCCESS || free_b < total_b / 4 + n * sizeof(complex<double>)) return false;
      void* raw = nullptr;
      const double t0 = wall_now();
      const int rc = qmg_malloc(&raw, n * sizeof(complex<double>));
      alloc_stats().seconds += wall_now() - t0; alloc_stats().mallocs++;
      if (rc != QMG_SUCCESS || !raw) return false;
      complex<double>* p = static_cast<complex<double>*>(raw);
      sh.cap[p] = n;
      sh.free_by_cap[n].push_back(p);
      sh.cached_elems += n;
    }
    return true;
  }
  static void release_all() {
    Shared& sh = shared();
    for (auto& kv : sh.free_by_cap)
      for (auto& p : kv.second) { sh.cap.erase(p); deallocate_vector(&p); }
    sh.free_by_cap.clear();
    sh.cached_elems = 0;
  }
};

// a solver's per-iteration (VERB_DETAIL) and closing lines for system k; in a batch of several the system's index follows the name
inline void report(inversion_verbose_struct* verb, const char* name, int nrhs, int k, int iter, double rel) {
  if (!verb || verb->verbosity != VERB_DETAIL) return;
  std::cout << verb->verb_prefix << name;
  if (nrhs > 1) std::cout << " rhs " << k;
  std::cout << " Iter " << iter << " RelTol " << rel << "\n";
}
inline void summary(inversion_verbose_struct* verb, const char* name, int nrhs, int k, bool ok_, int iter, double rel) {
  if (!verb || verb->verbosity == VERB_NONE) return;
  std::cout << verb->verb_prefix << name;
  if (nrhs > 1) std::cout << " rhs " << k;
  std::cout << (ok_ ? " Success " : " Fail ") << "Iter " << iter << " RelTol " << rel << "\n";
}

template <typename T> struct dtype_of;
template <> struct dtype_of<double> { enum { value = QMG_C64 }; };
template <> struct dtype_of<float> { enum { value = QMG_C32 }; };

// nrhs vectors, `stride` complex elements apart
template <typename T>
struct BatchT {
  complex<T>* p;
  size_t stride;
  int nrhs;
  BatchT() : p(0), stride(0), nrhs(0) {}
  BatchT(complex<T>* p_, size_t stride_, int nrhs_) : p(p_), stride(stride_), nrhs(nrhs_) {}
  complex<T>* vec(int k) const { return p + (size_t)k * stride; }
};
typedef BatchT<double> Batch;

// batch scratch, recycled like VecPool (whose unit is one complex<double>: an fp32 batch takes half as many units)
template <typename T>
struct BatchPoolT {
  VecPool pool;
  size_t stride;
  int nrhs;
  BatchPoolT(size_t n, int nrhs_) : pool((n * (size_t)nrhs_ * sizeof(complex<T>) + sizeof(complex<double>) - 1) / sizeof(complex<double>)), stride(n), nrhs(nrhs_) {}
  BatchT<T> get() { return BatchT<T>(reinterpret_cast<complex<T>*>(pool.get()), stride, nrhs); }
};
typedef BatchPoolT<double> BatchPool;

typedef std::vector<complex<double>> cvec;

template <typename T>
inline void bblas(int op, const cvec* a, const cvec* b, const BatchT<T>* x, const BatchT<T>* y, BatchT<T> z, size_t n, unsigned mask) {
  std::vector<double> fa, fb;
  if (a) { fa.resize(2 * z.nrhs); for (int k = 0; k < z.nrhs; k++) { fa[2 * k] = (*a)[k].real(); fa[2 * k + 1] = (*a)[k].imag(); } }
  if (b) { fb.resize(2 * z.nrhs); for (int k = 0; k < z.nrhs; k++) { fb[2 * k] = (*b)[k].real(); fb[2 * k + 1] = (*b)[k].imag(); } }
  ok(qmg_batch_blas_t(dtype_of<T>::value, op, a ? fa.data() : 0, b ? fb.data() : 0, x ? x->p : 0, y ? y->p : 0, z.p, n, z.nrhs, z.stride, mask, current_stream()), "qmg_batch_blas");
}
template <typename T> inline void bzero(BatchT<T> z, size_t n, unsigned mask) { bblas<T>(QMG_BOP_ZERO, 0, 0, 0, 0, z, n, mask); }
template <typename T> inline void bcopy(BatchT<T> z, BatchT<T> x, size_t n, unsigned mask) { bblas<T>(QMG_BOP_COPY, 0, 0, &x, 0, z, n, mask); }
template <typename T> inline void bcaxpy(const cvec& a, BatchT<T> x, BatchT<T> y, size_t n, unsigned mask) { bblas<T>(QMG_BOP_CAXPY, &a, 0, &x, 0, y, n, mask); }   // y += a x
template <typename T> inline void bcxpy(BatchT<T> x, BatchT<T> y, size_t n, unsigned mask) { bblas<T>(QMG_BOP_CXPY, 0, 0, &x, 0, y, n, mask); }                   // y += x
template <typename T> inline void bcaxpbyz(const cvec& a, BatchT<T> x, const cvec& b, BatchT<T> y, BatchT<T> z, size_t n, unsigned mask) { bblas<T>(QMG_BOP_CAXPBYZ, &a, &b, &x, &y, z, n, mask); }
template <typename T> inline void bxmyz(BatchT<T> x, BatchT<T> y, BatchT<T> z, size_t n, unsigned mask) {   // z = x - y
  const cvec one(z.nrhs, 1.0), mone(z.nrhs, -1.0);
  bcaxpbyz(one, x, mone, y, z, n, mask);
}
template <typename T> inline void bcxpyz(BatchT<T> x, BatchT<T> y, BatchT<T> z, size_t n, unsigned mask) {   // z = x + y
  const cvec one(z.nrhs, 1.0);
  bcaxpbyz(one, x, one, y, z, n, mask);
}

// per-system |x_k|^2; entries of frozen systems keep `fill`
template <typename T>
inline std::vector<double> bnorm2sq(BatchT<T> x, size_t n, unsigned mask, double fill = 0.0) {
  std::vector<double> raw(2 * x.nrhs, 0.0), out(x.nrhs, fill);
  ok(qmg_batch_reduce_t(dtype_of<T>::value, QMG_BRED_NORM2, x.p, 0, n, x.nrhs, x.stride, mask, raw.data(), current_stream()), "qmg_batch_reduce");
  for (int k = 0; k < x.nrhs; k++) if (is_active(mask, k)) out[k] = raw[2 * k];
  return out;
}
template <typename T>
inline std::vector<double> bdiffnorm2sq(BatchT<T> x, BatchT<T> y, size_t n, unsigned mask) {
  std::vector<double> raw(2 * x.nrhs, 0.0), out(x.nrhs, 0.0);
  ok(qmg_batch_reduce_t(dtype_of<T>::value, QMG_BRED_DIFFNORM2, x.p, y.p, n, x.nrhs, x.stride, mask, raw.data(), current_stream()), "qmg_batch_reduce");
  for (int k = 0; k < x.nrhs; k++) if (is_active(mask, k)) out[k] = raw[2 * k];
  return out;
}
// d[k][j] = <xs[j]_k, y_k>; xs: nj batches, as an array (a core's fixed one or two: `&p`, `rp`) or a vector (a basis)
template <typename T>
inline std::vector<cvec> bmultidot(const BatchT<T>* xs, int nj, BatchT<T> y, size_t n, unsigned mask) {
  std::vector<cvec> out(y.nrhs, cvec(nj, 0.0));
  int done = 0;
  while (done < nj) {   // the ABI takes up to 32 vector sets per call
    const int jj = (nj - done > 32) ? 32 : nj - done;
    std::vector<const void*> ptrs(jj);
    for (int j = 0; j < jj; j++) ptrs[j] = xs[done + j].p;
    std::vector<double> raw((size_t)2 * y.nrhs * jj, 0.0);
    ok(qmg_batch_multidot_t(dtype_of<T>::value, ptrs.data(), jj, y.p, n, y.nrhs, y.stride, mask, raw.data(), current_stream()), "qmg_batch_multidot");
    for (int k = 0; k < y.nrhs; k++)
      if (is_active(mask, k))
        for (int j = 0; j < jj; j++) out[k][done + j] = complex<double>(raw[((size_t)k * jj + j) * 2], raw[((size_t)k * jj + j) * 2 + 1]);
    done += jj;
  }
  return out;
}
template <typename T>
inline std::vector<cvec> bmultidot(const std::vector<BatchT<T> >& xs, int nj, BatchT<T> y, size_t n, unsigned mask) { return bmultidot(xs.data(), nj, y, n, mask); }
// y_k += sum_j c[k][j] xs[j]_k
template <typename T>
inline void bmulti_caxpy(const std::vector<cvec>& c, const BatchT<T>* xs, int nj, BatchT<T> y, size_t n, unsigned mask) {
  if (nj <= 0) return;
  std::vector<double> cf((size_t)2 * nj * y.nrhs, 0.0);
  std::vector<const void*> ptrs(nj);
  for (int j = 0; j < nj; j++) {
    ptrs[j] = xs[j].p;
    for (int k = 0; k < y.nrhs; k++) { cf[((size_t)j * y.nrhs + k) * 2] = c[k][j].real(); cf[((size_t)j * y.nrhs + k) * 2 + 1] = c[k][j].imag(); }
  }
  ok(qmg_batch_multi_caxpy_t(dtype_of<T>::value, cf.data(), ptrs.data(), nj, y.p, n, y.nrhs, y.stride, mask, current_stream()), "qmg_batch_multi_caxpy");
}
template <typename T>
inline void bmulti_caxpy(const std::vector<cvec>& c, const std::vector<BatchT<T> >& xs, int nj, BatchT<T> y, size_t n, unsigned mask) { bmulti_caxpy(c, xs.data(), nj, y, n, mask); }
// one flexible-GCR iteration's vector updates in one pass: w_k += sum_j c[k][j] Ws[j]_k ; r_k += a[k] w_k ; z_next_k = r_k (z_next.p != 0)
template <typename T>
inline void bgcr_update(const std::vector<cvec>& c, const std::vector<BatchT<T> >& Ws, int nj, BatchT<T> w, const cvec& a, BatchT<T> r, BatchT<T> z_next, size_t n, unsigned mask) {
  std::vector<double> cf((size_t)2 * (nj > 0 ? nj : 1) * w.nrhs, 0.0), af((size_t)2 * w.nrhs, 0.0);
  std::vector<const void*> ptrs(nj > 0 ? nj : 1, (const void*)0);
  for (int j = 0; j < nj; j++) {
    ptrs[j] = Ws[j].p;
    for (int k = 0; k < w.nrhs; k++) { cf[((size_t)j * w.nrhs + k) * 2] = c[k][j].real(); cf[((size_t)j * w.nrhs + k) * 2 + 1] = c[k][j].imag(); }
  }
  for (int k = 0; k < w.nrhs; k++) { af[2 * k] = a[k].real(); af[2 * k + 1] = a[k].imag(); }
  ok(qmg_batch_gcr_update_t(dtype_of<T>::value, nj > 0 ? cf.data() : 0, nj > 0 ? ptrs.data() : 0, nj, w.p, af.data(), r.p, z_next.p, n, w.nrhs, w.stride, mask, current_stream()),
     "qmg_batch_gcr_update");
}
// z_k = x_k across storage precisions (round / widen), active systems only
template <typename TD, typename TS>
inline void bconvert(BatchT<TD> z, BatchT<TS> x, size_t n, unsigned mask) {
  for (int k = 0; k < z.nrhs; k++)
    if (is_active(mask, k)) ok(qmg_convert(z.vec(k), dtype_of<TD>::value, x.vec(k), dtype_of<TS>::value, n, current_stream()), "qmg_convert");
}

}  // namespace qmg

// lhs_k = A rhs_k for the active systems
template <typename T> using batch_matrix_op_t = void (*)(qmg::BatchT<T> lhs, qmg::BatchT<T> rhs, unsigned mask, void* extra_data);
template <typename T> using batch_precond_op_t = void (*)(qmg::BatchT<T> lhs, qmg::BatchT<T> rhs, int size, unsigned mask, void* extra_data, inversion_verbose_struct* verb);
typedef batch_matrix_op_t<double> batch_matrix_op;
typedef batch_precond_op_t<double> batch_precond_op;

namespace qmg {
// r = b - A x for the active systems (tmp: scratch for A x), one counted operator application each; returns |r_k|^2
template <typename T>
inline std::vector<double> bresidual(BatchT<T> r, BatchT<T> x, BatchT<T> b, BatchT<T> tmp, int size, batch_matrix_op_t<T> matrix_vector, void* extra_info,
                                     unsigned mask, SolveLedger& led) {
  matrix_vector(tmp, x, mask, extra_info);
  led.count(mask);
  bxmyz(b, tmp, r, size, mask);
  return bnorm2sq(r, size, mask);
}

// the ledger of a solve of A phi = phi0 from its |b_k|^2, with x_k = 0 written for the systems whose right-hand side is zero
template <typename T>
inline SolveLedger open_ledger(BatchT<T> phi, BatchT<T> phi0, size_t n, unsigned mask, int max_iter, double eps, const std::vector<double>* eps_per_system = 0) {
  const SolveLedger led(bnorm2sq(phi0, n, mask), mask, max_iter, eps, eps_per_system);
  if (led.zero_b) bzero(phi, n, led.zero_b);
  return led;
}
// the systems of m open a solve (or a CG cycle): r = b under zero_guess, else r = b - A x (tmp: scratch); returns the active mask
template <typename T>
inline unsigned bopen(SolveLedger& led, unsigned m, BatchT<T> r, BatchT<T> x, BatchT<T> b, BatchT<T> tmp, int size, batch_matrix_op_t<T> matrix_vector,
                      void* extra_info, bool zero_guess) {
  if (!zero_guess) return led.open(m, bresidual(r, x, b, tmp, size, matrix_vector, extra_info, m, led));
  bcopy(r, b, size, m);
  return led.open(m, led.bsq);
}
// the closing line of every system of the mask, and the ledger's rows as inversion_info
inline std::vector<inversion_info> close_ledger(const SolveLedger& led, inversion_verbose_struct* verb, const char* name) {
  std::vector<inversion_info> inv(led.nrhs);
  for (int k = 0; k < led.nrhs; k++) {
    const SolveLedger::Row o = led.row(k);
    inv[k].success = o.success; inv[k].iter = o.iter; inv[k].resSq = o.resSq; inv[k].ops_count = o.ops_count; inv[k].name = name;
    if (is_active(led.mask, k)) summary(verb, name, led.nrhs, k, o.success, o.iter, led.rel(k));
  }
  return inv;
}

// a single-vector operator / preconditioner (the reference's callback types) as the operator of a batch of one system
struct MatrixOp1 { matrix_op_cplx f; void* data; };
struct PrecondOp1 { precond_op_cplx f; void* data; };
inline void matrix_op1(Batch lhs, Batch rhs, unsigned mask, void* op) {
  if (mask) ((MatrixOp1*)op)->f(lhs.p, rhs.p, ((MatrixOp1*)op)->data);
}
inline void precond_op1(Batch lhs, Batch rhs, int size, unsigned mask, void* op, inversion_verbose_struct* verb) {
  if (mask) ((PrecondOp1*)op)->f(lhs.p, rhs.p, size, ((PrecondOp1*)op)->data, verb);
}
inline inversion_info renamed(inversion_info inv, const std::string& name) { inv.name = name; return inv; }
}  // namespace qmg

// ---------------------------------------------------------------------------------------------
// MR(omega) (minv_vector_minres):  r = b - A x ; repeat: p = A r ; alpha = omega <p,r>/<p,p> ; x += alpha r ; r -= alpha p.
// `name` labels the printed lines (and inversion_info::name).  The recurrence re-anchors below 4 eps |b|.
// ---------------------------------------------------------------------------------------------
template <typename T>
inline std::vector<inversion_info> bmr_core(qmg::BatchT<T> phi, qmg::BatchT<T> phi0, int size, int max_iter, double eps, double omega,
                                            batch_matrix_op_t<T> matrix_vector, void* extra_info, unsigned mask, bool zero_guess,
                                            inversion_verbose_struct* verb = 0, const char* name = "MinRes") {
  const int nrhs = phi.nrhs;
  qmg::BatchPoolT<T> pool(phi.stride, nrhs);
  qmg::BatchT<T> r = pool.get(), p = pool.get();
  qmg::SolveLedger led = qmg::open_ledger(phi, phi0, size, mask, max_iter, eps);
  qmg::bopen(led, led.run, r, phi, phi0, p, size, matrix_vector, extra_info, zero_guess);
  const qmg::BatchT<T> rp[2] = {r, p};
  while (led.act) {
    matrix_vector(p, r, led.act, extra_info);
    led.count(led.act);
    // <r,p> and <p,p> in one pass over p; the new residual norm follows analytically:
    // |r - a p|^2 = |r|^2 - (2 omega - omega^2) |<p,r>|^2 / <p,p>   for a = omega <p,r>/<p,p>
    const std::vector<qmg::cvec> d2 = qmg::bmultidot(rp, 2, p, size, led.act);
    qmg::cvec alpha(nrhs, 0.0), malpha(nrhs, 0.0);
    unsigned upd = 0, renorm = 0;
    for (int k = 0; k < nrhs; k++) {
      if (!qmg::is_active(led.act, k)) continue;
      const complex<double> pr = std::conj(d2[k][0]);
      const double pp = d2[k][1].real();
      if (pp == 0.0) { led.breakdown(k); continue; }
      alpha[k] = omega * pr / pp; malpha[k] = -alpha[k];
      upd |= 1u << k;
      if (led.recur(k, (2.0 * omega - omega * omega) * std::norm(pr) / pp, 4.0)) renorm |= 1u << k;
    }
    qmg::bcaxpy(alpha, r, phi, size, upd);
    // r is only needed by a further iteration or by a true-norm re-anchoring: the residual update of a system's LAST
    // iteration is skipped (callers that want the residual recompute b - A x, as the K-cycle does); x and the returned |r|^2 are unaffected
    unsigned need_r = renorm;
    for (int k = 0; k < nrhs; k++) if (qmg::is_active(upd, k) && led.its[k] + 1 < max_iter) need_r |= 1u << k;
    qmg::bcaxpy(malpha, p, r, size, upd & need_r);
    if (renorm) {
      const std::vector<double> t = qmg::bnorm2sq(r, size, renorm);
      for (int k = 0; k < nrhs; k++) if (qmg::is_active(renorm, k)) led.anchor(k, t[k]);
    }
    for (int k = 0; k < nrhs; k++) {
      if (!qmg::is_active(upd, k)) continue;
      led.step(k);
      qmg::report(verb, name, nrhs, k, led.its[k], led.rel(k));
    }
    led.cap();
  }
  return qmg::close_ledger(led, verb, name);
}

// ---------------------------------------------------------------------------------------------
// BiCGStab(L) (Sleijpen & Fokkema 1993; minv_vector_bicgstab_l): the null-vector relaxation of tests/n13_wilson_kcycle/wilson_kcycle.cpp:359
// and the fine-level solver of the slab drivers.  `iter` counts BiCG steps per system; convergence and the cap are looked at
// at the end of an L-block.  The closing updates of a block go through one multi-vector pass each.
// ---------------------------------------------------------------------------------------------
template <typename T>
inline std::vector<inversion_info> bbicgstab_l_core(qmg::BatchT<T> phi, qmg::BatchT<T> phi0, int size, int max_iter, double eps, int L,
                                                    batch_matrix_op_t<T> matrix_vector, void* extra_info, unsigned mask, bool zero_guess,
                                                    inversion_verbose_struct* verb = 0, const char* name = "BiCGStab-L") {
  const int nrhs = phi.nrhs;
  qmg::BatchPoolT<T> pool(phi.stride, nrhs);
  std::vector<qmg::BatchT<T> > r(L + 1), u(L + 1);
  for (int i = 0; i <= L; i++) { r[i] = pool.get(); u[i] = pool.get(); }
  qmg::BatchT<T> rt = pool.get();
  qmg::SolveLedger led = qmg::open_ledger(phi, phi0, size, mask, max_iter, eps);
  const unsigned& act = led.act;
  qmg::bopen(led, led.run, r[0], phi, phi0, u[0], size, matrix_vector, extra_info, zero_guess);
  qmg::bcopy(rt, r[0], size, led.run);
  qmg::bzero(u[0], size, led.run);
  qmg::cvec rho0(nrhs, 1.0), alpha(nrhs, 0.0), omega(nrhs, 1.0);
  const qmg::cvec one(nrhs, 1.0);
  auto bdot1 = [&](qmg::BatchT<T> a, qmg::BatchT<T> b, unsigned m) {   // <a_k, b_k> per system
    const std::vector<qmg::cvec> d = qmg::bmultidot(&a, 1, b, size, m);
    qmg::cvec out(nrhs, 0.0);
    for (int k = 0; k < nrhs; k++) out[k] = d[k][0];
    return out;
  };
  std::vector<qmg::cvec> tau(nrhs, qmg::cvec((L + 1) * (L + 1), 0.0)), gamma(nrhs, qmg::cvec(L + 1, 0.0)), gammap(nrhs, qmg::cvec(L + 1, 0.0)),
      gammapp(nrhs, qmg::cvec(L + 1, 0.0));
  std::vector<std::vector<double> > sigma(nrhs, std::vector<double>(L + 1, 0.0));
  while (act) {
    for (int k = 0; k < nrhs; k++) if (qmg::is_active(act, k)) rho0[k] = -omega[k] * rho0[k];
    for (int j = 0; j < L && act; j++) {   // BiCG part
      const qmg::cvec rho1 = bdot1(rt, r[j], act);
      qmg::cvec mbeta(nrhs, 0.0);
      for (int k = 0; k < nrhs; k++) {
        if (!qmg::is_active(act, k)) continue;
        if (rho0[k] == 0.0) { led.breakdown(k); continue; }
        mbeta[k] = -(alpha[k] * rho1[k] / rho0[k]);
        rho0[k] = rho1[k];
      }
      if (!act) break;
      for (int i = 0; i <= j; i++) qmg::bcaxpbyz(one, r[i], mbeta, u[i], u[i], size, act);   // u_i = r_i - beta u_i
      matrix_vector(u[j + 1], u[j], act, extra_info);
      led.count(act);
      const qmg::cvec gam = bdot1(rt, u[j + 1], act);
      qmg::cvec malpha(nrhs, 0.0);
      for (int k = 0; k < nrhs; k++) {
        if (!qmg::is_active(act, k)) continue;
        if (gam[k] == 0.0) { led.breakdown(k); continue; }
        alpha[k] = rho0[k] / gam[k];
        malpha[k] = -alpha[k];
      }
      if (!act) break;
      for (int i = 0; i <= j; i++) qmg::bcaxpy(malpha, u[i + 1], r[i], size, act);
      matrix_vector(r[j + 1], r[j], act, extra_info);
      led.count(act);
      qmg::bcaxpy(alpha, u[0], phi, size, act);
      for (int k = 0; k < nrhs; k++) if (qmg::is_active(act, k)) led.its[k]++;
    }
    if (!act) break;
    for (int j = 1; j <= L && act; j++) {   // MR part: modified Gram-Schmidt on r_1..r_L
      for (int i = 1; i < j; i++) {
        const qmg::cvec d = bdot1(r[i], r[j], act);
        qmg::cvec mt(nrhs, 0.0);
        for (int k = 0; k < nrhs; k++) if (qmg::is_active(act, k)) { tau[k][i * (L + 1) + j] = d[k] / sigma[k][i]; mt[k] = -tau[k][i * (L + 1) + j]; }
        qmg::bcaxpy(mt, r[i], r[j], size, act);
      }
      const qmg::BatchT<T> two[2] = {r[j], r[0]};
      // <r_j, r_j> and <r_j, r_0> in one pass over r_j: d[k][0] = <r_j, r_j>, d[k][1] = <r_0, r_j> = conj <r_j, r_0>
      const std::vector<qmg::cvec> d = qmg::bmultidot(two, 2, r[j], size, act);
      for (int k = 0; k < nrhs; k++) {
        if (!qmg::is_active(act, k)) continue;
        sigma[k][j] = d[k][0].real();
        if (sigma[k][j] == 0.0) { led.breakdown(k); continue; }
        gammap[k][j] = std::conj(d[k][1]) / sigma[k][j];
      }
    }
    if (!act) break;
    std::vector<qmg::cvec> cx(nrhs, qmg::cvec(L, 0.0)), cr(nrhs, qmg::cvec(L, 0.0)), cu(nrhs, qmg::cvec(L, 0.0));
    for (int k = 0; k < nrhs; k++) {
      if (!qmg::is_active(act, k)) continue;
      qmg::cvec &g = gamma[k], &gp = gammap[k], &gpp = gammapp[k], &t = tau[k];
      g[L] = gp[L];
      omega[k] = g[L];
      for (int j = L - 1; j >= 1; j--) {
        g[j] = gp[j];
        for (int i = j + 1; i <= L; i++) g[j] -= t[j * (L + 1) + i] * g[i];
      }
      for (int j = 1; j < L; j++) {
        gpp[j] = g[j + 1];
        for (int i = j + 1; i < L; i++) gpp[j] += t[j * (L + 1) + i] * g[i + 1];
      }
      // x += gamma_1 r_0 + sum_{j<L} gamma''_j r_j ; r_0 -= sum_{j<=L} gamma'_j r_j ; u_0 -= sum_{j<=L} gamma_j u_j
      cx[k][0] = g[1];
      for (int j = 1; j < L; j++) cx[k][j] = gpp[j];
      for (int j = 1; j <= L; j++) { cr[k][j - 1] = -gp[j]; cu[k][j - 1] = -g[j]; }
    }
    qmg::bmulti_caxpy(cx, r.data(), L, phi, size, act);     // r_0..r_{L-1}; reads r_0 before it changes
    qmg::bmulti_caxpy(cr, r.data() + 1, L, r[0], size, act);
    qmg::bmulti_caxpy(cu, u.data() + 1, L, u[0], size, act);
    const std::vector<double> t2 = qmg::bnorm2sq(r[0], size, act);
    for (int k = 0; k < nrhs; k++) {
      if (!qmg::is_active(act, k)) continue;
      led.anchor(k, t2[k]);
      qmg::report(verb, name, nrhs, k, led.its[k], led.rel(k));
      led.settle(k);
    }
    led.cap();
  }
  return qmg::close_ledger(led, verb, name);
}


// ---------------------------------------------------------------------------------------------
// Flexible (variable-preconditioned) GCR with optional restarts (minv_vector_gcr*) -- the K-cycle's Krylov solver.
//   r = b - A x
//   loop:  z_k = M^-1 r (preconditioner; identity when precond == 0)
//          w_k = A z_k ; orthogonalise w_k against w_0..w_{k-1}
//          alpha = <w_k, r>/<w_k,w_k> ; x += alpha z'_k ; r -= alpha w_k
//   restart_freq > 0: the basis is dropped every restart_freq directions.
// The z_k are NOT orthogonalised explicitly.  With c_ik the Gram-Schmidt coefficients of w_k, the conjugate
// directions are z'_k = z_k + sum_{i<k} c_ik z'_i and x = x0 + sum_k alpha_k z'_k = x0 + sum_j y_j z_j, where y
// follows from alpha and c by a k x k back-substitution on the host (qmg::gcr_direction_weights): x is only brought
// up to date at a restart and at exit, by ONE multi-axpy.  All systems of a batch start together, so the basis index kb
// (and with it the restart points) is common; everything else is per system.
// ---------------------------------------------------------------------------------------------
template <typename T>
inline std::vector<inversion_info> bgcr_core(qmg::BatchT<T> phi, qmg::BatchT<T> phi0, int size, int max_iter, double eps, int restart_freq,
                                             batch_matrix_op_t<T> matrix_vector, void* extra_info, batch_precond_op_t<T> precond, void* precond_info,
                                             unsigned mask, bool zero_guess, inversion_verbose_struct* verb, const char* name,
                                             const std::vector<double>* eps_per_system = 0) {
  const int nrhs = phi.nrhs;
  const int basis_max = (restart_freq > 0) ? restart_freq : max_iter;
  qmg::BatchPoolT<T> pool(phi.stride, nrhs);
  qmg::BatchT<T> r = pool.get(), tmp = pool.get();
  std::vector<qmg::BatchT<T> > Z, W;        // raw search directions and orthogonalised images
  std::vector<std::vector<double> > Wnorm2;   // [basis index][system]
  std::vector<std::vector<qmg::cvec> > C(nrhs);   // C[system][k][i]: Gram-Schmidt coefficients of this cycle
  std::vector<qmg::cvec> alphas(nrhs);           // alphas[system][k]
  std::vector<int> used(nrhs, 0);                // directions system k has taken in this cycle
  auto flush_x = [&]() {                         // x_k += sum_j y_kj z_j for every system with pending directions
    int K = 0;
    unsigned m = 0;
    for (int k = 0; k < nrhs; k++) if (used[k] > 0) { m |= 1u << k; if (used[k] > K) K = used[k]; }
    if (!m) return;
    std::vector<qmg::cvec> y(nrhs, qmg::cvec(K, 0.0));
    for (int k = 0; k < nrhs; k++) {
      if (used[k] <= 0) continue;
      const qmg::cvec yk = qmg::gcr_direction_weights(alphas[k], C[k], used[k]);
      for (int j = 0; j < used[k]; j++) y[k][j] = yk[j];
      used[k] = 0;
    }
    qmg::bmulti_caxpy(y, Z, K, phi, size, m);
  };
  qmg::SolveLedger led = qmg::open_ledger(phi, phi0, size, mask, max_iter, eps, eps_per_system);   // (the K-cycle's inner tolerance depends on the system)
  const unsigned& act = led.act;
  qmg::bopen(led, led.run, r, phi, phi0, tmp, size, matrix_vector, extra_info, zero_guess);
  int kb = 0;
  bool z_ready = false;
  inversion_verbose_struct pverb(verb ? verb->precond_verbosity : VERB_NONE, verb ? verb->precond_verb_prefix : std::string(""));
  if (verb) { pverb.precond_verbosity = verb->precond_verbosity; pverb.precond_verb_prefix = verb->precond_verb_prefix; }
  while (act) {
    if (kb == (int)Z.size()) { Z.push_back(pool.get()); W.push_back(pool.get()); Wnorm2.push_back(std::vector<double>(nrhs, 0.0)); }
    for (int k = 0; k < nrhs; k++) { if ((int)C[k].size() <= kb) { C[k].push_back(qmg::cvec()); alphas[k].push_back(0.0); } }
    qmg::BatchT<T> z = Z[kb], w = W[kb];
    if (z.p == 0 || w.p == 0 || r.p == 0 || tmp.p == 0) {   // out of HBM: stop, report every active system as not converged
      std::cout << "[QMG-ERROR]: " << name << ": could not allocate basis vector " << kb << " for a batch of " << nrhs << " systems; size the batch with qmg::batch_systems_that_fit.\n";
      break;
    }
    if (precond) { qmg::bzero(z, size, act); precond(z, r, size, act, precond_info, &pverb); }
    else if (!z_ready) qmg::bcopy(z, r, size, act);   // (z_ready: the previous iteration's update pass wrote z = r already)
    z_ready = false;
    matrix_vector(w, z, act, extra_info);
    led.count(act);
    // ONE reduction pass and one host round trip per iteration: the Gram-Schmidt
    // coefficients c_i = <W_i, w>, <r, w> and <w, w> come from the same pass over the RAW w; for the orthogonalised w' = w - sum_i (c_i / N_i) W_i
    //   <w', w'> = <w, w> - sum_i |c_i|^2 / N_i          (the W_i are orthogonal)
    //   <r,  w'> = <r, w>                                (r is orthogonal to every W_i of the cycle: each step removed that component)
    // A system whose w' keeps less than 1e-6 of |w|^2 (w almost inside the span: the subtraction has lost its digits) takes the explicit dots.
    std::vector<qmg::cvec> d2(nrhs, qmg::cvec(2, 0.0));
    std::vector<qmg::BatchT<T> > basis(W.begin(), W.begin() + kb);
    basis.push_back(r); basis.push_back(w);
    std::vector<qmg::cvec> c = qmg::bmultidot(basis, kb + 2, w, size, act);
    unsigned explicit_dots = 0;
    for (int k = 0; k < nrhs; k++) {
      if (!qmg::is_active(act, k)) continue;
      double ww = c[k][kb + 1].real();
      const double ww_raw = ww;
      for (int i = 0; i < kb; i++) { ww -= std::norm(c[k][i]) / Wnorm2[i][k]; c[k][i] = -c[k][i] / Wnorm2[i][k]; }
      d2[k][0] = c[k][kb]; d2[k][1] = ww;
      if (!(ww > 1e-6 * ww_raw)) explicit_dots |= 1u << k;
      c[k].resize(kb);
      C[k][kb] = c[k];
    }
    // With these dots alpha is known BEFORE w is orthogonalised, so the Gram-Schmidt update of w, the residual update and (without a
    // preconditioner) the copy z_next = r go through ONE pass (qmg_batch_gcr_update_t: the same bits as the three separate passes).
    const bool deferred = explicit_dots == 0;
    if (!deferred && kb > 0) qmg::bmulti_caxpy(c, W, kb, w, size, act);
    if (explicit_dots) {
      const qmg::BatchT<T> rw[2] = {r, w};
      const std::vector<qmg::cvec> e2 = qmg::bmultidot(rw, 2, w, size, explicit_dots);
      for (int k = 0; k < nrhs; k++) if (qmg::is_active(explicit_dots, k)) d2[k] = e2[k];
    }
    qmg::cvec alpha(nrhs, 0.0), malpha(nrhs, 0.0);
    unsigned upd = 0, renorm = 0;
    // the true norm re-anchors the recurrence when it has lost digits and CONFIRMS a convergence the recurrence announces
    for (int k = 0; k < nrhs; k++) {
      if (!qmg::is_active(act, k)) continue;
      const double ww = d2[k][1].real();
      if (ww == 0.0) { led.breakdown(k); continue; }
      Wnorm2[kb][k] = ww;
      const complex<double> wr = std::conj(d2[k][0]);
      alpha[k] = wr / ww; malpha[k] = -alpha[k];
      alphas[k][kb] = alpha[k];
      used[k] = kb + 1;
      upd |= 1u << k;
      if (led.recur(k, std::norm(wr) / ww, 1.0)) renorm |= 1u << k;
    }
    if (deferred) {
      qmg::BatchT<T> z_next;
      if (!precond && kb + 1 < basis_max) {
        if (kb + 1 == (int)Z.size()) { Z.push_back(pool.get()); W.push_back(pool.get()); Wnorm2.push_back(std::vector<double>(nrhs, 0.0)); }
        z_next = Z[kb + 1];
      }
      qmg::bgcr_update(c, W, kb, w, malpha, r, z_next, size, upd);
      z_ready = z_next.p != 0;
    } else qmg::bcaxpy(malpha, w, r, size, upd);
    if (renorm) {
      const std::vector<double> t = qmg::bnorm2sq(r, size, renorm);
      for (int k = 0; k < nrhs; k++) if (qmg::is_active(renorm, k)) led.anchor(k, t[k]);
    }
    kb++;
    for (int k = 0; k < nrhs; k++) {
      if (!qmg::is_active(upd, k)) continue;
      led.step(k);
      qmg::report(verb, name, nrhs, k, led.its[k], led.rel(k));
    }
    if (kb == basis_max) flush_x();   // the basis is about to be reused: bring every pending x up to date (frozen systems too)
    if (act && kb == basis_max) {   // restart: true residual, drop the basis (before the iteration cap)
      const std::vector<double> t = qmg::bresidual(r, phi, phi0, tmp, size, matrix_vector, extra_info, act, led);
      kb = 0;
      z_ready = false;
      for (int k = 0; k < nrhs; k++) {
        if (!qmg::is_active(act, k)) continue;
        led.anchor(k, t[k]);
        if (verb && verb->verbosity >= VERB_RESTART_DETAIL) {
          std::cout << verb->verb_prefix << name;
          if (nrhs > 1) std::cout << " rhs " << k;
          std::cout << " restart at iter " << led.its[k] << " RelTol " << led.rel(k) << "\n";
        }
        led.settle(k);
      }
    }
    led.cap();
  }
  flush_x();
  return qmg::close_ledger(led, verb, name);
}

// ---------------------------------------------------------------------------------------------
// CG with restarts (minv_vector_cg, minv_vector_cg_restart; Hermitian positive definite operators: the coarsest solve on a
// normal-equation operator, stateful_multigrid.h:930-960).  Each cycle opens like a solve and runs at most restart_freq iterations;
// every live system starts each cycle together; a system that converges, completes a cycle without an iteration (a breakdown,
// <p, A p> == 0, at its first step) or reaches max_iter starts no other.  restart_freq <= 0: one cycle of max_iter iterations.
// zero_guess holds for the first cycle only.  The iteration lines carry the label "CG" whatever `name` is.
// ---------------------------------------------------------------------------------------------
template <typename T>
inline std::vector<inversion_info> bcg_core(qmg::BatchT<T> phi, qmg::BatchT<T> phi0, int size, int max_iter, double eps, int restart_freq,
                                            batch_matrix_op_t<T> matrix_vector, void* extra_info, unsigned mask, bool zero_guess,
                                            inversion_verbose_struct* verb, const char* name, const std::vector<double>* eps_per_system = 0) {
  const int nrhs = phi.nrhs;
  qmg::BatchPoolT<T> pool(phi.stride, nrhs);
  qmg::BatchT<T> r = pool.get(), p = pool.get(), Ap = pool.get();
  qmg::SolveLedger led = qmg::open_ledger(phi, phi0, size, mask, max_iter, eps, eps_per_system);
  const unsigned& act = led.act;
  const qmg::cvec one(nrhs, 1.0);
  unsigned live = (r.p && p.p && Ap.p) ? led.run : 0u;   // systems that may still start a cycle
  if (!live && led.run) std::cout << "[QMG-ERROR]: " << name << ": out of device memory for the CG work vectors\n";
  bool first = true;
  while (live) {
    // ---- one cycle: at most `chunk` iterations per system (chunk > 0: a live system has iterations left, or max_iter <= 0 and none opens)
    std::vector<int> chunk(nrhs, 0), done_in_cycle(nrhs, 0);
    for (int k = 0; k < nrhs; k++) {
      if (!qmg::is_active(live, k)) continue;
      const int left = max_iter - led.its[k];
      chunk[k] = (restart_freq > 0 && left > restart_freq) ? restart_freq : left;
    }
    qmg::bopen(led, live, r, phi, phi0, Ap, size, matrix_vector, extra_info, first && zero_guess);
    first = false;
    qmg::bcopy(p, r, size, live);
    while (act) {
      matrix_vector(Ap, p, act, extra_info);
      led.count(act);
      const std::vector<qmg::cvec> d = qmg::bmultidot(&p, 1, Ap, size, act);   // <p, A p>
      qmg::cvec alpha(nrhs, 0.0), malpha(nrhs, 0.0);
      unsigned upd = 0;
      for (int k = 0; k < nrhs; k++) {
        if (!qmg::is_active(act, k)) continue;
        const double pAp = d[k][0].real();
        if (pAp == 0.0) { led.breakdown(k); continue; }   // (this system's cycle ends; without an iteration in it, it starts no other)
        alpha[k] = led.rsq[k] / pAp; malpha[k] = -alpha[k];
        upd |= 1u << k;
      }
      qmg::bcaxpy(alpha, p, phi, size, upd);
      qmg::bcaxpy(malpha, Ap, r, size, upd);
      const std::vector<double> rn = qmg::bnorm2sq(r, size, upd);
      qmg::cvec beta(nrhs, 0.0);
      unsigned go_on = 0;
      for (int k = 0; k < nrhs; k++) {
        if (!qmg::is_active(upd, k)) continue;
        const double rsq_old = led.rsq[k];
        led.anchor(k, rn[k]);
        done_in_cycle[k]++;
        const bool done = led.step(k);
        qmg::report(verb, "CG", nrhs, k, led.its[k], led.rel(k));
        if (done) continue;
        beta[k] = rn[k] / rsq_old;
        if (done_in_cycle[k] >= chunk[k]) led.act &= ~(1u << k);   // the cycle's end, not the system's
        else go_on |= 1u << k;
      }
      qmg::bcaxpbyz(one, r, beta, p, p, size, go_on);   // p = r + beta p
    }
    // ---- which systems start another cycle: none on success, after a cycle without an iteration, at max_iter
    unsigned next = 0;
    for (int k = 0; k < nrhs; k++) {
      if (!qmg::is_active(live, k)) continue;
      if (restart_freq > 0 && !led.conv[k] && done_in_cycle[k] > 0 && led.its[k] < max_iter) next |= 1u << k;
    }
    live = next;
  }
  return qmg::close_ledger(led, verb, name);
}

// ---------------------------------------------------------------------------------------------
// Multi-shift CG (quantum-linalg's minv_vector_cg_m): (A + sigma_s) x[s]_k = b_k for every active system k and every shift s < S <= 16,
// A Hermitian positive definite, sigma_s >= 0 in any order, from ZERO initial guesses (the shifted residuals must stay collinear;
// a non-zero phi[s] is refused).  All S solutions are built in the Krylov space of the smallest shift sigma_0, on which the CG
// recurrence is anchored: one apply of A per iteration on the active systems, <p, A p> and <p, p> from one multidot (A0 = A +
// sigma_0 is never formed: <p, A0 p> = <p, A p> + sigma_0 <p, p>, and r -= alpha (A p + sigma_0 p) is one two-vector axpy), |r|^2,
// the scalars of every shift from cgm_coefficients, and ONE qmg_batch_cgm_update_t for the 2 S vector updates.
// Shift s of system k is frozen (leaves shift_masks[s]: neither read nor written again) when zeta_s |r_k| < eps |b_k|; that is the
// recurrence residual of the shifted system, known from host scalars, so every shift is checked every iteration.  A system leaves
// the mask when its smallest shift has converged (the larger ones have by then: zeta_s <= 1), at breakdown (<p, A0 p> == 0) or at
// max_iter.  Returns inv[k * S + s]: iter = the iteration at which the shift froze, ops_count = the system's applies so far,
// resSq = zeta_s^2 |r_k|^2.  phi[s]: the batch of solutions of shift s.
// ---------------------------------------------------------------------------------------------
template <typename T>
inline std::vector<inversion_info> bcg_m_core(const std::vector<qmg::BatchT<T> >& phi, qmg::BatchT<T> phi0, int size, int max_iter, double eps,
                                              const std::vector<double>& shifts, batch_matrix_op_t<T> matrix_vector, void* extra_info, unsigned mask,
                                              inversion_verbose_struct* verb, const char* name = "CG-M") {
  const int nrhs = phi0.nrhs, S = (int)shifts.size();
  std::vector<inversion_info> inv((size_t)nrhs * (S > 0 ? S : 0));
  for (auto& i : inv) i.name = name;
  if (S < 1 || S > 16 || (int)phi.size() != S) { std::cout << "[QMG-ERROR]: " << name << ": takes 1 to 16 shifts and one solution batch per shift\n"; return inv; }
  for (int s = 0; s < S; s++)
    if (!phi[s].p || phi[s].stride != phi0.stride || phi[s].nrhs != nrhs) { std::cout << "[QMG-ERROR]: " << name << ": solution batch " << s << " does not have the layout of the right-hand sides\n"; return inv; }
  int base = 0;
  for (int s = 1; s < S; s++) if (shifts[s] < shifts[base]) base = s;
  std::vector<double> dsigma(S);
  for (int s = 0; s < S; s++) dsigma[s] = shifts[s] - shifts[base];
  const double sigma0 = shifts[base];
  if (sigma0 < 0.0) { std::cout << "[QMG-ERROR]: " << name << ": negative shift " << sigma0 << "\n"; return inv; }
  for (int s = 0; s < S; s++) {
    const std::vector<double> g = qmg::bnorm2sq(phi[s], size, mask);
    for (int k = 0; k < nrhs; k++)
      if (qmg::is_active(mask, k) && g[k] != 0.0) {
        std::cout << "[QMG-ERROR]: " << name << ": non-zero initial guess (shift " << s << ", rhs " << k << "): multi-shift CG starts from zero\n";
        return inv;
      }
  }
  qmg::BatchPoolT<T> pool(phi0.stride, nrhs);
  qmg::BatchT<T> r = pool.get(), Ap = pool.get();
  std::vector<qmg::BatchT<T> > ps(S);
  bool have = r.p && Ap.p;
  for (int s = 0; s < S; s++) { ps[s] = pool.get(); have = have && ps[s].p; }
  // the ledger's |b|, rsq, iter, ops and system-level mask; the shifts' freezing by zeta, and with it success and resSq, is this core's own
  qmg::SolveLedger led(qmg::bnorm2sq(phi0, size, mask), mask, max_iter, eps);
  const unsigned& act = led.act;
  std::vector<double>&rsq = led.rsq, &bnorm = led.bnorm;
  std::vector<double> alpha_prev(nrhs, 1.0), beta_prev(nrhs, 0.0);
  std::vector<std::vector<double> > zeta(nrhs, std::vector<double>(S, 1.0)), zeta_prev(zeta);
  std::vector<unsigned> live(nrhs, 0u);            // per system: the shifts it still iterates
  std::vector<unsigned> shift_masks(S, 0u);        // per shift: the systems that still iterate it (the kernel's view of `live`)
  if (!have && mask) std::cout << "[QMG-ERROR]: " << name << ": out of device memory for the CG work vectors\n";
  if (have && max_iter > 0) led.act = led.run;
  for (int k = 0; k < nrhs; k++) {
    if (!qmg::is_active(mask, k)) continue;
    for (int s = 0; s < S; s++) { inv[(size_t)k * S + s].success = (bnorm[k] == 0.0); inv[(size_t)k * S + s].resSq = led.bsq[k]; }
    if (qmg::is_active(act, k)) live[k] = qmg::full_mask(S);
  }
  if (act) {
    qmg::bcopy(r, phi0, size, act);
    for (int s = 0; s < S; s++) qmg::bcopy(ps[s], phi0, size, act);
  }
  const qmg::BatchT<T> Ap_p[2] = {Ap, ps[base]};
  std::vector<const void*> xtab(S), ptab(S);
  for (int s = 0; s < S; s++) { xtab[s] = phi[s].p; ptab[s] = ps[s].p; }
  std::vector<double> a((size_t)S * nrhs), z((size_t)S * nrhs), c((size_t)S * nrhs), as(S), zs(S), cs(S);
  while (act) {
    matrix_vector(Ap, ps[base], act, extra_info);
    led.count(act);
    const std::vector<qmg::cvec> d = qmg::bmultidot(Ap_p, sigma0 != 0.0 ? 2 : 1, ps[base], size, act);   // <A p, p> (, <p, p>)
    std::vector<double> alpha(nrhs, 0.0);
    std::vector<qmg::cvec> rc(nrhs, qmg::cvec(2, 0.0));
    unsigned upd = 0;
    for (int k = 0; k < nrhs; k++) {
      if (!qmg::is_active(act, k)) continue;
      const double pAp = d[k][0].real() + (sigma0 != 0.0 ? sigma0 * d[k][1].real() : 0.0);
      if (pAp == 0.0) { led.breakdown(k); continue; }
      alpha[k] = rsq[k] / pAp;
      rc[k][0] = -alpha[k]; rc[k][1] = -alpha[k] * sigma0;
      upd |= 1u << k;
    }
    qmg::bmulti_caxpy(rc, Ap_p, sigma0 != 0.0 ? 2 : 1, r, size, upd);   // r -= alpha (A p + sigma_0 p)
    const std::vector<double> rn = qmg::bnorm2sq(r, size, upd);
    std::fill(a.begin(), a.end(), 0.0); std::fill(z.begin(), z.end(), 0.0); std::fill(c.begin(), c.end(), 0.0);
    std::fill(shift_masks.begin(), shift_masks.end(), 0u);
    for (int k = 0; k < nrhs; k++) {
      if (!qmg::is_active(upd, k)) continue;
      const double beta = rn[k] / rsq[k];
      qmg::cgm_coefficients(S, dsigma.data(), live[k], alpha[k], beta, alpha_prev[k], beta_prev[k], zeta[k].data(), zeta_prev[k].data(), as.data(), zs.data(), cs.data());
      for (int s = 0; s < S; s++) {
        if (!((live[k] >> s) & 1u)) continue;
        a[(size_t)s * nrhs + k] = as[s]; z[(size_t)s * nrhs + k] = zs[s]; c[(size_t)s * nrhs + k] = cs[s];
        shift_masks[s] |= 1u << k;
      }
      alpha_prev[k] = alpha[k]; beta_prev[k] = beta; rsq[k] = rn[k];
    }
    if (upd)
      qmg::ok(qmg_batch_cgm_update_t(qmg::dtype_of<T>::value, xtab.data(), ptab.data(), S, a.data(), z.data(), c.data(), shift_masks.data(), r.p, size, nrhs,
                                     r.stride, upd, qmg::current_stream()), "qmg_batch_cgm_update");
    for (int k = 0; k < nrhs; k++) {
      if (!qmg::is_active(upd, k)) continue;
      led.its[k]++;
      const double rnorm = std::sqrt(rsq[k]);
      qmg::report(verb, name, nrhs, k, led.its[k], rnorm / bnorm[k]);
      for (int s = 0; s < S; s++) {
        if (!((live[k] >> s) & 1u)) continue;
        inversion_info& o = inv[(size_t)k * S + s];
        o.iter = led.its[k]; o.resSq = zeta[k][s] * zeta[k][s] * rsq[k];
        if (std::fabs(zeta[k][s]) * rnorm < eps * bnorm[k]) { o.success = true; live[k] &= ~(1u << s); }
      }
      if (!((live[k] >> base) & 1u)) led.act &= ~(1u << k);   // the smallest shift has converged, the others before it (success is per shift)
    }
    led.cap();
  }
  for (int k = 0; k < nrhs; k++) {
    if (!qmg::is_active(mask, k)) continue;
    for (int s = 0; s < S; s++) {
      inversion_info& o = inv[(size_t)k * S + s];
      o.ops_count = led.ops[k];
      if (verb && verb->verbosity != VERB_NONE) {
        std::cout << verb->verb_prefix << name;
        if (nrhs > 1) std::cout << " rhs " << k;
        std::cout << " shift " << s << (o.success ? " Success " : " Fail ") << "Iter " << o.iter << " RelTol " << (bnorm[k] > 0 ? std::sqrt(o.resSq) / bnorm[k] : 0.0) << "\n";
      }
    }
  }
  return inv;
}

// ---------------------------------------------------------------------------------------------
// The reference-named single-vector entry points: the cores above on a batch of one system, from the
// initial guess in phi.  The opening r = b - A x0 counts in ops_count; the printed lines carry no system index.
// ---------------------------------------------------------------------------------------------
inline inversion_info minv_vector_minres(complex<double>* phi, complex<double>* phi0, int size, int max_iter, double eps, double omega,
                                         matrix_op_cplx matrix_vector, void* extra_info, inversion_verbose_struct* verb = 0) {
  qmg::MatrixOp1 a = {matrix_vector, extra_info};
  return qmg::renamed(bmr_core<double>(qmg::Batch(phi, size, 1), qmg::Batch(phi0, size, 1), size, max_iter, eps, omega, qmg::matrix_op1, &a, 1u, false, verb)[0],
                      "MinRes (relaxation parameter " + std::to_string(omega) + ")");
}
inline inversion_info minv_vector_cg(complex<double>* phi, complex<double>* phi0, int size, int max_iter, double eps, matrix_op_cplx matrix_vector,
                                     void* extra_info, inversion_verbose_struct* verb = 0) {
  qmg::MatrixOp1 a = {matrix_vector, extra_info};
  return bcg_core<double>(qmg::Batch(phi, size, 1), qmg::Batch(phi0, size, 1), size, max_iter, eps, -1, qmg::matrix_op1, &a, 1u, false, verb, "CG")[0];
}
inline inversion_info minv_vector_cg_restart(complex<double>* phi, complex<double>* phi0, int size, int max_iter, double eps, int restart_freq,
                                             matrix_op_cplx matrix_vector, void* extra_info, inversion_verbose_struct* verb = 0) {
  qmg::MatrixOp1 a = {matrix_vector, extra_info};
  return qmg::renamed(bcg_core<double>(qmg::Batch(phi, size, 1), qmg::Batch(phi0, size, 1), size, max_iter, eps, restart_freq, qmg::matrix_op1, &a, 1u, false, verb, "CG-restart")[0],
                      "Restarted CG(" + std::to_string(restart_freq) + ")");
}
inline inversion_info minv_vector_gcr(complex<double>* phi, complex<double>* phi0, int size, int max_iter, double eps, matrix_op_cplx op, void* opd,
                                      inversion_verbose_struct* verb = 0) {
  qmg::MatrixOp1 a = {op, opd};
  return bgcr_core<double>(qmg::Batch(phi, size, 1), qmg::Batch(phi0, size, 1), size, max_iter, eps, -1, qmg::matrix_op1, &a, 0, 0, 1u, false, verb, "GCR")[0];
}
inline inversion_info minv_vector_gcr_restart(complex<double>* phi, complex<double>* phi0, int size, int max_iter, double eps, int restart_freq,
                                              matrix_op_cplx op, void* opd, inversion_verbose_struct* verb = 0) {
  qmg::MatrixOp1 a = {op, opd};
  return bgcr_core<double>(qmg::Batch(phi, size, 1), qmg::Batch(phi0, size, 1), size, max_iter, eps, restart_freq, qmg::matrix_op1, &a, 0, 0, 1u, false, verb, "GCR-restart")[0];
}
inline inversion_info minv_vector_gcr_var_precond(complex<double>* phi, complex<double>* phi0, int size, int max_iter, double eps, matrix_op_cplx op,
                                                  void* opd, precond_op_cplx precond, void* precd, inversion_verbose_struct* verb = 0) {
  qmg::MatrixOp1 a = {op, opd};
  qmg::PrecondOp1 m = {precond, precd};
  return bgcr_core<double>(qmg::Batch(phi, size, 1), qmg::Batch(phi0, size, 1), size, max_iter, eps, -1, qmg::matrix_op1, &a, precond ? qmg::precond_op1 : 0, &m, 1u, false, verb, "VPGCR")[0];
}
inline inversion_info minv_vector_gcr_var_precond_restart(complex<double>* phi, complex<double>* phi0, int size, int max_iter, double eps,
                                                          int restart_freq, matrix_op_cplx op, void* opd, precond_op_cplx precond, void* precd,
                                                          inversion_verbose_struct* verb = 0) {
  qmg::MatrixOp1 a = {op, opd};
  qmg::PrecondOp1 m = {precond, precd};
  return bgcr_core<double>(qmg::Batch(phi, size, 1), qmg::Batch(phi0, size, 1), size, max_iter, eps, restart_freq, qmg::matrix_op1, &a, precond ? qmg::precond_op1 : 0, &m, 1u, false, verb,
                           "VPGCR-restart")[0];
}
// Multi-shift CG on one right-hand side: phi[s] = (A + shifts[s])^-1 phi0 for s < n_shift, every phi[s] zero on entry.  Argument order as
// quantum-linalg's minv_vector_cg_m is recalled (PARITY UNPINNED like the rest: neither the library nor a call site is in the reference tree).
// resid_freq_check and worst_first have no effect here: every shift's recurrence residual is checked in every iteration (host
// scalars only), and the recurrence is always anchored on the smallest shift.  Returns one inversion_info per shift.
inline std::vector<inversion_info> minv_vector_cg_m(complex<double>** phi, complex<double>* phi0, int n_shift, int size, int resid_freq_check, int max_iter,
                                                    double eps, double* shifts, matrix_op_cplx matrix_vector, void* extra_info, bool worst_first = false,
                                                    inversion_verbose_struct* verb = 0) {
  (void)resid_freq_check; (void)worst_first;
  qmg::MatrixOp1 a = {matrix_vector, extra_info};
  std::vector<qmg::Batch> x;
  for (int s = 0; s < n_shift; s++) x.push_back(qmg::Batch(phi[s], size, 1));
  return bcg_m_core<double>(x, qmg::Batch(phi0, size, 1), size, max_iter, eps, std::vector<double>(shifts, shifts + (n_shift > 0 ? n_shift : 0)), qmg::matrix_op1, &a, 1u, verb);
}
// `iter` counts BiCG steps
inline inversion_info minv_vector_bicgstab_l(complex<double>* phi, complex<double>* phi0, int size, int max_iter, double eps, int L,
                                             matrix_op_cplx matrix_vector, void* extra_info, inversion_verbose_struct* verb = 0) {
  qmg::MatrixOp1 a = {matrix_vector, extra_info};
  return qmg::renamed(bbicgstab_l_core<double>(qmg::Batch(phi, size, 1), qmg::Batch(phi0, size, 1), size, max_iter, eps, L, qmg::matrix_op1, &a, 1u, false, verb)[0],
                      "BiCGStab-" + std::to_string(L));
}

// ---------------------------------------------------------------------------------------------
// Richardson relaxation (null-vector generation, tests/n22...:289):
//   minv_vector_richardson(x, b, n, max_iter, tol, omega, check_freq, op, opdata)
//   x += omega (b - A x); the residual norm is only evaluated every check_freq iterations.
// ---------------------------------------------------------------------------------------------
inline inversion_info minv_vector_richardson(complex<double>* phi, complex<double>* phi0, int size, int max_iter, double eps, double omega,
                                             int check_freq, matrix_op_cplx matrix_vector, void* extra_info, inversion_verbose_struct* verb = 0) {
  inversion_info invif;
  invif.name = "Richardson";
  qmg::VecPool pool(size);
  complex<double>*r = pool.get(), *Ax = pool.get();
  const double bnorm = std::sqrt(norm2sq(phi0, size));
  int ops = 0, k = 0;
  double rsq = 0.0;
  bool conv = false;
  if (bnorm == 0.0) {   // A x = 0: x = 0 whatever the guess was, as in the batch cores
    zero_vector(phi, size);
    invif.success = true;
    qmg::summary(verb, "Richardson", 1, 0, true, 0, 0.0);
    return invif;
  }
  while (k < max_iter) {
    matrix_vector(Ax, phi, extra_info); ops++;
    caxpbyz(1.0, phi0, -1.0, Ax, r, size);
    if (check_freq > 0 && (k % check_freq) == 0) {
      rsq = norm2sq(r, size);
      if (bnorm == 0.0 || std::sqrt(rsq) < eps * bnorm) { conv = true; break; }
    }
    caxpy(omega, r, phi, size);
    k++;
  }
  if (!conv) {
    matrix_vector(Ax, phi, extra_info); ops++;
    rsq = diffnorm2sq(phi0, Ax, size);
    conv = (bnorm == 0.0) || (std::sqrt(rsq) < eps * bnorm);
  }
  invif.success = conv; invif.iter = k; invif.resSq = rsq; invif.ops_count = ops;
  qmg::summary(verb, "Richardson", 1, 0, conv, k, bnorm > 0 ? std::sqrt(rsq) / bnorm : 0.0);
  return invif;
}

#endif  // QMG_KRYLOV_HOST_ONLY
#endif
