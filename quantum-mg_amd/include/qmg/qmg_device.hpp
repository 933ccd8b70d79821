// qmg_device.hpp -- host-side C++ layer over the C-ABI (include/qmg_hip.h).
//
// The reference's arithmetic leaves come from quantum-linalg (`blas/generic_vector.h`, absent from
// the reference tree; call sites listed in SURVEY 2.2).  This header provides the leaves the
// multigrid hot path calls, under the SAME NAMES and argument order, operating on DEVICE pointers
// and implemented by libqmg_hip.so kernels.  There is no host fallback: every function forwards
// to the GPU library and reports failures the way the reference does ([QMG-ERROR] on std::cout).
#ifndef QMG_DEVICE_HPP
#define QMG_DEVICE_HPP

#include <cmath>
#include <complex>
#include <cstddef>
#include <cstdlib>
#include <ctime>
#include <iostream>
#include <string>
#include <vector>

#include "../../../include/qmg_hip.h"

using std::complex;

namespace qmg {

inline bool ok(int status, const char* what) {
  if (status != QMG_SUCCESS) {
    std::cout << "[QMG-ERROR]: " << what << " failed: " << qmg_status_string(status) << " (" << qmg_last_hip_error() << ")\n";
    return false;
  }
  return true;
}

// Current stream for all facade launches (NULL stream by default; one stream per host thread is enough
// because the reference's objects are not re-entrant either, stateful_multigrid.h:50).
inline void*& current_stream() {
  static thread_local void* s = nullptr;
  return s;
}

// ---- y-slab mode of this host thread ----
// Off: every Lattice2D is a whole periodic lattice (the reference's semantics).  On: every Lattice2D of this thread is the
// slab [rank Ly, (rank + 1) Ly) of a lattice with world x Ly rows; operator applies exchange halo rows with the neighbouring
// ranks (Stencil2D::launch), the Galerkin build exchanges the null vectors' halo rows (CoarseOperator2D), reductions are
// summed over the ranks inside the library, and gaussian_lattice draws the slab's rows of the single-domain vector.
// Everything else (BLAS-1, transfer, block orthonormalisation, the solvers) is slab-local and unchanged.
struct SlabContext { bool on; int world, rank; };
inline SlabContext& slab() { static thread_local SlabContext c = {false, 1, 0}; return c; }
inline bool slab_begin() {   // after qmg_comm_init_env (or qmg_comm_emulate_attach)
  int w = 1, r = 0;
  if (!ok(qmg_comm_world(&w, &r), "qmg_comm_world")) return false;
  slab() = {true, w, r};
  return ok(qmg_comm_set_distributed_reductions(1), "qmg_comm_set_distributed_reductions");
}
inline void slab_end() { slab() = {false, 1, 0}; qmg_comm_set_distributed_reductions(0); }

// A slab apply with its halo exchange hidden behind the interior rows (Stencil2D::launch, SlabWilson2D::apply): the exchange on a second stream,
// behind the producer of the right-hand side; the interior rows (1) meanwhile on the current stream; the boundary rows (2) after both.  Owns the
// stream and the two events, made on first use.  exchange(stream) and rows(which) return false to stop.  The next exchange overwrites the halos:
// it is ordered behind this boundary launch through ev_rhs of the next run.
struct HaloOverlap {
  void *comm_stream, *ev_rhs, *ev_halo;
  HaloOverlap() : comm_stream(0), ev_rhs(0), ev_halo(0) {}
  ~HaloOverlap() {
    if (comm_stream) { qmg_stream_sync(comm_stream); qmg_event_destroy(ev_rhs); qmg_event_destroy(ev_halo); qmg_stream_destroy(comm_stream); }
  }
  bool ready() {
    if (!comm_stream && (qmg_stream_create(&comm_stream) != QMG_SUCCESS || qmg_event_create(&ev_rhs) != QMG_SUCCESS || qmg_event_create(&ev_halo) != QMG_SUCCESS))
      comm_stream = 0;
    return comm_stream != 0;
  }
  template <typename Exchange, typename Rows>
  void run(Exchange exchange, Rows rows) {
    void* st = current_stream();
    ok(qmg_event_record(ev_rhs, st), "qmg_event_record");
    ok(qmg_stream_wait_event(comm_stream, ev_rhs), "qmg_stream_wait_event");
    if (!exchange(comm_stream)) return;
    ok(qmg_event_record(ev_halo, comm_stream), "qmg_event_record");
    if (!rows(1)) return;
    ok(qmg_stream_wait_event(st, ev_halo), "qmg_stream_wait_event");
    rows(2);
  }
 private:
  HaloOverlap(const HaloOverlap&);
  HaloOverlap& operator=(const HaloOverlap&);
};

// ---- staging helpers (host <-> device); the reference has no such step, tests index arrays directly ----
template <typename T> inline void upload(T* dev, const T* host, size_t n) { ok(qmg_memcpy_h2d(dev, host, n * sizeof(T), nullptr), "qmg_memcpy_h2d"); }
template <typename T> inline void download(T* host, const T* dev, size_t n) {
  ok(qmg_stream_sync(current_stream()), "qmg_stream_sync");
  ok(qmg_memcpy_d2h(host, dev, n * sizeof(T), nullptr), "qmg_memcpy_d2h");
}
template <typename T> inline T get_element(const T* dev, size_t i) { T v; download(&v, dev + i, 1); return v; }
template <typename T> inline void set_element(T* dev, size_t i, T v) { upload(dev + i, &v, 1); }
template <typename T> inline std::vector<T> to_host(const T* dev, size_t n) { std::vector<T> h(n); download(h.data(), dev, n); return h; }

}  // namespace qmg

// ======================= quantum-linalg names, device semantics =======================

namespace qmg {
// how much wall time this thread has spent inside the device allocator (hipMalloc / hipFree synchronise and, for GB-sized buffers, are not
// cheap): the drivers print it beside their solve times so that an allocation inside a timed region shows as what it is
struct AllocStats { double seconds; long mallocs, frees; };
inline AllocStats& alloc_stats() { static thread_local AllocStats s = {0.0, 0, 0}; return s; }
inline double wall_now() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; }
}  // namespace qmg
template <typename T> inline T* allocate_vector(size_t n) {
  void* p = nullptr;
  const double t0 = qmg::wall_now();
  const bool good = qmg::ok(qmg_malloc(&p, n * sizeof(T)), "allocate_vector");
  qmg::alloc_stats().seconds += qmg::wall_now() - t0; qmg::alloc_stats().mallocs++;
  return good ? static_cast<T*>(p) : nullptr;
}
template <typename T> inline void deallocate_vector(T** p) {
  if (p && *p) {
    const double t0 = qmg::wall_now();
    qmg_free(*p); *p = nullptr;
    qmg::alloc_stats().seconds += qmg::wall_now() - t0; qmg::alloc_stats().frees++;
  }
}

typedef complex<double> qmg_c;

inline void zero_vector(qmg_c* x, size_t n) { qmg::ok(qmg_zero_vector(x, n, qmg::current_stream()), "zero_vector"); }
inline void copy_vector(qmg_c* dst, const qmg_c* src, size_t n) { qmg::ok(qmg_copy_vector(dst, src, n, qmg::current_stream()), "copy_vector"); }
inline void cax(qmg_c a, qmg_c* x, size_t n) { qmg::ok(qmg_cax(a.real(), a.imag(), x, n, qmg::current_stream()), "cax"); }
inline void caxy(qmg_c a, const qmg_c* x, qmg_c* y, size_t n) { qmg::ok(qmg_caxy(a.real(), a.imag(), x, y, n, qmg::current_stream()), "caxy"); }
inline void caxpy(qmg_c a, const qmg_c* x, qmg_c* y, size_t n) { qmg::ok(qmg_caxpy(a.real(), a.imag(), x, y, n, qmg::current_stream()), "caxpy"); }
inline void cxpy(const qmg_c* x, qmg_c* y, size_t n) { qmg::ok(qmg_cxpy(x, y, n, qmg::current_stream()), "cxpy"); }
inline void cxpay(const qmg_c* x, qmg_c a, qmg_c* y, size_t n) { qmg::ok(qmg_cxpay(x, a.real(), a.imag(), y, n, qmg::current_stream()), "cxpay"); }
inline void caxpby(qmg_c a, const qmg_c* x, qmg_c b, qmg_c* y, size_t n) {
  qmg::ok(qmg_caxpby(a.real(), a.imag(), x, b.real(), b.imag(), y, n, qmg::current_stream()), "caxpby");
}
inline void cxpyz(const qmg_c* x, const qmg_c* y, qmg_c* z, size_t n) { qmg::ok(qmg_cxpyz(x, y, z, n, qmg::current_stream()), "cxpyz"); }
inline void caxpbyz(qmg_c a, const qmg_c* x, qmg_c b, const qmg_c* y, qmg_c* z, size_t n) {
  qmg::ok(qmg_caxpbyz(a.real(), a.imag(), x, b.real(), b.imag(), y, z, n, qmg::current_stream()), "caxpbyz");
}

// global reductions: result returned to the host (the Krylov drivers branch on it)
inline double norm2sq(const qmg_c* x, size_t n) { double r = 0; qmg::ok(qmg_norm2sq(x, n, nullptr, &r, qmg::current_stream()), "norm2sq"); return r; }
inline qmg_c dot(const qmg_c* x, const qmg_c* y, size_t n) {
  double r[2] = {0, 0};
  qmg::ok(qmg_dot(x, y, n, nullptr, r, qmg::current_stream()), "dot");
  return qmg_c(r[0], r[1]);
}
inline double diffnorm2sq(const qmg_c* x, const qmg_c* y, size_t n) { double r = 0; qmg::ok(qmg_diffnorm2sq(x, y, n, nullptr, &r, qmg::current_stream()), "diffnorm2sq"); return r; }
inline double norminf(const qmg_c* x, size_t n) { double r = 0; qmg::ok(qmg_norminf(x, n, nullptr, &r, qmg::current_stream()), "norminf"); return r; }

// orthogonal(v, w, n): v -= (<w,v>/<w,w>) w ; normalize(v, n): v /= ||v||   (null-vector preparation, tests/n13...:330-372)
inline void orthogonal(qmg_c* v, const qmg_c* w, size_t n) {
  const double ww = norm2sq(w, n);
  if (ww == 0.0) return;
  caxpy(-dot(w, v, n) / ww, w, v, n);
}
inline void normalize(qmg_c* v, size_t n) {
  const double nrm = std::sqrt(norm2sq(v, n));
  if (nrm > 0.0) cax(1.0 / nrm, v, n);
}

// Gaussian fill.  The reference draws from std::mt19937 + std::normal_distribution on the host
// (not portable across standard libraries); here a counter-based device generator keyed
// by `seed` -- same distribution, different stream of numbers.
inline void gaussian(qmg_c* x, size_t n, unsigned long long seed) { qmg::ok(qmg_gaussian(x, n, seed, qmg::current_stream()), "gaussian"); }
// a Gaussian vector on a lattice (Lx x Ly rows held here, nc per site): in y-slab mode the slab's rows of the vector the
// single-domain run draws with the same seed -- a decomposed run then works on the very same vectors
inline void gaussian_lattice(qmg_c* x, int Lx, int Ly, int nc, unsigned long long seed) {
  if (qmg::slab().on)
    qmg::ok(qmg_gaussian_slab(x, Lx, Ly * qmg::slab().world, qmg::slab().rank * Ly, Ly, nc, seed, qmg::current_stream()), "qmg_gaussian_slab");
  else
    qmg::ok(qmg_gaussian(x, (size_t)Lx * Ly * nc, seed, qmg::current_stream()), "gaussian");
}

// ---- verbosity / result structs of quantum-linalg (fields as used at stateful_multigrid.h:762-776, n13:125-132,464-466) ----
enum inversion_verbose_level { VERB_NONE = 0, VERB_SUMMARY = 1, VERB_RESTART_DETAIL = 2, VERB_DETAIL = 3 };

struct inversion_verbose_struct {
  inversion_verbose_level verbosity;
  std::string verb_prefix;
  inversion_verbose_level precond_verbosity;
  std::string precond_verb_prefix;
  inversion_verbose_struct(inversion_verbose_level v = VERB_NONE, std::string prefix = "")
      : verbosity(v), verb_prefix(prefix), precond_verbosity(VERB_NONE), precond_verb_prefix("") {}
};

struct inversion_info {
  bool success;
  int iter;
  double resSq;
  std::string name;
  int ops_count;
  inversion_info() : success(false), iter(0), resSq(0.0), name(""), ops_count(0) {}
};

#ifndef QLINALG_FCN_POINTER
#define QLINALG_FCN_POINTER
typedef void (*matrix_op_real)(double*, double*, void*);
typedef void (*matrix_op_cplx)(complex<double>*, complex<double>*, void*);
#endif
typedef void (*precond_op_cplx)(complex<double>*, complex<double>*, int, void*, inversion_verbose_struct*);

#endif
