// qmg_common.h -- shared device helpers for the gfx950 kernels of libqmg_hip.so.
#ifndef QMG_COMMON_H
#define QMG_COMMON_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/qmg_hip.h"

namespace qmg {

typedef double2 cplx;   // (x = re, y = im): one 16-byte global_load_dwordx4 / global_store_dwordx4

constexpr int WAVE = 64;          // CDNA4 wavefront
constexpr int BLOCK = 256;        // 4 waves = one per SIMD

// last HIP error text, for qmg_last_hip_error()
void set_hip_error(hipError_t e, const char* where);

#define QMG_HIP_CHECK(expr)                                  \
  do {                                                       \
    hipError_t _e = (expr);                                  \
    if (_e != hipSuccess) {                                  \
      ::qmg::set_hip_error(_e, #expr);                       \
      return QMG_ERR_HIP;                                    \
    }                                                        \
  } while (0)

#define QMG_LAUNCH_CHECK()                                   \
  do {                                                       \
    hipError_t _e = hipGetLastError();                       \
    if (_e != hipSuccess) {                                  \
      ::qmg::set_hip_error(_e, "kernel launch");             \
      return QMG_ERR_HIP;                                    \
    }                                                        \
  } while (0)

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

inline bool valid_lattice(int Lx, int Ly) { return Lx >= 2 && Ly >= 2 && !(Lx & 1) && !(Ly & 1); }

struct SlabHalo { const void* lo; const void* hi; long stride; int rows; };   // y-slab halos (qmg_stencil_apply_slab)
int generic_slab_apply(const qmg_stencil_desc* d, void* lhs, const void* rhs, unsigned pieces, int n, long vec_stride, const unsigned char* ridx,
                       hipStream_t st, const SlabHalo* slab, int mat32, int vec32);   // qmg_stencil_apply.hip: kernels B / B32 / C with halos (any nc; f32: complex<float> matrices and vectors)

// qmg_comm.hip: reductions of y-slab vectors are summed over the ranks (qmg_comm_set_distributed_reductions)
bool dist_reductions_on();
int dist_allreduce(double* buf_dev, int n, bool op_max, hipStream_t st);

// ---------------- complex arithmetic (explicit FMAs; 8 flop per MAC) ----------------
__device__ __forceinline__ cplx cmake(double re, double im) { return make_double2(re, im); }
__device__ __forceinline__ cplx cadd(cplx a, cplx b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ cplx csub(cplx a, cplx b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ cplx cconj(cplx a) { return make_double2(a.x, -a.y); }
__device__ __forceinline__ cplx cmul(cplx a, cplx b) {
  return make_double2(fma(a.x, b.x, -a.y * b.y), fma(a.x, b.y, a.y * b.x));
}
// acc += a*b
__device__ __forceinline__ void cmac(cplx& acc, cplx a, cplx b) {
  acc.x = fma(a.x, b.x, acc.x);
  acc.x = fma(-a.y, b.y, acc.x);
  acc.y = fma(a.x, b.y, acc.y);
  acc.y = fma(a.y, b.x, acc.y);
}
// acc += conj(a)*b
__device__ __forceinline__ void cmac_conj(cplx& acc, cplx a, cplx b) {
  acc.x = fma(a.x, b.x, acc.x);
  acc.x = fma(a.y, b.y, acc.x);
  acc.y = fma(a.x, b.y, acc.y);
  acc.y = fma(-a.y, b.x, acc.y);
}

// ---------------- cross-lane moves on doubles (DPP; no LDS traffic) ----------------
template <int CTRL>
__device__ __forceinline__ double dpp_move(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_mov_dpp(lo, CTRL, 0xF, 0xF, true);
  hi = __builtin_amdgcn_mov_dpp(hi, CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
// quad_perm:[1,0,3,2] -> lane ^ 1 ; quad_perm:[2,3,0,1] -> lane ^ 2
__device__ __forceinline__ double lane_xor1(double v) { return dpp_move<0xB1>(v); }
__device__ __forceinline__ double lane_xor2(double v) { return dpp_move<0x4E>(v); }

// Full 64-lane sum; every lane gets the total. (ds_swizzle/bpermute-free: row_shr + bcast is
// order-dependent, so use the butterfly via __shfl_xor for the cross-row steps.)
__device__ __forceinline__ double wave_sum(double v) {
  v += lane_xor1(v);
  v += lane_xor2(v);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
  v = fmax(v, lane_xor1(v));
  v = fmax(v, lane_xor2(v));
  v = fmax(v, __shfl_xor(v, 4));
  v = fmax(v, __shfl_xor(v, 8));
  v = fmax(v, __shfl_xor(v, 16));
  v = fmax(v, __shfl_xor(v, 32));
  return v;
}

// NV (a power of two) sums or maxima at once, by recursive halving: lane q < NV returns what wave_sum(v[q]) / wave_max(v[q]) returns, bit
// for bit; the other lanes return the same number for value (lane & (NV - 1)).  Level s pairs lane with lane ^ 2^s as the butterfly does, but
// a lane sends only the half of its live values whose index has bit s unlike its own lane bit, and adds what it receives to the half it
// keeps: a value's partial sums meet in the same pairs in the same level order, on the lanes whose low bits name the value, and a + b is
// b + a.  Once one value per lane is left the plain butterfly finishes it.  16 values: 8 + 4 + 2 + 1 + 1 + 1 = 17 exchanges of a double
// instead of 96, the first 12 of them DPP quad permutes.  Every lane of the wavefront must call it.
__device__ __forceinline__ double lane_xor_level(double v, int s) {   // lane ^ 2^s (s is a constant after unrolling)
  return s == 0 ? lane_xor1(v) : s == 1 ? lane_xor2(v) : __shfl_xor(v, 1 << s);
}
template <int NV, bool MAX = false>
__device__ __forceinline__ double wave_reduce_many(const double* v) {
  static_assert(NV >= 1 && NV <= WAVE && (NV & (NV - 1)) == 0, "wave_reduce_many: a power of two, at most one value per lane");
  const int lane = threadIdx.x & (WAVE - 1);
  double w[NV];
#pragma unroll
  for (int q = 0; q < NV; q++) w[q] = v[q];
  constexpr int LV = __builtin_ctz((unsigned)NV);   // halving levels
#pragma unroll
  for (int s = 0; s < LV; s++) {   // w[j] at the start of level s is value (j << s) | (lane & (2^s - 1))
    const bool up = (lane >> s) & 1;
#pragma unroll
    for (int j = 0; j < (NV >> (s + 1)); j++) {
      const double keep = up ? w[2 * j + 1] : w[2 * j], send = up ? w[2 * j] : w[2 * j + 1];
      const double got = lane_xor_level(send, s);
      w[j] = MAX ? fmax(keep, got) : keep + got;
    }
  }
#pragma unroll
  for (int s = LV; s < 6; s++) {
    const double got = lane_xor_level(w[0], s);
    w[0] = MAX ? fmax(w[0], got) : w[0] + got;
  }
  return w[0];
}

// First stage of the global reductions (qmg_batch.hip, qmg_blas.hip), at the end of a kernel of BLOCK threads: the block's NV sums (maxima)
// go to partial_out[q] -- wavefronts by wave_reduce_many, then the block's wavefronts in index order.
template <int NV, bool MAX = false>
__device__ __forceinline__ void block_reduce_store(double* v, double* partial_out) {
  __shared__ double sm[NV][BLOCK / WAVE];
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  const double w = wave_reduce_many<NV, MAX>(v);   // lane q: wave_max(v[q]) / wave_sum(v[q]), bit for bit
  if (lane < NV) sm[lane][wv] = w;
  __syncthreads();
  if (threadIdx.x < NV) {
    double t = sm[threadIdx.x][0];
#pragma unroll
    for (int w = 1; w < BLOCK / WAVE; w++) t = MAX ? fmax(t, sm[threadIdx.x][w]) : t + sm[threadIdx.x][w];
    partial_out[threadIdx.x] = t;
  }
}
constexpr int RED_BLOCKS = 1024;    // partials per reduction per system (4 blocks per CU)
inline unsigned red_grid(long n) {
  long b = (n + BLOCK - 1) / BLOCK;
  if (b > RED_BLOCKS) b = RED_BLOCKS;
  if (b < 1) b = 1;
  return (unsigned)b;
}

// Two-stage sum of N numbers per thread in a FIXED order, so that the result is deterministic.  First stage, at the end of a kernel of BLOCK
// threads: the block's N sums go to partials[blockIdx.x * N + q]; `sm` is the kernel's own __shared__ array.
template <int N>
__device__ __forceinline__ void block_partials(const double (&v)[N], double (&sm)[N][BLOCK / WAVE], double* __restrict__ partials) {
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
#pragma unroll
  for (int q = 0; q < N; q++) {
    const double w = wave_sum(v[q]);
    if (lane == 0) sm[q][wv] = w;
  }
  __syncthreads();
  if (threadIdx.x < N) {
    double t = 0.0;
    for (int w = 0; w < BLOCK / WAVE; w++) t += sm[threadIdx.x][w];
    partials[(long)blockIdx.x * N + threadIdx.x] = t;
  }
}
// second stage, one block: out[q] = scale * sum over the blocks in index order
template <int N>
__global__ void k_sum_partials(const double* __restrict__ partials, int nparts, double scale, double* __restrict__ out) {
  if (threadIdx.x < N) {
    double t = 0.0;
    for (int i = 0; i < nparts; i++) t += partials[(long)i * N + threadIdx.x];
    out[threadIdx.x] = t * scale;
  }
}

// ---------------- storage precision (qmg_dtype) ----------------
// Vectors and matrices are STORED as complex<double> (QMG_C64) or complex<float> (QMG_C32).  Except in the fine-stencil
// kernel A (which computes in the storage type), arithmetic and every reduction accumulate in fp64 registers: an element
// is widened when loaded and rounded once when stored, so an fp32 kernel moves half the bytes of its fp64 twin and
// differs from it by one rounding per stored element.
template <typename T> struct CStore;
template <> struct CStore<double> { typedef double2 type; };
template <> struct CStore<float> { typedef float2 type; };

template <typename T>
__device__ __forceinline__ cplx ldc(const void* base, long i) {
  if (sizeof(T) == 8) return reinterpret_cast<const cplx*>(base)[i];
  const float2 v = reinterpret_cast<const float2*>(base)[i];
  return make_double2((double)v.x, (double)v.y);
}
// read-once stream: bypass-on-evict hint
template <typename T>
__device__ __forceinline__ cplx ldc_nt(const void* base, long i) {
  if (sizeof(T) == 8) {
    const cplx* p = reinterpret_cast<const cplx*>(base) + i;
    cplx v;
    v.x = __builtin_nontemporal_load(&p->x);
    v.y = __builtin_nontemporal_load(&p->y);
    return v;
  }
  const long long raw = __builtin_nontemporal_load(reinterpret_cast<const long long*>(base) + i);
  return make_double2((double)__int_as_float((int)(raw & 0xFFFFFFFFll)), (double)__int_as_float((int)(raw >> 32)));
}
// ---- loads that keep the STORAGE form.  A conversion, mask or shift placed right behind a load makes the compiler wait for that load -- and, the
// counter being in-order, for every load issued before it -- on the spot: a loop of `value = widen(load)` runs one memory latency per element
// (seen in the ISA of every complex<float> kernel written that way: load, s_waitcnt vmcnt(0), convert, load, ...).  Staging code therefore
// loads RAW values first (all of them), and widens them where they are consumed.
template <typename T> struct RawC { typedef cplx type; };            // complex<double>: the value itself
template <> struct RawC<float> { typedef long long type; };          // the raw bits of a complex<float>
template <typename T> __device__ __forceinline__ typename RawC<T>::type ld_raw(const void* base, long i) {
  if constexpr (sizeof(T) == 8) return reinterpret_cast<const cplx*>(base)[i];
  else return reinterpret_cast<const long long*>(base)[i];
}
template <typename T> __device__ __forceinline__ typename RawC<T>::type ld_raw_nt(const void* base, long i) {
  if constexpr (sizeof(T) == 8) {
    const cplx* p = reinterpret_cast<const cplx*>(base) + i;
    cplx v;
    v.x = __builtin_nontemporal_load(&p->x);
    v.y = __builtin_nontemporal_load(&p->y);
    return v;
  } else return __builtin_nontemporal_load(reinterpret_cast<const long long*>(base) + i);
}
template <typename T> __device__ __forceinline__ typename RawC<T>::type zero_rawc() {
  if constexpr (sizeof(T) == 8) return make_double2(0.0, 0.0);
  else return 0ll;
}
template <typename T> __device__ __forceinline__ cplx widen_rawc(typename RawC<T>::type r) {
  if constexpr (sizeof(T) == 8) return r;
  else return make_double2((double)__int_as_float((int)(r & 0xFFFFFFFFll)), (double)__int_as_float((int)(r >> 32)));
}
// W consecutive elements as ONE 16-byte raw value ((double, 1) and (float, 2)), or (float, 1) as 8 bytes
template <typename T, int W> struct RawP { typedef typename RawC<T>::type type; };
template <> struct RawP<float, 2> { typedef float type __attribute__((ext_vector_type(4))); };
template <typename T, int W> __device__ __forceinline__ typename RawP<T, W>::type ld_rawp(const void* base, long ipack) {
  if constexpr (sizeof(T) == 4 && W == 2) return reinterpret_cast<const typename RawP<float, 2>::type*>(base)[ipack];
  else return ld_raw<T>(base, ipack);
}
template <typename T, int W> __device__ __forceinline__ typename RawP<T, W>::type ld_rawp_nt(const void* base, long ipack) {
  if constexpr (sizeof(T) == 4 && W == 2) return __builtin_nontemporal_load(reinterpret_cast<const typename RawP<float, 2>::type*>(base) + ipack);
  else return ld_raw_nt<T>(base, ipack);
}
template <typename T, int W> __device__ __forceinline__ void widen_rawp(typename RawP<T, W>::type r, cplx (&v)[W]) {
  if constexpr (sizeof(T) == 4 && W == 2) { v[0] = make_double2((double)r.x, (double)r.y); v[W - 1] = make_double2((double)r.z, (double)r.w); }
  else v[0] = widen_rawc<T>(r);
}
template <typename T, int W> __device__ __forceinline__ typename RawP<T, W>::type zero_rawp() {
  if constexpr (sizeof(T) == 4 && W == 2) { typename RawP<float, 2>::type z = {0.0f, 0.0f, 0.0f, 0.0f}; return z; }
  else return zero_rawc<T>();
}
template <typename T>
__device__ __forceinline__ void stc(void* base, long i, cplx v) {
  if (sizeof(T) == 8) reinterpret_cast<cplx*>(base)[i] = v;
  else reinterpret_cast<float2*>(base)[i] = make_float2((float)v.x, (float)v.y);
}
// W consecutive elements starting at element i*W: one 16-byte access per lane for (double, W = 1) and (float, W = 2).
// The (float, 2) form needs base 16-byte aligned (the launchers check and fall back to W = 1).
template <typename T, int W>
__device__ __forceinline__ void ldc_pack(const void* base, long ipack, cplx (&v)[W]) {
  if (sizeof(T) == 4 && W == 2) {
    const float4 r = reinterpret_cast<const float4*>(base)[ipack];
    v[0] = make_double2((double)r.x, (double)r.y);
    v[W - 1] = make_double2((double)r.z, (double)r.w);
  } else {
#pragma unroll
    for (int w = 0; w < W; w++) v[w] = ldc<T>(base, ipack * W + w);
  }
}
template <typename T, int W>
__device__ __forceinline__ void ldc_pack_nt(const void* base, long ipack, cplx (&v)[W]) {   // read-once streams
  if (sizeof(T) == 4 && W == 2) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    const f4 r = __builtin_nontemporal_load(reinterpret_cast<const f4*>(base) + ipack);
    v[0] = make_double2((double)r.x, (double)r.y);
    v[W - 1] = make_double2((double)r.z, (double)r.w);
  } else {
#pragma unroll
    for (int w = 0; w < W; w++) v[w] = ldc_nt<T>(base, ipack * W + w);
  }
}
template <typename T, int W>
__device__ __forceinline__ void stc_pack(void* base, long ipack, const cplx (&v)[W]) {
  if (sizeof(T) == 4 && W == 2) {
    reinterpret_cast<float4*>(base)[ipack] = make_float4((float)v[0].x, (float)v[0].y, (float)v[W - 1].x, (float)v[W - 1].y);
  } else {
#pragma unroll
    for (int w = 0; w < W; w++) stc<T>(base, ipack * W + w, v[w]);
  }
}
inline size_t dtype_size(int dtype) { return dtype == QMG_C32 ? 8 : 16; }
inline bool valid_dtype(int dtype) { return dtype == QMG_C64 || dtype == QMG_C32; }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ---------------- lock-step batches: the active systems of a call ----------------
constexpr int BATCH_MAX = 16;
struct BatchIdx { int n; int nt; unsigned char id[BATCH_MAX]; };   // nt: the batch is large enough for non-temporal reads (qmg_batch.hip)
inline BatchIdx expand_mask(unsigned mask, int nrhs) {
  BatchIdx b;
  b.n = 0;
  b.nt = 0;
  for (int k = 0; k < nrhs && k < BATCH_MAX; k++)
    if ((mask >> k) & 1u) b.id[b.n++] = (unsigned char)k;
  for (int k = b.n; k < BATCH_MAX; k++) b.id[k] = 0;
  return b;
}

// ---------------- apply epilogue (qmg_stencil_apply_epi_t, qmg_wilson_*_direct_epi): what a stencil kernel does with a finished site value ----------------
//   out = other_scale * other + acc_scale * acc      (other == nullptr: out = acc)      -- residuals b - A x, the Schur complement's r_e - D_eo t
//   dotv != nullptr: per-wavefront partial sums of conj(dotv) out (re, im) and |out|^2 go to `part`, [system slot][npart][4]   -- MR's <p,r>, <p,p>
// `other` and `dotv` are vectors with the layout, precision, stride and system numbering of lhs; only the parities the launch processes are
// touched.  Needs overwrite semantics (QMG_P_ZERO on the processed parities).  The dots are taken of the value AS STORED (rounded to the
// storage precision first), so they are the dots a separate pass over the stored vector would form.
struct Epilogue {
  const void* other;
  const void* dotv;
  double other_scale, acc_scale;
  double* part;
  long npart;        // partial slots per system (wavefronts of the launch)
  int on;
};
inline Epilogue no_epilogue() { Epilogue e; e.other = nullptr; e.dotv = nullptr; e.other_scale = 0.0; e.acc_scale = 1.0; e.part = nullptr; e.npart = 0; e.on = 0; return e; }
// qmg_batch.hip: the calling thread's MR slot.  begin: a partial buffer of nsys * npart * 4 doubles (grown on demand; nullptr on failure);
// finish: second stage -- the partials of the n systems `ids` summed in index order into the slot (conjugated to <p,r>), summed over ranks
// under distributed reductions.
double* mr_epilogue_begin(int nsys, long npart);
int mr_epilogue_finish(const unsigned char* ids, int n, long npart, hipStream_t st);

// qmg_batch.hip: the calling thread's reduction workspace.  Every reduction of the C ABI uses it -- the batch entry points, the single-vector
// ones (the batch ones at nrhs = 1) and the two that have no batch form (qmg_blas.hip: the maximum norm, the per-timeslice sums).  Calls of one
// host thread on different streams share it and must not overlap.
constexpr int BDOT_MAX = 32;     // vectors per batched multidot call
constexpr size_t WS_PARTIALS = (size_t)BATCH_MAX * RED_BLOCKS * 2 * BDOT_MAX;   // doubles
constexpr size_t WS_RESULTS = (size_t)BATCH_MAX * 2 * BDOT_MAX;
struct BatchWorkspace {
  double* partials = nullptr;   // WS_PARTIALS doubles (8 MiB)
  double* pinned = nullptr;     // host-pinned, device-visible results: WS_RESULTS doubles
  double* result = nullptr;     // the same in HBM: where the results go when they are summed over ranks first
  double* mr = nullptr;         // device-resident scalars of the MR smoother: [system][4] = Re<p,r>, Im<p,r>, <p,p>, - (qmg_batch_mr_*)
  double* epi_part = nullptr;   // partials of an apply's MR epilogue ([system slot][wavefront][4]), grown on demand
  size_t epi_cap = 0;
  unsigned* done = nullptr;              // blocks of the current final stage that have stored their result (device)
  unsigned long long* flag = nullptr;    // host-pinned, coherent: sequence number of the last final stage whose results are in `pinned`
  unsigned long long seq = 0;
  int device = -1;
};
int get_bws(BatchWorkspace** out);
// where a final stage writes its results: the caller's device pointer if there is one, else the workspace's HBM slot when they are summed over
// the ranks first (dist_reductions_on), else its pinned slot
double* result_slot(BatchWorkspace* ws, double* out_dev);
// `count` results at `res` (a result_slot) readable in ws->pinned when this returns; flagged: the final stage publishes ws->seq behind them
int results_to_host(BatchWorkspace* ws, const double* res, int count, bool flagged, hipStream_t st);

extern int g_reduce_spin;     // qmg_batch.hip; "reduce_spin"
extern int g_malloc_poison;   // qmg_runtime.hip; "malloc_poison"
// qmg_shutdown: the calling thread's reduction / norm workspaces (qmg_batch.hip, qmg_stencil.hip)
void release_batch_workspace();
void release_stencil_workspace();
void release_deflate_workspace();   // qmg_deflate.hip
void release_u1_workspace();        // qmg_u1.hip
void release_flow_workspace();      // qmg_flow.hip
void release_dwf_meas_workspace();  // qmg_dwf_meas.hip
void release_singlet_workspace();   // qmg_singlet.hip
extern int g_setup_fused; // qmg_setup.hip; "setup_fused"
extern int g_wilson_pair;      // qmg_wilson.hip; "wilson_pair"
extern int g_stencil_site;     // qmg_stencil_apply.hip; "stencil_site"
extern int g_stencil_pair;     // qmg_stencil_apply.hip; "stencil_pair"
extern int g_pair_prefetch;    // qmg_stencil.hip; "pair_prefetch"
extern int g_stencil_mfma;     // qmg_stencil_mfma.hip; "stencil_mfma"
extern long g_blas_nt_bytes;   // qmg_blas.hip; "blas_nt_mb"

// "malloc_poison": the library's own scratch is filled with 0xFF where it is created or grown, behind the allocation that has just
// synchronised the device.  The key off: one host branch, no launch.
inline int poison_new_scratch(void* p, size_t bytes) {
  if (g_malloc_poison) {
    QMG_HIP_CHECK(hipMemset(p, 0xFF, bytes));
    QMG_HIP_CHECK(hipDeviceSynchronize());
  }
  return QMG_SUCCESS;
}

// A device scratch buffer of the calling thread (declare it thread_local), grown on demand -- the only synchronous step of its users, and only
// when it grows -- and held until qmg_shutdown.  Calls of one host thread on different streams share it and must not overlap.
struct ThreadScratch {
  void* buf = nullptr;
  size_t bytes = 0;
  int device = -1;
  template <class T> int grow(size_t need, T** out) {
    int dev = 0;
    QMG_HIP_CHECK(hipGetDevice(&dev));
    if (device != dev || bytes < need) {
      if (buf && device == dev) QMG_HIP_CHECK(hipFree(buf));   // waits for the device: nothing still reads it
      *this = ThreadScratch();
      QMG_HIP_CHECK(hipMalloc(&buf, need));
      if (const int rc = poison_new_scratch(buf, need)) return rc;
      bytes = need;
      device = dev;
    }
    *out = (T*)buf;
    return QMG_SUCCESS;
  }
  void release() {
    if (buf) hipFree(buf);
    *this = ThreadScratch();
  }
};
inline bool fields_overlap(const void* a, size_t abytes, const void* b, size_t bbytes) {
  return (const char*)a < (const char*)b + bbytes && (const char*)b < (const char*)a + abytes;
}

// Memory-bound 1-D launches.  One 16-byte element per thread up to 2^18 blocks, grid-stride beyond: on this part a
// streaming copy reaches 6.2 TB/s at 262 144 blocks but only 5.4 TB/s at 8 192 (profiles/r01_membw_ceiling.txt).
inline unsigned grid_1d(size_t work_items, int per_block = BLOCK) {
  size_t b = (work_items + per_block - 1) / per_block;
  const size_t cap = 262144u;
  if (b > cap) b = cap;
  if (b == 0) b = 1;
  return (unsigned)b;
}
inline int rows_on_grid(long n) { return n > 65535 ? 65535 : (int)n; }   // grid.y: blocks walk the rows beyond it

// What every qmg_*_plan export writes: the n numbers of the plan, then -1 in whatever the caller's array holds beyond them.
inline void export_plan_ints(const int* v, int n, int* plan_out, int plan_len) {
  for (int i = 0; i < plan_len; i++) plan_out[i] = i < n ? v[i] : -1;
}

}  // namespace qmg

#endif
