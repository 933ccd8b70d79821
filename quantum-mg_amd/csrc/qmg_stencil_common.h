// qmg_stencil_common.h -- what the stencil-apply units share: the kernels' argument block and element loads / stores, the host-side request
// of one apply, and the launch functions the dispatcher (qmg_stencil_apply.hip) calls, one per kernel family:
//     qmg_stencil.hip       kernels A / A2: nc = 1, 2, 4, one matrix element per lane (+ the fused-norm form)
//     qmg_stencil_gen.hip   kernel B: any nc, LDS tile, vector FMAs (qmg_stencil_gen32.hip: kernel B32, its narrow-storage form)
//     qmg_stencil_mfma.hip  kernel C: nc in {8,12,16,24,32}, several right-hand sides on the matrix cores
#ifndef QMG_STENCIL_COMMON_H
#define QMG_STENCIL_COMMON_H

#include <string.h>
#include <type_traits>

#include "qmg_common.h"
#include "qmg_stencil_plan.h"

namespace qmg {

struct StencilArgs {
  const cplx* clover;
  const cplx* hopping;
  void* lhs;         // vectors: complex<double>, or complex<float> when vec32
  const void* rhs;
  int hr;            // Lx / 2: sites per half row
  int Ly;
  long half_vol;     // sites per parity
  long size_cm;      // complex elements per matrix field (both parities)
  unsigned pieces;
  int nrhs;
  long vec_stride;   // complex elements between right-hand sides
  int par_first;     // first parity processed
  int par_count;     // 1 or 2 (2: rows interleaved even/odd)
  int nrows;         // Ly * par_count
  double shift[2], eo_shift[2], dof_shift[2];
  unsigned char ridx[16];   // masked batches (qmg_stencil_apply_batch): right-hand side processed as column k; else unused
  int use_idx;       // 0: column k is right-hand side k
  int mat32;         // 1: clover / hopping point to complex<float> arrays (kernels B and C: qmg_stencil_apply_mat32, qmg_stencil_apply_t)
  int mat16;         // 1 (with mat32 = 1): they point to complex<half> arrays; the tile is widened to complex<float> on its way into LDS (kernel B32: qmg_stencil_apply_mat16)
  int vec32;         // 1: lhs / rhs are complex<float> (qmg_stencil_apply_t with QMG_C32: matrices AND vectors fp32)
  // y-slab of a larger lattice (kernel B only; qmg_stencil_apply_slab): rows -1 / Ly of the right-hand side come from these
  // buffers ([system][parity][hr][nc] complex, halo_stride elements between systems) instead of the periodic wrap
  const void* halo_lo;
  const void* halo_hi;
  long halo_stride;
  // fused |lhs_k|^2 (kernel A2 with NORM, qmg_stencil_apply_norm2): one partial per (row group, block, wavefront, system)
  double* norm_part;
  // apply epilogue (kernels B / B32, one system per launch): out = other_scale other + acc_scale acc, MR dots of out (qmg_common.h)
  Epilogue epi;
};

// The system a launch's k-th right-hand side belongs to (masked batches process a subset: a.ridx), WITHOUT touching memory: a.ridx[k] with a
// run-time k -- divergent or uniform -- is a vector load from the kernel-argument segment, and the `s_waitcnt vmcnt(0)` in front of its use also
// waits for every load issued before it: in kernels B / B32 that was the next piece's matrix prefetch, issued a few instructions earlier (the
// wavefront then sat out the whole latency before it computed on the current piece), in kernel C one more memory latency in front of every
// piece.  The sixteen bytes are four scalar registers; a lane picks its byte with selects and a shift.
__device__ __forceinline__ int system_index(const StencilArgs& a, int k) {
  unsigned long long w[2];
  __builtin_memcpy(w, a.ridx, 16);
  // one select and one shift (for a uniform k: scalar instructions).  A chain of selects per bit came out as a chain of scalar BRANCHES inside kernel
  // A2's next-system prefetch, whose load clauses they cut: 8 systems 0.93 -> 1.01 ms.
  const unsigned long long ww = (k & 8) ? w[1] : w[0];
  const int idx = (int)((ww >> (8 * (k & 7))) & 0xffull);
  return a.use_idx ? idx : k;
}
__device__ __forceinline__ long rhs_offset(const StencilArgs& a, int k) { return (long)system_index(a, k) * a.vec_stride; }
// Kernel A2 (k_stencil_pair) keeps the CONDITIONAL byte load: it is executed for masked batches only, and with it the compiler's schedule of the
// next-system prefetch is the faster one -- same box, 4096^2 staggered, 8 systems: 0.93 ms against 1.01 ms with system_index, whose code is free of
// the load but makes the compiler spread the waits of the two systems' requests differently; an explicit drain in front of the prefetch did not
// bring the 0.93 back (tools/apply_norm_ab.py, gpurun_out/ab_*.txt).  Measured, not understood.
__device__ __forceinline__ long rhs_offset_a(const StencilArgs& a, int k) { return (long)(a.use_idx ? (int)a.ridx[k] : k) * a.vec_stride; }

// vector element i of a complex<double> (V32 = false) or complex<float> (V32 = true) array, in fp64 registers
template <bool V32> __device__ __forceinline__ cplx ldv(const void* base, long i) { return V32 ? ldc<float>(base, i) : ldc<double>(base, i); }
template <bool V32> __device__ __forceinline__ void stv(void* base, long i, cplx v) { if (V32) stc<float>(base, i, v); else stc<double>(base, i, v); }
// A vector element in its STORAGE form (V32: the raw bits of a complex<float> in a double) and its widening.  Staging registers hold the raw
// form: a conversion right behind the load makes the compiler wait for that load -- and for everything issued before it -- on the spot.
template <bool V32> struct XRaw { typedef cplx type; };
template <> struct XRaw<true> { typedef double type; };
template <bool V32> __device__ __forceinline__ typename XRaw<V32>::type ldv_raw(const void* base, long i) {
  if constexpr (V32) return reinterpret_cast<const double*>(base)[i];
  else return reinterpret_cast<const cplx*>(base)[i];
}
template <bool V32> __device__ __forceinline__ cplx widen_raw(typename XRaw<V32>::type v) {
  if constexpr (V32) { struct F2 { float x, y; }; const F2 f = __builtin_bit_cast(F2, v); return cmake((double)f.x, (double)f.y); }
  else return v;
}
template <bool V32> __device__ __forceinline__ typename XRaw<V32>::type zero_raw() {
  if constexpr (V32) return 0.0;
  else return cmake(0.0, 0.0);
}

// the epilogue of one output element (qmg_common.h: Epilogue): returns the value to store, accumulates the MR dots of the value AS STORED
// ov / r: the element's `other` / `dotv` values, loaded by the caller at the START of the row (a load issued here, after the tile loop,
// would add a full memory latency to every block)
template <bool V32>
__device__ __forceinline__ cplx epilogue_value(const Epilogue& e, cplx ov, cplx r, cplx t, double (&d)[3]) {
  if (e.other) t = cmake(fma(e.other_scale, ov.x, e.acc_scale * t.x), fma(e.other_scale, ov.y, e.acc_scale * t.y));
  else if (e.acc_scale != 1.0) t = cmake(e.acc_scale * t.x, e.acc_scale * t.y);
  if (e.dotv) {
    const cplx sv = V32 ? cmake((double)(float)t.x, (double)(float)t.y) : t;
    d[0] = fma(r.x, sv.x, d[0]); d[0] = fma(r.y, sv.y, d[0]);      // conj(r) out
    d[1] = fma(r.x, sv.y, d[1]); d[1] = fma(-r.y, sv.x, d[1]);
    d[2] = fma(sv.x, sv.x, d[2]); d[2] = fma(sv.y, sv.y, d[2]);
  }
  return t;
}
// end of a kernel with an epilogue: one partial per wavefront of the launch, [slot][4] (system slot 0); every lane of the block calls it
// (the launchers cap grid.y for these launches, so that the one-block second stage sums a few thousand partials, not one per row)
__device__ __forceinline__ void epilogue_store_partials(const Epilogue& e, double (&d)[3]) {
  const double v[4] = {d[0], d[1], d[2], 0.0};
  const double s = wave_reduce_many<4>(v);   // lane q: wave_sum(v[q]), bit for bit (the fourth is a sum of zeros: 0.0)
  const int lane = threadIdx.x & (WAVE - 1);
  if (lane < 4) {
    const long w = ((long)blockIdx.y * gridDim.x + blockIdx.x) * (BLOCK / WAVE) + threadIdx.x / WAVE;
    e.part[w * 4 + lane] = s;
  }
}

template <bool NT>
__device__ __forceinline__ cplx ld(const cplx* p) {
  if (NT) {
    cplx v;
    v.x = __builtin_nontemporal_load(&p->x);
    v.y = __builtin_nontemporal_load(&p->y);
    return v;
  }
  return *p;
}

// matrix element i of a complex<double> (M32 = false) or complex<float> (M32 = true) array, widened to fp64
template <bool M32, bool NT>
__device__ __forceinline__ cplx ldm(const cplx* base, long i) {
  if (M32) {
    const float2* p = reinterpret_cast<const float2*>(base) + i;
    float2 v;
    if (NT) {
      const long long raw = __builtin_nontemporal_load(reinterpret_cast<const long long*>(p));
      v.x = __int_as_float((int)(raw & 0xFFFFFFFFll));
      v.y = __int_as_float((int)(raw >> 32));
    } else v = *p;
    return make_double2((double)v.x, (double)v.y);
  }
  return ld<NT>(base + i);
}

// a matrix element in its STORAGE form (M32: the raw 8 bytes of a complex<float>) -- staging registers hold this, the widening happens where the
// element is parked (qmg_common.h: a conversion behind each load serialises the loads)
template <bool M32> struct MRaw { typedef cplx type; };
template <> struct MRaw<true> { typedef long long type; };
template <bool M32, bool NT> __device__ __forceinline__ typename MRaw<M32>::type ldm_raw(const cplx* base, long i) {
  if constexpr (M32) {
    const long long* p = reinterpret_cast<const long long*>(base) + i;
    return NT ? __builtin_nontemporal_load(p) : *p;
  } else return ld<NT>(base + i);
}
template <bool M32> __device__ __forceinline__ cplx widen_mraw(typename MRaw<M32>::type r) {
  if constexpr (M32) return make_double2((double)__int_as_float((int)(r & 0xFFFFFFFFll)), (double)__int_as_float((int)(r >> 32)));
  else return r;
}
template <bool M32> __device__ __forceinline__ typename MRaw<M32>::type zero_mraw() {
  if constexpr (M32) return 0ll;
  else return make_double2(0.0, 0.0);
}
// two consecutive complex<float> matrix elements (16 B, element index i even) widened to fp64
template <bool NT>
__device__ __forceinline__ void ldm32_pair(const cplx* base, long i, cplx& v0, cplx& v1) {
  const double* p = reinterpret_cast<const double*>(reinterpret_cast<const float2*>(base) + i);   // 16-B aligned for even i
  long long r0, r1;
  if (NT) {
    r0 = __builtin_nontemporal_load(reinterpret_cast<const long long*>(p));
    r1 = __builtin_nontemporal_load(reinterpret_cast<const long long*>(p) + 1);
  } else {
    const double2 d = *reinterpret_cast<const double2*>(p);
    r0 = __double_as_longlong(d.x); r1 = __double_as_longlong(d.y);
  }
  v0 = make_double2((double)__int_as_float((int)(r0 & 0xFFFFFFFFll)), (double)__int_as_float((int)(r0 >> 32)));
  v1 = make_double2((double)__int_as_float((int)(r1 & 0xFFFFFFFFll)), (double)__int_as_float((int)(r1 >> 32)));
}

template <bool NT>
__device__ __forceinline__ void st(cplx* p, cplx v) {
  if (NT) {
    __builtin_nontemporal_store(v.x, &p->x);
    __builtin_nontemporal_store(v.y, &p->y);
  } else {
    *p = v;
  }
}

// kernel C: a wavefront's write -> read hand-off through its own LDS slice (a wavefront fence, not a block barrier)
__device__ __forceinline__ void wave_lds_handoff() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// ---------------- host side ----------------
enum class MatStorage { fp64, fp32, fp16 };   // how d->clover / d->hopping are stored: complex<double>, complex<float>, complex<half>

// One apply, as the C entry points hand it to the dispatcher (qmg_stencil_apply.hip: stencil_apply).
struct StencilRequest {
  const qmg_stencil_desc* d;
  void* lhs;
  const void* rhs;
  unsigned pieces;
  int nrhs;
  size_t vec_stride;
  const unsigned char* ridx = nullptr;     // masked batch: the system processed as column k; nullptr: column k is system k
  void* stream = nullptr;
  MatStorage mat = MatStorage::fp64;
  bool vec32 = false;                      // lhs / rhs are complex<float>
  const SlabHalo* slab = nullptr;          // y-slab: rows -1 / Ly of the right-hand side come from halo buffers
  double* norms_dev = nullptr;             // fused |lhs_k|^2 (qmg_stencil_apply_norm2)
  const qmg_apply_epilogue* epi = nullptr; // apply epilogue (qmg_stencil_apply_epi_t)
};
int stencil_apply(const StencilRequest& q);

// The launch functions take the filled argument block and the plan of the launch (qmg_stencil_plan.h: stencil_plan), and switch on the plan alone:
// instantiation, tile, grid and LDS bytes are the plan's.  Kernels A / A2 (qmg_stencil.hip):
int launch_stencil_norm(StencilArgs& a, const StencilPlan& pl, double* norms_dev, hipStream_t st);   // apply + |lhs_k|^2, fp64, nc = 1 or 2
int launch_stencil_pair(const StencilArgs& a, const StencilPlan& pl, hipStream_t st);                // fp64, both parities
int launch_stencil_elem(const StencilArgs& a, const StencilPlan& pl, hipStream_t st);
int norm_result_slot(double** res);   // the calling thread's default device slot for 16 norms
// kernel C (qmg_stencil_mfma.hip): the pass of the plan, a's vectors being those of the call
int launch_stencil_mfma(const StencilArgs& a, const StencilPlan& pl, int k0, hipStream_t st);
// kernels B32 (qmg_stencil_gen32.hip) and B (qmg_stencil_gen.hip)
int launch_stencil_gen32(StencilArgs& a, int nc, const StencilPlan& pl, hipStream_t st);
int launch_stencil_gen(StencilArgs& a, int nc, const StencilPlan& pl, hipStream_t st);
// ... and what the two share (qmg_stencil_gen.hip): the epilogue's partials around the launch
int gen_epilogue_begin(StencilArgs& a, const StencilPlan& pl, long& npart);   // asks for the partial buffer
int gen_epilogue_finish(const StencilArgs& a, long npart, hipStream_t st);
// Launch with dynamic LDS: above 64 KiB the kernel's limit is raised first.
template <typename... KArgs, typename... Args>
inline int launch_kernel(void (*kernel)(KArgs...), dim3 grid, size_t smem, hipStream_t st, const Args&... args) {
  if (smem > 64 * 1024) QMG_HIP_CHECK(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  kernel<<<grid, dim3(BLOCK), smem, st>>>(args...);
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

// Run-time value -> compile-time constant: f receives a std::integral_constant and picks the kernel instantiation from it.
template <typename F> inline int with_bool(bool v, F&& f) { return v ? f(std::true_type()) : f(std::false_type()); }
template <int... Vs, typename F> inline int with_int(int v, F&& f) {   // QMG_ERR_UNSUPPORTED: v is none of Vs
  int rc = QMG_ERR_UNSUPPORTED;
  (void)((v == Vs && ((rc = f(std::integral_constant<int, Vs>())), true)) || ...);
  return rc;
}
// the storage forms the kernels are built for, as (M32, V32, M16): fp64; complex<float> or complex<half> matrices with either vectors
template <typename F> inline int with_storage(const StencilPlan& pl, F&& f) {
  typedef std::true_type Y;
  typedef std::false_type N;
  const bool v32 = pl.storage & SST_V32;
  if (pl.storage & SST_M16) return v32 ? f(Y(), Y(), Y()) : f(Y(), N(), Y());
  if (v32) return f(Y(), Y(), N());
  if (pl.storage & SST_M32) return f(Y(), N(), N());
  return f(N(), N(), N());
}

}  // namespace qmg

#endif
