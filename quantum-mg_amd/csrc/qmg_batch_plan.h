// qmg_batch_plan.h -- which kernel serves a pass of a batch vector call (qmg_batch.hip): ONE host function (batch_plan) that the launchers switch on
// and that qmg_batch_plan() exports, so that the tests can ask for the route of a request and a retune of a threshold cannot move a kernel out
// from under its test (tests/test_gpu_batch_routes.py holds one row per route), after the model of qmg_transfer_plan.h and
// qmg_stencil_plan.h.  Host code only, no HIP call.
#ifndef QMG_BATCH_PLAN_H
#define QMG_BATCH_PLAN_H

#include "qmg_common.h"

namespace qmg {

// kernel families (the values are part of qmg_batch_plan()'s output: QMG_BF_* of include/qmg_hip.h)
enum BatchFamily {
  BF_NOTHING = QMG_BF_NOTHING,        // success with nothing launched: no active system, n = 0, or nj = 0 where that is a no-op
  BF_BLAS = QMG_BF_BLAS,           // k_bblas<OP, T, W>
  BF_MAXPY_SMALL = QMG_BF_MAXPY_SMALL,    // k_bmulti_caxpy_small<T, W>
  BF_MAXPY_LONG = QMG_BF_MAXPY_LONG,     // k_bmulti_caxpy<T, W>: bmulti_caxpy_run<T, W, NJ, NT>
  BF_MAXPY_SINGLE = QMG_BF_MAXPY_SINGLE,   // qmg_multi_caxpy (qmg_blas.hip: k_multi_caxpy, the one BLAS-1 kernel with no batch form), on the vector sets whose coefficient is not zero
  BF_GCR = QMG_BF_GCR,            // k_bgcr_update<T, W>
  BF_CGM = QMG_BF_CGM,            // k_bcgm_update<T, W>
  BF_REDUCE = QMG_BF_REDUCE,         // k_breduce<OP, T, W> + k_breduce_final
  BF_MULTIDOT = QMG_BF_MULTIDOT,       // k_bmultidot<KT, T, W> (+ k_breduce_final behind the last pass)
  BF_MR_DOTS = QMG_BF_MR_DOTS,        // k_bmultidot<2, T, W> + k_bmr_final
  BF_MR_UPDATE = QMG_BF_MR_UPDATE      // k_bmr_update<T, W, XSET>
};
// `variant` of a pass, as bits: the MR update, and the GCR update
enum { BPV_XSET = 1, BPV_ROUT = 2, BPV_ZNEXT = 1 };
enum { BATCH_PLAN_INTS = 5 };

// A vector of this many bytes and more per system is a LONG vector (an outer solve on the fine lattice).  There the multi-axpy keeps all loads of
// a chunk of 8 vector sets in flight (k_bmulti_caxpy; same-box A/B, C5 shape: the outer flexible GCR's 4096^2 updates 4 % of the solve faster, the
// coarse levels' few-microsecond launches 1 % slower with it, hence the threshold), the GCR update sends every chunk of its Gram-Schmidt sum
// through the multi-axpy (2 % of the C5-shape solve), and ONE complex<double> system goes to k_multi_caxpy (qmg_blas.hip), which takes up to 32
// vector sets per pass over y instead of 8 -- the same sums in the same order.
constexpr size_t BATCH_LONG_BYTES = (size_t)16 << 20;

constexpr int BMAXPY_J = 8;      // vector sets per multi-axpy / GCR launch (the coefficients travel as kernel arguments)
constexpr int CGM_J = 8;         // shifts per multi-shift CG launch (the coefficient tables travel as kernel arguments)
constexpr int CGM_CHUNK = 4;     // shifts per staged chunk of k_bcgm_update

// What the launchers look at.
struct BatchPlanRequest {
  int entry;                     // QMG_BE_*
  int dtype;                     // QMG_C64 | QMG_C32
  int op;                        // QMG_BE_BLAS: QMG_BOP_*; QMG_BE_REDUCE: QMG_BRED_*
  size_t n, stride;
  int nrhs;
  unsigned mask;
  int nj;                        // vector sets (multi-axpy, GCR update, multidot); shifts (CGM update)
  const unsigned* shift_masks;   // CGM update: nj masks
  int flags;                     // BPV_* (MR update: x_set, r_out wanted; GCR update: z_next given)
  int aligned;                   // every pointer of the call is 16-byte aligned
  long nt_bytes;                 // "blas_nt_mb" in bytes (g_blas_nt_bytes)
};

// The plan of one pass.  The first BATCH_PLAN_INTS members, in this order, are what qmg_batch_plan() writes; a member the family does not use is 0.
struct BatchPass {
  int family;    // BatchFamily
  int W;         // elements per 16-byte access: 1 or 2
  int nt;        // read-only operands are read non-temporally
  int J;         // what the pass takes: vector sets (multi-axpy 1..8, GCR 0..8), KT (multidot 8 / 4 / 2 / 1; MR dots 2), shifts (CGM 1..8)
  int variant;   // the BOP / BRED op; BPV_* bits (MR update, GCR update); CGM: the largest per-system count of iterated shifts of the launch
  // ----
  int at;        // first vector set / shift of the pass
  int next;      // where the caller asks again, -1 behind the last pass
  unsigned systems;   // the systems the launch serves (CGM: those with a shift of the launch left)
};

namespace batch_plan_detail {
inline size_t elem_bytes(int dtype) { return dtype == QMG_C32 ? 8 : 16; }
inline int count_bits(unsigned m) { int c = 0; for (; m; m &= m - 1) c++; return c; }
inline unsigned system_bits(unsigned mask, int nrhs) { return nrhs >= 32 ? mask : mask & ((1u << nrhs) - 1u); }
// which access width the arrays of a call allow: 2 complex<float> per 16-byte access needs 16-byte aligned bases, even element counts and
// even strides; complex<double> is always one element per access
inline int pack_width(const BatchPlanRequest& r) {
  if (r.dtype != QMG_C32) return 1;
  if ((r.n & 1) || (r.nrhs > 1 && (r.stride & 1))) return 1;
  return r.aligned ? 2 : 1;
}
// read-only operands of a batch whose active systems add up to `blas_nt_mb` MiB or more are streamed non-temporally
inline int reads_nt(const BatchPlanRequest& r, int nsys) {
  return r.nt_bytes > 0 && (long)((size_t)nsys * r.n * elem_bytes(r.dtype)) >= r.nt_bytes;
}
inline bool long_vector(const BatchPlanRequest& r) { return r.n * elem_bytes(r.dtype) >= BATCH_LONG_BYTES; }
inline BatchPass nothing(int at, int next = -1) {
  BatchPass p = {};
  p.family = BF_NOTHING;
  p.at = at;
  p.next = next;
  return p;
}
}  // namespace batch_plan_detail

// GCR update: how many of its nj vector sets go through the plain multi-axpy first.  All but the last chunk of 8; on long vectors every chunk.
inline int batch_gcr_lead(const BatchPlanRequest& r) {
  if (batch_plan_detail::long_vector(r)) return r.nj;
  return r.nj > BMAXPY_J ? ((r.nj - 1) / BMAXPY_J) * BMAXPY_J : 0;
}

// The plan of the pass that starts at vector set / shift `at` (0 for the first; the caller goes on with the pass's `next` until that is -1).
// The request is one the entry point accepts (qmg_batch_plan() and the entry points check that before they ask).
inline BatchPass batch_plan(const BatchPlanRequest& r, int at = 0) {
  using namespace batch_plan_detail;
  const unsigned act = system_bits(r.mask, r.nrhs);
  const int nact = count_bits(act);
  BatchPass p = {};
  p.at = at;
  p.next = -1;
  p.systems = act;
  p.W = pack_width(r);
  p.nt = reads_nt(r, nact);
  switch (r.entry) {
    case QMG_BE_BLAS:
      if (!nact || !r.n) return nothing(at);
      p.family = BF_BLAS;
      p.variant = r.op;
      return p;
    case QMG_BE_MULTI_CAXPY: {
      if (!nact || !r.n || r.nj <= at) return nothing(at);
      if (r.dtype == QMG_C64 && r.nrhs == 1 && long_vector(r)) {   // every vector set in one call (which chunks by its own 32)
        p.family = BF_MAXPY_SINGLE;
        return p;
      }
      p.family = long_vector(r) ? BF_MAXPY_LONG : BF_MAXPY_SMALL;
      p.J = r.nj - at < BMAXPY_J ? r.nj - at : BMAXPY_J;
      if (at + p.J < r.nj) p.next = at + p.J;
      return p;
    }
    case QMG_BE_GCR_UPDATE: {
      if (!nact || !r.n) return nothing(at);
      const int lead = batch_gcr_lead(r);
      if (at < lead) {   // the multi-axpy call on the first `lead` vector sets
        BatchPlanRequest m = r;
        m.entry = QMG_BE_MULTI_CAXPY;
        m.nj = lead;
        p = batch_plan(m, at);
        if (p.next < 0) p.next = lead;
        return p;
      }
      p.family = BF_GCR;
      p.J = r.nj - lead;
      p.variant = r.flags & BPV_ZNEXT;
      return p;
    }
    case QMG_BE_CGM_UPDATE: {
      if (!r.n || r.nj <= at) return nothing(at);
      const int sj = r.nj - at < CGM_J ? r.nj - at : CGM_J;
      const int next = at + sj < r.nj ? at + sj : -1;
      unsigned any = 0;
      int most = 0;
      for (int k = 0; k < r.nrhs && k < BATCH_MAX; k++) {
        int na = 0;
        for (int j = 0; j < sj; j++) na += (act & r.shift_masks[at + j]) >> k & 1u;
        if (na) any |= 1u << k;
        if (na > most) most = na;
      }
      if (!any) return nothing(at, next);   // a launch none of whose shifts is iterated by any system any more
      p.family = BF_CGM;
      p.nt = reads_nt(r, count_bits(any));
      p.J = sj;
      p.variant = most;
      p.next = next;
      p.systems = any;
      return p;
    }
    case QMG_BE_REDUCE:
      if (!nact) return nothing(at);
      p.family = BF_REDUCE;
      p.variant = r.op;
      return p;
    case QMG_BE_MULTIDOT: {
      if (!nact || r.nj <= at) return nothing(at);
      const int left = r.nj - at;   // chunks of 8 / 4 / 2 / 1 dots: y is re-read once per chunk (each dot is its own accumulation: the chunking changes no digit)
      p.family = BF_MULTIDOT;
      p.J = left >= 8 ? 8 : left >= 4 ? 4 : left >= 2 ? 2 : 1;
      if (at + p.J < r.nj) p.next = at + p.J;
      return p;
    }
    case QMG_BE_MR_DOTS:
      if (!nact) return nothing(at);
      p.family = BF_MR_DOTS;
      p.J = 2;
      return p;
    case QMG_BE_MR_UPDATE:
      if (!nact || !r.n) return nothing(at);
      p.family = BF_MR_UPDATE;
      p.variant = r.flags & (BPV_XSET | BPV_ROUT);
      return p;
    default:
      return nothing(at);
  }
}

}  // namespace qmg

#endif
