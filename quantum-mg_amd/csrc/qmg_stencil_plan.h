// qmg_stencil_plan.h -- which kernel serves a stencil apply: ONE host function (stencil_plan) that the dispatcher and the launch functions of the
// stencil units switch on and that qmg_stencil_plan() exports, so that the tests can ask for the route of a request and a retune of a threshold
// cannot move a kernel out from under its test (tests/test_gpu_stencil_routes.py holds one row per plan).
// Host code only, no HIP call: nothing here is seen by a kernel except GenLayout, which kernels B / B32 take by value.
#ifndef QMG_STENCIL_PLAN_H
#define QMG_STENCIL_PLAN_H

#include "qmg_common.h"

namespace qmg {

// kernel families (the values are part of qmg_stencil_plan()'s output, include/qmg_hip.h)
enum StencilFamily {
  SF_UNSUPPORTED = 0,   // the entry point returns QMG_ERR_UNSUPPORTED
  SF_ELEM = 1,          // kernel A:   k_stencil_elem<T, NC>
  SF_PAIR = 2,          // kernel A2:  k_stencil_pair<double, NC, ROWS, NORM, PF>
  SF_SITE = 3,          // kernel S:   k_stencil_site<ST, SHAPE, ZERO, BATCH>
  SF_GEN = 4,           // kernel B:   k_stencil_gen<PT, M32, KR, V32, EPI>
  SF_GEN32 = 5,         // kernel B32: k_stencil_gen32<PP, KR, V32, EPI, M16>
  SF_MFMA = 6,          // kernel C:   k_stencil_mfma<NC, MODE, M32, V32, VL, M16, PAIR>
  SF_VOLUME1 = 7,       // the 1 x 1 lattice: k_stencil_volume1<T>
  SF_NOTHING = 8,       // success with nothing launched (no piece asks for work)
  SF_INVALID = 9        // the entry point returns QMG_ERR_INVALID
};
// storage of an instantiation, as bits: matrices complex<float> or narrower, vectors complex<float>, matrices complex<half>
enum { SST_M32 = 1, SST_V32 = 2, SST_M16 = 4 };
// flags of an instantiation / launch
enum {
  SPF_EPI = 1,      // B / B32: the epilogue form (EPI)
  SPF_DOTS = 2,     // ... with the MR dots: grid.y capped, one partial per wavefront
  SPF_NORM = 4,     // A2: fused |lhs_k|^2 (NORM)
  SPF_PF = 8,       // A2: next-system prefetch (PF)
  SPF_ZERO = 16,    // S: ZERO; 1 x 1: the site is cleared first
  SPF_BATCH = 32,   // S: BATCH
  SPF_VL = 64,      // C: right-hand sides through LDS (VL)
  SPF_PAIR = 128,   // C: two sites per wavefront (PAIR; NC is then the pair's 16)
  SPF_SHIFT = 256   // 1 x 1: the shift term is applied
};
enum { STENCIL_PLAN_INTS = 12 };

// kernels B / B32: the tile of one block
struct GenLayout {
  int S;        // sites per block
  int H;        // c-slices per row
  int rs;       // padded LDS row stride (complex elements)
  int mat_elems;   // S * nc * nc
  int per_thread;  // ceil(mat_elems / BLOCK)
};
constexpr int GEN_MAX_PER_THREAD = 12;   // register-staged matrix elements per thread per piece

inline GenLayout make_gen_layout(int nc, int hr, bool mat32, int site_cap = 0) {
  GenLayout L;
  const int nc2 = nc * nc;
  int S = (BLOCK * GEN_MAX_PER_THREAD) / nc2;       // registers: S*nc^2 <= 256*12
  if (S > BLOCK / nc) S = BLOCK / nc;               // one (s,r) row per thread at least
  if (S > hr) S = hr;
  // fp32-stored matrices: the kernel is bound by bytes in flight per CU (one piece per resident block), not by HBM; with
  // half the bytes per piece, smaller tiles (more resident blocks) pay: 512^2, nc = 24: S = 5 1.81 ms, S = 2 1.59 ms
  if (mat32 && nc >= 16 && S > 2) S = 2;
  if (site_cap > 0 && S > site_cap) S = site_cap;
  if (S < 1) S = 1;
  L.S = S;
  int H = BLOCK / (S * nc);
  if (H < 1) H = 1;
  if (H > nc) H = nc;
  L.H = H;
  L.rs = nc + ((nc % 2 == 0) ? 1 : 0);
  L.mat_elems = S * nc2;
  L.per_thread = (L.mat_elems + BLOCK - 1) / BLOCK;
  return L;
}

// right-hand sides per pass of kernels B / B32: 8 accumulators from 5 systems, 4 for 2-4 systems, else 1
inline int gen_pass_width(int nrhs) { return (nrhs >= 5) ? 8 : (nrhs >= 2) ? 4 : 1; }

// What the dispatch reads of a request.
struct StencilPlanRequest {
  int site_entry;    // 1: the entries that call kernel S themselves (qmg_stencil_apply_h16, nc = 2 slabs): no decline, mat / vec32 give its storage
  int mat;           // matrices: 0 complex<double>, 1 complex<float>, 2 complex<half>
  int vec32;         // vectors complex<float>
  int Lx, Ly, nc;
  unsigned pieces;
  int nrhs;          // active systems of the call
  int holes;         // the active systems are not 0 .. nrhs-1 (an index table goes with the launch)
  int inplace;       // lhs == rhs
  int clover, hopping;   // d->clover / d->hopping present
  int norm;          // fused |lhs_k|^2 (qmg_stencil_apply_norm2)
  int epi;           // apply epilogue: 0 none, 1 without dotv, 2 with the MR dots
  int slab, rows;    // y-slab, and its `rows` (0 all, 1 interior, 2 the two boundary rows)
  int k_site, k_pair, k_mfma, k_prefetch;   // the tuning knobs stencil_site, stencil_pair, stencil_mfma, pair_prefetch
};

// The plan of one pass.  The first STENCIL_PLAN_INTS members, in this order, are what qmg_stencil_plan() writes; a member the family does not
// use is 0.
struct StencilPlan {
  int family;     // StencilFamily
  int storage;    // SST_* bits of the instantiation (kernel A in float, kernel S storage 1: M32 | V32; kernel S storage 0: all three)
  int NC;         // compile-time nc (A, A2, C, S); 0: nc is a run-time argument
  int P;          // PT (B), PP (B32), MODE (C), SHAPE (S), ROWS (A2)
  int K;          // KR (B, B32); systems of the pass (every other family)
  int flags;      // SPF_*
  int S, H;       // tile of kernels B / B32
  int smem;       // dynamic LDS bytes
  int gx, gy;     // grid
  int nk;         // systems this pass serves, from k0 on (a family other than C serves them all in one pass)
  // ----
  int status;     // QMG_SUCCESS, or what the entry point returns
  GenLayout L;
};

// What the entry points check of their own arguments before they reach the dispatcher, stated once: the entry points (qmg_stencil_apply.hip,
// qmg_site.hip) and the plan query qmg_stencil_plan() call the same predicates, so the query cannot accept what an entry point refuses.
namespace entry_rules {
inline bool fine_nc(int nc) { return nc == 1 || nc == 2 || nc == 4; }
inline bool batch_size_ok(int nrhs) { return nrhs >= 1 && nrhs <= 16; }   // the masked entries, the fused norm, the 16-bit entry, slabs
// narrow matrices: complex<float> under fp64 vectors serves the Galerkin levels only (not nc = 1, 2, 4); complex<half>: nc a multiple of 4 above 4
inline bool narrow_storage_served(int mat, int vec32, int nc) {
  if (mat == 2) return !(nc & 3) && nc != 4;
  if (mat == 1 && !vec32) return !fine_nc(nc);
  return true;
}
inline bool both_parities(unsigned pieces) {   // the fused norm: a parity left untouched would not be seen by the kernel
  return (pieces & (QMG_P_CLOVER_E | QMG_P_EO | QMG_P_SHIFT_E | QMG_P_ZERO_E)) && (pieces & (QMG_P_CLOVER_O | QMG_P_OE | QMG_P_SHIFT_O | QMG_P_ZERO_O));
}
inline bool epilogue_storage_valid(int mat, int vec32) { return !(vec32 && !mat); }
inline bool epilogue_storage_served(int mat, int nc) { return !(mat && fine_nc(nc)); }
// a slab in place only for the reference's aliased use (stencil_2d.h:1904): ONE parity written, from hops alone
inline bool slab_inplace_ok(unsigned pieces) { return !(both_parities(pieces) || (pieces & (QMG_P_CLOVER | QMG_P_SHIFT))); }
// slabs of any nc but 2 (kernels B / B32 / C): all rows in one launch; narrow storage on the Galerkin levels.  narrow_under: complex<half>
// matrices, or complex<float> matrices asked for apart from the vectors' type
inline bool slab_generic_served(int mat, bool narrow_under, int nc, int rows) { return rows == 0 && !(mat == 2 && (nc & 3)) && !(narrow_under && nc <= 4); }
}  // namespace entry_rules

namespace plan_detail {
constexpr unsigned EVEN_BITS = QMG_P_CLOVER_E | QMG_P_EO | QMG_P_SHIFT_E | QMG_P_ZERO_E;
constexpr unsigned ODD_BITS = QMG_P_CLOVER_O | QMG_P_OE | QMG_P_SHIFT_O | QMG_P_ZERO_O;
inline StencilPlan refused(int status) {
  StencilPlan pl = {};
  pl.family = status == QMG_ERR_INVALID ? SF_INVALID : SF_UNSUPPORTED;
  pl.status = status;
  return pl;
}
inline StencilPlan nothing(int nrhs) {
  StencilPlan pl = {};
  pl.family = SF_NOTHING;
  pl.nk = nrhs;
  return pl;
}

// Kernel S (nc = 2).  ST: 0 = complex<half> matrices + complex<float> vectors, 1 = complex<float>, 2 = complex<double>.  only_where_faster:
// *declined is set for the launches that kernel A does as well or better -- measured at 4096^2: fp64 M 1.10 ms both, fp64 batches of 8
// 0.63 ms (A) against 0.78 ms, fp64 D_eo 0.395 ms (site) against 0.425 ms.
inline StencilPlan site_plan(int ST, const StencilPlanRequest& r, bool only_where_faster, bool* declined) {
  *declined = false;
  if (r.nc != 2 || r.nrhs < 1 || r.nrhs > 16 || ST < 0 || ST > 2) return refused(QMG_ERR_UNSUPPORTED);
  const bool ev = r.pieces & EVEN_BITS, od = r.pieces & ODD_BITS;
  if (!ev && !od) return nothing(r.nrhs);
  const int par_first = ev ? 0 : 1, par_count = (ev && od) ? 2 : 1;
  const bool boundary_only = r.slab && r.rows == 2;
  const int y_count = boundary_only ? 2 : (r.slab && r.rows == 1) ? r.Ly - 2 : r.Ly;
  if (y_count <= 0) return nothing(r.nrhs);
  const long nrows = (long)y_count * par_count;
  // the compile-time shape, if every processed parity asks for the same complete set
  int sh[2] = {0, 0};
  bool zero = true;
  for (int q = 0; q < par_count; q++) {
    const int p = (par_count == 2) ? q : par_first;
    const bool cl = r.clover && ((r.pieces >> p) & 1u);
    const unsigned hm = r.hopping ? ((r.pieces >> (2 + 4 * p)) & 0xFu) : 0u;
    sh[q] = (hm == 0xFu) ? (cl ? 1 : 2) : 0;
    if (!((r.pieces >> (12 + p)) & 1u)) zero = false;
  }
  const int shape = (par_count == 2 && sh[0] != sh[1]) ? 0 : sh[0];
  if (only_where_faster && ST == 2 && !(r.nrhs == 1 && shape == 2)) { *declined = true; return refused(QMG_ERR_UNSUPPORTED); }
  const int lps = ST == 0 ? 1 : ST == 1 ? 2 : 4;   // lanes per site
  const long lanes = (long)(r.Lx / 2) * lps;
  StencilPlan pl = {};
  pl.family = SF_SITE;
  pl.storage = ST == 0 ? (SST_M32 | SST_V32 | SST_M16) : ST == 1 ? (SST_M32 | SST_V32) : 0;
  pl.NC = 2;
  pl.P = shape;
  pl.K = r.nrhs;
  pl.flags = ((zero && shape != 0) ? SPF_ZERO : 0) | (r.nrhs > 1 ? SPF_BATCH : 0);   // (shape 0 is built with the run-time zero test only)
  pl.gx = (int)((lanes + BLOCK - 1) / BLOCK);
  pl.gy = rows_on_grid(nrows);
  pl.nk = r.nrhs;
  return pl;
}
}  // namespace plan_detail

// The plan of the pass that starts at active system k0 (0 for the first; the caller goes on with k0 + nk while that is below r.nrhs).
inline StencilPlan stencil_plan(const StencilPlanRequest& r, int k0 = 0) {
  using namespace plan_detail;
  const int nrhs = r.nrhs, nc = r.nc;
  const bool mat32 = r.mat != 0, mat16 = r.mat == 2, vec32 = r.vec32 != 0, slab = r.slab != 0;
  if (nrhs < 1 || k0 < 0 || k0 >= nrhs || r.mat < 0 || r.mat > 2) return refused(QMG_ERR_INVALID);
  bool declined;
  if (r.site_entry) {
    if (nrhs > 16 || !valid_lattice(r.Lx, r.Ly)) return refused(QMG_ERR_INVALID);
    if (nc != 2) return refused(QMG_ERR_UNSUPPORTED);
    return site_plan(mat16 ? 0 : vec32 ? 1 : 2, r, false, &declined);
  }
  if (r.Lx == 1 && r.Ly == 1) {
    // the 1 x 1 lattice: the shift term alone, the one site counting as even; plain applies only
    if (slab || r.norm || r.epi) return refused(QMG_ERR_UNSUPPORTED);
    if (nc < 1 || nrhs > 16) return refused(QMG_ERR_INVALID);
    const int zero = (r.pieces & (QMG_P_ZERO_E | QMG_P_ZERO_O)) ? 1 : 0, shift_on = (r.pieces & QMG_P_SHIFT_E) ? 1 : 0;
    if (!zero && !shift_on) return nothing(nrhs);
    StencilPlan pl = {};
    pl.family = SF_VOLUME1;
    pl.storage = vec32 ? (SST_M32 | SST_V32) : 0;
    pl.K = nrhs;
    pl.flags = (zero ? SPF_ZERO : 0) | (shift_on ? SPF_SHIFT : 0);
    pl.gx = (nc * nrhs + 63) / 64;
    pl.gy = 1;
    pl.nk = nrhs;
    return pl;
  }
  if (!valid_lattice(r.Lx, r.Ly) || nc < 1) return refused(QMG_ERR_INVALID);
  if (vec32 && !mat32) return refused(QMG_ERR_UNSUPPORTED);   // fp32 vectors come with fp32 matrices (qmg_stencil_apply_t)
  const bool fine = nc == 1 || nc == 2 || nc == 4;   // kernels A / A2
  // narrow matrices under fp64 vectors: the Galerkin levels (kernels B / B32 / C); complex<half>: nc a multiple of 4 above 4
  if (!entry_rules::narrow_storage_served(r.mat, vec32, nc)) return refused(QMG_ERR_UNSUPPORTED);
  // nc = 2 in one storage precision: the site kernel (kernel S, qmg_site.hip)
  const bool one_precision = !mat16 && mat32 == vec32;
  if (slab && nc == 2 && !one_precision) return refused(QMG_ERR_UNSUPPORTED);   // slabs at nc = 2: kernel S, matrices and vectors in ONE precision (or its own 16-bit form)
  if (r.epi && (r.norm || nrhs != 1)) return refused(QMG_ERR_UNSUPPORTED);   // the epilogue is served for ONE system per launch, by kernels B / B32
  if (nc == 2 && one_precision && nrhs <= 16 && !r.norm && !r.epi && (slab || (vec32 ? (r.k_site & 2) : (r.k_site & 5)))) {
    const StencilPlan pl = site_plan(vec32 ? 1 : 2, r, !slab && !(r.k_site & 4), &declined);
    if (!declined) return pl;
  }

  const int hr = r.Lx / 2;
  // which parity halves have any work
  const bool ev = r.pieces & EVEN_BITS, od = r.pieces & ODD_BITS;
  if (!ev && !od) return nothing(nrhs);
  const int par_count = (ev && od) ? 2 : 1;
  const long nrows = (long)r.Ly * par_count;
  const int storage = (mat32 ? SST_M32 : 0) | (vec32 ? SST_V32 : 0) | (mat16 ? SST_M16 : 0);

  StencilPlan pl = {};
  pl.storage = storage;
  pl.K = nrhs;
  pl.nk = nrhs;

  // kernel A2 on its grid: lane groups over the half row, blocks over groups of ROWS rows (two where Ly is even: always, valid_lattice)
  auto pair_plan = [&](bool norm) {
    const int E = nc * nc, ROWS = (r.Ly % 2 == 0) ? 2 : 1;   // lanes per site (KA<double, NC>::E)
    // staggered-type batches (nc = 1): the variant that requests system k+1 ahead of system k's arithmetic -- 4096^2, 8 systems:
    // 1.04 -> 0.90 ms; at nc = 2 it loses 3 % (tools/apply_norm_ab.py), so not there
    const bool pf = nc == 1 && nrhs > 1 && r.k_prefetch;
    if (ROWS != 2 || (norm && nc == 4)) return refused(QMG_ERR_UNSUPPORTED);   // not built: odd Ly, the norm at nc = 4
    pl.family = SF_PAIR;
    pl.NC = nc;
    pl.P = ROWS;
    pl.flags = (norm ? SPF_NORM : 0) | (pf ? SPF_PF : 0);
    pl.smem = norm ? (int)(sizeof(double) * BLOCK * (size_t)nrhs) : 0;
    pl.gx = (hr + BLOCK / E - 1) / (BLOCK / E);
    pl.gy = rows_on_grid(r.Ly / ROWS);
    return pl;
  };

  if (r.norm) {
    // apply + |lhs_k|^2 in one pass: kernel A2 in fp64, nc = 1 or 2, every site written
    if (vec32 || mat32 || slab || r.holes || !(nc == 1 || nc == 2) || par_count != 2 || r.inplace || nrhs > 16) return refused(QMG_ERR_UNSUPPORTED);
    return pair_plan(true);
  }

  if (r.epi) {
    // out = other_scale other + acc_scale acc and the MR dots, in kernels B / B32 (any nc the generic kernels serve); the processed
    // parities must be overwritten (an accumulate into lhs and an `other` term at once has no single meaning)
    if (fine) return refused(QMG_ERR_UNSUPPORTED);   // kernels A / S / W: qmg_wilson_*_direct has its own epilogue, the rest falls back
    if ((ev && !(r.pieces & QMG_P_ZERO_E)) || (od && !(r.pieces & QMG_P_ZERO_O))) return refused(QMG_ERR_INVALID);
    if (r.inplace) return refused(QMG_ERR_INVALID);
  }

  // fp32: the one-site-per-lane-group kernel is the faster one (4096^2 Wilson: 0.573 ms against 0.592 ms for the paired
  // kernel, profiles/r02_kernel_rooflines.json: half the bytes per site leave the paired kernel's longer dependent chain
  // exposed), so the paired kernel serves fp64 only
  if (fine && par_count == 2 && r.k_pair && !vec32 && !r.inplace && !slab) return pair_plan(false);

  if (fine && !slab) {
    const int E = (vec32 && nc % 2 == 0) ? nc * nc / 2 : nc * nc;   // lanes per site (KA<T, NC>::E)
    pl.family = SF_ELEM;
    pl.NC = nc;
    pl.gx = (hr + BLOCK / E - 1) / (BLOCK / E);
    pl.gy = rows_on_grid(nrows);
    return pl;
  }

  // several right-hand sides against one matrix read: kernel C (f64 MFMA) from 4 systems up -- measured 512^2 nc = 24, 8 rhs:
  // 2.84 ms against 4.84 ms for the vector-FMA kernel B, which tops out near 10 TFLOP/s on LDS traffic; with 2-3 systems
  // kernel B's shared tile wins (nc = 8, 1024^2, 3 rhs: 1.06 vs 1.39 ms) and it serves every other nc
  // (nc <= 16: kernel B with one 4-accumulator pass still wins at exactly 4 systems -- nc = 8, 1024^2: 1.21 vs 1.52 ms;
  //  nc = 16, 512^2: 0.98 vs 1.08 ms -- so there the matrix cores take over from 5)
  if (nrhs >= (nc <= 16 ? 5 : 4) && r.k_mfma && (nc == 8 || nc == 12 || nc == 16 || nc == 24 || nc == 32)) {
    // up to 16 right-hand sides per pass share one read of the matrices
    constexpr int WAVES = BLOCK / WAVE;
    const int nk = (nrhs - k0 < 16) ? nrhs - k0 : 16;
    int mode = (r.k_mfma == 2 || nk > 8) ? 0 : 1;
    // 9-16 systems in fp64: the real-form tiles where they save MFMAs (nc = 24: 36 instead of 48 per piece; nc = 8: 4 instead of 8)
    if (mode == 0 && r.k_mfma == 1 && !mat32 && !vec32 && (nc == 24 || nc == 8)) mode = 2;
    // LDS per wavefront: the matrix tile of T colours (raw complex<float> rows of T + 2, or complex<double> rows of T + 1) and,
    // where the right-hand sides go through LDS (VL), a slice of 8 (MODE 1) or 16 vectors
    auto smem_of = [&](int T, bool vl) {
      return (mat32 ? sizeof(float2) * WAVES * T * (T + 2) : sizeof(cplx) * WAVES * T * (T + 1)) + (vl ? sizeof(cplx) * WAVES * (mode == 1 ? 8 : 16) * (T + 1) : 0);
    };
    pl.family = SF_MFMA;
    pl.P = mode;
    pl.K = nk;
    pl.nk = nk;
    pl.gy = rows_on_grid(nrows);
    if (nc == 8 && mode == 1 && !slab && (hr % 2 == 0)) {
      // nc = 8, up to 8 systems, whole lattice: two sites per wavefront (PAIR)
      pl.NC = 16;
      pl.flags = SPF_VL | SPF_PAIR;
      pl.smem = (int)smem_of(16, true);
      pl.gx = (hr / 2 + WAVES - 1) / WAVES;
    } else {
      const bool vl = !(mode == 0 && mat32);   // (fp32- and 16-bit-stored matrices with plain products: B operands straight from global memory)
      pl.NC = nc;
      pl.flags = vl ? SPF_VL : 0;
      pl.smem = (int)smem_of(nc, vl);
      pl.gx = (hr + WAVES - 1) / WAVES;
    }
    return pl;
  }

  if (nc > BLOCK) return refused(QMG_ERR_UNSUPPORTED);
  const int epi_flags = r.epi ? (SPF_EPI | (r.epi == 2 ? SPF_DOTS : 0)) : 0;
  // the epilogue's dots: a few thousand partials for the one-block second stage, so grid.y is capped and blocks walk rows
  auto grid_of = [&](const GenLayout& L) {
    pl.gx = (hr + L.S - 1) / L.S;
    pl.gy = rows_on_grid(nrows);
    if (r.epi == 2) {
      const int cap = pl.gx >= 2048 ? 1 : 2048 / pl.gx;
      if (pl.gy > cap) pl.gy = cap;
    }
  };
  if (mat32 && !(nc & 1) && !(slab && nc <= 4)) {   // (a slab's fp32 applies at nc = 4 keep kernel B's widening loads)
    // kernel B32: fp32 tile end to end (even nc); complex<half> matrices at nc a multiple of 4.  Where its tile does not fit, kernel B takes the launch.
    const GenLayout L = make_gen_layout(nc, hr, false);
    const int pp = mat16 ? (L.mat_elems / 4 + BLOCK - 1) / BLOCK : (L.mat_elems / 2 + BLOCK - 1) / BLOCK;
    if (!(pp < 1 || pp > (mat16 ? 3 : 6))) {
      int kr = gen_pass_width(nrhs);
      auto smem_of = [&](int k) { return (((size_t)L.S * nc * (nc + 2) * 8 + 15) & ~(size_t)15) + sizeof(cplx) * ((size_t)k * L.S * nc + (size_t)L.H * L.S * nc); };
      while (kr > 1 && smem_of(kr) > 48 * 1024) kr = (kr == 8) ? 4 : 1;
      const size_t smem = smem_of(kr);
      if (smem <= 64 * 1024) {
        pl.family = SF_GEN32;
        pl.P = pp;
        pl.K = kr;
        pl.flags = epi_flags;
        pl.S = L.S; pl.H = L.H; pl.L = L;
        pl.smem = (int)smem;
        grid_of(L);
        return pl;
      }
    }
  }
  if (mat16) return refused(QMG_ERR_UNSUPPORTED);   // complex<half> matrices are served by kernels B32 / C only
  // kernel B: fp64 tile, matrices stored as complex<double> or complex<float>
  GenLayout L = make_gen_layout(nc, hr, mat32);
  if (L.per_thread > GEN_MAX_PER_THREAD) return refused(QMG_ERR_UNSUPPORTED);   // nc > 55: S = 1 still too large
  // right-hand sides per pass of kernel B: 4 (2-4 systems) or 8 accumulators; if the tile plus the vectors of the pass do
  // not fit 64 KB of LDS (>= 2 blocks per CU) the tile shrinks first (nc = 16: 12 -> 6 sites), the pass second
  int kr = gen_pass_width(nrhs);
  auto smem_of = [&](const GenLayout& l, int k) { return sizeof(cplx) * ((size_t)l.S * nc * l.rs + (size_t)k * l.S * nc + (size_t)l.H * l.S * nc); };
  while (kr > 1 && smem_of(L, kr) > 64 * 1024 && L.S > 1) L = make_gen_layout(nc, hr, mat32, (L.S + 1) / 2);
  while (kr > 1 && smem_of(L, kr) > 64 * 1024) kr = (kr == 8) ? 4 : 1;
  const size_t smem = smem_of(L, kr);
  if (smem > 160 * 1024) return refused(QMG_ERR_UNSUPPORTED);
  pl.family = SF_GEN;
  pl.P = L.per_thread;
  pl.K = kr;
  pl.flags = epi_flags;
  pl.S = L.S; pl.H = L.H; pl.L = L;
  pl.smem = (int)smem;
  grid_of(L);
  return pl;
}

// the plan's input from a request's own data and the current knobs (qmg_stencil_apply.hip)
StencilPlanRequest plan_request(const qmg_stencil_desc* d, unsigned pieces, int nrhs, bool holes, bool inplace, int mat, bool vec32, const SlabHalo* slab);
// kernel S on its plan (qmg_site.hip)
int launch_stencil_site(const StencilPlan& pl, const qmg_stencil_desc* d, void* lhs, const void* rhs, unsigned pieces, int n, long vec_stride,
                        const unsigned char* ridx, hipStream_t st, const SlabHalo* slab);

}  // namespace qmg

#endif
