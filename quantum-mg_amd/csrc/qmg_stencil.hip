// qmg_stencil.hip -- fused even-odd stencil apply for gfx950 (MI355X): kernels A and A2, the fine operators (nc = 1, 2, 4).
//
// THIS FILE HOLDS THE HEADLINE KERNEL AND NOTHING ELSE: k_stencil_pair<double, 2, 2, ...> is what bench.py's flagship apply runs, and the
// sha256 of this file is the stamp under which bench.py and tools/summarize_profiles.py report its measured traffic.  The other kernel
// families (qmg_stencil_gen.hip: B; qmg_stencil_gen32.hip: B32; qmg_stencil_mfma.hip: C), the dispatcher and the C entry points (qmg_stencil_apply.hip) live in
// units of their own, so that an edit there leaves the stamp valid and an edit here invalidates it.
//
// Replaces the reference's un-fused pass structure
//     apply_M = clover sweep + 8 x {cshift copy, cMATxpy sweep} + 2 x caxpy      (stencil_2d.h:912-936)
// (~27 vector passes + 5 matrix passes) with ONE launch that reads every stencil
// matrix once, the right-hand side once (from HBM; neighbours come back out of L2) and writes
// the result once: 5 nc^2 c + 2 nc c bytes per site, the algorithmic minimum.
//
// Addressing (derived from lattice.h:75-81,204 and the loops of cshift_2d.h:60-119,149-210):
// an output site of parity p on row y at half-row column j has x = 2j + s, s = (y+p)&1, and its
// four neighbours live in the OPPOSITE parity half at
//     +x: (y, j+s)   -x: (y, j+s-1)   +y: (y+1, j)   -y: (y-1, j)        (periodic)
// The matrix multiplying a neighbour is stored at the OUTPUT site (stencil_2d.h:718-732), so a
// lane streams five arrays at one common offset.
//
// Kernel A (nc = 1, 2, 4): "element per lane".  nc^2 adjacent lanes own one site; lane (r,c)
// loads element M[r][c] of each of the five matrices, so every matrix load instruction of a
// wavefront is one fully coalesced 1 KiB segment (16 B per lane) -- the AoS (c1,c2)-fastest
// layout of the reference is already lane-contiguous and is NOT repacked.  The sum over c is a
// DPP quad-permute (no LDS).  Rows of both parities are interleaved in block order, so the
// even- and odd-output rows that share right-hand-side data run back to back on the same XCD
// (blocks per row is a multiple of 8 for power-of-two lattices) and the second use hits L2.

#include "qmg_stencil_common.h"

namespace qmg {

// ---------------------------------------------------------------------------------------------------------------------
// Kernel A lane layout, either storage precision.  A lane owns CW consecutive column entries of one matrix row, i.e. ONE
// 16-byte fragment of each matrix and of each vector it needs:
//     fp64: CW = 1  -- lane (r, c) holds M[r][c] and x[c]                      (nc^2 lanes per site)
//     fp32: CW = 2  -- lane (r, h) holds M[r][2h..2h+1] and x[2h..2h+1]        (nc^2/2 lanes per site; nc = 1: CW = 1, 8 bytes)
// so every matrix load of a wavefront is one coalesced 1-KiB segment in BOTH precisions (with 8-byte loads the fp32
// kernel would issue the same number of load instructions for half the bytes).  For Wilson fp32 (nc = 2) a lane then
// holds a whole matrix row and the whole site vector: the row sum needs no cross-lane step at all.  The kernel computes
// in the storage type T (the fine operator is the one place fp32 ARITHMETIC is used: SURVEY 8c states 5e-6 per apply).
template <typename T, int NC>
struct KA {
  typedef typename CStore<T>::type ct;
  static constexpr int CW = (sizeof(T) == 4 && NC % 2 == 0) ? 2 : 1;
  static constexpr int LPR = NC / CW;          // lanes per matrix row
  static constexpr int E = NC * LPR;           // lanes per site
  struct Frag { ct v[CW]; };
};

template <typename T> __device__ __forceinline__ typename CStore<T>::type czero() { typename CStore<T>::type z; z.x = (T)0; z.y = (T)0; return z; }
template <typename CT> __device__ __forceinline__ void cmac_t(CT& acc, CT a, CT b) {
  acc.x = fma(a.x, b.x, acc.x);
  acc.x = fma(-a.y, b.y, acc.x);
  acc.y = fma(a.x, b.y, acc.y);
  acc.y = fma(a.y, b.x, acc.y);
}
__device__ __forceinline__ float lane_xor1(float v) { return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true)); }
__device__ __forceinline__ float lane_xor2(float v) { return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, true)); }

typedef float v4f __attribute__((ext_vector_type(4)));

// fragment `idx` (in units of CW elements) of a T-typed array
template <typename T, int NC, bool NT>
__device__ __forceinline__ typename KA<T, NC>::Frag ld_frag(const void* base, long idx) {
  typename KA<T, NC>::Frag f;
  if constexpr (sizeof(T) == 8) {
    f.v[0] = ld<NT>(reinterpret_cast<const cplx*>(base) + idx);
  } else if constexpr (KA<T, NC>::CW == 2) {
    const v4f* p = reinterpret_cast<const v4f*>(base) + idx;
    const v4f r = NT ? __builtin_nontemporal_load(p) : *p;
    f.v[0].x = r.x; f.v[0].y = r.y; f.v[1].x = r.z; f.v[1].y = r.w;
  } else {
    const long long* p = reinterpret_cast<const long long*>(base) + idx;
    const long long raw = NT ? __builtin_nontemporal_load(p) : *p;
    f.v[0].x = __int_as_float((int)(raw & 0xFFFFFFFFll));
    f.v[0].y = __int_as_float((int)(raw >> 32));
  }
  return f;
}
template <typename T, int NC> __device__ __forceinline__ typename KA<T, NC>::Frag zero_frag() {
  typename KA<T, NC>::Frag f;
#pragma unroll
  for (int w = 0; w < KA<T, NC>::CW; w++) f.v[w] = czero<T>();
  return f;
}
template <typename T, int NC>
__device__ __forceinline__ void fmac(typename CStore<T>::type& acc, const typename KA<T, NC>::Frag& m, const typename KA<T, NC>::Frag& x) {
#pragma unroll
  for (int w = 0; w < KA<T, NC>::CW; w++) cmac_t(acc, m.v[w], x.v[w]);
}
// sum over the LPR lanes of a matrix row (adjacent lanes)
template <typename T, int NC> __device__ __forceinline__ void row_sum(typename CStore<T>::type& acc) {
  if (KA<T, NC>::LPR >= 2) { acc.x += lane_xor1(acc.x); acc.y += lane_xor1(acc.y); }
  if (KA<T, NC>::LPR >= 4) { acc.x += lane_xor2(acc.x); acc.y += lane_xor2(acc.y); }
}
// the shift coefficient on the diagonal, as a fragment: shift +- eo_shift +- dof_shift at column r (stencil_2d.h:890-908)
template <typename T, int NC>
__device__ __forceinline__ typename KA<T, NC>::Frag shift_frag(const StencilArgs& a, bool do_shift, int p, int r, int c0) {
  typename KA<T, NC>::Frag sh = zero_frag<T, NC>();
  if (do_shift) {
    const double sg = p ? -1.0 : 1.0;
    const double dg = (NC % 2 == 0) ? ((r < NC / 2) ? 1.0 : -1.0) : 0.0;
#pragma unroll
    for (int w = 0; w < KA<T, NC>::CW; w++)
      if (c0 + w == r) {
        sh.v[w].x = (T)(a.shift[0] + sg * a.eo_shift[0] + dg * a.dof_shift[0]);
        sh.v[w].y = (T)(a.shift[1] + sg * a.eo_shift[1] + dg * a.dof_shift[1]);
      }
  }
  return sh;
}
template <typename T, bool NTS>
__device__ __forceinline__ void st_elem(void* base, long i, typename CStore<T>::type v) {
  typedef typename CStore<T>::type ct;
  ct* p = reinterpret_cast<ct*>(base) + i;
  if (NTS) { __builtin_nontemporal_store(v.x, &p->x); __builtin_nontemporal_store(v.y, &p->y); }
  else *p = v;
}

template <typename T, int NC, bool NT, bool NTS>
__global__ __launch_bounds__(BLOCK) void k_stencil_elem(const StencilArgs a) {
  typedef KA<T, NC> K;
  typedef typename K::ct ct;
  typedef typename K::Frag Frag;
  constexpr int E = K::E, CW = K::CW, FPS = NC * NC / CW, VPS = NC / CW;   // fragments per site: matrix, vector
  const int e = threadIdx.x % E;
  const int r = e / K::LPR, c0 = (e % K::LPR) * CW;
  const int vf = e % K::LPR;            // this lane's vector fragment within a site
  const int j = blockIdx.x * (BLOCK / E) + threadIdx.x / E;
  if (j >= a.hr) return;   // whole site groups leave together (E divides BLOCK)

  for (int row = blockIdx.y; row < a.nrows; row += gridDim.y) {
    const int p = (a.par_count == 2) ? (row & 1) : a.par_first;
    const int y = (a.par_count == 2) ? (row >> 1) : row;
    const bool do_clover = a.clover && ((a.pieces >> p) & 1u);
    const unsigned hop_mask = a.hopping ? ((a.pieces >> (2 + 4 * p)) & 0xFu) : 0u;
    const bool do_shift = (a.pieces >> (10 + p)) & 1u;
    const bool do_zero = (a.pieces >> (12 + p)) & 1u;

    const long site = (long)p * a.half_vol + (long)y * a.hr + j;
    const long opp = (long)(1 - p) * a.half_vol;
    const int s = (y + p) & 1;
    int jp = j + s;     if (jp == a.hr) jp = 0;
    int jm = j + s - 1; if (jm < 0) jm = a.hr - 1;
    const int yp = (y + 1 == a.Ly) ? 0 : y + 1;
    const int ym = (y == 0) ? a.Ly - 1 : y - 1;
    long nb[4];
    nb[0] = opp + (long)y * a.hr + jp;
    nb[1] = opp + (long)yp * a.hr + j;
    nb[2] = opp + (long)y * a.hr + jm;
    nb[3] = opp + (long)ym * a.hr + j;

    // Stencil matrices: one coalesced 16-byte fragment per lane per matrix; kept in registers
    // across all right-hand sides.
    Frag m[5];
    m[4] = do_clover ? ld_frag<T, NC, NT>(a.clover, site * FPS + e) : zero_frag<T, NC>();
#pragma unroll
    for (int d = 0; d < 4; d++)
      m[d] = ((hop_mask >> d) & 1u) ? ld_frag<T, NC, NT>(a.hopping, ((long)d * a.size_cm) / CW + site * FPS + e) : zero_frag<T, NC>();
    const Frag sh = shift_frag<T, NC>(a, do_shift, p, r, c0);
    const bool need_own = do_clover || do_shift;

    for (int k = 0; k < a.nrhs; k++) {
      const ct* x = reinterpret_cast<const ct*>(a.rhs) + rhs_offset(a, k);
      ct* out = reinterpret_cast<ct*>(a.lhs) + rhs_offset(a, k);
      Frag xv[5];
#pragma unroll
      for (int d = 0; d < 4; d++)
        xv[d] = ((hop_mask >> d) & 1u) ? ld_frag<T, NC, false>(x, nb[d] * VPS + vf) : zero_frag<T, NC>();
      xv[4] = need_own ? ld_frag<T, NC, false>(x, site * VPS + vf) : zero_frag<T, NC>();

      ct acc = czero<T>();
      fmac<T, NC>(acc, m[4], xv[4]);                       // clover first, as the reference does
#pragma unroll
      for (int d = 0; d < 4; d++) fmac<T, NC>(acc, m[d], xv[d]);
      fmac<T, NC>(acc, sh, xv[4]);
      row_sum<T, NC>(acc);

      if (c0 == 0) {
        if (!do_zero) { const ct o = out[site * NC + r]; acc.x += o.x; acc.y += o.y; }
        st_elem<T, NTS>(out, site * NC + r, acc);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// Kernel A2 (nc = 1, 2, 4; both parities active): one lane group owns the EVEN and the ODD site
// of half-row column j on ROWS consecutive rows.  The two sites (y,j) of opposite parity are
// mutual x-neighbours (x = 2j and 2j+1, in an order set by y&1) and the rows share their
// y-neighbours, so the right-hand side is loaded into registers once for all 2*ROWS outputs:
// 2(ROWS+2) column values + 2 ROWS side values instead of 10 ROWS.  More importantly each
// wavefront now streams 2*ROWS*5 matrix fragments per lane (ROWS=2: 32 KiB of loads in flight per
// wave), which takes the launch out of the "a million 6-KiB waves" regime where wave dispatch,
// not HBM, sets the pace (tools/membw2.hip: 5.3 TB/s at 1M blocks vs 6.4-6.7 TB/s at 64K).
// ------------------------------------------------------------------------------------------
// NORM: the kernel also leaves |lhs_k|^2 of what it stored, as one partial per (block, system) in a.norm_part (summed in a
// fixed order by k_apply_norm_final) -- the residual norm of a Krylov step without re-reading the vector it has just written
// (16 of a staggered step's 56 B/site/rhs).  Inside the loop over the systems a lane only adds to its own LDS slot
// ([system][thread], dynamic shared memory): a wavefront reduction per system there (four ds_bpermute round trips in the
// dependent chain of every iteration) cost 0.15 ms on a 1.00 ms apply; the cross-lane sums happen once, after the loop.
// Lane groups past the end of the half row stay (on the last column, storing nothing) so that the block-wide steps see
// every thread.
// PF (batches): the right-hand side of system k+1 is requested before system k is multiplied, so a wavefront's loads stay in
// flight through its arithmetic and stores (the kernel sits at 2 waves/SIMD either way: 176 -> 2xx VGPRs).
template <typename T, int NC, int ROWS, bool NT, bool NTS, bool NORM = false, bool PF = false>
__global__ __launch_bounds__(BLOCK) void k_stencil_pair(const StencilArgs a) {
  typedef KA<T, NC> K;
  typedef typename K::ct ct;
  typedef typename K::Frag Frag;
  constexpr int E = K::E, CW = K::CW, FPS = NC * NC / CW, VPS = NC / CW;
  const int e = threadIdx.x % E;
  const int r = e / K::LPR, c0 = (e % K::LPR) * CW;
  const int vf = e % K::LPR;
  int j = blockIdx.x * (BLOCK / E) + threadIdx.x / E;
  bool live = true;
  if (j >= a.hr) {
    if (!NORM) return;
    live = false; j = a.hr - 1;
  }
  extern __shared__ double norm_sm[];
  if (NORM)
    for (int k = 0; k < a.nrhs; k++) norm_sm[k * BLOCK + threadIdx.x] = 0.0;
  const int ngroups = a.Ly / ROWS;

  bool do_clover[2], do_shift[2], do_zero[2];
  unsigned hop_mask[2];
  Frag sh[2];
#pragma unroll
  for (int p = 0; p < 2; p++) {
    do_clover[p] = a.clover && ((a.pieces >> p) & 1u);
    hop_mask[p] = a.hopping ? ((a.pieces >> (2 + 4 * p)) & 0xFu) : 0u;
    do_shift[p] = (a.pieces >> (10 + p)) & 1u;
    do_zero[p] = (a.pieces >> (12 + p)) & 1u;
    sh[p] = shift_frag<T, NC>(a, do_shift[p], p, r, c0);
  }
  const bool any_hop = (hop_mask[0] | hop_mask[1]) != 0u;
  int jl = j - 1; if (jl < 0) jl = a.hr - 1;
  int jr = j + 1; if (jr == a.hr) jr = 0;

  for (int grp = blockIdx.y; grp < ngroups; grp += gridDim.y) {
    const int y0 = grp * ROWS;

    // ---- stencil matrices: 2*ROWS*5 coalesced 16-byte fragments per lane
    Frag m[ROWS][2][5];
#pragma unroll
    for (int rr = 0; rr < ROWS; rr++)
#pragma unroll
      for (int p = 0; p < 2; p++) {
        const long site = (long)p * a.half_vol + (long)(y0 + rr) * a.hr + j;
        m[rr][p][4] = do_clover[p] ? ld_frag<T, NC, NT>(a.clover, site * FPS + e) : zero_frag<T, NC>();
#pragma unroll
        for (int d = 0; d < 4; d++)
          m[rr][p][d] = ((hop_mask[p] >> d) & 1u) ? ld_frag<T, NC, NT>(a.hopping, ((long)d * a.size_cm) / CW + site * FPS + e) : zero_frag<T, NC>();
      }

    // one system's right-hand side: rows y0-1 .. y0+ROWS at column j, both parities, and the one x-neighbour per row that
    // is not the partner site
    struct XF { Frag Ec[ROWS + 2], Oc[ROWS + 2], Es[ROWS], Os[ROWS]; };
    auto load_x = [&](XF& v, int k) {
      const ct* xe = reinterpret_cast<const ct*>(a.rhs) + rhs_offset_a(a, k);   // even half
      const ct* xo = xe + a.half_vol * NC;                                    // odd half
#pragma unroll
      for (int t = 0; t < ROWS + 2; t++) {
        int yy = y0 - 1 + t;
        if (yy < 0) yy = a.Ly - 1;
        if (yy >= a.Ly) yy -= a.Ly;
        const bool edge = (t == 0 || t == ROWS + 1);
        if (!edge || any_hop) {
          v.Ec[t] = ld_frag<T, NC, false>(xe, ((long)yy * a.hr + j) * VPS + vf);
          v.Oc[t] = ld_frag<T, NC, false>(xo, ((long)yy * a.hr + j) * VPS + vf);
        } else {
          v.Ec[t] = v.Oc[t] = zero_frag<T, NC>();
        }
      }
#pragma unroll
      for (int rr = 0; rr < ROWS; rr++) {
        const int y = y0 + rr;
        const int se = y & 1;                    // even site: x = 2j + se ; odd site: x = 2j + 1 - se
        if (any_hop) {
          v.Os[rr] = ld_frag<T, NC, false>(xo, ((long)y * a.hr + (se ? jr : jl)) * VPS + vf);
          v.Es[rr] = ld_frag<T, NC, false>(xe, ((long)y * a.hr + (se ? jl : jr)) * VPS + vf);
        } else {
          v.Os[rr] = v.Es[rr] = zero_frag<T, NC>();
        }
      }
    };

    XF cur;
    if (PF) load_x(cur, 0);
    for (int k = 0; k < a.nrhs; k++) {
      ct* out = reinterpret_cast<ct*>(a.lhs) + rhs_offset_a(a, k);
      double nrm = 0.0;
      XF nxt;
      if (!PF) load_x(cur, k);
      else {
        if (k + 1 < a.nrhs) load_x(nxt, k + 1);
        __builtin_amdgcn_sched_barrier(0);       // keep the scheduler from sinking the prefetch below the arithmetic
      }
      const Frag (&Ec)[ROWS + 2] = cur.Ec, (&Oc)[ROWS + 2] = cur.Oc;
      const Frag (&Es)[ROWS] = cur.Es, (&Os)[ROWS] = cur.Os;

#pragma unroll
      for (int rr = 0; rr < ROWS; rr++) {
        const int y = y0 + rr;
        const int se = y & 1;
#pragma unroll
        for (int p = 0; p < 2; p++) {
          // neighbours of the parity-p site (y, j); s = (y + p) & 1
          const int s = p ? (1 - se) : se;
          const Frag own = p ? Oc[rr + 1] : Ec[rr + 1];
          const Frag partner = p ? Ec[rr + 1] : Oc[rr + 1];     // opposite parity, same (y, j)
          const Frag side = p ? Es[rr] : Os[rr];                // opposite parity, (y, j + (s ? +1 : -1))
          Frag xv[4];
          xv[0] = s ? side : partner;                           // +x: (y, j + s)
          xv[2] = s ? partner : side;                           // -x: (y, j + s - 1)
          xv[1] = p ? Ec[rr + 2] : Oc[rr + 2];                  // +y
          xv[3] = p ? Ec[rr] : Oc[rr];                          // -y
          // values this parity does not ask for may be uninitialised memory: never let them into the sum
          const Frag zero = zero_frag<T, NC>();
          const Frag own_u = (do_clover[p] || do_shift[p]) ? own : zero;
          ct acc = czero<T>();
          fmac<T, NC>(acc, m[rr][p][4], own_u);
#pragma unroll
          for (int d = 0; d < 4; d++) fmac<T, NC>(acc, m[rr][p][d], ((hop_mask[p] >> d) & 1u) ? xv[d] : zero);
          fmac<T, NC>(acc, sh[p], own_u);
          row_sum<T, NC>(acc);
          const bool touch = do_clover[p] || hop_mask[p] || do_shift[p] || do_zero[p];
          if (c0 == 0 && touch && live) {
            const long o = ((long)p * a.half_vol + (long)y * a.hr + j) * NC + r;
            if (!do_zero[p]) { const ct prev = out[o]; acc.x += prev.x; acc.y += prev.y; }
            st_elem<T, NTS>(out, o, acc);
            if (NORM) { nrm = fma((double)acc.x, (double)acc.x, nrm); nrm = fma((double)acc.y, (double)acc.y, nrm); }
          }
        }
      }
      if (NORM) norm_sm[k * BLOCK + threadIdx.x] += nrm;
      if (PF && k + 1 < a.nrhs) cur = nxt;
    }
  }
  if (NORM) {
    __syncthreads();
    const int lane = threadIdx.x & (WAVE - 1);
    for (int k = threadIdx.x / WAVE; k < a.nrhs; k += BLOCK / WAVE) {
      double t = norm_sm[k * BLOCK + lane];
#pragma unroll
      for (int w = 1; w < BLOCK / WAVE; w++) t += norm_sm[k * BLOCK + w * WAVE + lane];
      t = wave_sum(t);
      if (lane == 0) a.norm_part[(long)k * ((long)gridDim.y * gridDim.x) + (long)blockIdx.y * gridDim.x + blockIdx.x] = t;   // [system][block]
    }
  }
}

// the partials of system q (contiguous: [system][block]), summed in a fixed order
__global__ __launch_bounds__(BLOCK) void k_apply_norm_final(const double* __restrict__ part, long nparts, double* __restrict__ out) {
  __shared__ double sm[BLOCK / WAVE];
  const int q = blockIdx.x;
  double t = 0.0;
  for (long i = threadIdx.x; i < nparts; i += BLOCK) t += part[(long)q * nparts + i];
  t = wave_sum(t);
  if ((threadIdx.x & (WAVE - 1)) == 0) sm[threadIdx.x / WAVE] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    double r = sm[0];
#pragma unroll
    for (int w = 1; w < BLOCK / WAVE; w++) r += sm[w];
    out[q] = r;
  }
}

int g_pair_prefetch = 1;   // tuning knob: 1 = kernel A2 prefetches the next system's right-hand side in fp64 batches

// partials of the fused norms (one buffer per host thread = per rank, grown on demand) and the default result slot
// part: the fused-norm partials of the calling thread.  One buffer per thread, so two calls of one thread on DIFFERENT streams would race on it:
// `done` is recorded behind every use and a call on another stream than the last one waits for it first (same stream: stream order suffices).
struct NormWorkspace { double* part = nullptr; size_t cap = 0; int device = -1; double* own = nullptr; int own_dev = -1;
                       hipEvent_t done = nullptr; hipStream_t last = nullptr; bool used = false; };
static thread_local NormWorkspace g_norm_ws;
void release_stencil_workspace() {   // qmg_shutdown (qmg_runtime.hip)
  if (g_norm_ws.part) (void)hipFree(g_norm_ws.part);
  if (g_norm_ws.own) (void)hipFree(g_norm_ws.own);
  if (g_norm_ws.done) (void)hipEventDestroy(g_norm_ws.done);
  g_norm_ws = NormWorkspace();
}
int norm_result_slot(double** res) {
  int dev = 0;
  QMG_HIP_CHECK(hipGetDevice(&dev));
  NormWorkspace& ws = g_norm_ws;
  if (ws.own_dev != dev) { QMG_HIP_CHECK(hipMalloc((void**)&ws.own, sizeof(double) * 16)); ws.own_dev = dev; }
  *res = ws.own;
  return QMG_SUCCESS;
}

// kernel A2, the instantiation and grid of the plan
static int launch_pair_kernel(const StencilArgs& a, const StencilPlan& pl, hipStream_t st) {
  const dim3 grid((unsigned)pl.gx, (unsigned)pl.gy);
  return with_int<1, 2, 4>(pl.NC, [&](auto nc_c) {
    return with_int<2>(pl.P, [&](auto rows_c) {   // (ROWS = 1 was odd Ly: no lattice has it, valid_lattice)
      return with_bool((pl.flags & SPF_NORM) != 0, [&](auto norm_c) {
        return with_bool((pl.flags & SPF_PF) != 0, [&](auto pf_c) {
          constexpr int NC = decltype(nc_c)::value, ROWS = decltype(rows_c)::value;
          constexpr bool NORM = decltype(norm_c)::value, PF = decltype(pf_c)::value;
          if constexpr ((PF && NC != 1) || (NORM && NC == 4)) return (int)QMG_ERR_UNSUPPORTED;   // not built: prefetch is nc = 1's, the norm nc = 1 and 2's
          else return launch_kernel(k_stencil_pair<double, NC, ROWS, true, true, NORM, PF>, grid, (size_t)pl.smem, st, a);
        });
      });
    });
  });
}

// apply + |lhs_k|^2 in one pass: kernel A2 with NORM, then the partials summed in a fixed order
int launch_stencil_norm(StencilArgs& a, const StencilPlan& pl, double* norms_dev, hipStream_t st) {
  const long nparts = (long)pl.gy * pl.gx;            // one partial per block and system
  int dev = 0;
  QMG_HIP_CHECK(hipGetDevice(&dev));
  NormWorkspace& ws = g_norm_ws;
  if (ws.device != dev || ws.cap < (size_t)nparts * a.nrhs) {
    if (ws.part && ws.device == dev) QMG_HIP_CHECK(hipFree(ws.part));   // (synchronises: no launch still writes the old buffer)
    ws.part = nullptr; ws.cap = 0;
    if (ws.device != dev && ws.done) { (void)hipEventDestroy(ws.done); ws.done = nullptr; }   // (an event belongs to the device it was created on)
    ws.used = false;
    QMG_HIP_CHECK(hipMalloc((void**)&ws.part, sizeof(double) * (size_t)nparts * a.nrhs));
    if (const int rc = poison_new_scratch(ws.part, sizeof(double) * (size_t)nparts * a.nrhs)) return rc;
    ws.cap = (size_t)nparts * a.nrhs; ws.device = dev;
  }
  a.norm_part = ws.part;
  if (!ws.done) QMG_HIP_CHECK(hipEventCreateWithFlags(&ws.done, hipEventDisableTiming));
  if (ws.used && ws.last != st) QMG_HIP_CHECK(hipStreamWaitEvent(st, ws.done, 0));   // the previous call's partials are still being summed on another stream
  if (const int rc = launch_pair_kernel(a, pl, st)) return rc;
  if (const int rc = launch_kernel(k_apply_norm_final, dim3(a.nrhs), 0, st, ws.part, nparts, norms_dev)) return rc;
  QMG_HIP_CHECK(hipEventRecord(ws.done, st));
  ws.last = st; ws.used = true;
  return QMG_SUCCESS;
}

int launch_stencil_pair(const StencilArgs& a, const StencilPlan& pl, hipStream_t st) { return launch_pair_kernel(a, pl, st); }

int launch_stencil_elem(const StencilArgs& a, const StencilPlan& pl, hipStream_t st) {
  const dim3 grid((unsigned)pl.gx, (unsigned)pl.gy);
  return with_int<1, 2, 4>(pl.NC, [&](auto nc_c) {
    constexpr int NC = decltype(nc_c)::value;
    if (pl.storage & SST_V32) return launch_kernel(k_stencil_elem<float, NC, true, true>, grid, 0, st, a);
    return launch_kernel(k_stencil_elem<double, NC, true, true>, grid, 0, st, a);
  });
}

}  // namespace qmg
