// qmg_stencil_mfma.hip -- kernel C of the stencil apply: the coarse operators' multi-rhs apply on the matrix cores.
// The dispatcher (qmg_stencil_apply.hip) calls launch_stencil_mfma with the filled argument block.

#include "qmg_stencil_common.h"

namespace qmg {

// ---------------------------------------------------------------------------------------------------------------------
// Kernel C (nc in {8,12,16,24,32}, 2..16 right-hand sides per pass): the coarse apply as a real contraction on the f64
// matrix cores.  With k right-hand sides against one matrix read the per-site work is the (nc x nc) . (nc x k) product
//     out[r][k] (+)= sum_piece sum_c M_piece(x)[r][c] * X_k(nb_piece(x))[c]
// and the arithmetic intensity rises from 0.5 flop/B to ~0.5 k flop/B; 16 right-hand sides move 5 nc^2 + 32 nc complex
// per site instead of 16 (5 nc^2 + 2 nc).  One wavefront owns one output site.  v_mfma_f64_16x16x4_f64 tiles:
//     A (16 x 4)  = M[16 t + (lane&15)][4 s + (lane>>4)]       each lane's 16 B carries (re, im)
//     B (4 x 16)  = X_{lane&15}[4 s + (lane>>4)]                one right-hand side per MFMA column
//     C (16 x 16) : row = 16 t + 4 i + (lane>>4), column = lane&15 for accumulator register i      (f64 C/D map)
// A complex MAC is four real MFMAs (re += ar.br - ai.bi ; im += ar.bi + ai.br).  Rows / k-steps beyond nc and columns
// beyond the rhs count are fed zeros.
// Matrix stream: a site's piece is nc^2 contiguous complex; the wavefront reads it with fully coalesced non-temporal
// 1-KiB loads (lane-linear), parks it in its own LDS slice with odd row stride nc+1 (conflict-free operand reads), and
// pulls A fragments from there.  Operand-layout loads straight from HBM touch half a cache line per 4 lanes and ran at
// 4.5 TB/s with the MFMAs removed; the staged stream is what the 5.8 TB/s single-rhs kernels use.  The slice is private
// to the wavefront, so the write->read hand-off is a wavefront fence, not a block barrier; the global loads of piece
// p+2 are in flight while piece p+1 computes.  The own-site vector in B layout IS the shift term's operand in C layout
// (k-step s = 4 t + i holds row 16 t + 4 i + (lane>>4)); it is re-read from L2 in the epilogue.
typedef double v4d __attribute__((ext_vector_type(4)));
typedef float v4f32 __attribute__((ext_vector_type(4)));

// MODE 0: four real MFMAs per complex tile product (plain).
// MODE 1: at most 8 right-hand sides: columns 0-7 carry Re X_k, columns 8-15 Im X_k, so P = Re(M).[Xr|Xi] and
//         Q = Im(M).[Xr|Xi] are TWO MFMAs per tile product; the epilogue recombines re_k = P[k] - Q[k+8],
//         im_k = P[k+8] + Q[k] with one lane exchange (lane ^ 8).
// (A three-multiplication complex product for 9-16 right-hand sides was measured SLOWER than MODE 0 -- 4.09 vs 3.63 ms
// at 512^2, nc = 24, 16 rhs: the extra f64 adds and the third accumulator cost more than the saved MFMA -- and dropped.)
// The f64 matrix pipe sustains 48 TFLOP/s on this part (tools/mfma_f64_rate.hip), which at nc = 24 is 2.7 ms of plain
// MFMA work per 512^2 apply against 2.4 ms of HBM time -- the MFMA count, not the byte count, is what MODE 1 cuts.
// MODE 2 (9-16 right-hand sides, fp64, VL): the REAL form of the product -- [yr; yi] = [[Mr, -Mi], [Mi, Mr]] [xr; xi], a (2 nc x 2 nc) real
//         matrix against a (2 nc x 16) real right-hand side: ONE MFMA per 16 x 4 tile of it, each lane pulling the double it needs
//         (re or im of M[r][c], sign by quadrant) straight out of the complex LDS tile.  The MFMA count is 2 nc/16 (rounded up) x nc/2
//         per piece instead of MODE 0's 4 x ceil(nc/16) x ceil(nc/4): nc = 24: 36 instead of 48 (48 real rows fill three tiles exactly,
//         24 complex rows waste a quarter of two), nc = 8: 4 instead of 8.  At 16 systems the kernel is MFMA-bound, so that is its time.
// M16 (with M32): the matrices are stored as complex<half> (NC % 4 == 0): a lane's 16-B load carries four elements, widened to the complex<float>
// tile when they are parked; everything behind the tile is the M32 form.
// (Measured and dropped: the all-complex<float> MODE 1 form with two pieces of prefetch under a 128-register cap (4 wavefronts per SIMD): nc = 24
// spills 16 registers and goes 1.44 -> 1.61 ms, nc = 12 / 16 within 4 %.  With complex<half> matrices and complex<float> vectors the same
// launch takes 1.21 ms for HALF the matrix bytes: at 8 systems the kernel's floor is its per-piece chain of LDS hand-offs and dependent MFMAs
// (four accumulators), not the stream.)
// PAIR (NC = 16, MODE 1, VL): the wavefront owns TWO adjacent nc = 8 sites of a row.  Their 8 x 8 matrices sit on the diagonal of the 16 x 16
// tile (the off-diagonal blocks are zeroed once and never written), their vectors side by side in the 16-wide vector slice -- the two sites'
// own-site and y-neighbour vectors are contiguous in memory, the x-neighbours are found per lane (they wrap at the row ends).  Same MFMA
// count per site as the one-site form (a 16-row tile is half empty at nc = 8 either way), HALF the loads, LDS hand-offs and address
// arithmetic per site: at nc = 8 the one-site form is bound by its instruction issue, not by the stream or the matrix pipe.
template <int NC, int MODE, bool M32, bool V32, bool VL, bool M16 = false, bool PAIR = false>
__global__ __launch_bounds__(BLOCK, (MODE == 1 && NC <= 24) ? 3 : 1) void k_stencil_mfma(const StencilArgs a, const int nk) {
  static_assert(MODE != 2 || (VL && !M32 && NC % 2 == 0), "MODE 2: fp64, right-hand sides through the LDS slice");
  static_assert(!M16 || (M32 && NC % 4 == 0), "16-bit matrices: the fp32 tile path, quads that stay inside a row");
  static_assert(!PAIR || (NC == 16 && MODE == 1 && VL), "PAIR: two nc = 8 sites, packed columns, vectors through the LDS slice");
  constexpr int SNC = PAIR ? NC / 2 : NC;            // colours of ONE site
  constexpr int MEL = PAIR ? 2 * SNC * SNC : NC * NC;   // stored matrix elements per piece per wavefront
  constexpr int RT = (MODE == 2) ? (2 * NC + 15) / 16 : (NC + 15) / 16, KS = (MODE == 2) ? NC / 2 : (NC + 3) / 4;
  constexpr int NACC = (MODE == 2) ? 1 : 2;
  // PACK (MODE 1, NC % 16 == 8: nc = 24 and the one-site nc = 8; matrices stored narrow): the last row tile has eight rows, so its A operand
  // carries Re M of them in tile rows 0-7 and Im M of the same rows in tile rows 8-15, and ONE MFMA into acc[0][RT - 1] yields P (C rows
  // 0-7) and Q (C rows 8-15) instead of two MFMAs half of whose rows are zeros: 3 per k-step instead of 4 at nc = 24, 1 instead of 2 at
  // nc = 8.  Every element of C still accumulates the same products in the same order, so the output bits do not change.
  // Not with complex<double> matrices: that form sits at its register cap (163 of 168 VGPRs), the packed one spills 21 of them and was
  // measured 12-16 % SLOWER (nc = 24, 8 systems, 512^2: 2.44 -> 2.73 ms; profiles/kernelc_pack_multidot.txt).
  constexpr bool PACK = MODE == 1 && NC % 16 == 8 && !PAIR && M32;
  static_assert(!PACK || VL, "PACK: the epilogue through the vector slice");
  // LDS row stride in tile elements: fp64 tile nc+1 complex (odd: conflict-free 16-B reads); fp32-stored matrices keep the
  // tile as raw complex<float> with stride nc+2 (even: 16-B aligned pair stores) -- half the LDS and half the staging
  // registers, widened to fp64 only as an MFMA operand
  constexpr int RS = M32 ? NC + 2 : NC + 1;
  constexpr int NG = (MEL + WAVE - 1) / WAVE;     // staged 16-B elements per lane per piece
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
  cplx* mlds = reinterpret_cast<cplx*>(smem_raw) + (size_t)wave * NC * RS;                // fp64 tile
  float2* mlds32 = reinterpret_cast<float2*>(smem_raw) + (size_t)wave * NC * RS;          // fp32 tile (M32)
  const int lr = lane & 15, lq = lane >> 4;
  const int j = (PAIR ? 2 : 1) * (blockIdx.x * (BLOCK / WAVE) + wave);   // (PAIR: the first site of the pair; the host launches it for even hr only)
  if (j >= a.hr) return;                      // whole wavefront leaves; the kernel has no block barriers
  if constexpr (PAIR) {                       // the off-diagonal blocks of the tile: zero for the whole launch
    for (int e = lane; e < NC * RS; e += WAVE) { if (M32) mlds32[e] = make_float2(0.0f, 0.0f); else mlds[e] = cmake(0.0, 0.0); }
    wave_lds_handoff();
  }
  const int kcol = (MODE == 1) ? (lr & 7) : lr;   // right-hand side this lane's MFMA column belongs to
  const bool kval = kcol < nk;                 // ... and whether it exists
  const long koff = (long)system_index(a, kcol & 15) * a.vec_stride;

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
    const int yp = (y + 1 == a.Ly) ? 0 : y + 1;
    const int ym = (y == 0) ? a.Ly - 1 : y - 1;
    int jp = j + s; if (jp == a.hr) jp = 0;
    int jm = j + s - 1; if (jm < 0) jm = a.hr - 1;
    // piece slots in the reference's accumulation order: clover, +x, +y, -x, -y
    const long nb[5] = {site, opp + (long)y * a.hr + jp, opp + (long)yp * a.hr + j, opp + (long)y * a.hr + jm, opp + (long)ym * a.hr + j};
    const bool act[5] = {do_clover, (bool)(hop_mask & 1u), (bool)(hop_mask & 2u), (bool)(hop_mask & 4u), (bool)(hop_mask & 8u)};

    // complex<float> matrices AND vectors: the products run on the f32 matrix pipe (v_mfma_f32_16x16x4_f32, twice the f64
    // rate on this part; same A / B / C lane maps as the f64 instruction), accumulating in fp32 like the rest of the fp32 path
    constexpr bool F32M = M32 && V32;
    typedef typename std::conditional<F32M, v4f32, v4d>::type accv;
    accv acc[NACC][RT];   // MODE 0: (re, im); MODE 1: (P, Q)
#pragma unroll
    for (int n = 0; n < NACC; n++)
#pragma unroll
      for (int t = 0; t < RT; t++) {
        if constexpr (F32M) acc[n][t] = (v4f32){0.0f, 0.0f, 0.0f, 0.0f};
        else acc[n][t] = (v4d){0.0, 0.0, 0.0, 0.0};
      }

    constexpr int NGP = M16 ? (MEL / 4 + WAVE - 1) / WAVE : (MEL / 2 + WAVE - 1) / WAVE;   // staged PAIRS (16-bit: QUADS) per lane per piece (narrow-stored matrices)
    // staging registers for the matrix stream (a second set, two pieces of prefetch, was measured SLOWER: 8 rhs 2.88 -> 3.10
    // ms; the registers cost a resident wavefront and the stream was not the limit -- profiles/r02_mfma_kernelC_variants.txt)
    constexpr int NGS = M32 ? NGP : NG;
    // How many pieces of the matrix stream a wavefront keeps in flight (register sets): ONE.  Deeper prefetch was measured for every shape
    // (register sets chosen by the staged elements per lane, <= 1 / <= 3 / <= 5; tools/kernelc_bench.py): two
    // sets cost fp64 nc = 24 a resident wavefront (round 2: 2.88 -> 3.10 ms); for the half-size fp32-stored stream they fit (124 -> 147 VGPRs)
    // and changed nothing (nc = 24, 8 systems: 1.43 -> 1.54 ms), and five sets at nc = 8 were slower (1.64 -> 1.83 ms): the wavefronts are
    // parked 60 % of their cycles (SQ_WAIT_ANY) with the matrix pipe 37 % busy, but more loads in flight per wavefront do not shorten that.
    // What did: the right-hand sides' system indices without a memory access (system_index) -- a.ridx[k] with a per-lane k is a vector load from
    // the kernel arguments whose result the vector loads' addresses waited for, one more memory latency in front of every piece (fp64 nc = 24,
    // 16 systems: 3.47 -> 2.90-3.00 ms; nc = 16 fp32-stored matrices, 8 systems: 0.905 -> 0.74 ms; nc = 12 fp64: 0.83 -> 0.75 ms).
    constexpr int PFD = 1;
    cplx G[PFD][NGS];   // M32: raw bits of two complex<float> per entry
    // Right-hand sides.  VL = false (round 1): each lane loads its B-operand entries X_k[4q + lq] straight from global memory --
    // 16 right-hand sides x 64-byte pieces per instruction, 16 cache lines touched per load, 6 loads per piece; going from 4
    // to 8 right-hand sides cost 0.48 ms of a 2.9 ms apply.  VL = true: the piece's nk x NC block is loaded COALESCED
    // (lane-linear over [k][c]: whole 384-byte site vectors), parked in a second LDS slice of the wavefront with rows padded
    // to NC+1 (conflict-free 16-byte fragment reads), and the B fragments are read from there just in time.  The epilogue
    // goes back the same way: results into the slice, then coalesced read-modify-write of the output vectors.
    constexpr int XS = NC + 1;                                   // padded row of the vector slice
    constexpr int XROWS = (MODE == 1) ? 8 : 16;                  // right-hand sides a pass can hold (MODE 1: at most 8)
    constexpr int NXG = (XROWS * NC + WAVE - 1) / WAVE;          // staged vector elements per lane per piece
    constexpr int XPF = (VL && NXG <= 2) ? PFD : 1;               // ... and of the right-hand sides (small blocks only: nc = 8, 12)
    // (the staged right-hand sides stay in their STORAGE form until they are parked: widening a complex<float> entry right after its load made the
    // compiler wait for each load in turn -- load, s_waitcnt vmcnt(0), convert, next load -- BEFORE it issued the piece's matrix loads: three
    // serial memory latencies per piece in the complex<float> forms, none of them overlapped with the MFMAs of the piece in hand)
    typedef typename std::conditional<V32, double, cplx>::type xraw;   // V32: the raw bits of a complex<float>
    xraw XG[XPF][VL ? NXG : 1];
    auto ld_xraw = [](const void* base, long i) -> xraw {       // base == nullptr: a column beyond the systems of the pass (zero)
      if constexpr (V32) return base ? reinterpret_cast<const double*>(base)[i] : 0.0;
      else return base ? reinterpret_cast<const cplx*>(base)[i] : cmake(0.0, 0.0);
    };
    auto widen_xraw = [](xraw v) -> cplx {
      if constexpr (V32) { struct F2 { float x, y; }; const F2 f = __builtin_bit_cast(F2, v); return cmake((double)f.x, (double)f.y); }
      else return v;
    };
    int ksys[VL ? NXG : 1];   // the system each of this lane's staged vector elements belongs to (row-invariant, no memory access: system_index)
    if constexpr (VL) {
#pragma unroll
      for (int g = 0; g < NXG; g++) { const int k = (g * WAVE + lane) / NC; ksys[g] = system_index(a, k < 16 ? k : 0); }
    }
    cplx* xlds = reinterpret_cast<cplx*>(smem_raw + (M32 ? sizeof(float2) : sizeof(cplx)) * (size_t)(BLOCK / WAVE) * NC * RS) + (size_t)wave * XROWS * XS;
    // MODE 1 needs only the half of X its column carries (re for columns 0-7, im for 8-15): one double per k-step
    typename std::conditional<MODE == 1, double, cplx>::type B[2][VL ? 1 : KS];
    auto nb_of = [&](int pc) -> long {            // neighbour site of piece slot pc
      return pc == 0 ? site : pc == 1 ? nb[1] : pc == 2 ? nb[2] : pc == 3 ? nb[3] : nb[4];
    };
    auto load_matrix = [&](int pc, int gs) {      // global -> registers, lane-linear, non-temporal
      const cplx* mbase = (pc == 0) ? a.clover : a.hopping;
      const long moff = ((pc == 0) ? 0 : (long)(pc - 1) * a.size_cm) + site * (SNC * SNC);   // (PAIR: the two sites' matrices are adjacent)
      if (M32) {   // pairs of complex<float> (M16: quads of complex<half>): 16 B per lane per load, kept as raw bits
#pragma unroll
        for (int g = 0; g < NGP; g++) {
          constexpr int PER = M16 ? 4 : 2;
          const int el = PER * (g * WAVE + lane);
          if (MEL % (PER * WAVE) == 0 || el < MEL) {
            const double* pp = M16 ? reinterpret_cast<const double*>(reinterpret_cast<const unsigned*>(mbase) + moff + el)
                                   : reinterpret_cast<const double*>(reinterpret_cast<const float2*>(mbase) + moff + el);
            G[gs][g].x = __builtin_nontemporal_load(pp);
            G[gs][g].y = __builtin_nontemporal_load(pp + 1);
          } else G[gs][g] = cmake(0.0, 0.0);
        }
      } else {
#pragma unroll
        for (int g = 0; g < NG; g++) {
          const int el = g * WAVE + lane;
          G[gs][g] = (MEL % WAVE == 0 || el < MEL) ? ldm<M32, true>(mbase, moff + el) : cmake(0.0, 0.0);
        }
      }
    };
    auto load_vectors = [&](int pc, int set, int xs) {    // the k right-hand sides at the piece's neighbour site (xs: XG register set)
      // a y-slab's rows -1 / Ly: the piece's neighbour row comes from the halo buffer ([system][parity][hr][NC]; a row-uniform choice)
      const bool h_hi = pc == 2 && a.halo_hi && y + 1 == a.Ly, h_lo = pc == 4 && a.halo_lo && y == 0;
      const void* vbase = h_hi ? a.halo_hi : h_lo ? a.halo_lo : a.rhs;
      const long vsite = (h_hi || h_lo) ? (long)(1 - p) * a.hr + j : nb_of(pc);
      const long vstride = (h_hi || h_lo) ? a.halo_stride : a.vec_stride;
      if constexpr (VL && PAIR) {                 // [k][two sites x 8]: the second site's x-neighbour is found per lane (row-end wrap)
        const int sp = (lane & 15) >> 3;          // (NC = 16 divides the wavefront: column = lane % 16 for every g)
        long vs = vsite + sp;                     // own site and y-neighbours: adjacent sites
        if (pc == 1) { int jq = j + sp + s; if (jq >= a.hr) jq -= a.hr; vs = opp + (long)y * a.hr + jq; }
        if (pc == 3) { int jq = j + sp + s - 1; if (jq < 0) jq += a.hr; vs = opp + (long)y * a.hr + jq; }
        const long so = vs * SNC + (lane & 7);
#pragma unroll
        for (int g = 0; g < NXG; g++) {
          const int k = (g * WAVE + lane) / NC;
          XG[xs][g] = ld_xraw((k < nk) ? vbase : nullptr, (long)ksys[g] * vstride + so);
        }
      } else if constexpr (VL) {                  // lane-linear over [k][c]: element e = g*64 + lane -> (k = e / NC, c = e % NC)
        const long so = vsite * NC;
#pragma unroll
        for (int g = 0; g < NXG; g++) {
          const int e = g * WAVE + lane;
          const int k = e / NC, c = e - k * NC;
          XG[xs][g] = ld_xraw((k < nk) ? vbase : nullptr, (long)ksys[g] * vstride + so + c);
        }
      } else {
        const long xo = (long)system_index(a, kval ? (kcol & 15) : 0) * vstride + vsite * NC;    // B-operand layout straight from global memory (a column beyond the pass: system 0's address, value zeroed)
        typename XRaw<V32>::type xr[KS];            // all of them requested before any is widened
        // (unconditional: a lane whose column is beyond the pass reads the pass's first system, a k-step beyond nc reads entry 0; both are zeroed
        // below.  A divergent branch around each load closed it with a full wait.)
#pragma unroll
        for (int q = 0; q < KS; q++) {
          const int c = 4 * q + lq;
          xr[q] = ldv_raw<V32>(vbase, xo + ((NC % 4 == 0 || c < NC) ? c : 0));
        }
#pragma unroll
        for (int q = 0; q < KS; q++) {
          const int c = 4 * q + lq;
          const cplx xw = widen_raw<V32>(xr[q]);
          const cplx xv = (kval && (NC % 4 == 0 || c < NC)) ? xw : cmake(0.0, 0.0);
          if constexpr (MODE == 1) B[set][q] = (lr < 8) ? xv.x : xv.y;
          else B[set][q] = xv;
        }
      }
    };
    auto park_piece = [&](int gs, int xs) {       // registers -> this wavefront's LDS slice, padded rows
      wave_lds_handoff();                         // the previous piece's fragment reads are done
      if (M32) {
#pragma unroll
        for (int g = 0; g < NGP; g++) {
          constexpr int PER = M16 ? 4 : 2;
          const int el = PER * (g * WAVE + lane);
          if (MEL % (PER * WAVE) == 0 || el < MEL) {
            // tile position of stored element el: row-major nc x nc -- PAIR: site sp = el / 64 owns the diagonal block (sp, sp)
            const int trow = PAIR ? (el >> 6) * SNC + ((el & 63) >> 3) : el / NC, tcol = PAIR ? (el >> 6) * SNC + (el & 7) : el % NC;
            if constexpr (M16) {   // (re, im) x 4 halves -> two 16-B stores of complex<float> pairs (RS even, el % 4 == 0: aligned, same row)
              typedef _Float16 h8 __attribute__((ext_vector_type(8)));
              typedef float f4 __attribute__((ext_vector_type(4)));
              const h8 hv = __builtin_bit_cast(h8, G[gs][g]);
              const f4 w0 = {(float)hv[0], (float)hv[1], (float)hv[2], (float)hv[3]}, w1 = {(float)hv[4], (float)hv[5], (float)hv[6], (float)hv[7]};
              float2* dst = mlds32 + trow * RS + tcol;
              *reinterpret_cast<f4*>(dst) = w0;
              *reinterpret_cast<f4*>(dst + 2) = w1;
            } else
              *reinterpret_cast<cplx*>(mlds32 + trow * RS + tcol) = G[gs][g];   // 16-B aligned: RS, el even
          }
        }
      } else {
#pragma unroll
        for (int g = 0; g < NG; g++) {
          const int el = g * WAVE + lane;
          const int trow = PAIR ? (el >> 6) * SNC + ((el & 63) >> 3) : el / NC, tcol = PAIR ? (el >> 6) * SNC + (el & 7) : el % NC;
          if (MEL % WAVE == 0 || el < MEL) mlds[trow * RS + tcol] = G[gs][g];
        }
      }
      if constexpr (VL) {                         // the right-hand sides of the same piece, rows padded
#pragma unroll
        for (int g = 0; g < NXG; g++) {
          const int e = g * WAVE + lane;
          const int k = e / NC, c = e - k * NC;
          if (k < XROWS) xlds[k * XS + c] = widen_xraw(XG[xs][g]);
        }
      }
      wave_lds_handoff();
    };
    auto mac_piece = [&](int set) {
      if constexpr (MODE == 2) {
        // operands of k-step q+1 are read from LDS while the MFMAs of k-step q issue; the scheduling barrier keeps the compiler from
        // hoisting ALL 48 operand reads of the piece in front of the first MFMA (238 VGPRs, one wavefront per SIMD)
        double av[2][RT], bv[2];
        auto fetch = [&](int q, int slot) {
          const int K = 4 * q + lq;                      // 0 .. 2 nc - 1: the first nc multiply Re x, the rest Im x
          const bool khi = K >= NC;
          const int kc = khi ? K - NC : K;
          bv[slot] = reinterpret_cast<const double*>(xlds + kcol * XS + kc)[khi ? 1 : 0];
#pragma unroll
          for (int t = 0; t < RT; t++) {
            const int R = 16 * t + lr;                   // 0 .. 2 nc - 1: the first nc are Re y, the rest Im y
            const bool rhi = R >= NC;
            const int rr = rhi ? R - NC : R;
            double v = 0.0;
            if ((2 * NC) % 16 == 0 || R < 2 * NC) {
              v = reinterpret_cast<const double*>(mlds + rr * RS + kc)[rhi != khi ? 1 : 0];   // diagonal quadrants: Re M; off-diagonal: Im M ...
              if (!rhi && khi) v = -v;                                                        // ... with a minus in the upper right one
            }
            av[slot][t] = v;
          }
        };
        fetch(0, 0);
#pragma unroll
        for (int q = 0; q < KS; q++) {
          if (q + 1 < KS) fetch(q + 1, (q + 1) & 1);
#pragma unroll
          for (int t = 0; t < RT; t++) acc[0][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[q & 1][t], bv[q & 1], acc[0][t], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
      } else {
#pragma unroll
      for (int q = 0; q < KS; q++) {
        cplx Af[RT];
#pragma unroll
        for (int t = 0; t < RT; t++) {
          const int r = 16 * t + lr, c = 4 * q + lq;
          if (PACK && t == RT - 1) {   // both halves of the tile read the row's element: tile rows 0-7 take its real part, rows 8-15 its imaginary part (into Af.x)
            Af[t] = cmake((double)reinterpret_cast<const float*>(mlds32 + (r - (lr & 8)) * RS + c)[lr >> 3], 0.0);
          } else if (M32) {
            const float2 mf = ((NC % 16 == 0 || r < NC) && (NC % 4 == 0 || c < NC)) ? mlds32[r * RS + c] : make_float2(0.0f, 0.0f);
            Af[t] = cmake((double)mf.x, (double)mf.y);
          } else
            Af[t] = ((NC % 16 == 0 || r < NC) && (NC % 4 == 0 || c < NC)) ? mlds[r * RS + c] : cmake(0.0, 0.0);
        }
        if constexpr (VL) {                       // B fragment of this k-step: X_{column}[4q + lq] from the wavefront's vector slice
          const int c = 4 * q + lq;
          if constexpr (PACK) B[set][0] = reinterpret_cast<const double*>(xlds + kcol * XS + c)[lr >> 3];   // (NC % 4 == 0) the half this column carries, read alone
          else {
          const cplx xv = (NC % 4 == 0 || c < NC) ? xlds[kcol * XS + c] : cmake(0.0, 0.0);
          if constexpr (MODE == 1) B[set][0] = (lr < 8) ? xv.x : xv.y;
          else B[set][0] = xv;
          }
        }
        constexpr int qb = VL ? 0 : 1;            // VL: the fragment sits in slot 0; else slot q
        if constexpr (F32M && MODE == 0) {
#pragma unroll
          for (int t = 0; t < RT; t++) {
            acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x4f32((float)Af[t].x, (float)B[set][q * qb].x, acc[0][t], 0, 0, 0);
            acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x4f32((float)Af[t].x, (float)B[set][q * qb].y, acc[1][t], 0, 0, 0);
          }
#pragma unroll
          for (int t = 0; t < RT; t++) {
            acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(-(float)Af[t].y, (float)B[set][q * qb].y, acc[0][t], 0, 0, 0);
            acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x4f32((float)Af[t].y, (float)B[set][q * qb].x, acc[1][t], 0, 0, 0);
          }
        } else if constexpr (F32M) {
#pragma unroll
          for (int t = 0; t < RT; t++) {
            if (PACK && t == RT - 1) {
              acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x4f32((float)Af[t].x, (float)B[set][q * qb], acc[0][t], 0, 0, 0);
            } else {
              acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x4f32((float)Af[t].x, (float)B[set][q * qb], acc[0][t], 0, 0, 0);
              acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x4f32((float)Af[t].y, (float)B[set][q * qb], acc[1][t], 0, 0, 0);
            }
          }
        } else if constexpr (MODE == 0) {
#pragma unroll
          for (int t = 0; t < RT; t++) {
            acc[0][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(Af[t].x, B[set][q * qb].x, acc[0][t], 0, 0, 0);
            acc[1][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(Af[t].x, B[set][q * qb].y, acc[1][t], 0, 0, 0);
          }
#pragma unroll
          for (int t = 0; t < RT; t++) {
            acc[0][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(-Af[t].y, B[set][q * qb].y, acc[0][t], 0, 0, 0);
            acc[1][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(Af[t].y, B[set][q * qb].x, acc[1][t], 0, 0, 0);
          }
        } else {
#pragma unroll
          for (int t = 0; t < RT; t++) {
            if (PACK && t == RT - 1) {
              acc[0][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(Af[t].x, B[set][q * qb], acc[0][t], 0, 0, 0);
            } else {
              acc[0][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(Af[t].x, B[set][q * qb], acc[0][t], 0, 0, 0);
              acc[1][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(Af[t].y, B[set][q * qb], acc[1][t], 0, 0, 0);
            }
          }
        }
      }
      }
    };

    // software pipeline over the ACTIVE piece slots (activity is uniform over the block): PFD pieces of the matrix stream (XPF of the
    // right-hand sides) are requested ahead of the piece that computes.  Register-set indices are compile-time constants after unrolling;
    // requests are issued oldest-needed-first, so the wait in front of a park leaves the younger ones in flight.
    unsigned am = (act[0] ? 1u : 0u) | (act[1] ? 2u : 0u) | (act[2] ? 4u : 0u) | (act[3] ? 8u : 0u) | (act[4] ? 16u : 0u);
    const int n = __popc(am);
    int lst[5];   // the active slots in order (constant indices only: stays in registers)
#pragma unroll
    for (int i = 0; i < 5; i++) { lst[i] = am ? __ffs(am) - 1 : 0; am &= am - 1; }
#pragma unroll
    for (int i = 0; i < PFD; i++)
      if (i < n) {
        load_matrix(lst[i], i);
        if (i == 0 || XPF > 1) load_vectors(lst[i], i & 1, XPF > 1 ? i : 0);
      }
#pragma unroll
    for (int i = 0; i < 5; i++) {
      if (i < n) {
        park_piece(i % PFD, XPF > 1 ? i % PFD : 0);   // the sets that held piece i are free again after this
        if (XPF == 1 && i + 1 < n) load_vectors(lst[i + 1], (i + 1) & 1, 0);
        if (i + PFD < n) {
          load_matrix(lst[i + PFD], i % PFD);
          if (XPF > 1) load_vectors(lst[i + PFD], (i + PFD) & 1, i % PFD);
        }
        mac_piece(i & 1);
      }
    }

    // epilogue: shift, accumulate, store.  Lane (lq, lr) owns rows 16 t + 4 i + lq of right-hand side lr.
    const double sg = p ? -1.0 : 1.0;
    if constexpr (VL) {
      // results into the vector slice [k][r] (the last piece's fragment reads are done), then lane-linear over [k][r]:
      // coalesced own-site read for the shift term, coalesced read-modify-write of the output
      wave_lds_handoff();
      if constexpr (MODE == 2) {   // real row R of system lr: Re (R < nc) or Im of output row R mod nc
#pragma unroll
        for (int t = 0; t < RT; t++) {
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const int R = 16 * t + 4 * i + lq;
            if ((2 * NC) % 16 == 0 || R < 2 * NC) reinterpret_cast<double*>(xlds + kcol * XS + (R >= NC ? R - NC : R))[R >= NC ? 1 : 0] = acc[0][t][i];
          }
        }
      } else {
#pragma unroll
      for (int t = 0; t < RT; t++) {
        if constexpr (PACK) {
          if (t == RT - 1) {   // the packed tile: P in C rows 0-7, Q of the same matrix rows in C rows 8-15 of ONE accumulator
            if constexpr (F32M) {   // f32 C/D map: rows 4 lq + i; Q sits in lane ^ 32, the other column half in lane ^ 8, both in lane ^ 40
#pragma unroll
              for (int i = 0; i < 4; i++) {
                const float own = acc[0][t][i];
                const double pp = (double)__shfl_xor(own, 8), q0 = (double)__shfl_xor(own, 32), qp = (double)__shfl_xor(own, 40);
                if (lq < 2 && lr < 8) xlds[kcol * XS + 16 * t + 4 * lq + i] = cmake((double)own - qp, pp + q0);
              }
            } else {                // f64 C/D map: rows 4 i + lq; P is register i, Q register i + 2
#pragma unroll
              for (int i = 0; i < 2; i++) {
                const double pp = __shfl_xor(acc[0][t][i], 8), qp = __shfl_xor(acc[0][t][i + 2], 8);
                if (lr < 8) xlds[kcol * XS + 16 * t + 4 * i + lq] = cmake(acc[0][t][i] - qp, pp + acc[0][t][i + 2]);
              }
            }
            continue;
          }
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int r = F32M ? 16 * t + 4 * lq + i : 16 * t + 4 * i + lq;   // C/D row of accumulator register i: the f32 instruction puts rows 4 lq .. 4 lq + 3 in a lane, the f64 one rows lq, lq + 4, ...
          cplx v;
          if (MODE == 0) v = cmake((double)acc[0][t][i], (double)acc[NACC - 1][t][i]);
          else {   // partner lane (lr ^ 8) holds the other half of the packed columns
            const double pp = (double)__shfl_xor(acc[0][t][i], 8), qp = (double)__shfl_xor(acc[NACC - 1][t][i], 8);
            v = cmake((double)acc[0][t][i] - qp, pp + (double)acc[NACC - 1][t][i]);
          }
          if (r < NC && (MODE != 1 || lr < 8)) xlds[kcol * XS + r] = v;
        }
      }
      }
      wave_lds_handoff();
#pragma unroll
      for (int g = 0; g < NXG; g++) {
        const int e = g * WAVE + lane;
        const int k = e / NC, r = e - k * NC;
        if (k < nk) {
          cplx v = xlds[k * XS + r];
          const long o = (long)ksys[g] * a.vec_stride + site * SNC + r;   // (PAIR: the second site's vector follows the first's)
          if (do_shift) {
            const double dg = (SNC % 2 == 0) ? (((PAIR ? (r & (SNC - 1)) : r) < SNC / 2) ? 1.0 : -1.0) : 0.0;
            const cplx sh = cmake(a.shift[0] + sg * a.eo_shift[0] + dg * a.dof_shift[0], a.shift[1] + sg * a.eo_shift[1] + dg * a.dof_shift[1]);
            cmac(v, sh, ldv<V32>(a.rhs, o));
          }
          if (!do_zero) v = cadd(ldv<V32>(a.lhs, o), v);
          stv<V32>(a.lhs, o, v);
        }
      }
      wave_lds_handoff();   // the next row's first park must not overtake these reads
    } else {
#pragma unroll
      for (int t = 0; t < RT; t++) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int r = F32M ? 16 * t + 4 * lq + i : 16 * t + 4 * i + lq;   // C/D row of accumulator register i: the f32 instruction puts rows 4 lq .. 4 lq + 3 in a lane, the f64 one rows lq, lq + 4, ...
          cplx v;
          if (MODE == 0) v = cmake((double)acc[0][t][i], (double)acc[NACC - 1][t][i]);
          else {   // partner lane (lr ^ 8) holds the other half of the packed columns
            const double pp = (double)__shfl_xor(acc[0][t][i], 8), qp = (double)__shfl_xor(acc[NACC - 1][t][i], 8);
            v = cmake((double)acc[0][t][i] - qp, pp + (double)acc[NACC - 1][t][i]);
          }
          if (r < NC && kval && (MODE != 1 || lr < 8)) {
            const long o = koff + site * NC + r;
            if (do_shift) {
              const double dg = (NC % 2 == 0) ? ((r < NC / 2) ? 1.0 : -1.0) : 0.0;
              const cplx sh = cmake(a.shift[0] + sg * a.eo_shift[0] + dg * a.dof_shift[0], a.shift[1] + sg * a.eo_shift[1] + dg * a.dof_shift[1]);
              cmac(v, sh, ldv<V32>(a.rhs, o));
            }
            if (!do_zero) v = cadd(ldv<V32>(a.lhs, o), v);
            stv<V32>(a.lhs, o, v);
          }
        }
      }
    }
  }
}

int g_stencil_mfma = 1;   // tuning knob: 1 = multi-rhs applies with nc in {8,12,16,24,32} run on the f64 matrix cores (kernel C); 2 = same, plain 4-MFMA products; 0 = off

// kernel C: one pass of up to 16 right-hand sides, from system k0 of the call on, sharing one read of the matrices
int launch_stencil_mfma(const StencilArgs& a, const StencilPlan& pl, int k0, hipStream_t st) {
  const dim3 grid((unsigned)pl.gx, (unsigned)pl.gy);
  const size_t smem = (size_t)pl.smem;
  const int nk = pl.K;
  StencilArgs b = a;
  b.lhs = (char*)a.lhs + (size_t)k0 * a.vec_stride * (a.vec32 ? 8 : 16);
  b.rhs = (const char*)a.rhs + (size_t)k0 * a.vec_stride * (a.vec32 ? 8 : 16);
  if (pl.flags & SPF_PAIR) {
    // nc = 8, up to 8 systems, whole lattice: two sites per wavefront (PAIR)
    return with_storage(pl, [&](auto m32, auto v32, auto m16) {
      return launch_kernel(k_stencil_mfma<16, 1, decltype(m32)::value, decltype(v32)::value, true, decltype(m16)::value, true>, grid, smem, st, b, nk);
    });
  }
  return with_int<8, 12, 16, 24, 32>(pl.NC, [&](auto nc_c) {
    return with_int<0, 1, 2>(pl.P, [&](auto mode_c) {
      return with_storage(pl, [&](auto m32, auto v32, auto m16) {
        constexpr int NC = decltype(nc_c)::value, MODE = decltype(mode_c)::value;
        constexpr bool M32 = decltype(m32)::value;
        if constexpr (MODE == 2 && M32) return (int)QMG_ERR_UNSUPPORTED;   // not built: the real form is fp64 only (mode is 2 for fp64 storage only)
        else return launch_kernel(k_stencil_mfma<NC, MODE, M32, decltype(v32)::value, !(MODE == 0 && M32), decltype(m16)::value>, grid, smem, st, b, nk);
      });
    });
  });
}

}  // namespace qmg
