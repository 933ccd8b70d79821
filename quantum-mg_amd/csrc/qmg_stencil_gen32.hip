// qmg_stencil_gen32.hip -- kernel B32 of the stencil apply: kernel B (qmg_stencil_gen.hip) for matrices stored as complex<float> or
// complex<half>, the tile kept in fp32 end to end.  A unit of its own because the two kernels' instantiations (72 here, 144 there) compile in
// parallel.  The dispatcher (qmg_stencil_apply.hip) calls launch_stencil_gen32 with the filled argument block.

#include "qmg_stencil_common.h"

namespace qmg {

// Kernel B32 (opt-in complex<float> matrix storage, even nc): kernel B with the tile kept in fp32 end to end -- 16-B
// loads carry two matrix elements, the staging registers and the LDS tile hold raw float pairs (half the registers, half
// the LDS: twice the resident blocks), and an element is widened to fp64 only when it is multiplied.  PP = staged PAIRS per
// thread.  Row stride nc + 2 floats-pairs: even (16-B aligned pair stores) and conflict-free for the 8-byte row reads.
// M16: the matrices are stored as complex<half> (qmg_stencil_apply_mat16; nc a multiple of 4): a 16-B load carries FOUR elements (PP = staged quads
// per thread), which are widened to complex<float> when they are parked -- the LDS tile and everything behind it are those of the fp32 form.
template <int PP, int KR, bool V32, bool EPI = false, bool M16 = false>
__global__ __launch_bounds__(BLOCK) void k_stencil_gen32(const StencilArgs a, const int nc, const GenLayout L) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int rs32 = nc + 2;
  float2* mlds = reinterpret_cast<float2*>(smem_raw);                                     // [S*nc rows][rs32] complex<float>
  cplx* xlds = reinterpret_cast<cplx*>(smem_raw + (((size_t)L.S * nc * rs32 * 8 + 15) & ~(size_t)15));   // [KR][S][nc]
  cplx* red = xlds + (size_t)KR * L.S * nc;                                               // [H][S*nc]

  const int tid = threadIdx.x;
  const int rows = L.S * nc;             // (s, r) pairs in this block
  const int h = tid / rows;              // slice id (threads beyond H*rows idle in the compute phase)
  const int sr = tid - h * rows;
  const bool worker = h < L.H;
  const int s_of = sr / nc;
  const int r_of = sr - s_of * nc;
  const int cchunk = (nc + L.H - 1) / L.H;
  const int c0 = h * cchunk;
  const int c1 = (c0 + cchunk < nc) ? c0 + cchunk : nc;

  const int j0 = blockIdx.x * L.S;
  const int nsite = (a.hr - j0 < L.S) ? a.hr - j0 : L.S;    // ragged last tile
  const long nc2 = (long)nc * nc;
  double edots[3] = {0.0, 0.0, 0.0};   // MR dots of the epilogue (EPI instantiations: one system per launch)

  for (int row = blockIdx.y; row < a.nrows; row += gridDim.y) {
    const int p = (a.par_count == 2) ? (row & 1) : a.par_first;
    const int y = (a.par_count == 2) ? (row >> 1) : row;
    const bool do_clover = a.clover && ((a.pieces >> p) & 1u);
    const unsigned hop_mask = a.hopping ? ((a.pieces >> (2 + 4 * p)) & 0xFu) : 0u;
    const bool do_shift = (a.pieces >> (10 + p)) & 1u;
    const bool do_zero = (a.pieces >> (12 + p)) & 1u;
    const unsigned piece_mask = hop_mask | (do_clover ? 16u : 0u);   // bit 4 = clover

    const long site0 = (long)p * a.half_vol + (long)y * a.hr + j0;
    const long opp = (long)(1 - p) * a.half_vol;
    const int s = (y + p) & 1;
    const int yp = (y + 1 == a.Ly) ? 0 : y + 1;
    const int ym = (y == 0) ? a.Ly - 1 : y - 1;
    cplx e_ov = cmake(0.0, 0.0), e_dv = cmake(0.0, 0.0);   // the epilogue's operands of this thread's output element, requested up front
    if (EPI && h == 0 && s_of < nsite) {
      const long o = rhs_offset(a, 0) + (site0 + s_of) * nc + r_of;
      if (a.epi.other) e_ov = ldv<V32>(a.epi.other, o);
      if (a.epi.dotv) e_dv = (a.epi.dotv == a.epi.other) ? e_ov : ldv<V32>(a.epi.dotv, o);
    }

    for (int k0 = 0; k0 < a.nrhs; k0 += KR) {
      const int nk = (a.nrhs - k0 < KR) ? a.nrhs - k0 : KR;
      cplx acc[KR];
#pragma unroll
      for (int kk = 0; kk < KR; kk++) acc[kk] = cmake(0.0, 0.0);

      // piece order: clover (4), +x, +y, -x, -y  -- the reference's accumulation order.  The active pieces (uniform over the block) are
      // walked by a loop the compiler unrolls, so the staging-register sets have compile-time indices: PF pieces are requested ahead of the
      // one that computes.  PF = 2 for the 16-bit storage: a piece is half the bytes of the fp32 form, so with one piece ahead a block
      // had half the bytes in flight and the kernel stopped at 0.61 of the HBM rate; two sets of quads cost what one set of pairs does.
      constexpr int PF = M16 ? 2 : 1;
      double2 stage[PF][PP];   // raw bits of two complex<float> (four complex<half>) each
      typename XRaw<V32>::type xstage[PF][KR];   // (storage form: widened when they are parked)
#pragma unroll
      for (int f = 0; f < PF; f++)
#pragma unroll
        for (int kk = 0; kk < KR; kk++) xstage[f][kk] = zero_raw<V32>();
      // bit oi of om: the oi-th piece of the order {clover, +x, +y, -x, -y} is active
      unsigned om = ((piece_mask >> 4) & 1u) | ((piece_mask & 0xFu) << 1);
      const int npc = __popc(om);
      int lst[5];
#pragma unroll
      for (int i = 0; i < 5; i++) { const int oi = om ? __ffs(om) - 1 : 0; lst[i] = (oi == 0) ? 4 : oi - 1; om &= om - 1; }
      auto prefetch = [&](int piece, int f) {
        const cplx* mbase = (piece == 4) ? a.clover : a.hopping;                 // (element offsets, so that the same
        long moff = (piece == 4) ? site0 * nc2 : (long)piece * a.size_cm + site0 * nc2;   //  code serves both matrix widths)
        const int lim = nsite * (int)nc2;
        const float2* m32 = reinterpret_cast<const float2*>(mbase) + moff;
        const unsigned* m16 = reinterpret_cast<const unsigned*>(mbase) + moff;   // complex<half>: 4 B per element
#pragma unroll
        for (int q = 0; q < PP; q++) {
          const int el = (M16 ? 4 : 2) * (tid + q * BLOCK);
          if (el < lim) {
            const double* pp = M16 ? reinterpret_cast<const double*>(m16 + el) : reinterpret_cast<const double*>(m32 + el);
            stage[f][q].x = __builtin_nontemporal_load(pp);
            stage[f][q].y = __builtin_nontemporal_load(pp + 1);
          } else stage[f][q] = make_double2(0.0, 0.0);
        }
        // neighbour vector element for (site, c) = tid / nc, tid % nc
        if (tid < nsite * nc) {
          const int sl = tid / nc, cc = tid - sl * nc;
          const int j = j0 + sl;
          long nbsite;
          if (piece == 4) nbsite = site0 + sl;
          else if (piece == 0) { int jp = j + s; if (jp == a.hr) jp = 0; nbsite = opp + (long)y * a.hr + jp; }
          else if (piece == 1) nbsite = opp + (long)yp * a.hr + j;
          else if (piece == 2) { int jm = j + s - 1; if (jm < 0) jm = a.hr - 1; nbsite = opp + (long)y * a.hr + jm; }
          else nbsite = opp + (long)ym * a.hr + j;
          // a slab's rows -1 / Ly: the opposite-parity row of the halo buffer (a row-uniform choice of base, stride and site: ONE load either way)
          const bool halo = (piece == 1 && a.halo_hi && y + 1 == a.Ly) || (piece == 3 && a.halo_lo && y == 0);
          const void* vbase = halo ? (piece == 1 ? a.halo_hi : a.halo_lo) : a.rhs;
          const long vstride = halo ? a.halo_stride : a.vec_stride;
          const long vsite = halo ? (long)(1 - p) * a.hr + j : nbsite;
#pragma unroll
          for (int kk = 0; kk < KR; kk++)
            if (kk < nk) xstage[f][kk] = ldv_raw<V32>(vbase, (long)system_index(a, k0 + kk) * vstride + vsite * nc + cc);
        }
      };
      // one piece: park set f (registers -> LDS), request piece `nextp` into the set just freed, compute
      auto do_piece = [&](int nextp, auto fc) {
        constexpr int f = decltype(fc)::value;
        __syncthreads();   // previous compute finished reading LDS
        // registers -> LDS (padded rows)
#pragma unroll
        for (int q = 0; q < PP; q++) {
          const int el = (M16 ? 4 : 2) * (tid + q * BLOCK);
          if (el < L.mat_elems) {   // (nc even: the pair never straddles a row; rs32 and cc even: 16-B aligned.  M16: nc % 4 == 0, the quad stays in its row)
            const int rowi = el / nc, cc = el - rowi * nc;
            if constexpr (M16) {
              typedef _Float16 h8 __attribute__((ext_vector_type(8)));
              typedef float f4 __attribute__((ext_vector_type(4)));
              const h8 hv = __builtin_bit_cast(h8, stage[f][q]);   // (re, im) x 4
              const f4 w0 = {(float)hv[0], (float)hv[1], (float)hv[2], (float)hv[3]}, w1 = {(float)hv[4], (float)hv[5], (float)hv[6], (float)hv[7]};
              *reinterpret_cast<f4*>(mlds + (size_t)rowi * rs32 + cc) = w0;
              *reinterpret_cast<f4*>(mlds + (size_t)rowi * rs32 + cc + 2) = w1;
            } else
              *reinterpret_cast<double2*>(mlds + (size_t)rowi * rs32 + cc) = stage[f][q];
          }
        }
        if (tid < L.S * nc) {
#pragma unroll
          for (int kk = 0; kk < KR; kk++) xlds[kk * rows + tid] = widen_raw<V32>(xstage[f][kk]);
        }
        // issue the global loads of the piece PF ahead (into the set just parked) before computing on this one
        if (nextp >= 0) prefetch(nextp, f);
        __syncthreads();
        if (worker && s_of < nsite) {
          const float2* mrow = mlds + (size_t)sr * rs32;
          const cplx* xs = xlds + s_of * nc;
          for (int cc = c0; cc < c1; cc++) {
            const float2 mf = mrow[cc];       // one 8-B LDS read serves all KR right-hand sides; widened here
            const cplx m = make_double2((double)mf.x, (double)mf.y);
#pragma unroll
            for (int kk = 0; kk < KR; kk++) cmac(acc[kk], m, xs[kk * rows + cc]);
          }
        }
      };
      if constexpr (PF == 1 && PP > 4) {
        // one piece ahead, large tiles (nc = 24: six staged pairs per thread): a plain loop.  Unrolled over the five pieces -- which is what the
        // smaller tiles get below: nc = 8, complex<float> vectors 185 -> 168 us per level-1 Schur hop of the C5 solve -- the compiler keeps every
        // piece's load addresses live: 89 -> 150 VGPRs, 171 with the epilogue, two wavefronts per SIMD instead of four, and the level-1 applies
        // of the C3 solve went 1.04 -> 1.15 ms.
        unsigned rest = ((piece_mask >> 4) & 1u) | ((piece_mask & 0xFu) << 1);
        auto pop = [&]() -> int { if (!rest) return -1; const int oi = __ffs(rest) - 1; rest &= rest - 1; return (oi == 0) ? 4 : oi - 1; };
        int cur = pop();
        if (cur >= 0) prefetch(cur, 0);
        while (cur >= 0) {
          const int nxt = pop();
          do_piece(nxt, std::integral_constant<int, 0>());
          cur = nxt;
        }
      } else {
#pragma unroll
        for (int i = 0; i < PF; i++)
          if (i < npc) prefetch(lst[i], i);
#pragma unroll
        for (int i = 0; i < 5; i++)
          if (i < npc) {
            const int nextp = (i + PF < npc) ? lst[i + PF] : -1;
            if (i % PF == 0) do_piece(nextp, std::integral_constant<int, 0>());
            else do_piece(nextp, std::integral_constant<int, PF - 1>());
          }
      }

      // shift term needs the own-site vector
      if (do_shift && worker && h == 0 && s_of < nsite) {
        const double sg = p ? -1.0 : 1.0;
        const double dg = (nc % 2 == 0) ? ((r_of < nc / 2) ? 1.0 : -1.0) : 0.0;
        const cplx sh = cmake(a.shift[0] + sg * a.eo_shift[0] + dg * a.dof_shift[0],
                              a.shift[1] + sg * a.eo_shift[1] + dg * a.dof_shift[1]);
#pragma unroll
        for (int kk = 0; kk < KR; kk++)
          if (kk < nk) cmac(acc[kk], sh, ldv<V32>(a.rhs, rhs_offset(a, k0 + kk) + (site0 + s_of) * nc + r_of));
      }
      // sum the H slices, one right-hand side at a time through the same LDS buffer
#pragma unroll
      for (int kk = 0; kk < KR; kk++) {
        if (kk >= nk) break;
        __syncthreads();
        if (worker) red[(size_t)h * rows + sr] = acc[kk];
        __syncthreads();
        if (h == 0 && s_of < nsite) {
          cplx t = red[sr];
          for (int hh = 1; hh < L.H; hh++) t = cadd(t, red[(size_t)hh * rows + sr]);
          const long o = rhs_offset(a, k0 + kk) + (site0 + s_of) * nc + r_of;
          if (!do_zero) t = cadd(ldv<V32>(a.lhs, o), t);
          if (EPI) t = epilogue_value<V32>(a.epi, e_ov, e_dv, t, edots);
          stv<V32>(a.lhs, o, t);
        }
      }
    }
  }
  if (EPI && a.epi.dotv) epilogue_store_partials(a.epi, edots);
}

// kernel B32: fp32 tile end to end (even nc); complex<half> matrices at nc a multiple of 4
int launch_stencil_gen32(StencilArgs& a, int nc, const StencilPlan& pl, hipStream_t st) {
  const GenLayout L = pl.L;
  const int kr = pl.K;
  const size_t smem = (size_t)pl.smem;
  const dim3 grid((unsigned)pl.gx, (unsigned)pl.gy);
  long npart;
  if (const int rc = gen_epilogue_begin(a, pl, npart)) return rc;
  const int rc = with_int<1, 2, 3, 4, 5, 6>(pl.P, [&](auto pp_c) {
    return with_storage(pl, [&](auto m32, auto v32, auto m16) {
      constexpr int PP = decltype(pp_c)::value;
      constexpr bool V32 = decltype(v32)::value, M16 = decltype(m16)::value;
      if constexpr (!decltype(m32)::value || (M16 && PP > 3)) return (int)QMG_ERR_UNSUPPORTED;   // not built: fp64 matrices are kernel B's, quads stop at 3
      else {
        if (kr == 8) return launch_kernel(k_stencil_gen32<PP, 8, V32, false, M16>, grid, smem, st, a, nc, L);
        if (kr == 4) return launch_kernel(k_stencil_gen32<PP, 4, V32, false, M16>, grid, smem, st, a, nc, L);
        if (pl.flags & SPF_EPI) return launch_kernel(k_stencil_gen32<PP, 1, V32, true, M16>, grid, smem, st, a, nc, L);
        return launch_kernel(k_stencil_gen32<PP, 1, V32, false, M16>, grid, smem, st, a, nc, L);
      }
    });
  });
  if (rc) return rc;
  return gen_epilogue_finish(a, npart, st);
}

}  // namespace qmg
