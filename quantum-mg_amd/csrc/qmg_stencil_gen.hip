// qmg_stencil_gen.hip -- kernel B of the stencil apply: any nc (the Galerkin coarse operators), one LDS tile per block, vector FMAs; and the
// tile layout and epilogue steps it shares with kernel B32 (qmg_stencil_gen32.hip).
// The dispatcher (qmg_stencil_apply.hip) calls launch_stencil_gen with the filled argument block.

#include "qmg_stencil_common.h"

namespace qmg {

// ------------------------------------------------------------------------------------------
// Kernel B: any nc (coarse operators, nc = 8, 24, ...).  One block owns S consecutive sites of
// one row.  Per piece (clover, 4 directions) the block copies the S matrices (S nc^2 x 16 B,
// contiguous in the reference layout) global -> registers -> LDS with fully coalesced 16-byte
// loads, software-pipelined one piece ahead, and the S neighbour vectors likewise.  Thread
// (s, r, h) then accumulates the h-th slice of sum_c M[s][r][c] x[s][c] out of LDS (rows padded
// by one element when nc is even so that 16 lanes of a ds_read_b128 hit 64 distinct banks), the
// H slices are summed through LDS, and one thread per (s, r) writes the result.
// The operation is HBM-bound (AI ~ 0.5 flop/B for one right-hand side): all that
// matters is that the matrix stream is coalesced and deep enough in flight.
// ------------------------------------------------------------------------------------------

// KR = right-hand sides per pass: the matrix tile parked in LDS is used for KR vectors (KR accumulators per thread), so a
// batch reads the matrices once per KR systems for ANY nc -- the vector-FMA counterpart of kernel C, and the better one
// where the 16x16 MFMA tile would be mostly padding (nc = 8: 1024^2, 8 rhs 2.0 ms on the matrix cores).
// EPI (KR = 1 only): the apply epilogue of qmg_common.h, a COMPILE-TIME switch -- as a run-time branch it cost every launch ~9 VGPRs and,
// for several tile shapes, a wavefront of occupancy.
template <int PT, bool M32, int KR, bool V32, bool EPI = false>
__global__ __launch_bounds__(BLOCK) void k_stencil_gen(const StencilArgs a, const int nc, const GenLayout L) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  cplx* mlds = reinterpret_cast<cplx*>(smem_raw);                    // [S*nc rows][rs]
  cplx* xlds = mlds + (size_t)L.S * nc * L.rs;                        // [KR][S][nc]
  cplx* red = xlds + (size_t)KR * L.S * nc;                           // [H][S*nc]

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

      // piece order: clover (4), +x, +y, -x, -y  -- the reference's accumulation order
      const int order[5] = {4, 0, 1, 2, 3};
      // fp32-stored matrices with even nc: a lane loads PAIRS of elements (16 B per load, as in the fp64 stream) -- with 8-B
      // loads the same number of load instructions moved half the bytes and the apply got no faster
      constexpr int PTS = PT + (PT & 1);
      const bool pairs = M32 && !(nc & 1);
      typename MRaw<M32>::type stage[PTS];            // storage form (widened when parked)
      typename XRaw<V32>::type xstage[KR];
#pragma unroll
      for (int kk = 0; kk < KR; kk++) xstage[kk] = zero_raw<V32>();
      int cur = -1;
      // find first active piece and prefetch it
      int oi = 0;
      while (oi < 5 && !((piece_mask >> order[oi]) & 1u)) oi++;
      auto prefetch = [&](int piece) {
        const cplx* mbase = (piece == 4) ? a.clover : a.hopping;                 // (element offsets, so that the same
        long moff = (piece == 4) ? site0 * nc2 : (long)piece * a.size_cm + site0 * nc2;   //  code serves both matrix widths)
        const int lim = nsite * (int)nc2;
        if (pairs) {
#pragma unroll
          for (int q = 0; q < PTS / 2; q++) {
            const int el = 2 * (tid + q * BLOCK);
            stage[2 * q] = zero_mraw<M32>(); stage[2 * q + 1] = zero_mraw<M32>();
            if (el < lim) {
              if constexpr (M32) {   // 16 bytes: two raw elements
                const long long* pp = reinterpret_cast<const long long*>(mbase) + moff + el;
                stage[2 * q] = __builtin_nontemporal_load(pp);
                stage[2 * q + 1] = __builtin_nontemporal_load(pp + 1);
              }
            }
          }
        } else {
#pragma unroll
          for (int q = 0; q < PT; q++) {
            const int el = tid + q * BLOCK;
            stage[q] = zero_mraw<M32>();
            if (el < lim) stage[q] = ldm_raw<M32, true>(mbase, moff + el);
          }
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
          // a slab's rows -1 / Ly: the opposite-parity row of the halo buffer (row-uniform choice)
          const bool hi = piece == 1 && a.halo_hi && y + 1 == a.Ly, lo = piece == 3 && a.halo_lo && y == 0;
          const long hsite = (long)(1 - p) * a.hr + j;
#pragma unroll
          for (int kk = 0; kk < KR; kk++)
            if (kk < nk) {
              const int ks = system_index(a, k0 + kk);
              if (hi) xstage[kk] = ldv_raw<V32>(a.halo_hi, (long)ks * a.halo_stride + hsite * nc + cc);
              else if (lo) xstage[kk] = ldv_raw<V32>(a.halo_lo, (long)ks * a.halo_stride + hsite * nc + cc);
              else xstage[kk] = ldv_raw<V32>(a.rhs, rhs_offset(a, k0 + kk) + nbsite * nc + cc);
            }
        }
      };
      if (oi < 5) { cur = order[oi]; prefetch(cur); }

      while (cur >= 0) {
        __syncthreads();   // previous compute finished reading LDS
        // registers -> LDS (padded rows)
        if (pairs) {
#pragma unroll
          for (int q = 0; q < PTS / 2; q++) {
            const int el = 2 * (tid + q * BLOCK);
            if (el < L.mat_elems) {   // (mat_elems and nc even: the pair never straddles a row)
              const int rowi = el / nc, cc = el - rowi * nc;
              mlds[(size_t)rowi * L.rs + cc] = widen_mraw<M32>(stage[2 * q]);
              mlds[(size_t)rowi * L.rs + cc + 1] = widen_mraw<M32>(stage[2 * q + 1]);
            }
          }
        } else {
#pragma unroll
          for (int q = 0; q < PT; q++) {
            const int el = tid + q * BLOCK;
            if (el < L.mat_elems) {
              const int rowi = el / nc, cc = el - rowi * nc;
              mlds[(size_t)rowi * L.rs + cc] = widen_mraw<M32>(stage[q]);
            }
          }
        }
        if (tid < L.S * nc) {
#pragma unroll
          for (int kk = 0; kk < KR; kk++) xlds[kk * rows + tid] = widen_raw<V32>(xstage[kk]);
        }
        // issue the next piece's global loads before computing on this one
        int nxt = -1;
        oi++;
        while (oi < 5 && !((piece_mask >> order[oi]) & 1u)) oi++;
        if (oi < 5) { nxt = order[oi]; prefetch(nxt); }
        __syncthreads();
        if (worker && s_of < nsite) {
          const cplx* mrow = mlds + (size_t)sr * L.rs;
          const cplx* xs = xlds + s_of * nc;
          for (int cc = c0; cc < c1; cc++) {
            const cplx m = mrow[cc];          // one LDS read of the matrix element serves all KR right-hand sides
#pragma unroll
            for (int kk = 0; kk < KR; kk++) cmac(acc[kk], m, xs[kk * rows + cc]);
          }
        }
        cur = nxt;
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

// the epilogue's dot partials: one slot per wavefront of the launch (system slot 0), summed by mr_epilogue_finish into the thread's MR slot
int gen_epilogue_begin(StencilArgs& a, const StencilPlan& pl, long& npart) {
  npart = 0;
  if (pl.flags & SPF_DOTS) {
    npart = (long)pl.gx * (long)pl.gy * (BLOCK / WAVE);
    a.epi.part = mr_epilogue_begin(1, npart);
    a.epi.npart = npart;
    if (!a.epi.part) return QMG_ERR_HIP;
  }
  return QMG_SUCCESS;
}
int gen_epilogue_finish(const StencilArgs& a, long npart, hipStream_t st) {
  if (!npart) return QMG_SUCCESS;
  const unsigned char id0 = a.ridx[0];
  return mr_epilogue_finish(&id0, 1, npart, st);
}

// kernel B: fp64 tile, matrices stored as complex<double> or complex<float>
int launch_stencil_gen(StencilArgs& a, int nc, const StencilPlan& pl, hipStream_t st) {
  const GenLayout L = pl.L;
  const int kr = pl.K;
  const size_t smem = (size_t)pl.smem;
  const dim3 grid((unsigned)pl.gx, (unsigned)pl.gy);
  long npart;
  if (const int rc = gen_epilogue_begin(a, pl, npart)) return rc;
  const int rc = with_int<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12>(pl.P, [&](auto pt_c) {
    return with_storage(pl, [&](auto m32, auto v32, auto m16) {
      constexpr int PT = decltype(pt_c)::value;
      constexpr bool M32 = decltype(m32)::value, V32 = decltype(v32)::value;
      if constexpr (decltype(m16)::value) return (int)QMG_ERR_UNSUPPORTED;   // not built: complex<half> matrices are kernel B32's and C's
      else {
        if (kr == 8) return launch_kernel(k_stencil_gen<PT, M32, 8, V32>, grid, smem, st, a, nc, L);
        if (kr == 4) return launch_kernel(k_stencil_gen<PT, M32, 4, V32>, grid, smem, st, a, nc, L);
        if (pl.flags & SPF_EPI) return launch_kernel(k_stencil_gen<PT, M32, 1, V32, true>, grid, smem, st, a, nc, L);
        return launch_kernel(k_stencil_gen<PT, M32, 1, V32>, grid, smem, st, a, nc, L);
      }
    });
  });
  if (rc) return rc;
  return gen_epilogue_finish(a, npart, st);
}

}  // namespace qmg
