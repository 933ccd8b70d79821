// qmg_transfer_mfma.hip -- the complex<float> restrict of a lock-step batch as a CONTRACTION on the matrix cores (transfer/transfer.h:455-511
// for up to 8 systems per pass).  The same form of the fp64 restrict and of both prolongs was no faster than the vector-FMA kernels of
// qmg_transfer.hip (the round-3 transfer profiles) and was removed.
//
// For one coarse site the batched restrict is a small dense product over the block's nel fine elements:
//   restrict   C[d][q]  = sum_e conj(N[d][e]) F[e][q]        (nvec x nel) . (nel x k)
// with N the null vectors (read once, the bulk of the bytes: nvec of the nvec + 2k vector passes), F the fine and C the coarse values of
// the k systems.  Arithmetic intensity k/(1 + 2k/nvec) complex MACs per loaded element: at k = 8 the vector-FMA kernels of
// qmg_transfer.hip need 64 FMA-pairs per 8 (fp32) or 16 (fp64) bytes and were bound by their cross-lane sums (restrict: 0.20-0.26 of the
// HBM rate in fp32, 0.56 in fp64) or their LDS broadcasts (prolong: 0.42-0.48 in fp32) -- a real contraction, so it goes to MFMA
// (v_mfma_f64_16x16x4_f64 for BOTH storage precisions: complex<float> operands are widened when they are pulled from LDS, so the sums are
// formed in fp64 and rounded once, as in every other fp32-storage kernel of the library -- at 8 systems the f64 matrix pipe needs ~60 % of
// the time the null-vector stream takes), which leaves the kernels with that stream as their only cost.
//
// Real form with the k <= 8 systems' real and imaginary parts as the 16 MFMA columns:
//   restrict   columns [Fr_0..7 | Fi_0..7];  P = Nr . [Fr|Fi],  Q = Ni . [Fr|Fi];   Cr = P[:, q] + Q[:, q+8],  Ci = P[:, q+8] - Q[:, q]
// so a complex product costs TWO real MFMAs per tile.  One wavefront owns one coarse site; a workgroup owns SX = 4 consecutive coarse sites
// of a coarse row, whose fine elements on one fine half-row are CONTIGUOUS (SX G elements, G = (bx/2) nc_f): the workgroup stages a chunk
// of the null vectors [nvec][rows of the chunk][SX G] and of the fine vectors in LDS with whole-line coalesced loads and the wavefronts
// pull their MFMA operands from there (row strides odd in 8-byte words: the 16 lanes of an operand column hit 16 different LDS words).
// Operand maps (as kernel C of qmg_stencil_mfma.hip): lane = 16 lq + lr; A (16 x 4): row lr, k lq; B (4 x 16): k lq, column lr;
// C (16 x 16): column lr, row 4 i + lq in accumulator register i.
#include "qmg_common.h"
#include "qmg_transfer_plan.h"

namespace qmg {

struct XferGeomM {      // (the geometry of qmg_transfer.hip, restated: the two files share no header beyond qmg_common.h)
  int fhr, fLy, fnc, chr, cLy, cnc, bx, by;
  long fhalf_vol, fsize;
};
struct PassIdsM { int n; int id[8]; };

__device__ __forceinline__ long m_coarse_site_index(const XferGeomM& g, int cx, int cy) {
  const int p = (cx + cy) & 1;
  return (long)(cy + p * g.cLy) * g.chr + (cx >> 1);
}
__device__ __forceinline__ int m_pick_id(const PassIdsM& p, int q) {   // run-time slot -> system id without indexing the by-value struct
  const int a = (q & 1) ? p.id[1] : p.id[0], b = (q & 1) ? p.id[3] : p.id[2], c = (q & 1) ? p.id[5] : p.id[4], d = (q & 1) ? p.id[7] : p.id[6];
  const int ab = (q & 2) ? b : a, cd = (q & 2) ? d : c;
  return (q & 4) ? cd : ab;
}

typedef double v4d __attribute__((ext_vector_type(4)));
__device__ __forceinline__ v4d mfma64(double a, double b, v4d c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// first fine element of half-row `rr` (0 .. 2 by - 1: parity-major) of the block row cy, at the column where coarse site cx0 starts
__device__ __forceinline__ long m_run_base(const XferGeomM& g, int cy, int rr, int cx0) {
  const int p = rr / g.by, y = cy * g.by + (rr - p * g.by);
  return ((long)p * g.fhalf_vol + (long)y * g.fhr + (long)cx0 * (g.bx / 2)) * g.fnc;
}

// ---------------------------------------------------------------------------------------------------------------------
// restrict: coarse[q][ci][d] += sum_e conj(null[d][e]) fine[q][e]
// ---------------------------------------------------------------------------------------------------------------------
template <typename T, int MT>
__global__ __launch_bounds__(BLOCK) void k_brestrict_mfma(const void* __restrict__ nullv, int nvec, const void* __restrict__ fine, void* __restrict__ coarse,
                                                          const XferGeomM g, const PassIdsM ids, long cstride, long fstride, const MfmaTile L) {
  typedef typename CStore<T>::type ct;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  ct* nt = reinterpret_cast<ct*>(smem_raw);                  // [nvec][Dstride]
  ct* ft = nt + (size_t)nvec * L.Dstride;                    // [8][Fstride]
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
  const int lr = lane & 15, lq = lane >> 4;
  const int ns = ids.n;
  const int cLx = 2 * g.chr;
  const int cx0 = blockIdx.x * L.SX;
  const int nsx = (cLx - cx0 < L.SX) ? cLx - cx0 : L.SX;
  const int G = L.G, rowlen = nsx * G;                       // elements of the workgroup's sites on one fine half-row
  const ct* nul = reinterpret_cast<const ct*>(nullv);
  const ct* fin = reinterpret_cast<const ct*>(fine);
  ct zero; zero.x = 0; zero.y = 0;
  for (int cy = blockIdx.y; cy < g.cLy; cy += gridDim.y) {
    v4d P[MT], Q[MT];
#pragma unroll
    for (int t = 0; t < MT; t++) { P[t] = (v4d)(0); Q[t] = (v4d)(0); }
    for (int c = 0; c < L.nchunk; c++) {
      const int rr0 = c * L.CR;
      __syncthreads();   // the previous chunk's operand reads are done
      // ---- stage the chunk: null vectors [d][rl][u], fine vectors [q][rl][u]; u runs over the contiguous rowlen elements of a half-row.
      // A thread owns (rl, u) positions and walks the vectors at them: the index arithmetic (two divisions) is done once per position, the
      // loop over d / q only adds strides (the first version divided per element and was bound by its address arithmetic: 21 us per tile).
      {
        const int pairs = L.CR * rowlen;
        const int dgroups = (pairs < BLOCK) ? BLOCK / pairs : 1;
        const int my_dg = (pairs < BLOCK) ? tid / pairs : 0;
        const int pstep = (pairs < BLOCK) ? pairs : BLOCK;
        if (my_dg < dgroups)
          for (int pr = (pairs < BLOCK) ? tid - my_dg * pairs : tid; pr < pairs; pr += pstep) {
            const int rl = pr / rowlen, u = pr - rl * rowlen;
            const long gbase = m_run_base(g, cy, rr0 + rl, cx0) + u;
            const int lidx = rl * (L.SX * G) + u;
            // batches of 8 loads in flight per thread, then the 8 LDS stores (a load -> store loop is one memory latency per element)
            for (int d0 = my_dg; d0 < nvec; d0 += 8 * dgroups) {
              ct v[8];
#pragma unroll
              for (int k = 0; k < 8; k++) { const int d = d0 + k * dgroups; v[k] = zero; if (d < nvec) v[k] = nul[(long)d * g.fsize + gbase]; }
#pragma unroll
              for (int k = 0; k < 8; k++) { const int d = d0 + k * dgroups; if (d < nvec) nt[(size_t)d * L.Dstride + lidx] = v[k]; }
            }
            {
              ct v[8];
#pragma unroll
              for (int k = 0; k < 8; k++) { const int q = my_dg + k * dgroups; v[k] = zero; if (q < ns) v[k] = fin[(long)m_pick_id(ids, q) * fstride + gbase]; }
#pragma unroll
              for (int k = 0; k < 8; k++) { const int q = my_dg + k * dgroups; if (q < 8) ft[(size_t)q * L.Fstride + lidx] = v[k]; }
            }
          }
      }
      __syncthreads();
      if (wv < nsx) {
        const int ksteps = L.CR * G / 4;
        const int q = lr & 7, comp = lr >> 3;
        for (int ks = 0; ks < ksteps; ks++) {
          const int kk = 4 * ks + lq;
          const int rl = kk / G, el = kk - rl * G;
          const int u = rl * (L.SX * G) + wv * G + el;
          const ct fv = ft[(size_t)q * L.Fstride + u];
          const double b = comp ? (double)fv.y : (double)fv.x;
#pragma unroll
          for (int t = 0; t < MT; t++) {
            const int d = 16 * t + lr;
            ct nv = nt[(size_t)(d < nvec ? d : 0) * L.Dstride + u];   // (a select between a load and a constant struct becomes a select of addresses)
            if (d >= nvec) { nv.x = 0; nv.y = 0; }
            P[t] = mfma64((double)nv.x, b, P[t]);
            Q[t] = mfma64((double)nv.y, b, Q[t]);
          }
        }
      }
    }
    // ---- epilogue: column lr = q (re part of system q) for lr < 8, q + 8 (im part) otherwise; partner column lr ^ 8
    if (wv < nsx) {
      const long ci = m_coarse_site_index(g, cx0 + wv, cy);
      ct* cor = reinterpret_cast<ct*>(coarse);
#pragma unroll
      for (int t = 0; t < MT; t++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const double px = __shfl_xor(P[t][i], 8), qx = __shfl_xor(Q[t][i], 8);
          const int d = 16 * t + 4 * i + lq;
          if (lr < 8 && lr < ns && d < nvec) {
            const double re = P[t][i] + qx, im = px - Q[t][i];     // Cr = P[q] + Q[q+8], Ci = P[q+8] - Q[q]
            // (read here, not before the tile loop: held across it the eight values cost restrict<float, 2> a wavefront of occupancy -- 155 VGPRs --
            // and 2048^2 -> 512^2 x 24 went from 1.10 back to 1.49 ms)
            ct* o = cor + (long)m_pick_id(ids, lr) * cstride + ci * g.cnc + d;
            const ct v = *o;
            ct w;
            w.x = (T)((double)v.x + re); w.y = (T)((double)v.y + im);
            *o = w;
          }
        }
    }
  }
}

// C-linkage-free launcher for qmg_transfer.hip, for a pass whose plan (transfer_plan, qmg_transfer_plan.h) is XF_BRESTRICT_MFMA.  The matrix
// cores serve where they are the faster kernel AFTER the vector-FMA restricts stopped waiting for their loads one by one (qmg_common.h,
// RawC): complex<float>, 5-8 systems, from the nc = 2 fine level to >= 16 null vectors (2048^2 -> 512^2 x 24: 1.09 against 1.33 ms).
// Elsewhere the vector kernels are equal or better (512^2 -> 128^2 x 24, 8 systems: 0.55 against 0.58 ms; 1024^2 -> 256^2 x 8: 0.29 against
// 0.34; every shape at <= 4 systems: 0.17-0.72 against 0.33-1.03 ms; round-3 transfer profiles), and so are the fp64 restrict and both prolongs.
int restrict_batch_mfma(const XferPlan& pl, const void* nullvecs, int nvec, const void* fine, void* coarse, int fhr, int fLy, int fnc, int chr, int cLy, int cnc, int bx, int by,
                        long fhalf_vol, long fsize, const int* ids8, int n, long cstride, long fstride, hipStream_t st) {
  if (pl.family != XF_BRESTRICT_MFMA) return QMG_ERR_INVALID;
  const XferGeomM g = {fhr, fLy, fnc, chr, cLy, cnc, bx, by, fhalf_vol, fsize};
  PassIdsM ids;
  ids.n = n;
  for (int q = 0; q < 8; q++) ids.id[q] = ids8[q];
  const MfmaTile L = pl.tile;
  const size_t smem = pl.smem;
  dim3 grid((unsigned)((2 * g.chr + L.SX - 1) / L.SX), g.cLy > 65535 ? 65535u : (unsigned)g.cLy);
  if (pl.MT == 1) {
    if (smem > 64 * 1024) QMG_HIP_CHECK(hipFuncSetAttribute((const void*)k_brestrict_mfma<float, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    k_brestrict_mfma<float, 1><<<grid, BLOCK, smem, st>>>(nullvecs, nvec, fine, coarse, g, ids, cstride, fstride, L);
  } else if (pl.MT == 2) {
    if (smem > 64 * 1024) QMG_HIP_CHECK(hipFuncSetAttribute((const void*)k_brestrict_mfma<float, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    k_brestrict_mfma<float, 2><<<grid, BLOCK, smem, st>>>(nullvecs, nvec, fine, coarse, g, ids, cstride, fstride, L);
  } else {
    return QMG_ERR_INVALID;
  }
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

}  // namespace qmg
