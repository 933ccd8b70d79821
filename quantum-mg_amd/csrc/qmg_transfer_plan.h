// qmg_transfer_plan.h -- which kernel serves a restrict / prolong request: ONE host function (transfer_plan, qmg_transfer.hip) that the
// launch code switches on and that qmg_transfer_plan() exports, so that the tests can ask for the route of a request and a retune of the
// thresholds cannot move a kernel out from under its test (tests/test_gpu_transfer_routes.py holds one row per plan).
// Host code only: nothing here is seen by a kernel except MfmaTile, which k_brestrict_mfma takes by value.
#pragma once
#include <stddef.h>

namespace qmg {

// kernel families (the values are part of qmg_transfer_plan()'s output, include/qmg_hip.h)
enum XferFamily {
  XF_UNSUPPORTED = 0,        // the entry point returns QMG_ERR_UNSUPPORTED
  XF_RESTRICT = 1,           // k_restrict<T, W>: one system, even block width
  XF_RESTRICT_GENERIC = 2,   // k_restrict_generic<T>: one system, odd block width
  XF_PROLONG = 3,            // k_prolong<T, W>: one system
  XF_BRESTRICT_MFMA = 4,     // k_brestrict_mfma<float, MT> (qmg_transfer_mfma.hip)
  XF_BRESTRICT_SMALL = 5,    // k_brestrict_small<T, KB, NVT>
  XF_BRESTRICT_TILE = 6,     // k_brestrict_tile<T, KB>
  XF_BPROLONG_TILE = 7,      // k_bprolong_tile<T, KB, NVB>
  XF_RESTRICT_NV32 = 8,      // k_restrict<double, 2, float>
  XF_PROLONG_NV32 = 9        // k_prolong<double, 2, float>
};
enum { XFER_OP_RESTRICT = 0, XFER_OP_PROLONG = 1, XFER_PLAN_INTS = 8 };

// NVB of the complex<float> prolong of 5-8 systems with at least that many null vectors (k_bprolong_tile<float, 8, NVB>)
constexpr int BPROLONG_NVB_F32 = 12;

struct MfmaTile { int SX, CR, nchunk, Dstride, Fstride, G, R; };

// tile shape of the matrix-core restrict for a block shape, or SX = 0 when that kernel does not serve it
inline MfmaTile make_mfma_tile(int bx, int by, int fnc, int nvec, size_t esz) {
  MfmaTile L;
  L.SX = 0;
  if ((bx & 1) || nvec > 32) return L;
  L.G = (bx / 2) * fnc;
  L.R = 2 * by;
  int best = 0;
  for (int cr = 1; cr <= L.R; cr++) {
    if (L.R % cr || (cr * L.G) % 4) continue;            // elements of a site per chunk: a multiple of the MFMA's K extent
    const size_t bytes = (size_t)(nvec + 8) * ((size_t)cr * 4 * L.G + 1) * esz;
    if (bytes <= 60 * 1024) best = cr;
  }
  if (!best) return L;
  L.SX = 4;
  L.CR = best;
  L.nchunk = L.R / best;
  L.Dstride = L.CR * L.SX * L.G + 1;                     // odd in elements: operand columns spread over the LDS words
  L.Fstride = L.CR * L.SX * L.G + 1;
  return L;
}

// The plan of one pass (up to 8 systems).  The first XFER_PLAN_INTS members, in this order, are what qmg_transfer_plan() writes; a member
// that the family does not use is 0.
struct XferPlan {
  int family;        // XferFamily
  int KB;            // systems per pass the kernel is instantiated for (1: system by system)
  int NV;            // NVT of k_brestrict_small, NVB of k_bprolong_tile
  int MT;            // 16-row tiles of the matrix-core restrict
  int CR, nchunk;    // its fine half-rows per chunk and its chunks
  int small_pairs;   // its staging form: a full workgroup's CR * SX * G positions are fewer than BLOCK
  int W;             // elements per lane of the one-system kernels
  // ---- launch parameters that follow from the above and the geometry
  int SX;            // sites per tile (k_bprolong_tile)
  size_t smem;       // dynamic LDS bytes
  MfmaTile tile;
};

// left: active systems not yet served by an earlier pass (this pass takes min(left, 8)); n_total: active systems of the call
XferPlan transfer_plan(int op, int f32, int null32, int nvec, int fLx, int fLy, int fnc, int cLx, int cLy, int n_total, int left, bool aligned);

}  // namespace qmg
