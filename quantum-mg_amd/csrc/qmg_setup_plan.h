// qmg_setup_plan.h -- which launch serves a multigrid SETUP request: ONE host function (setup_plan) that qmg_block_orthonormalize_n,
// qmg_coarse_build(_slab) (csrc/qmg_setup.hip) and qmg_build_rbjacobi (csrc/qmg_fill.hip) switch on and that qmg_setup_plan() exports, after
// the model of qmg_dwf_plan.h / qmg_transfer_plan.h: the tests ask for the answer to a request, hold one GPU row per reachable answer
// (tests/test_gpu_setup_routes.py) and prove on the CPU that no answer lacks a row (tests/test_host_setup_plan.py), so that a retune of the
// thresholds below cannot move a shape out from under its test.  Host code only, no HIP call.
#ifndef QMG_SETUP_PLAN_H
#define QMG_SETUP_PLAN_H

#include "qmg_common.h"

namespace qmg {

// the `op` argument (the values are part of qmg_setup_plan()'s interface, include/qmg_hip.h)
enum SetupOp {
  SETUP_OP_ORTHO = 0,      // qmg_block_orthonormalize_n
  SETUP_OP_GALERKIN = 1,   // qmg_coarse_build / qmg_coarse_build_slab
  SETUP_OP_CINV = 2        // qmg_build_rbjacobi
};
// families (the values are part of qmg_setup_plan()'s output; 0 and 3 mean what they mean in qmg_dwf_plan.h)
enum SetupFamily {
  SUF_UNSUPPORTED = 0,       // the entry point returns QMG_ERR_UNSUPPORTED
  SUF_ORTHO_LDS = 1,         // k_block_ortho<TPB>: the block's tile in LDS, `passes` passes in one launch
  SUF_ORTHO_PASSES = 2,      // block_orthonormalize_passes (qmg_transfer.hip): the reference's full-lattice restrict / prolong / axpy triples
  SUF_INVALID = 3,           // the entry point returns QMG_ERR_INVALID
  SUF_GALERKIN = 4,          // k_galerkin: one workgroup per coarse site
  SUF_GALERKIN_PROBES = 5,   // coarse_build_probes (qmg_transfer.hip): 9 probes per coarse colour
  SUF_CINV = 6               // k_clover_inverse (+ k_identity_cm, k_rb_hopping): one block per site
};
enum {
  SUP_LDS_OPTIN = 1,    // more dynamic LDS than a kernel gets unasked: hipFuncSetAttribute before the launch
  SUP_IDLE_GROUP = 2,   // block orthonormalisation: the last workgroup has groups that own no block
  SUP_STRIDED = 4       // fewer workgroups than blocks / sites: the grid-stride loop takes a second trip
};
enum { SETUP_PLAN_INTS = 8 };

constexpr size_t SETUP_LDS_CAP_BYTES = 150 * 1024;       // a tile beyond this goes to the full-lattice fallback (gfx950 has 160 KB per workgroup)
constexpr size_t SETUP_LDS_UNASKED_BYTES = 64 * 1024;    // dynamic LDS a kernel may use without the opt-in
constexpr size_t ORTHO_SMALL_TILE_BYTES = 24 * 1024;     // block orthonormalisation packs further blocks into a workgroup up to this much tile LDS
constexpr long SETUP_MAX_WORKGROUPS = 262144;            // grid cap of k_block_ortho and k_galerkin; the rest is walked
constexpr int GAL_MAXOUT = 4;                            // k_galerkin's output entries per thread: nc_c^2 <= 4 * 256, i.e. nc_c <= 32
constexpr long CINV_MAX_BLOCKS = 256 * 16;               // grid cap of k_clover_inverse
constexpr int CINV_MAX_NC = 32;                          // k_clover_inverse holds [C | 1] in LDS: 32 nc^2 bytes

// The first SETUP_PLAN_INTS members, in this order, are what qmg_setup_plan() writes; a member that the family does not use is 0.
struct SetupPlan {
  int family;       // SetupFamily
  int tpb;          // k_block_ortho's TPB: threads per block of the null vectors (32, 64, 128, 256)
  int groups;       // k_block_ortho: blocks per workgroup
  int workgroups;   // the grid
  int lds;          // dynamic LDS bytes
  int flags;        // SUP_*
  int outs;         // k_galerkin: output entries per thread that hold a value, ceil(nc_c^2 / 256)
  int threads;      // threads per workgroup
  // ----
  int status;       // QMG_SUCCESS, or what the entry point returns
};

namespace setup_detail {
inline SetupPlan refused(int status) {
  SetupPlan pl = {};
  pl.family = status == QMG_ERR_INVALID ? SUF_INVALID : SUF_UNSUPPORTED;
  pl.status = status;
  return pl;
}
inline SetupPlan fallback(int family) {
  SetupPlan pl = {};
  pl.family = family;
  pl.status = QMG_SUCCESS;
  return pl;
}
// regular (fLx / cLx) x (fLy / cLy) blocks of build_mapping (transfer.h:410-448, 130-134)
inline bool valid_blocking(int fLx, int fLy, int fnc, int cLx, int cLy, int cnc) {
  if (!valid_lattice(fLx, fLy) || !valid_lattice(cLx, cLy) || fnc < 1 || cnc < 1) return false;
  return !(fLx % cLx || fLy % cLy);
}

// qmg_block_orthonormalize_n
inline SetupPlan ortho_plan(int fLx, int fLy, int fnc, int cLx, int cLy, int nvec, int passes) {
  if (nvec < 1 || passes < 1 || passes > 2 || !valid_blocking(fLx, fLy, fnc, cLx, cLy, nvec)) return refused(QMG_ERR_INVALID);
  const int bx = fLx / cLx, by = fLy / cLy;
  const int nel = bx * by * fnc;
  int TPB = 32;
  while (TPB < nel && TPB < BLOCK) TPB <<= 1;
  int groups = (TPB >= 64) ? 1 : 2;   // a workgroup is at least one wavefront
  const size_t tile_bytes = sizeof(cplx) * (size_t)nvec * nel;
  const size_t red_bytes = sizeof(double) * 2 * (BLOCK / WAVE);
  size_t smem = tile_bytes * groups + red_bytes;
  if (!g_setup_fused || (bx & 1) || smem > SETUP_LDS_CAP_BYTES) return fallback(SUF_ORTHO_PASSES);
  while (groups * 2 * TPB <= BLOCK && tile_bytes * groups * 2 <= ORTHO_SMALL_TILE_BYTES) groups *= 2;   // small tiles: several blocks per workgroup
  smem = tile_bytes * groups + red_bytes;
  const long ncs = (long)cLx * cLy;
  const long need = (ncs + groups - 1) / groups;
  SetupPlan pl = {};
  pl.family = SUF_ORTHO_LDS;
  pl.tpb = TPB;
  pl.groups = groups;
  pl.workgroups = (int)(need > SETUP_MAX_WORKGROUPS ? SETUP_MAX_WORKGROUPS : need);
  pl.lds = (int)smem;
  pl.flags = (smem > SETUP_LDS_UNASKED_BYTES ? SUP_LDS_OPTIN : 0) | (ncs % groups ? SUP_IDLE_GROUP : 0) | (need > SETUP_MAX_WORKGROUPS ? SUP_STRIDED : 0);
  pl.threads = TPB * groups;
  pl.status = QMG_SUCCESS;
  return pl;
}

// qmg_coarse_build (slab = 0) / qmg_coarse_build_slab with halos (slab = 1)
inline SetupPlan galerkin_plan(int fLx, int fLy, int fnc, int cLx, int cLy, int cnc, int slab) {
  if (!valid_blocking(fLx, fLy, fnc, cLx, cLy, cnc)) return refused(QMG_ERR_INVALID);
  const size_t smem = sizeof(cplx) * ((size_t)3 * fnc * cnc + (size_t)fnc * fnc);
  if (!g_setup_fused || cnc * cnc > GAL_MAXOUT * BLOCK || smem > SETUP_LDS_CAP_BYTES) {
    if (slab) return refused(QMG_ERR_UNSUPPORTED);   // the full-lattice probe passes have no halo step
    return fallback(SUF_GALERKIN_PROBES);
  }
  const long ncs = (long)cLx * cLy;
  SetupPlan pl = {};
  pl.family = SUF_GALERKIN;
  pl.workgroups = (int)(ncs > SETUP_MAX_WORKGROUPS ? SETUP_MAX_WORKGROUPS : ncs);
  pl.lds = (int)smem;
  pl.flags = (smem > SETUP_LDS_UNASKED_BYTES ? SUP_LDS_OPTIN : 0) | (ncs > SETUP_MAX_WORKGROUPS ? SUP_STRIDED : 0);
  pl.outs = (cnc * cnc + BLOCK - 1) / BLOCK;
  pl.threads = BLOCK;
  pl.status = QMG_SUCCESS;
  return pl;
}

// qmg_build_rbjacobi: clover = the descriptor has a clover field, any_shift = one of its six shift numbers is not zero
inline SetupPlan cinv_plan(int Lx, int Ly, int nc, int clover, int any_shift) {
  if (!valid_lattice(Lx, Ly) || nc < 1) return refused(QMG_ERR_INVALID);
  if (nc > CINV_MAX_NC) return refused(QMG_ERR_UNSUPPORTED);
  if (!clover && !any_shift) return refused(QMG_ERR_INVALID);   // stencil_2d.h:1471-1475
  const long vol = (long)Lx * Ly;
  SetupPlan pl = {};
  pl.family = SUF_CINV;
  pl.workgroups = (int)(vol > CINV_MAX_BLOCKS ? CINV_MAX_BLOCKS : vol);
  pl.lds = (int)(sizeof(cplx) * 2 * nc * nc);
  pl.flags = vol > CINV_MAX_BLOCKS ? SUP_STRIDED : 0;   // a block serves more than one site
  pl.threads = BLOCK;
  pl.status = QMG_SUCCESS;
  return pl;
}
}  // namespace setup_detail

// op ORTHO:    (fLx, fLy, fnc) -> (cLx, cLy), ncv = nvec, a = passes
// op GALERKIN: (fLx, fLy, fnc) -> (cLx, cLy), ncv = cnc,  a = on a slab with halos
// op CINV:     (fLx, fLy, fnc) = the stencil's (Lx, Ly, nc), a = clover present, b = any shift; cLx, cLy, ncv are not looked at
// Reads the tuning knob "setup_fused".
inline SetupPlan setup_plan(int op, int fLx, int fLy, int fnc, int cLx, int cLy, int ncv, int a, int b) {
  using namespace setup_detail;
  if (op == SETUP_OP_ORTHO) return ortho_plan(fLx, fLy, fnc, cLx, cLy, ncv, a);
  if (op == SETUP_OP_GALERKIN) return galerkin_plan(fLx, fLy, fnc, cLx, cLy, ncv, a != 0);
  if (op == SETUP_OP_CINV) return cinv_plan(fLx, fLy, fnc, a != 0, b != 0);
  return refused(QMG_ERR_INVALID);
}

}  // namespace qmg

#endif
