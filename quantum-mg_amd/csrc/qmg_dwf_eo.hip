// qmg_dwf_eo.hip -- the 4D even-odd Schur complement of the Shamir domain-wall operator, STRAIGHT FROM THE GAUGE LINKS.
//
// D = A + H with A = clover + shift site-local and H the hops (diagonal in s).  A does not depend on the links, is the same matrix at every
// site of a parity and is block diagonal in spin: with d_p = 3 w + shift +- eo_shift (+ even, - odd)
//   sigma 0:  d_p - (lower shift along s) + m e_0 e_{Ls-1}^T        sigma 1: the mirror under s -> Ls-1-s
// so A_p^-1 is a geometric scan plus a rank-one wall correction:
//   g_s = sum_{s' <= s} d^-(s-s'+1) h_s',      y_s = g_s - q d^-(s+1) g_{Ls-1},      q = m / (1 + m d^-Ls)
// (sigma 1: g_s = sum_{s' >= s} d^-(s'-s+1) h_s', y_s = g_s - q d^-(Ls-s) g_0).  The powers d^-k and q are formed on the host in fp64
// (qmg_dwf_eo_plan.h: dwf_eo_coef), rounded once to the kernel's scalar and come in by value.  M_p = A_p - H_{p,1-p} A_{1-p}^-1 H_{1-p,p} is two launches:
//   kernel K   lhs_p = (ZERO_p ? 0 : lhs_p) + alpha A_p^-1 (H_{p,1-p} rhs_{1-p})     -- every hop in registers (kernel D, shape 2), then the scan
//   kernel I   lhs_p = alpha A_p^-1 rhs_p                                            -- kernel K with the hop replaced by the own chunk
//   stage 2    lhs_p = A_p x_p + H_{p,1-p} t_{1-p}                                   -- kernel D's shape 1 with x and t behind separate pointers
// Gamma5 (psi(s, sigma) -> (-1)^sigma psi(Ls-1-s, sigma)) is a slice index and a sign: kernel K and stage 2 take it on the load of their
// source, stage 2 on its store, so Gamma5 M Gamma5 = M^dagger (real m and shifts) costs the launches and bytes of M.
//
// Lane mapping: kernel D's -- one lane per (site, s) with the two spin components as one chunk, rows (parity, y) over grid.y, block-uniform
// bases, links loaded once per row and kept across the systems of a batch.  The exchange along s: every lane puts its chunk h into LDS, one
// barrier, then walks the distance k = 0 .. Ls-1 with the UNIFORM coefficient d^-(k+1): h(s-k, 0), h(s+k, 1) for its own g and chunk k of its
// site for the two wall sums g_{Ls-1}(sigma 0), g_0(sigma 1), which every lane of the site forms itself (the reads are a broadcast).  Nothing
// depends on how Ls divides the wavefront; the block is Ls floor(256 / Ls) lanes, so a site never straddles a block, and lanes past the end of
// a half row stay for the barrier and skip their loads' result and the store.  Two LDS buffers alternate, so one barrier per (row, system)
// suffices: 2 x 256 chunks = 16 KiB per block in fp64, 8 KiB in fp32.
#include "qmg_dwf_eo_plan.h"
#include "qmg_lane.h"   // uni, gld, fmac2, dwf::hop_acc

namespace qmg {

// T: the kernel's scalar.  Every coefficient arrives in it, rounded once on the host from the fp64 values of dwf_eo_coef.
template <typename T>
struct DwfEoArgs {
  const void* gauge;       // [mu][site] complex<T>
  void* lhs;
  const void* rhs;         // kernel K / I: the source; stage 2: x
  const void* aux;         // stage 2: t
  int hr, Ly, Ls;
  long half_vol;
  unsigned pieces;
  int nrhs;                // active systems
  long vec_stride;
  int par_first, par_count, nrows;
  int g5_in, g5_out;
  T hw, mr, mi, ar, ai;            // -w/2, the wall mass, alpha
  T d[2][2];                       // d_p
  T q[2][2];                       // m / (1 + m d_p^-Ls)
  T pw[2][DWF_LS_MAX + 1][2];      // d_p^-k, k = 0 .. Ls
  int ridx[16];
};

// ---- kernels K (HOP) and I (!HOP): lhs_p (+)= alpha A_p^-1 h, h = H_{p,1-p} [Gamma5] rhs_{1-p} or rhs_p ----
template <typename T, bool HOP, bool ZERO, bool BATCH>
__global__ __launch_bounds__(DWF_BLOCK_MAX) void k_dwf_eo_inv5(const DwfEoArgs<T> a) {
  using namespace dwf;
  typedef T R;
  typedef T v4 __attribute__((ext_vector_type(4)));   // a lane's chunk: (sigma 0 re, im, sigma 1 re, im)
  constexpr unsigned CH = 4u * sizeof(T);
  __shared__ v4 xch[2][DWF_BLOCK_MAX];
  const int tid = threadIdx.x;
  // dwf::lane_of<true>, written out: through it the eight hop instantiations come out with the operands of one v_add_lshl_u32 exchanged,
  // and the kernels are held to the parent's device code text (profiles/dwf_lane_refactor.txt).
  const int t = blockIdx.x * blockDim.x + tid;
  const bool live = t < a.hr * a.Ls;      // a site is live or not as a whole: the block and the half row are multiples of Ls lanes
  const int jt = t / a.Ls, s = t - jt * a.Ls;
  const int j = live ? jt : 0;            // a lane past the end loads what lane (0, s) loads and stores nothing
  const int base = tid - s;               // the site's chunks in LDS: base .. base + Ls - 1, all in this block
  const int sr = a.g5_in ? a.Ls - 1 - s : s;           // Gamma5 on the load: the slice the source chunks come from ...
  const R g5 = a.g5_in ? (R)-1 : (R)1;                 // ... and the sign of their sigma 1
  const unsigned off_own = (unsigned)(j * a.Ls + s) * CH;
  const unsigned off_src = (unsigned)(j * a.Ls + sr) * CH;
  const long sys_bytes = a.vec_stride * (long)(2 * sizeof(T));
  const long row_bytes = (long)a.hr * a.Ls * CH;
  const R hw = a.hw, alx = a.ar, aly = a.ai;
  int buf = 0;
  for (int row = blockIdx.y; row < a.nrows; row += gridDim.y) {
    int p, y;
    row_py(a, row, p, y);
    const bool do_zero = ZERO || ((a.pieces >> (12 + p)) & 1u);
    const Row<T> r = row_of<T, HOP>(a, p, y, j, row_bytes);
    const unsigned off_xp = (unsigned)(r.jp * a.Ls + sr) * CH, off_xm = (unsigned)(r.jm * a.Ls + sr) * CH;
    const R qx = a.q[p][0], qy = a.q[p][1];
    const int nsys = BATCH ? a.nrhs : 1;
    for (int k = 0; k < nsys; k++) {
      const long off = (long)a.ridx[k] * sys_bytes;
      const char* x = reinterpret_cast<const char*>(a.rhs) + off;
      char* out = reinterpret_cast<char*>(a.lhs) + off;
      __attribute__((address_space(1))) v4* dst = (__attribute__((address_space(1))) v4*)(uni(out + r.row_own) + off_own);
      v4 h;
      if (HOP) {
        const gchar* bx = uni(x + r.row_x);
        v4 xr[4];
        xr[0] = gld<v4>(bx, off_xp);
        xr[1] = gld<v4>(uni(x + r.row_yp), off_src);
        xr[2] = gld<v4>(bx, off_xm);
        xr[3] = gld<v4>(uni(x + r.row_ym), off_src);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int d = 0; d < 4; d++) { xr[d].z *= g5; xr[d].w *= g5; }
        R a0x = (R)0, a0y = (R)0, a1x = (R)0, a1y = (R)0;
        hop_acc<T>(xr, r.lx, r.ly, hw, a0x, a0y, a1x, a1y);
        h = (v4){a0x, a0y, a1x, a1y};
      } else {
        h = gld<v4>(uni(x + r.row_own), off_own);
      }
      xch[buf][tid] = h;
      __syncthreads();
      // the scan along s: distance k2 with the uniform coefficient d^-(k2+1)
      R g0x = (R)0, g0y = (R)0, g1x = (R)0, g1y = (R)0;   // g_s of sigma 0 (from below) and of sigma 1 (from above)
      R w0x = (R)0, w0y = (R)0, w1x = (R)0, w1y = (R)0;   // the wall sums g_{Ls-1} (sigma 0) and g_0 (sigma 1)
      R c0x = (R)0, c0y = (R)0, c1x = (R)0, c1y = (R)0;   // d^-(s+1) and d^-(Ls-s)
      for (int k2 = 0; k2 < a.Ls; k2++) {
        const R px = a.pw[p][k2 + 1][0], py = a.pw[p][k2 + 1][1];
        const R rx = a.pw[p][a.Ls - k2][0], ry = a.pw[p][a.Ls - k2][1];
        const bool lo_in = k2 <= s, hi_in = s + k2 < a.Ls;
        const v4 vl = xch[buf][base + (lo_in ? s - k2 : s)], vh = xch[buf][base + (hi_in ? s + k2 : s)], vk = xch[buf][base + k2];
        fmac2<R>(g0x, g0y, px, py, lo_in ? vl.x : (R)0, lo_in ? vl.y : (R)0);
        fmac2<R>(g1x, g1y, px, py, hi_in ? vh.z : (R)0, hi_in ? vh.w : (R)0);
        fmac2<R>(w0x, w0y, rx, ry, vk.x, vk.y);          // d^-(Ls-k2) h(k2, 0)
        fmac2<R>(w1x, w1y, px, py, vk.z, vk.w);          // d^-(k2+1) h(k2, 1)
        if (k2 == s) { c0x = px; c0y = py; }
        if (k2 == a.Ls - 1 - s) { c1x = px; c1y = py; }
      }
      // y = g - (q c) wall
      const R e0x = -(qx * c0x - qy * c0y), e0y = -(qx * c0y + qy * c0x);
      const R e1x = -(qx * c1x - qy * c1y), e1y = -(qx * c1y + qy * c1x);
      fmac2<R>(g0x, g0y, e0x, e0y, w0x, w0y);
      fmac2<R>(g1x, g1y, e1x, e1y, w1x, w1y);
      v4 prev = {(R)0, (R)0, (R)0, (R)0};
      if (!do_zero && live) prev = *dst;
      R o0x = prev.x, o0y = prev.y, o1x = prev.z, o1y = prev.w;
      fmac2<R>(o0x, o0y, alx, aly, g0x, g0y);
      fmac2<R>(o1x, o1y, alx, aly, g1x, g1y);
      const v4 o = {o0x, o0y, o1x, o1y};
      if (live) __builtin_nontemporal_store(o, dst);
      buf ^= 1;
    }
  }
}

// ---- the second stage of M: lhs_p = [Gamma5] (A_p [Gamma5] x_p + H_{p,1-p} t_{1-p}), overwriting; one parity ----
template <typename T, bool BATCH>
__global__ __launch_bounds__(DWF_BLOCK_MAX) void k_dwf_eo_schur2(const DwfEoArgs<T> a) {
  using namespace dwf;
  typedef T R;
  typedef T v4 __attribute__((ext_vector_type(4)));
  typedef T v2 __attribute__((ext_vector_type(2)));
  constexpr unsigned CH = 4u * sizeof(T);
  const Lane ln = lane_of<false>(a.hr, a.Ls);
  if (!ln.live) return;
  const int t = ln.t, j = ln.j, s = ln.s;
  // fifth dimension: sigma = 0 takes slice s - 1 (times -1; across the wall slice Ls - 1 times m), sigma = 1 slice s + 1 (the wall: slice 0)
  const int s_lo = s > 0 ? s - 1 : a.Ls - 1, s_hi = s + 1 < a.Ls ? s + 1 : 0;
  const R clx = s > 0 ? (R)-1 : a.mr, cly = s > 0 ? (R)0 : a.mi;
  const R chx = s + 1 < a.Ls ? (R)-1 : a.mr, chy = s + 1 < a.Ls ? (R)0 : a.mi;
  const int rev = a.Ls - 1;
  const R g5i = a.g5_in ? (R)-1 : (R)1, g5o = a.g5_out ? (R)-1 : (R)1;
  const unsigned off_t = (unsigned)t * CH;                                                         // the hop sources: t, never reflected
  const unsigned off_own = (unsigned)(j * a.Ls + (a.g5_in ? rev - s : s)) * CH;                    // x, through Gamma5 on the load
  const unsigned off_lo = (unsigned)(j * a.Ls + (a.g5_in ? rev - s_lo : s_lo)) * CH;
  const unsigned off_hi = (unsigned)(j * a.Ls + (a.g5_in ? rev - s_hi : s_hi)) * CH + CH / 2;
  const unsigned off_dst = (unsigned)(j * a.Ls + (a.g5_out ? rev - s : s)) * CH;                   // Gamma5 on the store
  const long sys_bytes = a.vec_stride * (long)(2 * sizeof(T));
  const long row_bytes = (long)a.hr * a.Ls * CH;
  const R hw = a.hw;
  const int p = a.par_first;
  const R dx = a.d[p][0], dy = a.d[p][1];
  for (int y = blockIdx.y; y < a.Ly; y += gridDim.y) {
    const Row<T> r = row_of<T, true>(a, p, y, j, row_bytes);
    const unsigned off_xp = (unsigned)(r.jp * a.Ls + s) * CH, off_xm = (unsigned)(r.jm * a.Ls + s) * CH;
    const int nsys = BATCH ? a.nrhs : 1;
    for (int k = 0; k < nsys; k++) {
      const long off = (long)a.ridx[k] * sys_bytes;
      const char* x = reinterpret_cast<const char*>(a.rhs) + off;
      const char* tv = reinterpret_cast<const char*>(a.aux) + off;
      char* out = reinterpret_cast<char*>(a.lhs) + off;
      const gchar* bx = uni(tv + r.row_x);
      v4 xr[4];
      xr[0] = gld<v4>(bx, off_xp);
      xr[1] = gld<v4>(uni(tv + r.row_yp), off_t);
      xr[2] = gld<v4>(bx, off_xm);
      xr[3] = gld<v4>(uni(tv + r.row_ym), off_t);
      const gchar* bo = uni(x + r.row_own);
      const v4 own = gld<v4>(bo, off_own);
      const v2 lo = gld<v2>(bo, off_lo), hi = gld<v2>(bo, off_hi);
      __builtin_amdgcn_sched_barrier(0);
      R a0x = (R)0, a0y = (R)0, a1x = (R)0, a1y = (R)0;
      fmac2<R>(a0x, a0y, dx, dy, own.x, own.y);
      fmac2<R>(a1x, a1y, dx, dy, g5i * own.z, g5i * own.w);
      fmac2<R>(a0x, a0y, clx, cly, lo.x, lo.y);
      fmac2<R>(a1x, a1y, chx, chy, g5i * hi.x, g5i * hi.y);
      hop_acc<T>(xr, r.lx, r.ly, hw, a0x, a0y, a1x, a1y);
      const v4 o = {a0x, a0y, g5o * a1x, g5o * a1y};
      __builtin_nontemporal_store(o, (__attribute__((address_space(1))) v4*)(uni(out + r.row_own) + off_dst));
    }
  }
}

template <typename T>
static void launch_dwf_eo(const DwfEoArgs<T>& a, const DwfEoPlan& pl, hipStream_t st) {
  const dim3 grid((unsigned)pl.gx, (unsigned)pl.gy);
  const unsigned bl = (unsigned)pl.block;
  const bool zero = pl.flags & DPF_ZERO, batch = pl.flags & DPF_BATCH;
  if (pl.family == DEF_SCHUR2) {
    if (batch) k_dwf_eo_schur2<T, true><<<grid, bl, 0, st>>>(a); else k_dwf_eo_schur2<T, false><<<grid, bl, 0, st>>>(a);
  } else if (pl.family == DEF_INV5) {
    if (batch) k_dwf_eo_inv5<T, false, true, true><<<grid, bl, 0, st>>>(a); else k_dwf_eo_inv5<T, false, true, false><<<grid, bl, 0, st>>>(a);
  } else if (zero) {
    if (batch) k_dwf_eo_inv5<T, true, true, true><<<grid, bl, 0, st>>>(a); else k_dwf_eo_inv5<T, true, true, false><<<grid, bl, 0, st>>>(a);
  } else {
    if (batch) k_dwf_eo_inv5<T, true, false, true><<<grid, bl, 0, st>>>(a); else k_dwf_eo_inv5<T, true, false, false><<<grid, bl, 0, st>>>(a);
  }
}

// one launch of a planned request
template <typename T>
static void eo_launch(const qmg_stencil_desc* d, const DwfEoPlan& pl, const DwfEoCoef& co, const void* gauge, int Ls, double mr, double mi, double w, void* lhs,
                      const void* rhs, const void* aux, unsigned pieces, double ar, double ai, unsigned flags, const BatchIdx& b, size_t vec_stride, hipStream_t st) {
  DwfEoArgs<T> a;
  dwf_fill_rows(a, gauge, lhs, rhs, d->Lx, d->Ly, Ls, pieces, b, vec_stride, pl.par_first, pl.par_count);
  a.aux = aux;
  a.g5_in = (flags & QMG_DWF_G5_IN) ? 1 : 0; a.g5_out = (flags & QMG_DWF_G5_OUT) ? 1 : 0;
  a.hw = (T)(-0.5 * w); a.mr = (T)mr; a.mi = (T)mi; a.ar = (T)ar; a.ai = (T)ai;
  for (int p = 0; p < 2; p++)
    for (int c = 0; c < 2; c++) {
      a.d[p][c] = (T)co.d[p][c]; a.q[p][c] = (T)co.q[p][c];
      for (int k = 0; k <= DWF_LS_MAX; k++) a.pw[p][k][c] = (T)co.pw[p][k][c];
    }
  launch_dwf_eo<T>(a, pl, st);
}
static int eo_run(int dtype, const qmg_stencil_desc* d, const DwfEoPlan& pl, const DwfEoCoef& co, const void* gauge, int Ls, double mr, double mi, double w,
                  void* lhs, const void* rhs, const void* aux, unsigned pieces, double ar, double ai, unsigned flags, const BatchIdx& b, size_t vec_stride,
                  hipStream_t st) {
  if (dtype == QMG_C64) eo_launch<double>(d, pl, co, gauge, Ls, mr, mi, w, lhs, rhs, aux, pieces, ar, ai, flags, b, vec_stride, st);
  else eo_launch<float>(d, pl, co, gauge, Ls, mr, mi, w, lhs, rhs, aux, pieces, ar, ai, flags, b, vec_stride, st);
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

}  // namespace qmg

using namespace qmg;

extern "C" {

int qmg_dwf_eo_plan(int dtype, int Lx, int Ly, int Ls, int kernel, unsigned pieces, int n_active, int inplace, int* plan_out, int plan_len) {
  const DwfEoPlan pl = dwf_eo_plan(dtype, Lx, Ly, Ls, kernel, pieces, n_active, inplace);
  return export_dw_plan(pl, pl.lds, plan_out, plan_len);
}

int qmg_dwf_inv5(int dtype, const qmg_stencil_desc* d, int Ls, double mass_re, double mass_im, double wilson_coeff, void* lhs, const void* rhs, unsigned pieces,
                 double alpha_re, double alpha_im, int nrhs, size_t vec_stride, unsigned mask, void* stream) {
  if (!lhs || !rhs || !aligned16(lhs) || !aligned16(rhs) || !std::isfinite(alpha_re) || !std::isfinite(alpha_im)) return QMG_ERR_INVALID;
  if (int rc = dw_eo_valid(dtype, d, Ls, nrhs, vec_stride)) return rc;
  const BatchIdx b = expand_mask(mask, nrhs);
  const DwfEoPlan pl = dwf_eo_plan(dtype, d->Lx, d->Ly, Ls, DEK_INV5, pieces, b.n, lhs == rhs);
  if (dw_eo_refused(pl)) return pl.status;
  DwfEoCoef co;
  if (int rc = dwf_eo_coef(d, Ls, mass_re, mass_im, wilson_coeff, dw_eo_need(pl), &co)) return rc;
  if (pl.family == DEF_NOTHING) return QMG_SUCCESS;
  return eo_run(dtype, d, pl, co, 0, Ls, mass_re, mass_im, wilson_coeff, lhs, rhs, 0, pieces, alpha_re, alpha_im, 0, b, vec_stride, as_stream(stream));
}

int qmg_dwf_hops_inv5(int dtype, const qmg_stencil_desc* d, const void* gauge, int Ls, double mass_re, double mass_im, double wilson_coeff, void* lhs,
                      const void* rhs, unsigned pieces, double alpha_re, double alpha_im, unsigned flags, int nrhs, size_t vec_stride, unsigned mask, void* stream) {
  if (!gauge || !lhs || !rhs || !aligned16(gauge) || !aligned16(lhs) || !aligned16(rhs)) return QMG_ERR_INVALID;
  if (!std::isfinite(alpha_re) || !std::isfinite(alpha_im) || (flags & ~(unsigned)QMG_DWF_G5_IN)) return QMG_ERR_INVALID;
  if (int rc = dw_eo_valid(dtype, d, Ls, nrhs, vec_stride)) return rc;
  const BatchIdx b = expand_mask(mask, nrhs);
  const DwfEoPlan pl = dwf_eo_plan(dtype, d->Lx, d->Ly, Ls, DEK_HOPS_INV5, pieces, b.n, lhs == rhs);
  if (dw_eo_refused(pl)) return pl.status;
  DwfEoCoef co;
  if (int rc = dwf_eo_coef(d, Ls, mass_re, mass_im, wilson_coeff, dw_eo_need(pl), &co)) return rc;
  if (pl.family == DEF_NOTHING) return QMG_SUCCESS;
  return eo_run(dtype, d, pl, co, gauge, Ls, mass_re, mass_im, wilson_coeff, lhs, rhs, 0, pieces, alpha_re, alpha_im, flags, b, vec_stride, as_stream(stream));
}

int qmg_dwf_schur_apply(int dtype, const qmg_stencil_desc* d, const void* gauge, int Ls, double mass_re, double mass_im, double wilson_coeff, void* lhs,
                        const void* rhs, void* tmp, int parity, unsigned flags, int nrhs, size_t vec_stride, unsigned mask, void* stream) {
  if (!gauge || !lhs || !rhs || !tmp || !aligned16(gauge) || !aligned16(lhs) || !aligned16(rhs) || !aligned16(tmp)) return QMG_ERR_INVALID;
  if ((parity != 0 && parity != 1) || (flags & ~(unsigned)(QMG_DWF_G5_IN | QMG_DWF_G5_OUT)) || lhs == rhs || tmp == rhs || tmp == lhs) return QMG_ERR_INVALID;
  if (int rc = dw_eo_valid(dtype, d, Ls, nrhs, vec_stride)) return rc;
  const BatchIdx b = expand_mask(mask, nrhs);
  // stage 1 (kernel K): tmp_o = -A_o^-1 H_{o,p} [Gamma5] rhs_p;  stage 2: lhs_p = [Gamma5] (A_p [Gamma5] rhs_p + H_{p,o} tmp_o)
  const DwEoStages s = dw_eo_stages(parity);
  const DwfEoPlan pl1 = dwf_eo_plan(dtype, d->Lx, d->Ly, Ls, DEK_HOPS_INV5, s.pieces1, b.n, 0);
  const DwfEoPlan pl2 = dwf_eo_plan(dtype, d->Lx, d->Ly, Ls, DEK_SCHUR2, s.pieces2, b.n, 0);
  if (dw_eo_refused(pl1)) return pl1.status;
  if (dw_eo_refused(pl2)) return pl2.status;
  DwfEoCoef co;
  if (int rc = dwf_eo_coef(d, Ls, mass_re, mass_im, wilson_coeff, 3u, &co)) return rc;
  if (pl1.family == DEF_NOTHING || pl2.family == DEF_NOTHING) return QMG_SUCCESS;
  hipStream_t st = as_stream(stream);
  if (int rc = eo_run(dtype, d, pl1, co, gauge, Ls, mass_re, mass_im, wilson_coeff, tmp, rhs, 0, s.pieces1, -1.0, 0.0, flags & QMG_DWF_G5_IN, b, vec_stride, st)) return rc;
  return eo_run(dtype, d, pl2, co, gauge, Ls, mass_re, mass_im, wilson_coeff, lhs, rhs, tmp, s.pieces2, 1.0, 0.0, flags, b, vec_stride, st);
}

}  // extern "C"
