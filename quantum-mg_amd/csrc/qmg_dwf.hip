// qmg_dwf.hip -- the Shamir domain-wall operator (operators/dwf.h): the stored-stencil fill and the apply STRAIGHT FROM THE GAUGE LINKS.
//
// A site carries 2 Ls complex numbers, component c = 2 s + sigma (s = 0 .. Ls-1 the fifth-dimension slice, sigma the spin).  With w the
// Wilson coefficient, m the wall mass and M5 in the stencil's identity shift, D = clover + hopping + shift:
//   clover   3w on the diagonal;  out(s+1, 0) -= psi(s, 0),  out(s, 1) -= psi(s+1, 1)  (s = 0 .. Ls-2);
//            out(0, 0) += m psi(Ls-1, 0),  out(Ls-1, 1) += m psi(0, 1)
//   hopping  diagonal in s, on every slice the 2 x 2 spin blocks of the Wilson operator (qmg_fill.hip: k_wilson_fill)
// As a stored stencil that is nc = 2 Ls: 5 (2 Ls)^2 complex numbers per site of which all but O(Ls) are zeros (21 KB per site at Ls = 8 in
// fp64).  Kernel D forms the entries in registers from the four links a site touches and streams the vector in, the vector out and the links:
// 64 Ls + 32 B/site in fp64, 32 Ls + 16 in fp32.
//
// Lane mapping: one lane per (site, s) pair; it holds the two spin components of its slice as ONE chunk (32 B in fp64, 16 B in fp32).
// Lanes run along c and then along x, so the own-site, +-y and +-x chunks of a wavefront are each one contiguous run of the even-odd layout.
// The fifth-dimension partners -- sigma = 0 of slice s - 1 (the wall: Ls - 1, times m), sigma = 1 of slice s + 1 (the wall: 0, times m) -- are
// half chunks of the SAME site, inside the cache lines the wavefront loads for its own chunks: they are read again from cache, not
// exchanged across lanes, so nothing depends on how Ls divides the wavefront (Ls = 3, 6, 12: sites straddle wavefronts).  The Ls lanes of
// a site read the same four links (one fetch, broadcast).  Rows (parity, y) go over grid.y, so every base address is uniform in a block.
// Kernel D serves one parity row per block row; kernel D2 serves the full operator with both parities of a column per lane (after kernel W2):
// 8 chunk loads per pair instead of 10, twice the bytes of a wavefront in flight -- 0.56 against 0.62 ms at 2048^2, Ls = 8 in fp64.
// Piece sets served: the ones kernel W serves (qmg_wilson.hip) -- clover + every hop (+ shift) of the processed parities, or every hop
// alone (then lhs == rhs is allowed for one parity); everything else returns QMG_ERR_UNSUPPORTED and the stored stencil serves it.
#include "qmg_lane.h"   // uni, gld, fmac2
#include "qmg_dwf_plan.h"

namespace qmg {

struct DwfArgs {
  const void* gauge;       // [mu][site] complex<T>
  void* lhs;
  const void* rhs;
  int hr, Ly, Ls;
  long half_vol;
  unsigned pieces;
  int nrhs;                // active systems
  long vec_stride;
  int par_first, par_count, nrows;
  double w, mr, mi;
  double shift[2], eo_shift[2], dof_shift[2];
  int ridx[16];
};

// ---- the stored form: the full nc = 2 Ls clover and hopping fields, zeros included (layout of include/qmg_hip.h) ----
// one thread per (site, row, column); the hopping entries are k_wilson_fill's single multiplications
__global__ __launch_bounds__(BLOCK) void k_dwf_fill(cplx* __restrict__ clover, cplx* __restrict__ hop, const cplx* __restrict__ g, int hr, int Ly, int Ls,
                                                    double mr, double mi, double w) {
  const long half_vol = (long)hr * Ly, vol = 2 * half_vol;
  const int nc = 2 * Ls;
  const long nc2 = (long)nc * nc, cm = vol * nc2;
  const double hw = -0.5 * w;
  for (long t = (long)blockIdx.x * BLOCK + threadIdx.x; t < cm; t += (long)gridDim.x * BLOCK) {
    const long i = t / nc2;
    const int e = (int)(t - i * nc2);
    const int r = e / nc, c = e - r * nc;
    const int sr = r >> 1, gr = r & 1, sc = c >> 1, gc = c & 1;
    cplx cl = cmake(0.0, 0.0);
    if (r == c) cl = cmake(3.0 * w, 0.0);
    else if (gr == 0 && gc == 0 && sr == sc + 1) cl = cmake(-1.0, 0.0);       // out(s+1, 0) -= psi(s, 0)
    else if (gr == 1 && gc == 1 && sc == sr + 1) cl = cmake(-1.0, 0.0);       // out(s, 1) -= psi(s+1, 1)
    else if (r == 0 && c == nc - 2) cl = cmake(mr, mi);                       // out(0, 0) += m psi(Ls-1, 0)
    else if (r == nc - 1 && c == 1) cl = cmake(mr, mi);                       // out(Ls-1, 1) += m psi(0, 1)
    clover[t] = cl;
    cplx h0 = cmake(0.0, 0.0), h1 = h0, h2 = h0, h3 = h0;
    if (sr == sc) {
      const int p = (int)(i / half_vol);
      const long wi = i - (long)p * half_vol;
      const int y = (int)(wi / hr), j = (int)(wi - (long)y * hr);
      const int s = (y + p) & 1;
      int jm = j + s - 1; if (jm < 0) jm = hr - 1;
      const int ym = (y == 0) ? Ly - 1 : y - 1;
      const cplx ux = g[i], uy = g[vol + i];
      const cplx uxb = cconj(g[(long)(1 - p) * half_vol + (long)y * hr + jm]);
      const cplx uyb = cconj(g[vol + (long)(1 - p) * half_vol + (long)ym * hr + j]);
      if (gr == gc) {   // -w/2 U
        h0 = cmake(hw * ux.x, hw * ux.y); h1 = cmake(hw * uy.x, hw * uy.y);
        h2 = cmake(hw * uxb.x, hw * uxb.y); h3 = cmake(hw * uyb.x, hw * uyb.y);
      } else if (gr == 0) {   // [0][1]: +x U/2, +y -i U/2, -x -U/2, -y i U/2
        h0 = cmake(0.5 * ux.x, 0.5 * ux.y); h1 = cmake(0.5 * uy.y, -0.5 * uy.x);
        h2 = cmake(-0.5 * uxb.x, -0.5 * uxb.y); h3 = cmake(-0.5 * uyb.y, 0.5 * uyb.x);
      } else {                // [1][0]: +x U/2, +y i U/2, -x -U/2, -y -i U/2
        h0 = cmake(0.5 * ux.x, 0.5 * ux.y); h1 = cmake(-0.5 * uy.y, 0.5 * uy.x);
        h2 = cmake(-0.5 * uxb.x, -0.5 * uxb.y); h3 = cmake(0.5 * uyb.y, -0.5 * uyb.x);
      }
    }
    hop[t] = h0; hop[cm + t] = h1; hop[2 * cm + t] = h2; hop[3 * cm + t] = h3;
  }
}

// what a lane needs of its slice besides the data: the fifth-dimension coefficients and the diagonal shifts of both parities
// (One struct for the partners s_lo / s_hi, their offsets and the four wall coefficients, shared with k_dwf_eo_schur2, moved a scalar load in
// the four fp32 batch instantiations of kernels D / D2 and reordered all four of stage 2: not kept, profiles/dwf_lane_refactor.txt.)
template <typename R>
struct DwfCoef {
  R clx, cly, chx, chy;        // times psi(s_lo, sigma 0) and psi(s_hi, sigma 1): -1 inside, m across the wall
  R hw, cw;                    // -w/2, 3w
  double d0, d1;               // sign of the dof_shift for sigma = 0, 1: + for c = 2 s + sigma < nc / 2 = Ls
};
template <typename R>
__device__ __forceinline__ DwfCoef<R> dwf_coef(const DwfArgs& a, int s) {
  DwfCoef<R> c;
  c.clx = s > 0 ? (R)-1 : (R)a.mr; c.cly = s > 0 ? (R)0 : (R)a.mi;
  c.chx = s + 1 < a.Ls ? (R)-1 : (R)a.mr; c.chy = s + 1 < a.Ls ? (R)0 : (R)a.mi;
  c.hw = (R)(-0.5 * a.w); c.cw = (R)(3.0 * a.w);
  c.d0 = (2 * s < a.Ls) ? 1.0 : -1.0; c.d1 = (2 * s + 1 < a.Ls) ? 1.0 : -1.0;
  return c;
}

// One (site, s) pair's result from its chunks xr = {+x, +y, -x, -y}, own, the two fifth-dimension half chunks and its four links (backward
// ones already conjugated), then the store.  SHAPE 1: clover + hops (+ shift); 2: hops alone (own, lo, hi are not read).
template <typename T, int SHAPE>
__device__ __forceinline__ void dwf_site(const T __attribute__((ext_vector_type(4))) (&xr)[4], const T __attribute__((ext_vector_type(4))) & own,
                                         const T __attribute__((ext_vector_type(2))) & lo, const T __attribute__((ext_vector_type(2))) & hi, const T (&lx)[4],
                                         const T (&ly)[4], const DwfCoef<T>& co, const DwfArgs& a, int p, bool do_shift, bool do_zero, gchar* dst_chunk) {
  typedef T R;
  typedef T v4 __attribute__((ext_vector_type(4)));
  const R h = (R)0.5;
  __attribute__((address_space(1))) v4* dst = (__attribute__((address_space(1))) v4*)dst_chunk;
  // acc0 = row sigma 0, acc1 = row sigma 1
  R a0x = (R)0, a0y = (R)0, a1x = (R)0, a1y = (R)0;
  if (SHAPE == 1) {
    fmac2<R>(a0x, a0y, co.cw, (R)0, own.x, own.y);
    fmac2<R>(a1x, a1y, co.cw, (R)0, own.z, own.w);
    fmac2<R>(a0x, a0y, co.clx, co.cly, lo.x, lo.y);
    fmac2<R>(a1x, a1y, co.chx, co.chy, hi.x, hi.y);
  }
#pragma unroll
  for (int d = 0; d < 4; d++) {
    const R ux = lx[d], uy = ly[d];
    const R dx = co.hw * ux, dy = co.hw * uy;   // diagonal: -w/2 U
    R m01x, m01y, m10x, m10y;                   // [0][1] and [1][0]
    if (d == 0) { m01x = h * ux; m01y = h * uy; m10x = m01x; m10y = m01y; }                           // +x: U/2 both
    else if (d == 2) { m01x = -h * ux; m01y = -h * uy; m10x = m01x; m10y = m01y; }                    // -x: -U/2 both
    else if (d == 1) { m01x = h * uy; m01y = -h * ux; m10x = -h * uy; m10y = h * ux; }                // +y: -i U/2, i U/2
    else { m01x = -h * uy; m01y = h * ux; m10x = h * uy; m10y = -h * ux; }                            // -y: i U/2, -i U/2
    const v4 v = xr[d];
    fmac2<R>(a0x, a0y, dx, dy, v.x, v.y);
    fmac2<R>(a0x, a0y, m01x, m01y, v.z, v.w);
    fmac2<R>(a1x, a1y, m10x, m10y, v.x, v.y);
    fmac2<R>(a1x, a1y, dx, dy, v.z, v.w);
  }
  if (SHAPE == 1 && do_shift) {   // shift +- eo_shift (+ even, - odd) +- dof_shift on the diagonal
    const double sg = p ? -1.0 : 1.0;
    fmac2<R>(a0x, a0y, (R)(a.shift[0] + sg * a.eo_shift[0] + co.d0 * a.dof_shift[0]), (R)(a.shift[1] + sg * a.eo_shift[1] + co.d0 * a.dof_shift[1]), own.x, own.y);
    fmac2<R>(a1x, a1y, (R)(a.shift[0] + sg * a.eo_shift[0] + co.d1 * a.dof_shift[0]), (R)(a.shift[1] + sg * a.eo_shift[1] + co.d1 * a.dof_shift[1]), own.z, own.w);
  }
  v4 o = {a0x, a0y, a1x, a1y};
  if (!do_zero) { const v4 prev = *dst; o.x += prev.x; o.y += prev.y; o.z += prev.z; o.w += prev.w; }
  __builtin_nontemporal_store(o, dst);
}

// ---- kernel D: lhs (+)= pieces(D) rhs from the links ----
// T: storage and arithmetic scalar.  SHAPE 1: clover + hops (+ shift); 2: hops alone.  ZERO: every processed parity is overwritten.
template <typename T, int SHAPE, bool ZERO, bool BATCH>
__global__ __launch_bounds__(BLOCK) void k_dwf_direct(const DwfArgs a) {
  typedef T R;
  typedef T v4 __attribute__((ext_vector_type(4)));   // a lane's chunk: (sigma 0 re, im, sigma 1 re, im)
  typedef T v2 __attribute__((ext_vector_type(2)));   // half a chunk, a link
  constexpr unsigned CH = 4u * sizeof(T), GB = 2u * sizeof(T);
  const dwf::Lane ln = dwf::lane_of<false>(a.hr, a.Ls);
  if (!ln.live) return;
  const int t = ln.t, j = ln.j, s = ln.s;
  // fifth dimension: sigma = 0 takes slice s - 1 (times -1; across the wall slice Ls - 1 times m), sigma = 1 slice s + 1 (the wall: slice 0)
  const int s_lo = s > 0 ? s - 1 : a.Ls - 1, s_hi = s + 1 < a.Ls ? s + 1 : 0;
  const DwfCoef<R> co = dwf_coef<R>(a, s);
  const unsigned off_own = (unsigned)t * CH;
  const unsigned off_lo = (unsigned)(j * a.Ls + s_lo) * CH, off_hi = (unsigned)(j * a.Ls + s_hi) * CH + CH / 2;
  const unsigned goff_j = (unsigned)j * GB;
  const long sys_bytes = a.vec_stride * (long)(2 * sizeof(T));
  const long row_bytes = (long)a.hr * a.Ls * CH;
  for (int row = blockIdx.y; row < a.nrows; row += gridDim.y) {
    int p, y;
    dwf::row_py(a, row, p, y);
    const bool do_shift = (a.pieces >> (10 + p)) & 1u;
    const bool do_zero = ZERO || ((a.pieces >> (12 + p)) & 1u);
    // dwf::row_of<T, true>, written out: through it all 16 instantiations keep their registers and, to within one, their instruction count
    // but not their order (the helper forms the rows before off_xp / off_xm); held to the parent's text (profiles/dwf_lane_refactor.txt).
    const int sx = (y + p) & 1;
    int jp = j + sx;     if (jp == a.hr) jp = 0;
    int jm = j + sx - 1; if (jm < 0) jm = a.hr - 1;
    const int yp = (y + 1 == a.Ly) ? 0 : y + 1;
    const int ym = (y == 0) ? a.Ly - 1 : y - 1;
    const unsigned off_xp = (unsigned)(jp * a.Ls + s) * CH, off_xm = (unsigned)(jm * a.Ls + s) * CH;
    const long row_own = ((long)p * a.Ly + y) * row_bytes;
    const long row_x = ((long)(1 - p) * a.Ly + y) * row_bytes, row_yp = ((long)(1 - p) * a.Ly + yp) * row_bytes, row_ym = ((long)(1 - p) * a.Ly + ym) * row_bytes;
    // links: own Ux, Uy and the -x / -y neighbours' (opposite parity), conjugated for the backward directions
    const long vol = 2 * a.half_vol;
    const char* gc = reinterpret_cast<const char*>(a.gauge);
    const gchar* g_own_x = uni(gc + ((long)p * a.half_vol + (long)y * a.hr) * GB);
    const gchar* g_own_y = uni(gc + (vol + (long)p * a.half_vol + (long)y * a.hr) * GB);
    const gchar* g_xm = uni(gc + ((long)(1 - p) * a.half_vol + (long)y * a.hr) * GB);
    const gchar* g_ym = uni(gc + (vol + (long)(1 - p) * a.half_vol + (long)ym * a.hr) * GB);
    const v2 u0 = gld<v2>(g_own_x, goff_j), u1 = gld<v2>(g_own_y, goff_j), u2 = gld<v2>(g_xm, (unsigned)jm * GB), u3 = gld<v2>(g_ym, goff_j);
    const R lx[4] = {u0.x, u1.x, u2.x, u3.x}, ly[4] = {u0.y, u1.y, -u2.y, -u3.y};
    const int nsys = BATCH ? a.nrhs : 1;
    for (int k = 0; k < nsys; k++) {
      const long off = (long)a.ridx[k] * sys_bytes;
      const char* x = reinterpret_cast<const char*>(a.rhs) + off;
      char* out = reinterpret_cast<char*>(a.lhs) + off;
      // ---- load phase
      const gchar* bx = uni(x + row_x);
      v4 xr[4];
      xr[0] = gld<v4>(bx, off_xp);
      xr[1] = gld<v4>(uni(x + row_yp), off_own);
      xr[2] = gld<v4>(bx, off_xm);
      xr[3] = gld<v4>(uni(x + row_ym), off_own);
      v4 own = xr[0];
      v2 lo = {xr[0].x, xr[0].y}, hi = lo;   // placeholders where the shape does not read them
      if (SHAPE == 1) {
        const gchar* bo = uni(x + row_own);
        own = gld<v4>(bo, off_own);
        lo = gld<v2>(bo, off_lo);
        hi = gld<v2>(bo, off_hi);
      }
      __builtin_amdgcn_sched_barrier(0);
      dwf_site<T, SHAPE>(xr, own, lo, hi, lx, ly, co, a, p, do_shift, do_zero, uni(out + row_own) + off_own);
    }
  }
}

// Kernel D2: BOTH parities of column j on row y per lane -- the full operator (clover + every hop on both parities), after kernel W2
// (qmg_wilson.hip).  Each site's own chunk is an x-neighbour of the other and one back-x link is the other's own link: 8 chunk loads per
// pair instead of 10, and twice the bytes of a wavefront in flight.  Per-slice arithmetic = dwf_site: kernel D's results bit for bit.
template <typename T, bool ZERO, bool BATCH>
__global__ __launch_bounds__(BLOCK) void k_dwf_pair(const DwfArgs a) {
  typedef T R;
  typedef T v4 __attribute__((ext_vector_type(4)));
  typedef T v2 __attribute__((ext_vector_type(2)));
  constexpr unsigned CH = 4u * sizeof(T), GB = 2u * sizeof(T);
  const dwf::Lane ln = dwf::lane_of<false>(a.hr, a.Ls);
  if (!ln.live) return;
  const int t = ln.t, j = ln.j, s = ln.s;
  const int s_lo = s > 0 ? s - 1 : a.Ls - 1, s_hi = s + 1 < a.Ls ? s + 1 : 0;
  const DwfCoef<R> co = dwf_coef<R>(a, s);
  const int jl = (j == 0) ? a.hr - 1 : j - 1, jr = (j + 1 == a.hr) ? 0 : j + 1;
  const unsigned off_own = (unsigned)t * CH, off_l = (unsigned)(jl * a.Ls + s) * CH, off_r = (unsigned)(jr * a.Ls + s) * CH;
  const unsigned off_lo = (unsigned)(j * a.Ls + s_lo) * CH, off_hi = (unsigned)(j * a.Ls + s_hi) * CH + CH / 2;
  const unsigned goff_j = (unsigned)j * GB, goff_l = (unsigned)jl * GB;
  const long sys_bytes = a.vec_stride * (long)(2 * sizeof(T));
  const long row_bytes = (long)a.hr * a.Ls * CH;
  const bool shE = (a.pieces >> 10) & 1u, shO = (a.pieces >> 11) & 1u;
  const bool zE = ZERO || ((a.pieces >> 12) & 1u), zO = ZERO || ((a.pieces >> 13) & 1u);
  for (int y = blockIdx.y; y < a.Ly; y += gridDim.y) {
    const int sE = y & 1;                          // the even site of column j sits at x = 2j + sE, the odd one at 2j + 1 - sE
    const int yp = (y + 1 == a.Ly) ? 0 : y + 1, ym = (y == 0) ? a.Ly - 1 : y - 1;
    const long rowE = (long)y * row_bytes, rowO = ((long)a.Ly + y) * row_bytes;
    const long rowE_up = (long)yp * row_bytes, rowE_dn = (long)ym * row_bytes;
    const long rowO_up = ((long)a.Ly + yp) * row_bytes, rowO_dn = ((long)a.Ly + ym) * row_bytes;
    // the x-neighbour each site does not get from its partner: sE = 0: E's -x (odd row, j-1) and O's +x (even row, j+1); sE = 1: mirrored
    const unsigned off_oth_O = sE ? off_r : off_l;      // in the ODD row, for the even site
    const unsigned off_oth_E = sE ? off_l : off_r;      // in the EVEN row, for the odd site
    // links: own of both sites, the one back-x link that is not the partner's own, two back-y links
    const long vol = 2 * a.half_vol;
    const char* gc = reinterpret_cast<const char*>(a.gauge);
    const gchar* gxE = uni(gc + ((long)y * a.hr) * GB);
    const gchar* gxO = uni(gc + (a.half_vol + (long)y * a.hr) * GB);
    const gchar* gyE = uni(gc + (vol + (long)y * a.hr) * GB);
    const gchar* gyO = uni(gc + (vol + a.half_vol + (long)y * a.hr) * GB);
    const gchar* gyE_dn = uni(gc + (vol + (long)ym * a.hr) * GB);                 // Uy of the EVEN sites of row y-1: the odd site's back-y link
    const gchar* gyO_dn = uni(gc + (vol + a.half_vol + (long)ym * a.hr) * GB);    // ... of the ODD sites: the even site's
    const v2 uxE = gld<v2>(gxE, goff_j), uxO = gld<v2>(gxO, goff_j), uyE = gld<v2>(gyE, goff_j), uyO = gld<v2>(gyO, goff_j);
    const v2 ubx = gld<v2>(sE ? gxE : gxO, goff_l);     // sE = 0: Ux of the odd site at j-1 (the even site's back-x); sE = 1: Ux of the even site at j-1
    const v2 ubyE = gld<v2>(gyO_dn, goff_j), ubyO = gld<v2>(gyE_dn, goff_j);
    const int nsys = BATCH ? a.nrhs : 1;
    for (int k = 0; k < nsys; k++) {
      const long off = (long)a.ridx[k] * sys_bytes;
      const char* x = reinterpret_cast<const char*>(a.rhs) + off;
      char* out = reinterpret_cast<char*>(a.lhs) + off;
      const gchar* bE = uni(x + rowE);
      const gchar* bO = uni(x + rowO);
      const v4 ownE = gld<v4>(bE, off_own), ownO = gld<v4>(bO, off_own);
      const v4 othO = gld<v4>(bO, off_oth_O), othE = gld<v4>(bE, off_oth_E);
      const v4 upE = gld<v4>(uni(x + rowO_up), off_own), dnE = gld<v4>(uni(x + rowO_dn), off_own);   // the even site's +-y neighbours: odd rows
      const v4 upO = gld<v4>(uni(x + rowE_up), off_own), dnO = gld<v4>(uni(x + rowE_dn), off_own);
      const v2 loE = gld<v2>(bE, off_lo), hiE = gld<v2>(bE, off_hi), loO = gld<v2>(bO, off_lo), hiO = gld<v2>(bO, off_hi);
      __builtin_amdgcn_sched_barrier(0);
      {   // even site: +x = odd row at j + sE, -x = odd row at j + sE - 1
        const v2 bx = sE ? uxO : ubx;                    // Ux at the even site's -x neighbour
        const R lx[4] = {uxE.x, uyE.x, bx.x, ubyE.x}, ly[4] = {uxE.y, uyE.y, -bx.y, -ubyE.y};
        const v4 xr[4] = {sE ? othO : ownO, upE, sE ? ownO : othO, dnE};
        dwf_site<T, 1>(xr, ownE, loE, hiE, lx, ly, co, a, 0, shE, zE, uni(out + rowE) + off_own);
      }
      {   // odd site: +x = even row at j + 1 - sE, -x = even row at j - sE
        const v2 bx = sE ? ubx : uxE;                    // Ux at the odd site's -x neighbour
        const R lx[4] = {uxO.x, uyO.x, bx.x, ubyO.x}, ly[4] = {uxO.y, uyO.y, -bx.y, -ubyO.y};
        const v4 xr[4] = {sE ? ownE : othE, upO, sE ? othE : ownE, dnO};
        dwf_site<T, 1>(xr, ownO, loO, hiO, lx, ly, co, a, 1, shO, zO, uni(out + rowO) + off_own);
      }
    }
  }
}

template <typename T, int SHAPE>
static void launch_dwf_s(const DwfArgs& a, bool zero, bool batch, dim3 grid, hipStream_t st) {
  if (zero) { if (batch) k_dwf_direct<T, SHAPE, true, true><<<grid, BLOCK, 0, st>>>(a); else k_dwf_direct<T, SHAPE, true, false><<<grid, BLOCK, 0, st>>>(a); }
  else { if (batch) k_dwf_direct<T, SHAPE, false, true><<<grid, BLOCK, 0, st>>>(a); else k_dwf_direct<T, SHAPE, false, false><<<grid, BLOCK, 0, st>>>(a); }
}
template <typename T>
static void launch_dwf(const DwfArgs& a, const DwfPlan& pl, hipStream_t st) {
  const dim3 grid((unsigned)pl.gx, (unsigned)pl.gy);
  if (pl.family == DF_PAIR) {
    const bool zero = pl.flags & DPF_ZERO, batch = pl.flags & DPF_BATCH;
    if (zero) { if (batch) k_dwf_pair<T, true, true><<<grid, BLOCK, 0, st>>>(a); else k_dwf_pair<T, true, false><<<grid, BLOCK, 0, st>>>(a); }
    else { if (batch) k_dwf_pair<T, false, true><<<grid, BLOCK, 0, st>>>(a); else k_dwf_pair<T, false, false><<<grid, BLOCK, 0, st>>>(a); }
    return;
  }
  if (pl.shape == 1) launch_dwf_s<T, 1>(a, pl.flags & DPF_ZERO, pl.flags & DPF_BATCH, grid, st);
  else launch_dwf_s<T, 2>(a, pl.flags & DPF_ZERO, pl.flags & DPF_BATCH, grid, st);
}

}  // namespace qmg

using namespace qmg;

extern "C" {

int qmg_dwf_fill(void* clover, void* hopping, const void* gauge, int Lx, int Ly, int Ls, double mass_re, double mass_im, double wilson_coeff, void* stream) {
  if (!clover || !hopping || !gauge || !valid_lattice(Lx, Ly) || Ls < DWF_LS_MIN || Ls > DWF_LS_MAX) return QMG_ERR_INVALID;
  k_dwf_fill<<<grid_1d((size_t)Lx * Ly * 4 * Ls * Ls), BLOCK, 0, as_stream(stream)>>>((cplx*)clover, (cplx*)hopping, (const cplx*)gauge, Lx / 2, Ly, Ls, mass_re,
                                                                                    mass_im, wilson_coeff);
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

int qmg_dwf_plan(int dtype, int Lx, int Ly, int Ls, unsigned pieces, int n_active, int inplace, int* plan_out, int plan_len) {
  const DwfPlan pl = dwf_plan(dtype, Lx, Ly, Ls, pieces, n_active, inplace);
  return export_dw_plan(pl, pl.shape, plan_out, plan_len);
}

int qmg_dwf_apply_direct(int dtype, const qmg_stencil_desc* d, const void* gauge, int Ls, double mass_re, double mass_im, double wilson_coeff, void* lhs,
                         const void* rhs, unsigned pieces, int nrhs, size_t vec_stride, unsigned mask, void* stream) {
  if (!d || !gauge || !lhs || !rhs || d->nc != 2 * Ls || !aligned16(gauge) || !aligned16(lhs) || !aligned16(rhs)) return QMG_ERR_INVALID;
  if (int rc = dwf_entry_check(dtype, d->Lx, d->Ly, Ls, nrhs, vec_stride)) return rc;
  const BatchIdx b = expand_mask(mask, nrhs);
  const DwfPlan pl = dwf_plan(dtype, d->Lx, d->Ly, Ls, pieces, b.n, lhs == rhs);
  if (pl.family == DF_NOTHING) return QMG_SUCCESS;
  if (pl.family != DF_DIRECT && pl.family != DF_PAIR) return pl.status;
  DwfArgs a;
  dwf_fill_rows(a, gauge, lhs, rhs, d->Lx, d->Ly, Ls, pieces, b, vec_stride, pl.par_first, pl.par_count);
  a.w = wilson_coeff; a.mr = mass_re; a.mi = mass_im;
  for (int i = 0; i < 2; i++) { a.shift[i] = d->shift[i]; a.eo_shift[i] = d->eo_shift[i]; a.dof_shift[i] = d->dof_shift[i]; }
  hipStream_t st = as_stream(stream);
  if (dtype == QMG_C64) launch_dwf<double>(a, pl, st); else launch_dwf<float>(a, pl, st);
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

}  // extern "C"
