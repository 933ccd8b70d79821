// qmg_mobius.hip -- the Moebius domain-wall operator: the stored-stencil fill and the apply of D and of D^dagger STRAIGHT FROM THE GAUGE LINKS.
//
// The layout of the Shamir operator (qmg_dwf.hip): a site carries 2 Ls complex numbers, c = 2 s + sigma.  With L the fifth-dimension hop
//   (L psi)(s, 0) = psi(s-1, 0) (s >= 1),  (L psi)(0, 0) = -m psi(Ls-1, 0);   (L psi)(s, 1) = psi(s+1, 1) (s <= Ls-2),  (L psi)(Ls-1, 1) = -m psi(0, 1)
// H the hopping blocks of k_wilson_fill on every slice (diagonal in s) and d_w = 2 w + M5:
//   D = (d_w + H) (b5 + c5 L) + (1 - L) = A + H B,     A = alpha + kappa L,  alpha = b5 d_w + 1,  kappa = c5 d_w - 1,     B = b5 + c5 L
// A and B commute, B and H do not: Gamma5 D Gamma5 is A^+ + H^+ B^+, not D^+ = A^+ + B^+ H^+.  So the two operators are two kernels, both on
// the (site, s) lane geometry of qmg_lane.h (one lane per (site, s) with its two spin components as one chunk, rows (parity, y) over grid.y,
// block-uniform bases, the links loaded once per row and kept across the systems of a batch), both 64 Ls + 32 B/site in fp64:
//   k_mobius_load    D: the hop source chi = b5 psi + c5 L psi is formed ON THE LOAD.  Next to the chunk of each of its four neighbours a
//                    lane reads the sigma 0 half of slice s-1 and the sigma 1 half of slice s+1 of that neighbour (across the wall: times
//                    -m) -- halves of the cache lines the wavefront has just asked for, read again as kernel D reads them for the own site.
//                    No LDS, no barrier, 256 lanes.
//   k_mobius_result  D^+ = Gamma5 (A' + B' H) Gamma5, A', B' with conj(m): the hop sum g of a slice is mixed ON THE RESULT, exchanged along s
//                    through LDS as kernel K does it (qmg_dwf_eo.hip): blocks of Ls floor(256 / Ls) lanes so that a site never straddles a
//                    block, one barrier per (row, system), two alternating buffers; a lane past the end of the half row stays for the barrier as
//                    lane (0, s) and stores nothing.  Gamma5 (psi(s, sigma) -> (-1)^sigma psi(Ls-1-s, sigma)) is a slice index and a sign, on
//                    the load and on the store.
// Served: the full operator on both parities (clover + every hop of both; shift pieces and QMG_P_ZERO_* per parity optional); everything else
// returns QMG_ERR_UNSUPPORTED and the stored stencil serves it.
#include "qmg_lane.h"   // uni, gld, fmac2, dwf::lane_of, row_py, row_of, hop_acc
#include "qmg_mobius_plan.h"

namespace qmg {

struct MobiusArgs {
  const void* gauge;       // [mu][site] complex<T>
  void* lhs;
  const void* rhs;
  int hr, Ly, Ls;
  long half_vol;
  unsigned pieces;
  int nrhs;                // active systems
  long vec_stride;
  int par_first, par_count, nrows;
  double hw, alpha, kappa, b5, c5;   // -w/2; A = alpha + kappa L; B = b5 + c5 L
  double wk[2], wc[2];               // across the wall: -m kappa and -m c5 (conj(m) for D^+)
  double shift[2], eo_shift[2], dof_shift[2];   // as added to the diagonal (conjugated for D^+)
  int ridx[16];
};

// ---- the stored form: clover = A, hopping = H B, the full nc = 2 Ls fields, zeros included (layout of include/qmg_hip.h) ----
// Every entry is its exact value rounded once: a hopping entry is (coefficient of B) x (-w/2 or 1/2) x (a link, its parts swapped or
// negated), up to four doubles and, across the wall, a complex product whose parts can cancel -- formed in double-double.
struct dd { double h, l; };
__device__ __forceinline__ dd dd_prod(double a, double b) {   // a b, exactly
  const double p = a * b;
  return {p, fma(a, b, -p)};
}
__device__ dd dd_mul(dd a, dd b) {
#pragma clang fp contract(off)
  const double p = a.h * b.h;
  double e = fma(a.h, b.h, -p);
  e = fma(a.h, b.l, e);
  e = fma(a.l, b.h, e);
  const double h = p + e;
  return {h, e - (h - p)};
}
__device__ dd dd_add(dd a, dd b) {
#pragma clang fp contract(off)
  const double s = a.h + b.h, v = s - a.h;
  double e = (a.h - (s - v)) + (b.h - v);
  e += a.l + b.l;
  const double h = s + e;
  return {h, e - (h - s)};
}
struct MobiusFill { double hw, alpha, kappa, b5, c5, mr, mi, wk[2]; };

// one thread per (site, row, column)
__global__ __launch_bounds__(BLOCK) void k_mobius_fill(cplx* __restrict__ clover, cplx* __restrict__ hop, const cplx* __restrict__ g, int hr, int Ly, int Ls,
                                                       const MobiusFill f) {
  const long half_vol = (long)hr * Ly, vol = 2 * half_vol;
  const int nc = 2 * Ls;
  const long nc2 = (long)nc * nc, cm = vol * nc2;
  for (long t = (long)blockIdx.x * BLOCK + threadIdx.x; t < cm; t += (long)gridDim.x * BLOCK) {
    const long i = t / nc2;
    const int e = (int)(t - i * nc2);
    const int r = e / nc, c = e - r * nc;
    const int sr = r >> 1, gr = r & 1, sc = c >> 1, gc = c & 1;
    // what column (sc, gc) is to row slice sr under L for spin gc: the slice itself, the partner inside, the partner across the wall, or nothing
    const bool self = sr == sc;
    const bool wall = gc == 0 ? (sr == 0 && sc == Ls - 1) : (sr == Ls - 1 && sc == 0);
    const bool inside = !wall && (gc == 0 ? sr == sc + 1 : sc == sr + 1);
    cplx cl = cmake(0.0, 0.0);
    if (gr == gc) {
      if (self) cl = cmake(f.alpha, 0.0);
      else if (wall) cl = cmake(f.wk[0], f.wk[1]);
      else if (inside) cl = cmake(f.kappa, 0.0);
    }
    clover[t] = cl;
    cplx h[4] = {cmake(0.0, 0.0), cmake(0.0, 0.0), cmake(0.0, 0.0), cmake(0.0, 0.0)};
    const bool through_c5 = (wall || inside) && f.c5 != 0.0;
    if (self || through_c5) {
      dd br = {self ? f.b5 : f.c5, 0.0}, bi = {0.0, 0.0};    // the coefficient of B
      if (!self && wall) { br = dd_prod(-f.mr, f.c5); bi = dd_prod(-f.mi, f.c5); }
      const int p = (int)(i / half_vol);
      const long wi = i - (long)p * half_vol;
      const int y = (int)(wi / hr), j = (int)(wi - (long)y * hr);
      const int s = (y + p) & 1;
      int jm = j + s - 1; if (jm < 0) jm = hr - 1;
      const int ym = (y == 0) ? Ly - 1 : y - 1;
      const cplx u[4] = {g[i], g[vol + i], cconj(g[(long)(1 - p) * half_vol + (long)y * hr + jm]), cconj(g[vol + (long)(1 - p) * half_vol + (long)ym * hr + j])};
#pragma unroll
      for (int mu = 0; mu < 4; mu++) {
        // the spin entry [gr][gc] of direction mu is k (vx + i vy): k = -w/2 on the diagonal, 1/2 off it, v the link, its parts swapped or negated
        double k = f.hw, vx = u[mu].x, vy = u[mu].y;
        if (gr != gc) {
          k = 0.5;
          const bool up = gr == 0;   // [0][1]
          if (mu == 2) { vx = -vx; vy = -vy; }                                                              // -x: -U/2 both
          else if (mu == 1) { const double ax = vx; vx = up ? vy : -vy; vy = up ? -ax : ax; }              // +y: -i U/2, i U/2
          else if (mu == 3) { const double ax = vx; vx = up ? -vy : vy; vy = up ? ax : -ax; }              // -y: i U/2, -i U/2
        }
        const dd tx = dd_prod(k, vx), ty = dd_prod(k, vy);
        const dd nty = {-ty.h, -ty.l};
        const dd re = dd_add(dd_mul(br, tx), dd_mul(bi, nty)), im = dd_add(dd_mul(br, ty), dd_mul(bi, tx));
        h[mu] = cmake(re.h, im.h);
      }
    }
    hop[t] = h[0]; hop[cm + t] = h[1]; hop[2 * cm + t] = h[2]; hop[3 * cm + t] = h[3];
  }
}

// what a lane needs of its slice besides the data: the coefficients of its two fifth-dimension partners in A and in B, and the diagonal shifts
template <typename R>
struct MobiusCoefLane {
  R klx, kly, khx, khy;        // A: times psi(s_lo, sigma 0) and psi(s_hi, sigma 1): kappa inside, -m kappa across the wall
  R clx, cly, chx, chy;        // B: c5 inside, -m c5 across the wall
  R al, b5, hw;
};
// s: the slice whose row of L is taken (its partners are s - 1 for sigma 0 and s + 1 for sigma 1; the wall sits below 0 and above Ls - 1)
template <typename R>
__device__ __forceinline__ MobiusCoefLane<R> mobius_coef_lane(const MobiusArgs& a, int s) {
  MobiusCoefLane<R> c;
  const bool lo_in = s > 0, hi_in = s + 1 < a.Ls;
  c.klx = (R)(lo_in ? a.kappa : a.wk[0]); c.kly = (R)(lo_in ? 0.0 : a.wk[1]);
  c.khx = (R)(hi_in ? a.kappa : a.wk[0]); c.khy = (R)(hi_in ? 0.0 : a.wk[1]);
  c.clx = (R)(lo_in ? a.c5 : a.wc[0]); c.cly = (R)(lo_in ? 0.0 : a.wc[1]);
  c.chx = (R)(hi_in ? a.c5 : a.wc[0]); c.chy = (R)(hi_in ? 0.0 : a.wc[1]);
  c.al = (R)a.alpha; c.b5 = (R)a.b5; c.hw = (R)a.hw;
  return c;
}
// shift +- eo_shift (+ even, - odd) +- dof_shift (+ for c = 2 s + sigma < Ls) times the own chunk, added to the two spin rows of slice s
template <typename R>
__device__ __forceinline__ void mobius_shift(const MobiusArgs& a, int p, int s, const R __attribute__((ext_vector_type(4))) & own, R& a0x, R& a0y, R& a1x, R& a1y) {
  const double sg = p ? -1.0 : 1.0;
  const double d0 = (2 * s < a.Ls) ? 1.0 : -1.0, d1 = (2 * s + 1 < a.Ls) ? 1.0 : -1.0;
  fmac2<R>(a0x, a0y, (R)(a.shift[0] + sg * a.eo_shift[0] + d0 * a.dof_shift[0]), (R)(a.shift[1] + sg * a.eo_shift[1] + d0 * a.dof_shift[1]), own.x, own.y);
  fmac2<R>(a1x, a1y, (R)(a.shift[0] + sg * a.eo_shift[0] + d1 * a.dof_shift[0]), (R)(a.shift[1] + sg * a.eo_shift[1] + d1 * a.dof_shift[1]), own.z, own.w);
}

// ---- op 0: lhs (+)= D rhs, the hop source mixed along s on the load ----
template <typename T, bool ZERO, bool BATCH>
__global__ __launch_bounds__(BLOCK) void k_mobius_load(const MobiusArgs a) {
  using namespace dwf;
  typedef T R;
  typedef T v4 __attribute__((ext_vector_type(4)));   // a lane's chunk: (sigma 0 re, im, sigma 1 re, im)
  typedef T v2 __attribute__((ext_vector_type(2)));   // half a chunk
  constexpr unsigned CH = 4u * sizeof(T);
  const Lane ln = lane_of<false>(a.hr, a.Ls);
  if (!ln.live) return;
  const int j = ln.j, s = ln.s;
  const int s_lo = s > 0 ? s - 1 : a.Ls - 1, s_hi = s + 1 < a.Ls ? s + 1 : 0;
  const MobiusCoefLane<R> co = mobius_coef_lane<R>(a, s);
  const unsigned in_own = (unsigned)s * CH, in_lo = (unsigned)s_lo * CH, in_hi = (unsigned)s_hi * CH + CH / 2;   // inside a site
  const long sys_bytes = a.vec_stride * (long)(2 * sizeof(T));
  const long row_bytes = (long)a.hr * a.Ls * CH;
  for (int row = blockIdx.y; row < a.nrows; row += gridDim.y) {
    int p, y;
    row_py(a, row, p, y);
    const bool do_shift = (a.pieces >> (10 + p)) & 1u;
    const bool do_zero = ZERO || ((a.pieces >> (12 + p)) & 1u);
    const Row<T> r = row_of<T, true>(a, p, y, j, row_bytes);
    const unsigned site = (unsigned)(j * a.Ls) * CH, site_p = (unsigned)(r.jp * a.Ls) * CH, site_m = (unsigned)(r.jm * a.Ls) * CH;
    const int nsys = BATCH ? a.nrhs : 1;
    for (int k = 0; k < nsys; k++) {
      const long off = (long)a.ridx[k] * sys_bytes;
      const char* x = reinterpret_cast<const char*>(a.rhs) + off;
      char* out = reinterpret_cast<char*>(a.lhs) + off;
      // ---- load phase: of the own site and of each neighbour the chunk and the two fifth-dimension halves
      const gchar* bx = uni(x + r.row_x);
      const gchar* byp = uni(x + r.row_yp);
      const gchar* bym = uni(x + r.row_ym);
      const gchar* bo = uni(x + r.row_own);
      v4 xr[4];
      v2 xl[4], xh[4];
      xr[0] = gld<v4>(bx, site_p + in_own); xl[0] = gld<v2>(bx, site_p + in_lo); xh[0] = gld<v2>(bx, site_p + in_hi);
      xr[1] = gld<v4>(byp, site + in_own);  xl[1] = gld<v2>(byp, site + in_lo);  xh[1] = gld<v2>(byp, site + in_hi);
      xr[2] = gld<v4>(bx, site_m + in_own); xl[2] = gld<v2>(bx, site_m + in_lo); xh[2] = gld<v2>(bx, site_m + in_hi);
      xr[3] = gld<v4>(bym, site + in_own);  xl[3] = gld<v2>(bym, site + in_lo);  xh[3] = gld<v2>(bym, site + in_hi);
      const v4 own = gld<v4>(bo, site + in_own);
      const v2 lo = gld<v2>(bo, site + in_lo), hi = gld<v2>(bo, site + in_hi);
      __builtin_amdgcn_sched_barrier(0);
      // chi = b5 psi + c5 L psi of the four neighbours, in registers
#pragma unroll
      for (int d = 0; d < 4; d++) {
        R c0x = co.b5 * xr[d].x, c0y = co.b5 * xr[d].y, c1x = co.b5 * xr[d].z, c1y = co.b5 * xr[d].w;
        fmac2<R>(c0x, c0y, co.clx, co.cly, xl[d].x, xl[d].y);
        fmac2<R>(c1x, c1y, co.chx, co.chy, xh[d].x, xh[d].y);
        xr[d] = (v4){c0x, c0y, c1x, c1y};
      }
      R a0x = (R)0, a0y = (R)0, a1x = (R)0, a1y = (R)0;
      fmac2<R>(a0x, a0y, co.al, (R)0, own.x, own.y);
      fmac2<R>(a1x, a1y, co.al, (R)0, own.z, own.w);
      fmac2<R>(a0x, a0y, co.klx, co.kly, lo.x, lo.y);
      fmac2<R>(a1x, a1y, co.khx, co.khy, hi.x, hi.y);
      hop_acc<T>(xr, r.lx, r.ly, co.hw, a0x, a0y, a1x, a1y);
      if (do_shift) mobius_shift<R>(a, p, s, own, a0x, a0y, a1x, a1y);
      __attribute__((address_space(1))) v4* dst = (__attribute__((address_space(1))) v4*)(uni(out + r.row_own) + site + in_own);
      v4 o = {a0x, a0y, a1x, a1y};
      if (!do_zero) { const v4 prev = *dst; o.x += prev.x; o.y += prev.y; o.z += prev.z; o.w += prev.w; }
      __builtin_nontemporal_store(o, dst);
    }
  }
}

// ---- op 1: lhs (+)= D^+ rhs = Gamma5 (A' + B' H) Gamma5 rhs, the hop sum mixed along s in LDS ----
// The lane of slice s works on phi = Gamma5 psi: it reads slice Ls-1-s of psi (sigma 1 negated) for the hops and for A', puts its hop sum
// g(s) into LDS, takes g(s-1, 0) and g(s+1, 1) of its site from there, and stores (sigma 1 negated) to slice Ls-1-s.
template <typename T, bool ZERO, bool BATCH>
__global__ __launch_bounds__(DWF_BLOCK_MAX) void k_mobius_result(const MobiusArgs a) {
  using namespace dwf;
  typedef T R;
  typedef T v4 __attribute__((ext_vector_type(4)));
  typedef T v2 __attribute__((ext_vector_type(2)));
  constexpr unsigned CH = 4u * sizeof(T);
  __shared__ v4 xch[2][DWF_BLOCK_MAX];
  const int tid = threadIdx.x;
  const Lane ln = lane_of<true>(a.hr, a.Ls);      // a site is live or not as a whole: the block and the half row are multiples of Ls lanes
  const bool live = ln.live;
  const int j = ln.j, s = ln.s;
  const int base = tid - s;                       // the site's chunks in LDS: base .. base + Ls - 1, all in this block
  const int s_lo = s > 0 ? s - 1 : a.Ls - 1, s_hi = s + 1 < a.Ls ? s + 1 : 0;
  const int rev = a.Ls - 1;
  const MobiusCoefLane<R> co = mobius_coef_lane<R>(a, s);
  const unsigned in_own = (unsigned)(rev - s) * CH, in_lo = (unsigned)(rev - s_lo) * CH, in_hi = (unsigned)(rev - s_hi) * CH + CH / 2;   // Gamma5 on the load
  const long sys_bytes = a.vec_stride * (long)(2 * sizeof(T));
  const long row_bytes = (long)a.hr * a.Ls * CH;
  int buf = 0;
  for (int row = blockIdx.y; row < a.nrows; row += gridDim.y) {
    int p, y;
    row_py(a, row, p, y);
    const bool do_shift = (a.pieces >> (10 + p)) & 1u;
    const bool do_zero = ZERO || ((a.pieces >> (12 + p)) & 1u);
    const Row<T> r = row_of<T, true>(a, p, y, j, row_bytes);
    const unsigned site = (unsigned)(j * a.Ls) * CH, site_p = (unsigned)(r.jp * a.Ls) * CH, site_m = (unsigned)(r.jm * a.Ls) * CH;
    const int nsys = BATCH ? a.nrhs : 1;
    for (int k = 0; k < nsys; k++) {
      const long off = (long)a.ridx[k] * sys_bytes;
      const char* x = reinterpret_cast<const char*>(a.rhs) + off;
      char* out = reinterpret_cast<char*>(a.lhs) + off;
      __attribute__((address_space(1))) v4* dst = (__attribute__((address_space(1))) v4*)(uni(out + r.row_own) + site + in_own);   // Gamma5 on the store
      const gchar* bx = uni(x + r.row_x);
      const gchar* bo = uni(x + r.row_own);
      v4 xr[4];
      xr[0] = gld<v4>(bx, site_p + in_own);
      xr[1] = gld<v4>(uni(x + r.row_yp), site + in_own);
      xr[2] = gld<v4>(bx, site_m + in_own);
      xr[3] = gld<v4>(uni(x + r.row_ym), site + in_own);
      const v4 own = gld<v4>(bo, site + in_own);                                     // psi(Ls-1-s): phi(s) up to the sign of sigma 1
      const v2 lo = gld<v2>(bo, site + in_lo), hi = gld<v2>(bo, site + in_hi);       // phi(s_lo, 0) and -phi(s_hi, 1)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int d = 0; d < 4; d++) { xr[d].z = -xr[d].z; xr[d].w = -xr[d].w; }
      R g0x = (R)0, g0y = (R)0, g1x = (R)0, g1y = (R)0;
      hop_acc<T>(xr, r.lx, r.ly, co.hw, g0x, g0y, g1x, g1y);
      xch[buf][tid] = (v4){g0x, g0y, g1x, g1y};
      __syncthreads();
      const v4 gl = xch[buf][base + s_lo], gh = xch[buf][base + s_hi];
      // r = A' phi + B' g on slice s
      R a0x = (R)0, a0y = (R)0, a1x = (R)0, a1y = (R)0;
      fmac2<R>(a0x, a0y, co.al, (R)0, own.x, own.y);
      fmac2<R>(a1x, a1y, co.al, (R)0, -own.z, -own.w);
      fmac2<R>(a0x, a0y, co.klx, co.kly, lo.x, lo.y);
      fmac2<R>(a1x, a1y, co.khx, co.khy, -hi.x, -hi.y);
      fmac2<R>(a0x, a0y, co.b5, (R)0, g0x, g0y);
      fmac2<R>(a1x, a1y, co.b5, (R)0, g1x, g1y);
      fmac2<R>(a0x, a0y, co.clx, co.cly, gl.x, gl.y);
      fmac2<R>(a1x, a1y, co.chx, co.chy, gh.z, gh.w);
      a1x = -a1x; a1y = -a1y;                                                        // Gamma5 on the store
      if (do_shift) mobius_shift<R>(a, p, rev - s, own, a0x, a0y, a1x, a1y);
      v4 o = {a0x, a0y, a1x, a1y};
      if (!do_zero && live) { const v4 prev = *dst; o.x += prev.x; o.y += prev.y; o.z += prev.z; o.w += prev.w; }
      if (live) __builtin_nontemporal_store(o, dst);
      buf ^= 1;
    }
  }
}

template <typename T>
static void launch_mobius(const MobiusArgs& a, const MobiusPlan& pl, hipStream_t st) {
  const dim3 grid((unsigned)pl.gx, (unsigned)pl.gy);
  const unsigned bl = (unsigned)pl.block;
  const bool zero = pl.flags & DPF_ZERO, batch = pl.flags & DPF_BATCH;
  if (pl.family == MF_LOAD) {
    if (zero) { if (batch) k_mobius_load<T, true, true><<<grid, bl, 0, st>>>(a); else k_mobius_load<T, true, false><<<grid, bl, 0, st>>>(a); }
    else { if (batch) k_mobius_load<T, false, true><<<grid, bl, 0, st>>>(a); else k_mobius_load<T, false, false><<<grid, bl, 0, st>>>(a); }
  } else {
    if (zero) { if (batch) k_mobius_result<T, true, true><<<grid, bl, 0, st>>>(a); else k_mobius_result<T, true, false><<<grid, bl, 0, st>>>(a); }
    else { if (batch) k_mobius_result<T, false, true><<<grid, bl, 0, st>>>(a); else k_mobius_result<T, false, false><<<grid, bl, 0, st>>>(a); }
  }
}

}  // namespace qmg

using namespace qmg;

extern "C" {

int qmg_mobius_fill(void* clover, void* hopping, const void* gauge, int Lx, int Ly, int Ls, double mass_re, double mass_im, double wilson_coeff, double M5,
                    double b5, double c5, void* stream) {
  if (!clover || !hopping || !gauge || !valid_lattice(Lx, Ly) || Ls < DWF_LS_MIN || Ls > DWF_LS_MAX) return QMG_ERR_INVALID;
  MobiusCoef co;
  if (int rc = mobius_coef(mass_re, mass_im, wilson_coeff, M5, b5, c5, &co)) return rc;
  const MobiusFill f = {-0.5 * wilson_coeff, co.alpha, co.kappa, b5, c5, mass_re, mass_im, {co.wk[0], co.wk[1]}};
  hipStream_t st = as_stream(stream);
  k_mobius_fill<<<grid_1d((size_t)Lx * Ly * 4 * Ls * Ls), BLOCK, 0, st>>>((cplx*)clover, (cplx*)hopping, (const cplx*)gauge, Lx / 2, Ly, Ls, f);
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

int qmg_mobius_plan(int dtype, int Lx, int Ly, int Ls, int op, unsigned pieces, int n_active, int inplace, int* plan_out, int plan_len) {
  const MobiusPlan pl = mobius_plan(dtype, Lx, Ly, Ls, op, pieces, n_active, inplace);
  return export_dw_plan(pl, pl.lds, plan_out, plan_len);
}

int qmg_mobius_apply_direct(int dtype, const qmg_stencil_desc* d, const void* gauge, int Ls, double mass_re, double mass_im, double wilson_coeff, double M5,
                            double b5, double c5, int op, void* lhs, const void* rhs, unsigned pieces, int nrhs, size_t vec_stride, unsigned mask,
                            void* stream) {
  if (!d || !gauge || !lhs || !rhs || d->nc != 2 * Ls || !aligned16(gauge) || !aligned16(lhs) || !aligned16(rhs)) return QMG_ERR_INVALID;
  if (int rc = dwf_entry_check(dtype, d->Lx, d->Ly, Ls, nrhs, vec_stride)) return rc;
  MobiusCoef co;
  if (int rc = mobius_coef(mass_re, mass_im, wilson_coeff, M5, b5, c5, &co)) return rc;
  const BatchIdx b = expand_mask(mask, nrhs);
  const MobiusPlan pl = mobius_plan(dtype, d->Lx, d->Ly, Ls, op, pieces, b.n, lhs == rhs);
  if (pl.family == MF_NOTHING) return QMG_SUCCESS;
  if (pl.family != MF_LOAD && pl.family != MF_RESULT) return pl.status;
  MobiusArgs a;
  dwf_fill_rows(a, gauge, lhs, rhs, d->Lx, d->Ly, Ls, pieces, b, vec_stride, 0, 2);
  const double cj = op == MOP_DAGGER ? -1.0 : 1.0;   // D^+: conj(m) in A', B', and the conjugated shifts
  a.hw = -0.5 * wilson_coeff; a.alpha = co.alpha; a.kappa = co.kappa; a.b5 = b5; a.c5 = c5;
  a.wk[0] = co.wk[0]; a.wk[1] = cj * co.wk[1];
  a.wc[0] = -mass_re * c5; a.wc[1] = cj * -mass_im * c5;
  a.shift[0] = d->shift[0]; a.shift[1] = cj * d->shift[1];
  a.eo_shift[0] = d->eo_shift[0]; a.eo_shift[1] = cj * d->eo_shift[1];
  a.dof_shift[0] = d->dof_shift[0]; a.dof_shift[1] = cj * d->dof_shift[1];
  hipStream_t st = as_stream(stream);
  if (dtype == QMG_C64) launch_mobius<double>(a, pl, st); else launch_mobius<float>(a, pl, st);
  QMG_LAUNCH_CHECK();
  return QMG_SUCCESS;
}

}  // extern "C"
