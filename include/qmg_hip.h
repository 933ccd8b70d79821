/* qmg_hip.h -- C-ABI of libqmg_hip.so: the MI355X (gfx950) drop-in for quantum-mg's
 * multigrid hot path (stencil apply, cshift, restrict/prolong, global reductions).
 *
 * The reference (weinbe2/quantum-mg) is a header-only C++ library with no FFI of its own;
 * its hot path is entered through the `matrix_op_cplx` callback
 *     void (*)(complex<double>* lhs, complex<double>* rhs, void* extra_data)
 * (stencil/stencil_2d.h:15-19) and through public methods of Stencil2D / TransferMG that
 * operate on the PUBLIC arrays `clover`, `hopping`, `null_vectors` (stencil_2d.h:148-210,
 * transfer/transfer.h:79).  This ABI is therefore STATELESS: every entry point takes the
 * raw arrays + lattice extents exactly as the reference method receives them, except that
 * all array pointers are DEVICE (HBM) addresses.  The reference's pointer-swap trick for
 * operator variants (perform_swap_dagger, stencil_2d.h:1142-1178) maps onto passing a
 * different `clover`/`hopping` pair in the descriptor.  The C++ facade in
 * quantum-mg_amd/include/qmg/ rebuilds the reference class surface on top of this file;
 * INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions
 *  - all complex data: interleaved (re,im) double == std::complex<double>
 *  - layouts (reference README.md:4-11): vector (eo,y,x,c); matrix (eo,y,x,c1,c2) row-major;
 *    hopping (mu,eo,y,x,c1,c2), mu in {+x,+y,-x,-y}; site i = (y + p*Ly)*Lx/2 + x/2
 *  - Lx, Ly even and >= 2 (cshift_2d.h:62,79 step two rows at a time)
 *  - extents are 64-bit internally (the reference's `int` size_hopping overflows at
 *    1024^2 x 24^2 x 4, lattice.h:23,40)
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are
 *    asynchronous on that stream unless stated otherwise
 *  - return value: qmg_status (0 = success).  Nothing here falls back to the CPU: a call
 *    that cannot run on the GPU returns an error.
 */
#ifndef QMG_HIP_H
#define QMG_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  QMG_SUCCESS = 0,
  QMG_ERR_INVALID = 1,      /* bad extents / NULL array / unsupported nc             */
  QMG_ERR_HIP = 2,          /* a HIP runtime call failed (qmg_last_hip_error())      */
  QMG_ERR_UNSUPPORTED = 3,  /* valid in the reference but not built yet              */
  QMG_ERR_NO_DEVICE = 4
} qmg_status;

/* Storage precision of device arrays.  The reference is fp64 only (stencil_2d.h:17-18); QMG_C32 is the fp32 instantiation
 * BASELINE configs[4] asks for: complex<float> storage of vectors, matrices and null vectors, half the bytes of every
 * HBM-bound kernel.  Reductions always accumulate and return fp64. */
typedef enum { QMG_C64 = 0, QMG_C32 = 1 } qmg_dtype;

/* cshift directions / parities: names and values identical to cshift/cshift_2d.h:13-36 */
typedef enum {
  QMG_CSHIFT_FROM_0 = 1, QMG_CSHIFT_FROM_XP1 = 2, QMG_CSHIFT_FROM_YP1 = 3, QMG_CSHIFT_FROM_XM1 = 4, QMG_CSHIFT_FROM_YM1 = 5,
  QMG_CSHIFT_FROM_XP2 = 6, QMG_CSHIFT_FROM_YP2 = 7, QMG_CSHIFT_FROM_XM2 = 8, QMG_CSHIFT_FROM_YM2 = 9,
  QMG_CSHIFT_FROM_XP1YP1 = 10, QMG_CSHIFT_FROM_XM1YP1 = 11, QMG_CSHIFT_FROM_XM1YM1 = 12, QMG_CSHIFT_FROM_XP1YM1 = 13
} qmg_cshift_dir;   /* only the distance-1 shifts (1..5) are implemented, as in the reference (:120-129) */
typedef enum { QMG_EO_FROM_EVEN = 1, QMG_EO_FROM_ODD = 2, QMG_EO_FROM_EVENODD = 3 } qmg_eo;
/* hopping direction index mu = 0..3 is {+x,+y,-x,-y} (stencil/stencil_2d.h:25-40) */

/* Which pieces of  lhs (+)= M rhs  one fused launch applies.  Each reference method is one mask:
 *   apply_M            (stencil_2d.h:912-936)  QMG_P_ALL
 *   apply_M_clover     (:694-703)              QMG_P_CLOVER
 *   apply_M_eo / _oe   (:706-802)              QMG_P_EO / QMG_P_OE      (even / odd OUTPUT sites)
 *   ... one direction  (:736-841)              QMG_P_EO_XP1 << dir, QMG_P_OE_XP1 << dir
 *   apply_M_shift      (:865-909)              QMG_P_SHIFT
 *   apply_M_ee / _oo   (:666-692)              QMG_P_CLOVER_E|QMG_P_SHIFT_E with eo/dof shift zeroed
 * QMG_P_ZERO_E/_O overwrite that half instead of accumulating into it (the C wrappers'
 * zero_vector + apply, :2571-2576, in one pass).  A half with no bit set is not touched. */
enum {
  QMG_P_CLOVER_E = 1u << 0,  QMG_P_CLOVER_O = 1u << 1,
  QMG_P_EO_XP1 = 1u << 2, QMG_P_EO_YP1 = 1u << 3, QMG_P_EO_XM1 = 1u << 4, QMG_P_EO_YM1 = 1u << 5,
  QMG_P_OE_XP1 = 1u << 6, QMG_P_OE_YP1 = 1u << 7, QMG_P_OE_XM1 = 1u << 8, QMG_P_OE_YM1 = 1u << 9,
  QMG_P_SHIFT_E = 1u << 10, QMG_P_SHIFT_O = 1u << 11,
  QMG_P_ZERO_E = 1u << 12,  QMG_P_ZERO_O = 1u << 13,
  QMG_P_CLOVER = 3u, QMG_P_EO = 0xFu << 2, QMG_P_OE = 0xFu << 6, QMG_P_HOPPING = 0xFFu << 2,
  QMG_P_SHIFT = 3u << 10, QMG_P_ZERO = 3u << 12,
  QMG_P_ALL = 0xFFFu
};

/* The public data of a Stencil2D (stencil_2d.h:148-177) as the kernels need it. */
typedef struct {
  int Lx, Ly, nc;
  const void* clover;      /* device, Lx*Ly*nc*nc complex, or NULL (stencil has no clover)   */
  const void* hopping;     /* device, 4*Lx*Ly*nc*nc complex, or NULL                         */
  double shift[2];         /* identity shift (mass)                         (:170)           */
  double eo_shift[2];      /* +even / -odd                                  (:173)           */
  double dof_shift[2];     /* +top half / -bottom half of the dof, nc even  (:177)           */
} qmg_stencil_desc;

/* ---------------- runtime ---------------- */
int qmg_init(int device);                       /* hipSetDevice + sanity; QMG_ERR_NO_DEVICE if none */
int qmg_device_count(int* n);
const char* qmg_status_string(int status);
const char* qmg_last_hip_error(void);
const char* qmg_version(void);
int qmg_malloc(void** dev_ptr, size_t bytes);   /* replaces allocate_vector<T> for device arrays */
int qmg_free(void* dev_ptr);
/* With the tuning key "malloc_poison" on: `bytes` bytes at dev_ptr are set to 0xFF on `stream` (asynchronous).  With the key off: nothing,
 * no launch.  For a facade's pools: a recycled scratch block leaves the pool looking like a fresh qmg_malloc. */
int qmg_poison_scratch(void* dev_ptr, size_t bytes, void* stream);
int qmg_shutdown(void);                         /* ordered teardown for the calling host thread: device sync, then the library's per-thread workspaces are released */
int qmg_mem_info(size_t* free_bytes, size_t* total_bytes);   /* HBM free / total on the current device: batch sizing */
int qmg_memcpy_h2d(void* dst_dev, const void* src_host, size_t bytes, void* stream);  /* synchronous when stream == NULL */
int qmg_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes, void* stream);
int qmg_memcpy_d2d(void* dst_dev, const void* src_dev, size_t bytes, void* stream);
int qmg_memset_zero(void* dev_ptr, size_t bytes, void* stream);
int qmg_stream_create(void** stream);
int qmg_stream_destroy(void* stream);
int qmg_stream_sync(void* stream);
int qmg_event_create(void** ev);
int qmg_event_destroy(void* ev);
int qmg_event_record(void* ev, void* stream);
int qmg_stream_wait_event(void* stream, void* ev);                     /* later work on `stream` waits for ev (no host sync) */
int qmg_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms);   /* synchronises on ev_stop */

/* ---------------- cshift (cshift/cshift_2d.h:45-236) ---------------- */
/* lhs(opposite half) = rhs(neighbour); dof complex numbers per site. */
int qmg_cshift(void* lhs, const void* rhs, int cdir, int eo, int dof, int Lx, int Ly, void* stream);

/* ---------------- stencil apply (stencil/stencil_2d.h:666-936, 2418-2453, 2571-2716) ---------------- */
/* lhs (+)= pieces(M) rhs, fused in one launch.  nrhs >= 1 independent right-hand sides stored
 * `vec_stride` complex elements apart share one read of the stencil matrices (vec_stride is
 * ignored for nrhs == 1).  lhs and rhs must not overlap, except that a call with only
 * QMG_P_EO (or only QMG_P_OE) pieces may pass lhs == rhs: it reads one half and writes the
 * other (the reference's in-place use, stencil_2d.h:1904, staggered.h:236). */
int qmg_stencil_apply(const qmg_stencil_desc* d, void* lhs, const void* rhs, unsigned pieces,
                      int nrhs, size_t vec_stride, void* stream);
/* The apply with the norms of its results from the same pass: lhs_k (+)= pieces(M) rhs_k and norms[k] = |lhs_k|^2 (the
 * apply followed by quantum-linalg's norm2sq -- call sites stateful_multigrid.h:880,884 -- without re-reading the vector: 40 instead of 56 B/site/rhs for
 * the staggered operator).  fp64, nc = 1 or 2, pieces touching BOTH parities, lhs != rhs, nrhs <= 16; anything else, or a
 * call while distributed reductions are on, is QMG_ERR_UNSUPPORTED.  lhs receives the bytes qmg_stencil_apply writes; the
 * norms are summed in a fixed order (run-to-run reproducible), not in qmg_norm2sq's order (they agree to rounding).
 * norms_dev: nrhs doubles in device memory or NULL; norms_host: nrhs doubles or NULL (then the stream is synchronised). */
int qmg_stencil_apply_norm2(const qmg_stencil_desc* d, void* lhs, const void* rhs, unsigned pieces, int nrhs, size_t vec_stride,
                            double* norms_dev, double* norms_host, void* stream);
/* Same, for a lock-step batch of at most 16 systems of which only those with their bit set in `mask` are read or
 * written.  With nc in {8,12,16,24,32} and two or more active systems the apply runs as an (nc x nc).(nc x k)
 * contraction on the f64 matrix cores (v_mfma_f64_16x16x4_f64), the matrices read once for all k.
 * Read set of every apply of this family, the Wilson and domain-wall applies from the links included (tests/test_gpu_isolation.py runs each
 * route with everything else set to NaN): of rhs, the parity some selected piece takes as a source -- a clover or shift bit of parity p reads
 * rhs_p, a hop bit of parity p reads rhs_{1-p}, a bit whose field is NULL selects nothing; of lhs, the halves a piece accumulates into -- a
 * half that QMG_P_ZERO_E / QMG_P_ZERO_O clears is written without being read, a half no piece names is neither read nor written.  Never
 * read: the elements between the systems (vec_stride beyond the vector's length), the halo rows of a parity no hop takes as a source, and
 * any operand's segment of a system outside `mask` (entries without a mask serve every system). */
int qmg_stencil_apply_batch(const qmg_stencil_desc* d, void* lhs, const void* rhs, unsigned pieces,
                            int nrhs, size_t vec_stride, unsigned mask, void* stream);

/* OPT-IN storage format: d->clover / d->hopping point to complex<float> copies of the matrices (qmg_c64_to_c32); vectors,
 * shifts and all arithmetic stay fp64.  Halves the matrix stream of an HBM-bound coarse apply.  Meant for operators that
 * only precondition (the K-cycle inside a flexible fp64 outer solver); parity: equal to 1e-13 to the fp64 apply of the
 * ROUNDED matrices.  nc = 1, 2, 4 return QMG_ERR_UNSUPPORTED.  nrhs <= 16, mask as in qmg_stencil_apply_batch. */
int qmg_stencil_apply_mat32(const qmg_stencil_desc* d, void* lhs, const void* rhs, unsigned pieces,
                            int nrhs, size_t vec_stride, unsigned mask, void* stream);
/* The same with the matrices stored as complex<half> (qmg_convert_to_c16) and vectors of either precision; nc a multiple of 4 and > 4
 * (QMG_ERR_UNSUPPORTED otherwise).  qmg_stencil_apply_epi_t takes mat32 = 2 for this storage. */
int qmg_stencil_apply_mat16_t(int vec_dtype, const qmg_stencil_desc* d, void* lhs, const void* rhs, unsigned pieces,
                              int nrhs, size_t vec_stride, unsigned mask, void* stream);
int qmg_c64_to_c32(void* dst_f32, const void* src_f64, size_t n, void* stream);

/* ---------------- operator construction from U(1) links (device side) ---------------- */
/* gauge: nc=1 LatticeGauge (mu,eo,y,x), 2*Lx*Ly complex. */
int qmg_wilson_fill(void* clover, void* hopping, const void* gauge, int Lx, int Ly, double wilson_coeff, void* stream); /* wilson.h:153-209 */
int qmg_staggered_fill(void* hopping, const void* gauge, int Lx, int Ly, void* stream);                                /* staggered.h:50-72 */
int qmg_laplace_fill(void* clover, void* hopping, const void* gauge, int Lx, int Ly, void* stream);                    /* gaugedlaplace.h:45-68 */

/* ---------------- U(1) gauge generation and observables (u1/u1_utils.h) ---------------- */
/* Phase field: DEVICE double[2 Lx Ly], phase[mu*V + site] (gauge_coord_to_index); compact links U = exp(i A) in the same order.
 * heatbath_noncompact_update (u1_utils.h:607-757) as a four-colour PARALLEL heatbath (x-links of even / odd rows, y-links of
 * even / odd columns are conditionally independent): same Gibbs measure as the reference's sequential sweep, different
 * update order and random stream.  `seed` and the running sweep number `first_sweep` key a counter-based generator. */
int qmg_u1_heatbath_noncompact(double* phase, int Lx, int Ly, double beta, int n_update, unsigned long long seed,
                               unsigned long long first_sweep, void* stream);
int qmg_u1_phase_to_gauge(void* gauge, const double* phase, size_t n, void* stream);   /* polar_vector: U = exp(i A) */
int qmg_u1_gauge_to_phase(double* phase, const void* gauge, size_t n, void* stream);   /* A = arg U (what write_gauge_u1 stores) */
/* out_host[0..1] = average plaquette (get_plaquette_u1, :424-462), out_host[2] = topological charge (get_topo_u1, :465-508) */
int qmg_u1_plaquette(const void* gauge, int Lx, int Ly, double* out_host, void* stream);
int qmg_u1_noncompact_action(const double* phase, int Lx, int Ly, double beta, double* out_host, void* stream);   /* :386-421 */
/* Field tools (u1_utils.h:183-383, 545-603).  gauge: DEVICE complex<double>[2 Lx Ly] as above; trans: a DEVICE complex<double>[Lx Ly]
 * nc = 1 colour vector; all asynchronous on `stream`.  The three random fills draw from the counter-based generator of the heatbath,
 * keyed by (seed, mu, site): the result depends on neither launch geometry nor call order, and reproduces the DISTRIBUTION of the
 * reference's fields, not its std::mt19937 stream.  (lorentz_gauge_fix_u1, :511-542, is an unfinished stub there and is not offered.) */
int qmg_u1_hot_gauge(void* gauge, int Lx, int Ly, unsigned long long seed, void* stream);                  /* rand_gauge_u1: phases uniform in (-pi, pi) */
int qmg_u1_gauss_gauge(void* gauge, int Lx, int Ly, double beta, unsigned long long seed, void* stream);   /* gauss_gauge_u1: N(0, 1/|beta|); beta == 0: hot */
int qmg_u1_random_trans(void* trans, int Lx, int Ly, unsigned long long seed, void* stream);               /* rand_trans_u1 */
/* apply_gauge_trans_u1: U_mu(x) <- g(x) U_mu(x) conj g(x + mu), in place, one pass */
int qmg_u1_gauge_transform(void* gauge, const void* trans, int Lx, int Ly, void* stream);
/* apply_ape_smear_u1: n_iter times U_mu <- P[U_mu + alpha (upper staple + lower staple)], P[z] = z / |z|, P[0] = 1 (no (1 - alpha) factor,
 * as in the reference); both directions from the previous iterate, one launch per iteration.  smeared == gauge is allowed; n_iter == 0 copies. */
int qmg_u1_ape_smear(void* smeared, const void* gauge, int Lx, int Ly, double alpha, int n_iter, void* stream);
/* create_instanton_u1 / create_noncompact_instanton_u1, in place, with the reference's centring arithmetic */
int qmg_u1_instanton(void* gauge, int Lx, int Ly, double Q, int x0, int y0, void* stream);
int qmg_u1_noncompact_instanton(double* phase, int Lx, int Ly, double Q, void* stream);

/* ---- molecular dynamics of two-flavour Wilson HMC for compact U(1) (csrc/qmg_hmc.hip; not in the reference); fp64 only ----
 * H = 1/2 sum pi^2 + beta sum_x (1 - cos P(x)) + phi^dag (D^dag D)^-1 phi, D the Wilson operator with wilson_coeff 1.
 * theta, pi: DEVICE double[2 Lx Ly] in the (mu, eo, y, x) order; gauge: the links exp(i theta), DEVICE complex<double>[2 Lx Ly]. */
enum { QMG_HMC_GAUGE_ONLY = 1u };   /* flags of qmg_hmc_momentum_update: no fermion force, X and Y may be null */
/* pi -= dt (dS_g/dtheta + dS_f/dtheta) in one pass; X = (D^dag D)^-1 phi, Y = D X: DEVICE complex<double>[2 Lx Ly] */
int qmg_hmc_momentum_update(double* pi, const void* gauge, const void* X, const void* Y, int Lx, int Ly, double beta, double dt, unsigned flags, void* stream);
/* pi -= dt (dS_g/dtheta + sum_j weights[j] Ff(X[j], Y[j])) in one pass: the kick of a rational (one-flavour RHMC) pseudofermion action, Ff the
 * bilinear of the two-flavour force.  X, Y: HOST arrays of n_poles DEVICE spinors, X[j] = (D^dag D + mu_j^2)^-1 phi, Y[j] = D X[j]; weights: HOST
 * double[n_poles].  16 poles per launch, further poles in further launches.  n_poles = 0 or QMG_HMC_GAUGE_ONLY: the pure-gauge kick (X, Y,
 * weights may be null).  n_poles = 1 with weight 1 gives the bits of the two-flavour entry above. */
int qmg_hmc_momentum_update_poles(double* pi, const void* gauge, const void* const* X, const void* const* Y, const double* weights, int n_poles, int Lx, int Ly,
                                  double beta, double dt, unsigned flags, void* stream);
/* pi -= dt (dS_g/dtheta + sum_j weights[j] Fs(W[j])) in one pass: the kick of staggered pseudofermions on the even sites, two tastes (one pole
 * of weight 1) or rooted (one-taste RHMC).  With D = m + H, A = m^2 - H^2: W[j] = X_j (+) (H X_j)_o, X_j = (A_ee + mu_j^2)^-1 phi_e, and
 * Fs_mu(x) = eta_mu(x) eps(x) Im[U_mu(x) conj(W(x)) W(x+mu)].  W: HOST array of n_poles DEVICE complex<double>[Lx Ly] vectors (nc = 1, even-odd
 * layout); weights: HOST double[n_poles].  16 poles per launch, further poles in further launches.  n_poles = 0 or QMG_HMC_GAUGE_ONLY: the
 * pure-gauge kick of qmg_hmc_momentum_update (W, weights may be null). */
int qmg_hmc_momentum_update_staggered(double* pi, const void* gauge, const void* const* W, const double* weights, int n_poles, int Lx, int Ly, double beta, double dt,
                                      unsigned flags, void* stream);
/* pi -= dt (dS_g/dtheta + sum_j weights[j] sum_s Ff(X[j](.; s), Y[j](.; s))) in one pass: the kick of two-flavour domain-wall pseudofermions
 * (include/qmg/hmc_dwf.hpp), Ff the bilinear of the two-flavour Wilson force on the two spin components of slice s.  X, Y: HOST arrays of n_pairs
 * DEVICE complex<double>[2 Ls Lx Ly] full-lattice vectors (nc = 2 Ls, c = 2 s + sigma, even-odd layout); weights: HOST double[n_pairs], any sign.
 * QMG_HMC_DWF_G5_Y reads every Y[j] as Gamma5 Y[j] (slice Ls-1-s, the sign of sigma 1 flipped).  2 <= Ls <= 32; 4 pairs per launch, further
 * pairs in further launches.  n_pairs = 0 or QMG_HMC_GAUGE_ONLY: the pure-gauge kick of qmg_hmc_momentum_update, its bits (X, Y, weights may be
 * null).  No atomics: the sums over s and j run in a fixed order. */
enum { QMG_HMC_DWF_G5_Y = 2u };
int qmg_hmc_momentum_update_dwf(double* pi, const void* gauge, const void* const* X, const void* const* Y, const double* weights, int n_pairs, int Ls, int Lx, int Ly,
                                double beta, double dt, unsigned flags, void* stream);
/* What qmg_hmc_momentum_update_dwf launches (host only): plan_out = (family, lanes per site, block, gx, gy, LDS bytes, launches, pairs per
 * launch).  family: 0 unsupported, 1 the fused kernel, 2 the pure-gauge kick, 3 invalid. */
int qmg_hmc_dwf_plan(int Lx, int Ly, int Ls, int n_pairs, unsigned flags, int* plan_out, int plan_len);
/* theta += dt pi ; gauge = exp(i theta) in one pass over n = 2 Lx Ly links */
int qmg_hmc_link_update(double* theta, void* gauge, const double* pi, size_t n, double dt, void* stream);
/* One step of a pure-gauge inner loop in one launch:  pi -= dt_kick beta C^T sin P(gauge_in) ;  theta += dt_drift pi ;  gauge_out = exp(i theta).
 * The bits of qmg_hmc_momentum_update (QMG_HMC_GAUGE_ONLY, dt_kick) followed by qmg_hmc_link_update (dt_drift) in pi, theta and the links.
 * gauge_out != gauge_in (neighbours are read from gauge_in); overlapping or null fields, bad extents and a NaN beta or dt are refused with
 * QMG_ERR_INVALID and nothing is written. */
int qmg_hmc_gauge_step(double* theta, void* gauge_out, const void* gauge_in, double* pi, int Lx, int Ly, double beta, double dt_kick, double dt_drift, void* stream);
/* pi ~ N(0, 1) per link from the counter-based generator, a function of (seed, trajectory) alone; n even */
int qmg_hmc_momentum_refresh(double* pi, size_t n, unsigned long long seed, unsigned long long trajectory, void* stream);
/* the generator seed of random field `field` (0 momenta, 1 pseudofermion noise, 2 Metropolis number) of a trajectory */
unsigned long long qmg_hmc_stream_seed(unsigned long long seed, unsigned long long trajectory, int field);

/* ---- stout-smeared links for the Wilson fermions of the HMC above, and the chain rule of their force (csrc/qmg_stout.hip; not in the
 * reference); fp64 only ----
 * One level: theta^(k+1) = theta^(k) - rho C^T sin P^(k), i.e. U^(k+1)_mu(x) = U^(k)_mu(x) exp(-i rho (dS_w/dtheta^(k))_mu(x)), S_w = sum_x (1 - cos P):
 * an Euler step of the Wilson flow of length rho, gauge covariant.  With (C F)(x) = F_x(x) + F_y(x+xhat) - F_x(x+yhat) - F_y(x) the Jacobian of a
 * level is the symmetric J_k = 1 - rho C^T diag(cos P^(k)) C.  Fermions on V = U^(n), gauge action on U = U^(0):
 *   F^(n) = sum_j w_j Ff(X_j, Y_j) on V,   F^(k) = J_k F^(k+1),   pi -= dt (beta C^T sin P^(0) + F^(0)).
 * Forces F: DEVICE double[2 Lx Ly] in the (mu, eo, y, x) order of the momenta.  Every entry refuses odd or non-positive extents, null
 * pointers, negative counts and a non-finite rho with QMG_ERR_INVALID and leaves its outputs untouched. */
/* levels[k] = level k + 1, k = 0 .. n_levels - 1: DEVICE complex<double>[n_levels][2 Lx Ly], each from the level before (level 0 is `gauge`,
 * which is not copied); one launch per level.  n_levels == 0 does nothing (levels may be null).  levels must not overlap gauge. */
int qmg_u1_stout_smear(void* levels, const void* gauge, int Lx, int Ly, double rho, int n_levels, void* stream);
/* F = sum_j weights[j] Ff(X[j], Y[j]) with the links `gauge`, WRITTEN to F, Ff the bilinear of qmg_hmc_momentum_update.  X, Y, weights: the
 * pole lists of qmg_hmc_momentum_update_poles (HOST arrays of DEVICE spinors, HOST weights); 16 poles per launch, further launches add.
 * n_poles = 0 zeroes F (X, Y, weights may be null).  Two flavours is one pole of weight 1. */
int qmg_hmc_fermion_force(double* F, const void* gauge, const void* const* X, const void* const* Y, const double* weights, int n_poles, int Lx, int Ly, void* stream);
/* F_out = J_k F_in on the links gauge_k of level k, one pass; F_out is overwritten, F_out != F_in (refused otherwise) */
int qmg_u1_stout_force_level(double* F_out, const double* F_in, const void* gauge_k, int Lx, int Ly, double rho, void* stream);
/* pi -= dt (beta C^T sin P + J_0 F_in) in one pass over the thin links `gauge`: the gauge force and the last level of the chain rule from the
 * same plaquettes.  dt = 0 returns the momenta bit for bit; rho = 0 is the gauge kick plus F_in.  pi must not overlap F_in. */
int qmg_hmc_momentum_update_stout(double* pi, const void* gauge, const double* F_in, int Lx, int Ly, double beta, double rho, double dt, void* stream);

/* ---- gradient (Wilson) flow and Wilson / Polyakov loops for compact U(1) (csrc/qmg_flow.hip; not in the reference); fp64, single domain ----
 * d theta / dt = -dS_w/dtheta, S_w = sum_x (1 - cos P(x)): the gauge force of qmg_hmc_momentum_update at beta = 1.  Luescher's third-order
 * Runge-Kutta step in two registers, Z = -eps dS_w/dtheta:  A = Z, theta += A/4;  A = 8/9 Z - 17/36 A, theta += A;  A = 3/4 Z - A, theta += A.
 * theta, acc: DEVICE double[2 Lx Ly] in the (mu, eo, y, x) order; gauge*: the links exp(i theta), DEVICE complex<double>[2 Lx Ly]. */
/* one stage (1, 2, 3), one launch: Z from gauge_in, acc and theta updated in place, gauge_out = exp(i theta); gauge_out != gauge_in */
int qmg_u1_flow_stage(double* theta, double* acc, void* gauge_out, const void* gauge_in, int Lx, int Ly, double eps, int stage, void* stream);
/* n_steps full steps; gauge = exp(i theta) on entry and on return.  n_steps == 0 or eps == 0 leave both fields bit for bit. */
int qmg_u1_flow(double* theta, void* gauge, int Lx, int Ly, double eps, int n_steps, void* stream);
/* lattice averages of the planar R x T loops, 1 <= R <= r_max <= Lx/2, 1 <= T <= t_max <= Ly/2, from running line products (two passes
 * over the lattice per pair): out_host[2 ((R-1) t_max + (T-1))] = real part, [.. + 1] = imaginary part.  Synchronous. */
int qmg_u1_wilson_loops(const void* gauge, int Lx, int Ly, int r_max, int t_max, double* out_host, void* stream);
/* Polyakov loops: out_host[0..1] = average over y of prod_x U_x(x, y), out_host[2..3] = average over x of prod_y U_y(x, y).  Synchronous. */
int qmg_u1_polyakov(const void* gauge, int Lx, int Ly, double* out_host, void* stream);

/* ---------------- stencil variants (device side) ---------------- */
/* build_dagger_stencil (stencil_2d.h:1080-1139); also serves build_rbj_dagger_stencil (:1989-2060). */
int qmg_build_dagger(void* dagger_clover, void* dagger_hopping, const void* clover, const void* hopping,
                     int Lx, int Ly, int nc, void* stream);
/* build_rbjacobi_stencil (stencil_2d.h:1452-1601): cinv = (clover + shifts)^-1, rb clover = 1,
 * rb hopping_mu(x) = hopping_mu(x) . cinv(x+mu).  nc <= 32. */
int qmg_build_rbjacobi(void* cinv, void* rb_clover, void* rb_hopping, const qmg_stencil_desc* d, void* stream);
/* batched nc x nc conjugate transpose (cMATcopy_conjtrans_square) */
int qmg_cmat_conjtrans(void* out, const void* in, size_t nsite, int nc, void* stream);

/* ---------------- BLAS-1 on device vectors (the quantum-linalg leaves the path calls) ---------------- */
/* n = number of complex elements; scalars are (re,im) pairs passed by value.  One system is the batch entry at nrhs = 1: these ten run
 * qmg_batch_blas_t(QMG_C64, QMG_BOP_*, ...) with nrhs = 1, mask = 1 (same kernels, same operation order: DESIGN 4). */
int qmg_zero_vector(void* x, size_t n, void* stream);
int qmg_copy_vector(void* dst, const void* src, size_t n, void* stream);
int qmg_cax(double ar, double ai, void* x, size_t n, void* stream);                                   /* x *= a            */
int qmg_caxy(double ar, double ai, const void* x, void* y, size_t n, void* stream);                   /* y  = a x          */
int qmg_caxpy(double ar, double ai, const void* x, void* y, size_t n, void* stream);                  /* y += a x          */
int qmg_cxpy(const void* x, void* y, size_t n, void* stream);                                         /* y += x            */
int qmg_cxpay(const void* x, double ar, double ai, void* y, size_t n, void* stream);                  /* y  = x + a y      */
int qmg_caxpby(double ar, double ai, const void* x, double br, double bi, void* y, size_t n, void* stream);            /* y = a x + b y */
int qmg_cxpyz(const void* x, const void* y, void* z, size_t n, void* stream);                         /* z  = x + y        */
int qmg_caxpbyz(double ar, double ai, const void* x, double br, double bi, const void* y, void* z, size_t n, void* stream); /* z = a x + b y */
/* y += sum_{i<k} a_i x_i in one pass. coeffs: HOST array of 2k doubles (re,im); xs: HOST array of k device pointers. */
int qmg_multi_caxpy(const double* coeffs, const void* const* xs, int k, void* y, size_t n, void* stream);
/* y[site,c] = scale[c] * x[site,shuffle[c]]  (caxy_shuffle_pattern; gamma5 / sigma1 / chiral projections,
 * wilson.h:74-143, coarse.h:498-657).  nc <= 64; scale/shuffle are HOST arrays of length nc. */
int qmg_caxy_pattern(const double* scale, const int* shuffle, int nc, const void* x, void* y, size_t nsite, void* stream);
/* complex Gaussian fill, unit variance per real component, counter-based (reproducible, layout-independent) */
int qmg_gaussian(void* x, size_t n, unsigned long long seed, void* stream);

/* ---------------- global reductions ---------------- */
/* Two-stage (wavefront DPP + LDS block) deterministic reductions.  `out_dev` is a DEVICE buffer
 * (1 double for real results, 2 for dot) written asynchronously; `out_host`, if non-NULL, receives a
 * copy and makes the call synchronous.  Either may be NULL, not both.  The sums (norm2sq, dot, diffnorm2sq, multidot) are the batch
 * reductions below at nrhs = 1, mask = 1: the same kernels, the same summation order, and the same way to the host ("reduce_spin"). */
int qmg_norm2sq(const void* x, size_t n, double* out_dev, double* out_host, void* stream);
int qmg_dot(const void* x, const void* y, size_t n, double* out_dev, double* out_host, void* stream);   /* sum conj(x) y */
int qmg_diffnorm2sq(const void* x, const void* y, size_t n, double* out_dev, double* out_host, void* stream);
int qmg_norminf(const void* x, size_t n, double* out_dev, double* out_host, void* stream);
/* k dot products <x_i, y>, i < k, in one pass over y (GCR orthogonalisation). xs: HOST array of k device pointers.
 * out: 2k doubles. k <= 64 (more than 32: two passes of 32 and the rest; every dot is its own sum). */
int qmg_multidot(const void* const* xs, int k, const void* y, size_t n, double* out_dev, double* out_host, void* stream);
/* reductions/reductions.h:24-87: per-timeslice (per-y) norm2sq / dot. out: Ly (or 2*Ly) doubles.  (Results wanted on the host alone pass through
 * the reduction workspace: Ly <= 2^19.) */
int qmg_norm2sq_cv_timeslice(const void* cv, int Lx, int Ly, int nc, double* out_dev, double* out_host, void* stream);
int qmg_dot_cv_timeslice(const void* a, const void* b, int Lx, int Ly, int nc, double* out_dev, double* out_host, void* stream);
/* redot_cv_timeslice (reductions/reductions.h:47-66): sum[y] = Re sum_{x,c} conj(a) b, Ly doubles */
int qmg_redot_cv_timeslice(const void* a, const void* b, int Lx, int Ly, int nc, double* out_dev, double* out_host, void* stream);
/* gaussian_wall_source (reductions/reductions.h:90-162): cv = real Gaussian (mean + deviation N(0,1), imaginary part 0) on the elements with
 * y == timeslice and component == color, zero elsewhere; QMG_ERR_INVALID for timeslice >= Ly or color >= nc (the reference prints and returns).
 * The numbers come from the library's counter-based generator keyed by (seed, element index), not from std::mt19937 (see qmg_gaussian). */
int qmg_gaussian_wall_source(void* cv, int Lx, int Ly, int nc, int timeslice, int color, unsigned long long seed, double deviation, double mean, void* stream);

/* ---------------- transfer (transfer/transfer.h) ---------------- */
/* Null vectors are passed as the reference holds them: nvec fine vectors, vector-major
 * (null_vectors[d][k], transfer.h:79), contiguous with stride fine_size_cv.  Blocks are the
 * regular (fLx/cLx) x (fLy/cLy) rectangles of build_mapping (:410-448). */
int qmg_prolong(const void* nullvecs, int nvec, const void* coarse, void* fine,
                int fLx, int fLy, int fnc, int cLx, int cLy, int cnc, void* stream);     /* fine += P coarse   (:455-480) */
int qmg_restrict(const void* nullvecs, int nvec, const void* fine, void* coarse,
                 int fLx, int fLy, int fnc, int cLx, int cLy, int cnc, void* stream);    /* coarse += R fine   (:487-511) */
/* block_orthonormalize, one pass, in place (:514-607); cholesky (cLx*cLy*nvec*nvec complex) may be NULL. */
int qmg_block_orthonormalize(void* nullvecs, int nvec, int fLx, int fLy, int fnc, int cLx, int cLy,
                             void* cholesky, void* stream);
/* `passes` (1 or 2) passes in ONE launch -- the TransferMG constructor runs two (:160-174), the factor saved in the first:
 * each block's nvec x (bx by nc_f) tile is read once, orthonormalised in LDS, written once.  Asynchronous, no allocation. */
int qmg_block_orthonormalize_n(void* nullvecs, int nvec, int fLx, int fLy, int fnc, int cLx, int cLy,
                               void* cholesky, int passes, void* stream);

/* block_bi_orthonormalize, one pass, in place (:610-769): separate prolongator / restrictor vectors made block
 * bi-orthonormal (R^dag P = 1 per block); block_L / block_U (cLx*cLy*nvec*nvec complex each) may be NULL. */
int qmg_block_bi_orthonormalize(void* prolong_vecs, void* restrict_vecs, int nvec, int fLx, int fLy, int fnc, int cLx, int cLy,
                                void* block_L, void* block_U, void* stream);

/* ---------------- Galerkin coarse operator (operators/coarse.h:90-444) ---------------- */
int qmg_coarse_build(void* coarse_clover, void* coarse_hopping, const qmg_stencil_desc* fine,
                     const void* nullvecs, const void* restrict_vecs /* or NULL */,
                     int cLx, int cLy, int cnc, void* stream);

/* What the setup entry points do with a request: the answer of the one host function (csrc/qmg_setup_plan.h) that
 * qmg_block_orthonormalize_n, qmg_coarse_build(_slab) and qmg_build_rbjacobi switch on.  Host only, no HIP call; reads the tuning knob
 * "setup_fused".
 *   op 0 ORTHO     (fLx, fLy, fnc) -> (cLx, cLy), ncv = nvec, a = passes
 *   op 1 GALERKIN  (fLx, fLy, fnc) -> (cLx, cLy), ncv = cnc,  a = on a slab with halos (0 / 1)
 *   op 2 CINV      (fLx, fLy, fnc) = the stencil's (Lx, Ly, nc), a = clover present, b = one of the six shift numbers is not zero;
 *                  cLx, cLy, ncv are not looked at
 * Writes 8 ints and -1 into the rest of plan_out:
 *   family      0 unsupported (the call returns QMG_ERR_UNSUPPORTED: nc > 32 for CINV, a slab build that the probe passes would serve),
 *               1 k_block_ortho (the block's tile in LDS), 2 the full-lattice orthonormalisation passes (odd block width, tile beyond
 *               150 KB of LDS, "setup_fused" 0), 3 invalid (the call returns QMG_ERR_INVALID; any other op as well), 4 k_galerkin,
 *               5 the probe passes (cnc > 32, more than 150 KB of LDS, "setup_fused" 0), 6 k_clover_inverse
 *   tpb         k_block_ortho: threads per block of the null vectors, the power of two >= bx by fnc in 32 .. 256
 *   groups      k_block_ortho: blocks per workgroup (1 .. 8; tiles up to 24 KB share a workgroup)
 *   workgroups  the grid: min(ceil(blocks / groups), 262144), min(coarse sites, 262144), min(sites, 4096)
 *   lds         dynamic LDS bytes per workgroup
 *   flags       1 LDS opt-in (more than 64 KB) | 2 the last workgroup has groups without a block | 4 the grid-stride loop takes a second trip
 *   outs        k_galerkin: output entries per thread in use, ceil(cnc^2 / 256) in 1 .. 4
 *   threads     threads per workgroup
 * (a member the family does not use is 0).  QMG_ERR_INVALID: plan_out missing or plan_len below 8. */
int qmg_setup_plan(int op, int fLx, int fLy, int fnc, int cLx, int cLy, int ncv, int a, int b, int* plan_out, int plan_len);

/* ---------------- lock-step batches of independent right-hand sides ---------------- */
/* A batch vector is nrhs <= 16 vectors of n complex at a common `stride` (complex elements).  `mask` selects the
 * ACTIVE systems; a frozen system is neither read nor written.  A system's arithmetic (including the reduction
 * order) does not depend on the batch it is in; the single-vector entry points above are these at nrhs = 1.  Scalars are per system:
 * a[2k], a[2k+1] = re, im. */
typedef enum { QMG_BOP_ZERO = 0, QMG_BOP_COPY = 1, QMG_BOP_CAX = 2, QMG_BOP_CAXPY = 3, QMG_BOP_CXPY = 4, QMG_BOP_CAXPBYZ = 5,
               QMG_BOP_CAXY = 6, QMG_BOP_CXPAY = 7, QMG_BOP_CAXPBY = 8, QMG_BOP_CXPYZ = 9 } qmg_batch_op;
/* ZERO: z = 0; COPY: z = x; CAX: z *= a; CAXPY: z += a x; CXPY: z += x; CAXPBYZ: z = a x + b y;
 * CAXY: z = a x; CXPAY: z = x + a z; CAXPBY: z = a x + b z; CXPYZ: z = x + y.  z may alias x or y in CAXPBYZ and CXPYZ. */
int qmg_batch_blas(int op, const double* a, const double* b, const void* x, const void* y, void* z, size_t n,
                   int nrhs, size_t stride, unsigned mask, void* stream);
/* y_k += sum_j c[j][k] xs[j]_k ; coeffs[(j*nrhs + k)*2 + {0,1}]; xs: HOST array of nj batch base pointers */
int qmg_batch_multi_caxpy(const double* coeffs, const void* const* xs, int nj, void* y, size_t n,
                          int nrhs, size_t stride, unsigned mask, void* stream);
typedef enum { QMG_BRED_NORM2 = 0, QMG_BRED_DOT = 1, QMG_BRED_DIFFNORM2 = 2 } qmg_batch_red;
/* out_host[2k], out_host[2k+1] for each active system k; returns when the results are on the host (tuning key "reduce_spin": by polling a
 * host word behind them, the stream itself is then not synchronised; 0: hipStreamSynchronize) */
int qmg_batch_reduce(int op, const void* x, const void* y, size_t n, int nrhs, size_t stride, unsigned mask,
                     double* out_host, void* stream);
/* out_host[(k*nj + j)*2 + {0,1}] = <xs[j]_k, y_k>, nj <= 32; returns when the results are on the host (as qmg_batch_reduce) */
int qmg_batch_multidot(const void* const* xs, int nj, const void* y, size_t n, int nrhs, size_t stride, unsigned mask,
                       double* out_host, void* stream);
/* transfer.h:455-511 for the batch: the nvec null vectors are read once per 8 active systems */
int qmg_prolong_batch(const void* nullvecs, int nvec, const void* coarse, void* fine, int fLx, int fLy, int fnc,
                      int cLx, int cLy, int cnc, int nrhs, size_t cstride, size_t fstride, unsigned mask, void* stream);
int qmg_restrict_batch(const void* nullvecs, int nvec, const void* fine, void* coarse, int fLx, int fLy, int fnc,
                       int cLx, int cLy, int cnc, int nrhs, size_t fstride, size_t cstride, unsigned mask, void* stream);

/* ---------------- the path in either storage precision (`_t` = typed) ---------------- */
/* Same operations as the entry points above with the storage type of EVERY array argument (vectors, matrices in the
 * descriptor, null vectors) given by `dtype` (qmg_dtype); host-side scalars and reduction results stay double.  With
 * QMG_C64 they ARE the entry points above.  With QMG_C32: the fine kernels (nc = 1, 2, 4) compute in fp32, the coarse
 * vector-FMA kernels (B / B32) widen to fp64 in registers and round once on store, the coarse multi-rhs kernel (C: 4-5 systems up,
 * nc in {8,12,16,24,32}) multiplies on the f32 matrix cores with fp32 accumulators, reductions accumulate in fp64.
 * Parity bar: relative L2 <= 5e-6 per apply against the fp64 oracle on the same (rounded) inputs.
 * fp32 arrays should be 16-byte aligned with even strides (anything qmg_malloc returns is); otherwise the kernels fall
 * back to 8-byte accesses.  nrhs <= 16, `mask` selects the active systems (nrhs = 1, mask = 1 for a single vector). */
int qmg_convert(void* dst, int dst_dtype, const void* src, int src_dtype, size_t n, void* stream);   /* element-wise copy / round / widen */
int qmg_stencil_apply_t(int dtype, const qmg_stencil_desc* d, void* lhs, const void* rhs, unsigned pieces,
                        int nrhs, size_t vec_stride, unsigned mask, void* stream);
int qmg_batch_blas_t(int dtype, int op, const double* a, const double* b, const void* x, const void* y, void* z, size_t n,
                     int nrhs, size_t stride, unsigned mask, void* stream);
int qmg_batch_multi_caxpy_t(int dtype, const double* coeffs, const void* const* xs, int nj, void* y, size_t n,
                            int nrhs, size_t stride, unsigned mask, void* stream);
/* The three vector updates of one flexible-GCR iteration (quantum-linalg's minv_vector_gcr_var_precond_restart as called at
 * multigrid/stateful_multigrid.h:977-996 and tests/n13_wilson_kcycle/wilson_kcycle.cpp:459) in ONE pass, for the active systems k:
 *   w_k += sum_j c[j][k] ws[j]_k   (Gram-Schmidt against the cycle's directions; nj >= 0, coeffs as for qmg_batch_multi_caxpy_t)
 *   r_k += a[k] w_k                (a = -alpha; a[2k], a[2k+1] = re, im)
 *   z_next_k = r_k                 (z_next != NULL: the next search direction of an un-preconditioned GCR)
 * bit for bit qmg_batch_multi_caxpy_t, qmg_batch_blas_t(QMG_BOP_CAXPY), qmg_batch_blas_t(QMG_BOP_COPY) in that order.  w, r, z_next distinct. */
int qmg_batch_gcr_update_t(int dtype, const double* coeffs, const void* const* ws, int nj, void* w, const double* a, void* r, void* z_next,
                           size_t n, int nrhs, size_t stride, unsigned mask, void* stream);
/* The vector updates of one multi-shift CG iteration (quantum-linalg's minv_vector_cg_m; qmg/krylov.hpp: bcg_m_core) in ONE pass, for
 * every shift s < ns (1 <= ns <= 16) and every system k of mask & shift_masks[s]:
 *   x[s]_k += a[s][k] p[s]_k
 *   p[s]_k  = z[s][k] r_k + c[s][k] p[s]_k
 * xs, ps: tables of ns batch base pointers (as xs of qmg_batch_multi_caxpy_t); a, z, c: REAL coefficients, [s * nrhs + k] (CG on a
 * Hermitian operator has no others).  shift_masks[s]: the systems that still iterate shift s; a (system, shift) pair outside it is
 * neither read nor written, and a shift whose mask is 0 costs nothing.  r is read once per element for all shifts (once per 8 shifts
 * when ns > 8): 1 + 2 ns vector reads and 2 ns writes per system instead of the 4 ns reads and 2 ns writes of the separate passes.
 * bit for bit qmg_batch_blas_t(QMG_BOP_CAXPY) with (a, 0) on x[s], then qmg_batch_blas_t(QMG_BOP_CAXPBYZ) with (z, 0), (c, 0) on
 * r, p[s] -> p[s].  The 2 ns vectors and r are distinct. */
int qmg_batch_cgm_update_t(int dtype, const void* const* xs, const void* const* ps, int ns, const double* a, const double* z, const double* c,
                           const unsigned* shift_masks, const void* r, size_t n, int nrhs, size_t stride, unsigned mask, void* stream);
int qmg_batch_reduce_t(int dtype, int op, const void* x, const void* y, size_t n, int nrhs, size_t stride, unsigned mask,
                       double* out_host, void* stream);
int qmg_batch_multidot_t(int dtype, const void* const* xs, int nj, const void* y, size_t n, int nrhs, size_t stride, unsigned mask,
                         double* out_host, void* stream);
/* The K-cycle's smoother, MR(omega) of quantum-linalg's minv_vector_minres (call sites multigrid/stateful_multigrid.h:851-860, 1037-1046),
 * with EVERY SCALAR ON THE DEVICE: the smoothers run a fixed number of iterations (their tolerance, 1e-15, is never met), so no host
 * decision depends on <p,r> / <p,p> and the host round trip of each iteration can go.  Per step, after p = A r:
 *   qmg_batch_mr_dots_t     <p_k,r_k>, <p_k,p_k> of the active systems into the calling thread's device slot (one pass over p and r;
 *                           same two-stage deterministic reduction, hence the same bits, as qmg_batch_multidot_t; summed over ranks
 *                           under distributed reductions).  A stencil apply with the MR epilogue (qmg_stencil_apply_epi_t) fills the
 *                           same slot from the apply's own pass instead.
 *   qmg_batch_mr_update_t   alpha_k = omega <p_k,r_k> / <p_k,p_k> formed on the device (0 when <p_k,p_k> == 0);
 *                           x (+)= alpha r_in ;  r_out = r_in - alpha p.  x_set: x = alpha r_in (first step from x0 = 0);
 *                           r_out == NULL: residual not wanted; r_out may alias r_in.
 *   qmg_batch_mr_read_dots  the slot (4 doubles per system: Re<p,r>, Im<p,r>, <p,p>, -) on the host; synchronises (tests). */
/* A stencil apply with an EPILOGUE on every finished site value of the processed parities (kernels B / B32: any nc but 1, 2, 4; one
 * system per launch), instead of separate BLAS-1 passes over the result:
 *   out = other_scale * other + acc_scale * acc   (other == NULL: out = acc_scale * acc)  -- the residual b - A x of stateful_multigrid.h:863-866 /
 *         1023-1029, the Schur complement's r_e - D'_eo t of stencil_2d.h:1894-1907;
 *   dotv != NULL: <out, dotv> and <out, out> go to the calling thread's MR slot (qmg_batch_mr_update_t consumes them) -- minv_vector_minres's
 *         <p,r> and <p,p> with p = out, r = dotv, from the apply's own pass.
 * other / dotv: vectors with lhs's layout, precision and stride (element `system * vec_stride` onwards is used, like lhs and rhs).  Needs
 * overwrite semantics (QMG_P_ZERO on the processed parities); lhs must differ from rhs, other and dotv.  mat32: the matrices are complex<float>
 * (qmg_stencil_apply_mat32's storage) with dtype's vectors.  QMG_ERR_UNSUPPORTED: this operator is not served with an epilogue (nc = 1, 2, 4:
 * see qmg_wilson_apply_direct_epi) -- run the separate passes.
 * Read set: system `system` alone, in all four vectors -- rhs by the parity rule of qmg_stencil_apply_batch, other and dotv on the processed
 * parities only, lhs nowhere (it is overwritten); no other system, no element between the systems.  A refused call reads and writes nothing. */
typedef struct { const void* other; double other_scale, acc_scale; const void* dotv; } qmg_apply_epilogue;
int qmg_stencil_apply_epi_t(int dtype, int mat32, const qmg_stencil_desc* d, void* lhs, const void* rhs, unsigned pieces, size_t vec_stride, int system,
                            const qmg_apply_epilogue* epi, void* stream);
/* qmg_wilson_apply_direct / qmg_wilson_hops_direct with the same epilogue (kernel W, nc = 2, both storage precisions): ONE system per launch
 * (exactly one bit of `mask`), whole lattice or slab with all its rows (rows = 0). */
int qmg_wilson_apply_direct_epi(int dtype, const qmg_stencil_desc* d, const void* gauge, int gauge_Ly, int y0, double wilson_coeff, void* lhs, const void* rhs,
                                const void* halo_lo, const void* halo_hi, unsigned pieces, int nrhs, size_t vec_stride, size_t halo_stride, unsigned mask,
                                const qmg_apply_epilogue* epi, void* stream);
int qmg_wilson_hops_direct_epi(int dtype, const qmg_stencil_desc* d, const void* gauge, int gauge_Ly, int y0, double wilson_coeff, double hop_scale, void* lhs,
                               const void* rhs, const void* halo_lo, const void* halo_hi, unsigned pieces, int nrhs, size_t vec_stride, size_t halo_stride,
                               unsigned mask, const qmg_apply_epilogue* epi, void* stream);
int qmg_batch_mr_dots_t(int dtype, const void* r, const void* p, size_t n, int nrhs, size_t stride, unsigned mask, void* stream);
int qmg_batch_mr_update_t(int dtype, double omega, void* x, const void* r_in, void* r_out, const void* p, int x_set, size_t n, int nrhs,
                          size_t stride, unsigned mask, void* stream);
int qmg_batch_mr_read_dots(double* out_host, int nrhs, void* stream);
/* ONE basis V shared by every system of a batch (coarsest-level deflation and its Lanczos eigensolver, include/qmg/eigen.hpp):
 * nv <= 128 vectors of n elements, vector j at V + j * ldv (ldv >= n), storage dtype as V's and B's; systems as in the batch entry
 * points (nrhs <= 16, stride, mask).  Coefficient arrays are indexed [(k * nv + j) * 2 + {0,1}] (system k, basis vector j).
 * Every call reads each element of V once and each element of B once; fp64 accumulation for both storage types.  Under
 * distributed reductions (y-slabs) the entry points return QMG_ERR_UNSUPPORTED.
 *   qmg_basis_dot_t      C[k][j] = <v_j, b_k> for the active systems (deterministic two-stage reduction: the same bits run to run);
 *                        out_on_device: `out` is device memory and the call does not synchronise, else host memory (returns with them there).
 *   qmg_basis_update_t   b_k += sum_j C[k][j] v_j; coeffs in device memory (coeffs_on_device) or host memory.
 *   qmg_batch_deflate_t  e_k = sum_j v_j <v_j, b_k> inv_lambda[j] (e overwritten; inv_lambda: nv doubles in device memory): the dot,
 *                        a device-side final reduce-and-scale and the update in stream order; nothing synchronises. */
int qmg_basis_dot_t(int dtype, const void* V, int nv, size_t ldv, const void* B, size_t n, int nrhs, size_t stride, unsigned mask,
                    double* out, int out_on_device, void* stream);
int qmg_basis_update_t(int dtype, const double* coeffs, int coeffs_on_device, const void* V, int nv, size_t ldv, void* B, size_t n,
                       int nrhs, size_t stride, unsigned mask, void* stream);
int qmg_batch_deflate_t(int dtype, const void* V, int nv, size_t ldv, const double* inv_lambda, const void* B, void* E, size_t n,
                        int nrhs, size_t stride, unsigned mask, void* stream);
int qmg_prolong_batch_t(int dtype, const void* nullvecs, int nvec, const void* coarse, void* fine, int fLx, int fLy, int fnc,
                        int cLx, int cLy, int cnc, int nrhs, size_t cstride, size_t fstride, unsigned mask, void* stream);
int qmg_restrict_batch_t(int dtype, const void* nullvecs, int nvec, const void* fine, void* coarse, int fLx, int fLy, int fnc,
                         int cLx, int cLy, int cnc, int nrhs, size_t fstride, size_t cstride, unsigned mask, void* stream);
/* The same two operations (transfer/transfer.h:455-511) on complex<double> vectors with the null vectors STORED as complex<float> -- the narrow copy a
 * preconditioner level keeps of its prolongator (half of the transfer's bytes; arithmetic fp64: the result is the fp64 operation with the rounded
 * null vectors).  System by system through the single-vector kernels: meant for ONE active system (several share one read of the fp64 null vectors in
 * qmg_*_batch_t instead).  Even fnc and block width, null vectors 16-byte aligned; QMG_ERR_UNSUPPORTED otherwise. */
int qmg_prolong_batch_nv32(const void* nullvecs_c32, int nvec, const void* coarse, void* fine, int fLx, int fLy, int fnc,
                           int cLx, int cLy, int cnc, int nrhs, size_t cstride, size_t fstride, unsigned mask, void* stream);
int qmg_restrict_batch_nv32(const void* nullvecs_c32, int nvec, const void* fine, void* coarse, int fLx, int fLy, int fnc,
                            int cLx, int cLy, int cnc, int nrhs, size_t fstride, size_t cstride, unsigned mask, void* stream);
/* Which kernel serves a restrict (op = 0) or prolong (op = 1) request: the answer of the one host function every transfer launch above
 * switches on.  Host only, no HIP call.  dtype: the vectors' storage; null32 = 1: the _nv32 entry points (dtype QMG_C64); n_active: the
 * number of active systems of the call (1..16); aligned16: whether the null vectors and (one-system kernels) the fine vector are 16-byte
 * aligned.  Writes 8 ints per pass of up to 8 systems (one pass where the systems are served one by one) and -1 into the rest of plan_out:
 *   family  0 unsupported (the call returns QMG_ERR_UNSUPPORTED), 1 k_restrict, 2 k_restrict_generic, 3 k_prolong, 4 k_brestrict_mfma,
 *           5 k_brestrict_small, 6 k_brestrict_tile, 7 k_bprolong_tile, 8 / 9 k_restrict / k_prolong with complex<float> null vectors
 *   KB      systems the kernel is instantiated for (1: system by system)
 *   NV      NVT of k_brestrict_small, NVB of k_bprolong_tile
 *   MT, CR, nchunk, small  k_brestrict_mfma: row tiles, fine half-rows per chunk, chunks, and whether a full workgroup stages fewer
 *           positions than it has threads
 *   W       elements per lane of the one-system kernels
 * (a member the family does not use is 0).  QMG_ERR_INVALID: a request the entry points reject, or plan_len too short. */
int qmg_transfer_plan(int op, int dtype, int null32, int nvec, int fLx, int fLy, int fnc, int cLx, int cLy, int cnc, int n_active,
                      int aligned16, int* plan_out, int plan_len);

/* Which kernel serves a stencil apply: the answer of the one host function every stencil launch switches on, at the CURRENT values of the
 * tuning knobs stencil_site, stencil_pair, stencil_mfma and pair_prefetch.  Host only, no HIP call.
 * entry: the entry point (QMG_SE_*); mat: matrices 0 complex<double>, 1 complex<float>, 2 complex<half>; vec32: complex<float> vectors
 * (QMG_SE_MASKED stands for qmg_stencil_apply_batch / _t / _mat32 / _mat16_t by these two); n_active: the active systems; holes: they are
 * not systems 0 .. n_active-1 (QMG_SE_EPI: the system is not 0); inplace: lhs == rhs; has_clover / has_hopping: the descriptor's pointers
 * are set; epilogue: 0, 1 (no dotv) or 2 (with the dots), QMG_SE_EPI only; slab_rows: `rows` of QMG_SE_SLAB.
 * Writes 12 ints per pass (one pass, except kernel C: one per 16 systems) and -1 into the rest of plan_out:
 *   family   0 unsupported (the call returns QMG_ERR_UNSUPPORTED), 1 k_stencil_elem (A), 2 k_stencil_pair (A2), 3 k_stencil_site (S),
 *            4 k_stencil_gen (B), 5 k_stencil_gen32 (B32), 6 k_stencil_mfma (C), 7 the 1 x 1 lattice, 8 success with nothing launched,
 *            9 invalid (the call returns QMG_ERR_INVALID)
 *   storage  of the instantiation: 1 narrow matrices | 2 complex<float> vectors | 4 complex<half> matrices
 *   NC       compile-time nc (A, A2, S, C; C's two-site form: 16); 0 where nc is a run-time argument
 *   P        PT (B), PP (B32), MODE (C), SHAPE (S), ROWS (A2)
 *   K        KR (B, B32), else the systems of the pass
 *   flags    1 EPI | 2 with dots (grid.y capped) | 4 NORM | 8 PF | 16 ZERO | 32 BATCH | 64 VL | 128 PAIR | 256 shift term (1 x 1)
 *   S, H     tile of B / B32;  smem: dynamic LDS bytes;  gx, gy: the grid;  nk: systems the pass serves
 * QMG_ERR_INVALID: arguments no entry point can be called with, or plan_len too short. */
enum { QMG_SE_APPLY = 0, QMG_SE_MASKED = 1, QMG_SE_H16 = 2, QMG_SE_NORM2 = 3, QMG_SE_EPI = 4, QMG_SE_SLAB = 5 };
int qmg_stencil_plan(int entry, int mat, int vec32, int Lx, int Ly, int nc, unsigned pieces, int n_active, int holes, int inplace,
                     int has_clover, int has_hopping, int epilogue, int slab_rows, int* plan_out, int plan_len);

/* Which kernel serves each pass of a batch vector call (qmg_batch_blas_t ... qmg_batch_mr_update_t): the answer of the one host function
 * every launcher of those entry points switches on, at the CURRENT value of the tuning knob blas_nt_mb.  Host only, no HIP call.
 * entry: the entry point (QMG_BE_*); op: the QMG_BOP_* of QMG_BE_BLAS, the QMG_BRED_* of QMG_BE_REDUCE, else 0; n, stride, nrhs, mask: as
 * the entry point takes them; nj: the vector sets of QMG_BE_MULTI_CAXPY / _GCR_UPDATE / _MULTIDOT, the shifts of QMG_BE_CGM_UPDATE (with
 * shift_masks[nj]), else 0; flags: QMG_BE_MR_UPDATE 1 x_set | 2 r_out given, QMG_BE_GCR_UPDATE 1 z_next given; aligned16: every pointer
 * of the call is 16-byte aligned.  Writes 5 ints per pass, in launch order, and -1 into the rest of plan_out (5 * max_passes ints):
 *   family   QMG_BF_*: 0 success with nothing launched (no active system, n = 0, no vector set; a multi-shift launch none of whose
 *            shifts is iterated any more), 1 k_bblas, 2 k_bmulti_caxpy_small, 3 k_bmulti_caxpy (vectors of 16 MiB and more per system),
 *            4 qmg_multi_caxpy (ONE complex<double> system of 16 MiB and more), 5 k_bgcr_update, 6 k_bcgm_update,
 *            7 k_breduce, 8 k_bmultidot, 9 k_bmultidot<2> + k_bmr_final, 10 k_bmr_update
 *   W        elements per 16-byte access: 2 for complex<float> with aligned pointers, even n and (nrhs > 1) even stride, else 1
 *   nt       read-only operands are read non-temporally (the active systems add up to blas_nt_mb MiB)
 *   J        what the pass takes: vector sets (multi-axpy 1..8, GCR update 0..8), dots per pass over y (multidot 8 / 4 / 2 / 1; MR dots 2),
 *            shifts (multi-shift update 1..8)
 *   variant  the op (families 1, 7); the flags (families 5, 10); family 6: the largest number of shifts of the launch that one system
 *            still iterates
 * (a member the family does not use is 0).  QMG_ERR_INVALID: a request the entry point rejects, or more passes than max_passes. */
enum { QMG_BE_BLAS = 0, QMG_BE_MULTI_CAXPY = 1, QMG_BE_GCR_UPDATE = 2, QMG_BE_CGM_UPDATE = 3, QMG_BE_REDUCE = 4, QMG_BE_MULTIDOT = 5,
       QMG_BE_MR_DOTS = 6, QMG_BE_MR_UPDATE = 7 };
enum { QMG_BF_NOTHING = 0, QMG_BF_BLAS = 1, QMG_BF_MAXPY_SMALL = 2, QMG_BF_MAXPY_LONG = 3, QMG_BF_MAXPY_SINGLE = 4, QMG_BF_GCR = 5,
       QMG_BF_CGM = 6, QMG_BF_REDUCE = 7, QMG_BF_MULTIDOT = 8, QMG_BF_MR_DOTS = 9, QMG_BF_MR_UPDATE = 10 };
int qmg_batch_plan(int entry, int dtype, int op, size_t n, size_t stride, int nrhs, unsigned mask, int nj, const unsigned* shift_masks,
                   int flags, int aligned16, int* plan_out, int max_passes);

/* 16-bit storage of the fine operator (SURVEY 8f-4 "16-bit-storage smoother"; nc = 2 only): d->clover / d->hopping point to
 * complex<half> copies (qmg_convert_to_c16), vectors are complex<float>, arithmetic fp32: 112 B/site instead of 192.  The
 * rounding (2^-11) perturbs the OPERATOR, so this is for applies inside a preconditioner only. */
int qmg_convert_to_c16(void* dst_c16, const void* src, int src_dtype, size_t n, void* stream);
int qmg_convert_from_c16(void* dst, int dst_dtype, const void* src_c16, size_t n, void* stream);   /* complex<half> -> QMG_C64 / QMG_C32, exact */
int qmg_stencil_apply_h16(const qmg_stencil_desc* d, void* lhs, const void* rhs, unsigned pieces,
                          int nrhs, size_t vec_stride, unsigned mask, void* stream);

/* ---------------- multi-GPU: independent right-hand sides per rank ---------------- */
/* The path shards over right-hand sides; every rank holds a replica of the stencil/transfer data and
 * there is no halo exchange.  The one collective is a sum all-reduce (RCCL over xGMI) of a small
 * vector of per-RHS reduction results, once per Krylov reduction step, so all ranks take the same
 * convergence decision.  Rank 0 creates the 128-byte id and ships it by any host channel. */
int qmg_comm_get_unique_id(void* id128);
int qmg_comm_init(const void* id128, int world, int rank);      /* collective; after qmg_init(local_rank) */
/* qmg_comm_init with the id fetched through the launcher's rendezvous: QMG_COMM_ID_HEX (256 hex digits) if set, else one
 * TCP exchange with rank 0 on MASTER_ADDR : QMG_COMM_PORT (default MASTER_PORT + 1).  Bounded waits (QMG_COMM_TIMEOUT_S,
 * default 120 s): a missing rank is an error return, never a hang. */
int qmg_comm_init_env(int world, int rank);
int qmg_comm_rendezvous(void* blob128, int world, int rank);   /* the TCP leg alone: rank 0's 128 bytes reach every rank (host only) */
/* *all_ok = 1 iff every rank passed ok != 0 (one tiny all-reduce): lets an error on one rank stop all ranks together
 * instead of leaving the others blocked in the next collective. */
int qmg_comm_all_ok(int ok, int* all_ok);
int qmg_comm_world(int* world, int* rank);
int qmg_allreduce_sum_f64(double* buf_dev, size_t n, void* stream);   /* in place, async; no-op when world == 1 */
int qmg_comm_finalize(void);

/* ---------------- y-slab domain decomposition of ONE lattice ----------------
 * The reference is single-process and marks where this goes: cshift/cshift_2d.h:39-42,72,89 ("Becomes MPI").  Rank r of R
 * holds rows [r Ly/R, (r+1) Ly/R) of the global lattice as an ordinary even-odd lattice of Ly/R rows (Ly/R even, so the
 * colouring of a slab is the global one); every array keeps the layout of section 3.  Three pieces:
 *   qmg_halo_exchange         first / last row of a vector -> the neighbouring ranks' halo buffers (RCCL send/recv on xGMI;
 *                             one rank: device copies = the periodic wrap).  Halo buffer: [system][parity][Lx/2][nc] complex.
 *   qmg_stencil_apply_slab    the apply with rows -1 / Ly read from the halo buffers; `rows` splits it into the interior
 *                             (no halo needed: overlaps the exchange) and the two boundary rows.  nc = 2 in this round.
 *   qmg_comm_set_distributed_reductions   reductions of slab vectors are summed over the ranks inside the library.
 * Stencil arrays of a slab: qmg_wilson_fill_slab from the global gauge field (32 B/site, replicated). */
#define QMG_SLAB_H16 0x100   /* or-ed into the storage argument: matrices stored as complex<half> (vectors QMG_C32) */
#define QMG_SLAB_M32 0x200   /* nc != 2: matrices stored as complex<float> whatever the vectors' type (a preconditioner level's narrow Galerkin copy) */
#define QMG_SLAB_M16 0x400   /* nc != 2, a multiple of 4: matrices stored as complex<half> whatever the vectors' type */
int qmg_halo_exchange(int dtype, const void* vec, int Lx, int Ly_local, int nc, void* halo_lo, void* halo_hi, int nrhs, size_t vec_stride,
                      size_t halo_stride, void* stream);
/* rows of one parity only (parities: bit 0 even sites' rows, bit 1 odd sites' rows): what a D_eo / D_oe piece reads; the vectors of the
 * even-odd Schur systems are half-length, the other parity's rows do not exist */
int qmg_halo_exchange_parity(int dtype, const void* vec, int Lx, int Ly_local, int nc, void* halo_lo, void* halo_hi, int nrhs, size_t vec_stride,
                             size_t halo_stride, unsigned parities, void* stream);
int qmg_stencil_apply_slab(int storage, const qmg_stencil_desc* d, void* lhs, const void* rhs, const void* halo_lo, const void* halo_hi,
                           unsigned pieces, int nrhs, size_t vec_stride, size_t halo_stride, unsigned mask, int rows, void* stream);
int qmg_wilson_fill_slab(void* clover, void* hopping, const void* gauge_global, int Lx, int Ly_global, int y0, int Ly_local, double wilson_coeff,
                         void* stream);
int qmg_comm_set_distributed_reductions(int on);
/* setup on slabs: the Galerkin build with the null vectors' halo rows, and a Gaussian vector that equals the slab's rows of the
 * single-domain qmg_gaussian vector with the same seed (so a decomposed run draws the single-domain run's vectors) */
int qmg_coarse_build_slab(void* cclover, void* chopping, const qmg_stencil_desc* fine, const void* nullvecs, const void* restrict_vecs, int cLx, int cLy, int cnc,
                          const void* P_halo_lo, const void* P_halo_hi, size_t halo_stride, void* stream);
int qmg_gaussian_slab(void* x, int Lx, int Ly_global, int y0, int Ly_local, int nc, unsigned long long seed, void* stream);
/* right-block-Jacobi hopping on a slab: after qmg_build_rbjacobi(cinv, rb_clover, NULL, d) and a halo exchange of cinv (nc^2 components) */
int qmg_rb_hopping_slab(void* rb_hopping, const qmg_stencil_desc* d, const void* cinv, const void* cinv_halo_lo, const void* cinv_halo_hi, void* stream);
/* build_dagger_stencil (stencil_2d.h:1080-1139) on a y-slab.  ym_halo_hi: the `hi` buffer of qmg_halo_exchange applied to the -y hopping
 * field (hopping + 3 size_cm, nc^2 components per site); yp_halo_lo: the `lo` buffer of the exchange of the +y field (hopping + size_cm). */
int qmg_build_dagger_slab(void* dclover, void* dhopping, const void* clover, const void* hopping, int Lx, int Ly, int nc,
                          const void* ym_halo_hi, const void* yp_halo_lo, void* stream);
/* The nc = 1 operator fills on a y-slab (rows y0 .. y0 + Ly_local - 1, y0 even) from the GLOBAL gauge field, as qmg_wilson_fill_slab:
 * Staggered2D (staggered.h:50-72) and GaugedLaplace2D (gaugedlaplace.h:45-68). */
int qmg_staggered_fill_slab(void* hopping, const void* gauge_global, int Lx, int Ly_global, int y0, int Ly_local, void* stream);
int qmg_laplace_fill_slab(void* clover, void* hopping, const void* gauge_global, int Lx, int Ly_global, int y0, int Ly_local, void* stream);
/* Test transport: `world` host threads of one process act as ranks on one GPU (device copies + host sums behind thread barriers),
 * because one-GPU boxes cannot run two RCCL ranks.  Everything above the transport is the code the RCCL path runs. */
int qmg_comm_emulate_begin(int world);
int qmg_comm_emulate_attach(int rank);
int qmg_comm_emulate_end(void);

/* ---------------- the Wilson operator straight from the gauge links (csrc/qmg_wilson.hip, kernel W) ----------------
 * Same result as qmg_wilson_fill + qmg_stencil_apply (operators/wilson.h:153-209 + stencil_2d.h:912-936), without the stored
 * matrices: 96 B/site instead of 384 in fp64 (48 instead of 192 in fp32).  d: the vectors' lattice (nc = 2) and the shifts;
 * gauge: links in `dtype` on the lattice Lx x gauge_Ly, the vectors covering its rows y0 .. y0 + d->Ly - 1.  Whole lattice:
 * gauge_Ly = d->Ly, y0 = 0, halos NULL, rows 0.  y-slab: halos from qmg_halo_exchange, rows as in qmg_stencil_apply_slab.
 * Piece sets served: clover + every hop of the processed parities (shift pieces optional), or every hop alone;
 * QMG_ERR_UNSUPPORTED otherwise -- the stored stencil serves the rest. */
int qmg_wilson_apply_direct(int dtype, const qmg_stencil_desc* d, const void* gauge, int gauge_Ly, int y0, double wilson_coeff, void* lhs, const void* rhs,
                            const void* halo_lo, const void* halo_hi, unsigned pieces, int nrhs, size_t vec_stride, size_t halo_stride, unsigned mask, int rows,
                            void* stream);
/* The hops of the RIGHT-BLOCK-JACOBI Wilson stencil (stencil_2d.h:1556-1581, H'_mu(x) = H_mu(x) . cinv(x + mu)) from the links, for
 * a cinv that is `hop_scale` times the identity at every site (real mass, no eo / dof shift; hop_scale = the [0][0] entry
 * qmg_build_rbjacobi left in cinv): 128 instead of 320 B per written site for the D'_eo / D'_oe of a Schur-complement apply.
 * pieces: every hop of the processed parities and nothing else (QMG_ERR_UNSUPPORTED otherwise).  fp64: bit for bit the stored
 * right-block-Jacobi hopping through the site kernel. */
int qmg_wilson_hops_direct(int dtype, const qmg_stencil_desc* d, const void* gauge, int gauge_Ly, int y0, double wilson_coeff, double hop_scale, void* lhs,
                           const void* rhs, const void* halo_lo, const void* halo_hi, unsigned pieces, int nrhs, size_t vec_stride, size_t halo_stride,
                           unsigned mask, int rows, void* stream);
/* What the four entries (these two and their _epi forms) do with a request: the answer of the one host function their launch switches on, at
 * the current "wilson_pair".  Host only, no HIP call.  Lx, Ly, nc: the vectors' lattice (d); halos: both halo buffers are given; layout_ok:
 * what only the entry point sees of the buffers -- the halos come as a pair, and with nrhs > 1 vec_stride holds a vector and halo_stride a halo
 * row; scaled: the qmg_wilson_hops_direct entries; n_active: the systems whose mask bit is set (0 .. 16); inplace: lhs == rhs; rows as in
 * qmg_stencil_apply_slab; epi: 0 without an epilogue, else 1 | 2 (other is set) | 4 (dotv is set) | 8 (dotv == other) | 16 (dotv == rhs) |
 * 32 (other or dotv is lhs).  Writes 16 ints and -1 into the rest of plan_out:
 *   family  0 unsupported (the call returns QMG_ERR_UNSUPPORTED), 1 k_wilson_direct (kernel W: one site per lane group), 2 success with nothing
 *           launched, 3 invalid (the call returns QMG_ERR_INVALID), 4 k_wilson_pair (kernel W2: the full operator -- shape 1 on both parities --,
 *           both parities of a column per lane group; "wilson_pair" >= 1), 5 k_wilson_pair2 (W2 on two rows per lane group: "wilson_pair" >= 2,
 *           one system, an even run of consecutive rows, emode 0 or 1)
 *   lps     lanes per site: 2 in fp64, 1 in fp32
 *   block   threads per block
 *   gx, gy  the grid: gx blocks cover the lps * Lx/2 lanes of a half row; gy blocks walk the rows -- (parity, y) for family 1, y for 4, row pairs
 *           for 5 --: min(rows, 65535) of them, and with the dots at most max(1, 2048 / gx)
 *   flags   1 ZERO (every processed parity is overwritten) | 2 BATCH (more than one system) | 4 complex<float> | 8 the launch leaves the MR dots
 *   shape   1 clover + hops (+ shift), 2 hops alone, 3 hops alone times hop_scale (the hops entries)
 *   emode   the epilogue as the kernel is compiled for it: 0 none, 1 dots against the right-hand side (shape 1: nothing extra is loaded),
 *           2 out = other_scale other + acc_scale acc, 3 the same and dots against `other`, 4 dots against a separate vector
 *   nk      the systems served
 *   y_first, y_count, boundary_only   the rows of the launch: y_first .. y_first + y_count - 1, or rows 0 and Ly - 1
 *   npart   partials of the MR dots: gx * gy * 4, one per wavefront; 0 without dots
 *   status  what the call returns (pointer checks apart)
 *   par_first, par_count   the processed parities
 * (a member the family does not use is 0).  The status of a request, in this precedence -- Stencil2D falls back to the stored stencil on
 * QMG_ERR_UNSUPPORTED alone, so the order is part of the contract:
 *    1. the hops entries refuse QMG_P_CLOVER | QMG_P_SHIFT pieces: UNSUPPORTED   (then the entry's pointer checks: INVALID)
 *    2. dtype, rows outside 0 .. 2, n_active outside 0 .. 16, a lattice (Lx x Ly, Lx x gauge_Ly) that is not even x even and >= 2 x 2, y0 negative or
 *       odd or y0 + Ly > gauge_Ly: INVALID
 *    3. nc != 2: UNSUPPORTED
 *    4. !layout_ok, or no halos with gauge_Ly != Ly or rows != 0 (a slab needs its halos): INVALID
 *    5. n_active == 0: nothing
 *    6. an epilogue with n_active != 1: UNSUPPORTED
 *    7. an epilogue vector that is lhs: INVALID
 *    8. other and dotv both set and different: UNSUPPORTED
 *    9. no piece names a parity: nothing
 *   10. no row: rows == 1 on Ly == 2: nothing
 *   11. a piece set that is not shape 1 or 2 on every processed parity alike, or a hops entry with a shape other than 2: UNSUPPORTED
 *   12. inplace with shape 1 or both parities: INVALID
 *   13. an epilogue without QMG_P_ZERO on every processed parity, or inplace: INVALID
 * QMG_ERR_INVALID from qmg_wilson_plan itself: plan_out missing or plan_len below 16. */
int qmg_wilson_plan(int dtype, int Lx, int Ly, int nc, int gauge_Ly, int y0, int halos, int layout_ok, int scaled, unsigned pieces, int n_active, int inplace,
                    int rows, unsigned epi, int* plan_out, int plan_len);

/* ---------------- the Shamir domain-wall operator (operators/dwf.h; csrc/qmg_dwf.hip) ----------------
 * nc = 2 Ls components per site, c = 2 s + sigma (s the fifth-dimension slice, sigma the spin); Ls = 2 .. 32.  D = clover + hopping + shift:
 *   clover   3w on the diagonal;  out(s+1, 0) -= psi(s, 0) and out(s, 1) -= psi(s+1, 1) for s = 0 .. Ls-2;
 *            out(0, 0) += m psi(Ls-1, 0) and out(Ls-1, 1) += m psi(0, 1)   (m = mass_re + i mass_im, the wall mass)
 *   hopping  diagonal in s, the 2 x 2 spin blocks of qmg_wilson_fill on every slice
 *   shift    the domain-wall height M5 goes into the stencil's identity shift (the reference's default is -1)
 * qmg_dwf_fill writes the stored form -- the full nc x nc clover and hopping fields, zeros included -- that the dagger, right-block-Jacobi and
 * Galerkin builds read; fp64, on the device. */
int qmg_dwf_fill(void* clover, void* hopping, const void* gauge, int Lx, int Ly, int Ls, double mass_re, double mass_im, double wilson_coeff, void* stream);
/* lhs (+)= pieces(D) rhs without stored matrices (kernels D / D2): 64 Ls + 32 B/site in fp64 (32 Ls + 16 in fp32) instead of the stored stencil's
 * 5 (2 Ls)^2 complex numbers per site.  d: Lx, Ly, nc (= 2 Ls) and the three shifts with the stencil's semantics (its matrix pointers are
 * ignored); gauge: the links in `dtype`; whole lattice only.  Piece sets served: those of qmg_wilson_apply_direct -- clover + every hop of the
 * processed parities (shift pieces and QMG_P_ZERO optional), or every hop alone, where lhs == rhs is allowed for one parity;
 * QMG_ERR_UNSUPPORTED otherwise (the stored stencil serves the rest).  QMG_ERR_INVALID, before anything is launched: a dtype other than
 * QMG_C64 / QMG_C32, Ls outside 2 .. 32, d->nc != 2 Ls, nrhs outside 1 .. 16, a vec_stride shorter than a vector, pointers that are not
 * 16-byte aligned.  mask as in qmg_stencil_apply_batch. */
int qmg_dwf_apply_direct(int dtype, const qmg_stencil_desc* d, const void* gauge, int Ls, double mass_re, double mass_im, double wilson_coeff,
                         void* lhs, const void* rhs, unsigned pieces, int nrhs, size_t vec_stride, unsigned mask, void* stream);
/* What qmg_dwf_apply_direct does with a request: the answer of the one host function its launch switches on.  Host only, no HIP call.
 * n_active: the systems whose mask bit is set (0 .. 16); inplace: lhs == rhs.  Writes 8 ints and -1 into the rest of plan_out:
 *   family  0 unsupported (the call returns QMG_ERR_UNSUPPORTED), 1 k_dwf_direct (kernel D), 2 success with nothing launched, 3 invalid
 *           (the call returns QMG_ERR_INVALID), 4 k_dwf_pair (kernel D2: the full operator -- shape 1 on both parities --, both parities of a
 *           column per lane)
 *   lps     lanes per site: Ls, a lane owns one (site, s) pair with its two spin components
 *   block   threads per block
 *   gx, gy  the grid: gx blocks cover the lps * Lx/2 lanes of a half row, gy = min(rows, 65535) blocks walk the rows: (parity, y) of the
 *           processed parities for kernel D, y for kernel D2
 *   flags   1 ZERO (every processed parity is overwritten) | 2 BATCH (more than one system) | 4 complex<float>
 *   shape   1 clover + hops (+ shift), 2 hops alone
 *   nk      the systems served
 * (a member the family does not use is 0).  QMG_ERR_INVALID: plan_out missing or plan_len below 8. */
int qmg_dwf_plan(int dtype, int Lx, int Ly, int Ls, unsigned pieces, int n_active, int inplace, int* plan_out, int plan_len);

/* ---------------- the even-odd Schur complement of the domain-wall operator, from the links (csrc/qmg_dwf_eo.hip) ----------------
 * D = A + H: A = clover + shift is site-local, H the hops.  With d_p = 3 w + shift +- eo_shift (+ even, - odd sites) A_p is, per spin, the
 * Ls x Ls matrix  d_p - (lower shift along s) + m e_0 e_{Ls-1}^T  (sigma 0; sigma 1 mirrored under s -> Ls-1-s), inverted in the kernel by a
 * geometric scan along s plus the rank-one wall correction; the powers of 1/d_p are formed on the host in fp64.
 * Common to the three entries: d gives Lx, Ly, nc = 2 Ls and the shifts (matrix pointers ignored); qmg_dwf_apply_direct's validity rules
 * (QMG_C64 / QMG_C32, Ls in 2 .. 32, nrhs in 1 .. 16, 16-byte alignment, vec_stride at least a vector); mask as in qmg_stencil_apply_batch.
 * Refused before anything is launched:  dof_shift != 0 -- QMG_ERR_UNSUPPORTED (the diagonal is not constant along s);  |d_p| <= 1 for a
 * processed or inverted parity -- QMG_ERR_UNSUPPORTED (outside the domain-wall regime the scan's powers grow);  1 + m d_p^-Ls == 0 or any
 * coefficient (mass, wilson_coeff, shifts, alpha) not finite -- QMG_ERR_INVALID. */
enum { QMG_DWF_G5_IN = 1, QMG_DWF_G5_OUT = 2 };   /* Gamma5 psi(s, sigma) = (-1)^sigma psi(Ls-1-s, sigma) on the load of the source / on the store */
/* kernel I: lhs_p = alpha A_p^-1 rhs_p on the parities named by QMG_P_CLOVER_E / QMG_P_CLOVER_O (any other bit: QMG_ERR_UNSUPPORTED);
 * overwrites; lhs == rhs is allowed. */
int qmg_dwf_inv5(int dtype, const qmg_stencil_desc* d, int Ls, double mass_re, double mass_im, double wilson_coeff, void* lhs, const void* rhs,
                 unsigned pieces, double alpha_re, double alpha_im, int nrhs, size_t vec_stride, unsigned mask, void* stream);
/* kernel K: lhs_p = (QMG_P_ZERO_p ? 0 : lhs_p) + alpha A_p^-1 (H_{p,1-p} rhs_{1-p}).  pieces: all four hop bits of each processed parity plus
 * optional QMG_P_ZERO_*; any clover or shift bit, or a partial hop set: QMG_ERR_UNSUPPORTED.  flags: QMG_DWF_G5_IN (the hop source is
 * Gamma5 rhs) or 0.  lhs == rhs is allowed when exactly one parity is processed (QMG_ERR_INVALID otherwise). */
int qmg_dwf_hops_inv5(int dtype, const qmg_stencil_desc* d, const void* gauge, int Ls, double mass_re, double mass_im, double wilson_coeff, void* lhs,
                      const void* rhs, unsigned pieces, double alpha_re, double alpha_im, unsigned flags, int nrhs, size_t vec_stride, unsigned mask,
                      void* stream);
/* lhs_p = Gamma5^{out} M_p Gamma5^{in} rhs_p,  M_p = A_p - H_{p,1-p} A_{1-p}^-1 H_{1-p,p},  p = parity (0 even, 1 odd); flags: QMG_DWF_G5_IN |
 * QMG_DWF_G5_OUT.  Two launches (kernel K into tmp, then the second stage), whatever the flags.  Only the 1-p half of tmp is written; the 1-p
 * halves of lhs and rhs are not touched.  lhs, rhs and tmp are three different arrays (QMG_ERR_INVALID otherwise). */
int qmg_dwf_schur_apply(int dtype, const qmg_stencil_desc* d, const void* gauge, int Ls, double mass_re, double mass_im, double wilson_coeff, void* lhs,
                        const void* rhs, void* tmp, int parity, unsigned flags, int nrhs, size_t vec_stride, unsigned mask, void* stream);
/* What the three entries launch: the answer of the one host function they switch on.  Host only, no HIP call.
 * kernel: 0 kernel I (pieces as qmg_dwf_inv5), 1 kernel K (pieces as qmg_dwf_hops_inv5), 2 the second stage of M (pieces:
 * QMG_P_CLOVER_p | the four hops of p | QMG_P_SHIFT_p | QMG_P_ZERO_p of exactly one parity).  Writes 8 ints and -1 into the rest of plan_out:
 *   family  0 unsupported, 1 k_dwf_eo_inv5 with the hops (kernel K), 2 success with nothing launched, 3 invalid, 4 k_dwf_eo_inv5 on the own
 *           chunk (kernel I), 5 k_dwf_eo_schur2 (the second stage)
 *   lps     lanes per site: Ls
 *   block   threads per block: Ls floor(256 / Ls) -- a multiple of Ls, so that the lanes of a site never straddle a block
 *   gx, gy  the grid: gx blocks cover the Ls Lx/2 lanes of a half row, gy = min(rows, 65535) blocks walk the (parity, y) rows
 *   flags   qmg_dwf_plan's: 1 every processed parity overwritten, 2 more than one system, 4 complex<float>
 *   lds     bytes of LDS per block (the exchange along s; 0 for the second stage)
 *   nk      the systems served
 * QMG_ERR_INVALID: plan_out missing or plan_len below 8. */
int qmg_dwf_eo_plan(int dtype, int Lx, int Ly, int Ls, int kernel, unsigned pieces, int n_active, int inplace, int* plan_out, int plan_len);

/* ---------------- the Moebius domain-wall operator, from the links (csrc/qmg_mobius.hip) ----------------
 * The layout of the Shamir operator: nc = 2 Ls, c = 2 s + sigma, Ls = 2 .. 32.  With L the fifth-dimension hop
 *   (L psi)(s, 0) = psi(s-1, 0) (s >= 1),  (L psi)(0, 0) = -m psi(Ls-1, 0);   (L psi)(s, 1) = psi(s+1, 1) (s <= Ls-2),  (L psi)(Ls-1, 1) = -m psi(0, 1)
 * and H the hopping blocks of qmg_wilson_fill on every slice, d_w = 2 w + M5:
 *   D = (d_w + H) (b5 + c5 L) + (1 - L) = A + H B,   A = alpha + kappa L,  alpha = b5 d_w + 1,  kappa = c5 d_w - 1,   B = b5 + c5 L.
 * b5 = 1, c5 = 0 and w = 1 is the Shamir operator with shift = M5.  M5 is an argument here (B multiplies it); the three shifts of a descriptor
 * keep the stencil's meaning and are added to the diagonal of D afterwards (conjugated for D^dagger).
 * qmg_mobius_fill writes the stored form in fp64, zeros included: clover = A, hopping = H B (no longer diagonal in s); every entry is its
 * exact value rounded once (formed in double-double). */
int qmg_mobius_fill(void* clover, void* hopping, const void* gauge, int Lx, int Ly, int Ls, double mass_re, double mass_im, double wilson_coeff, double M5,
                    double b5, double c5, void* stream);
/* lhs (+)= op(D) rhs (+ shifts) without stored matrices: op 0 is D (the hop source b5 psi + c5 L psi is formed on the load: the lane reads the two
 * fifth-dimension halves of each neighbour next to its chunk, from the cache lines the wavefront has just asked for), op 1 is D^dagger =
 * Gamma5 (A' + B' H) Gamma5 with conj(m) in A', B' (the hop sum of a slice is exchanged along s in LDS; Gamma5 is a slice index and a sign on the
 * load and on the store).  64 Ls + 32 B/site in fp64.  Served: the full operator on both parities -- clover + every hop of both, the shift
 * pieces and QMG_P_ZERO_* optional per parity; every other piece set QMG_ERR_UNSUPPORTED (the stored stencil serves it).  QMG_ERR_INVALID,
 * before anything is launched: what qmg_dwf_apply_direct refuses; op outside 0 / 1; lhs == rhs; a mass, wilson_coeff, M5, b5 or c5 that is
 * not finite.  mask, batches and the stream as in qmg_dwf_apply_direct. */
int qmg_mobius_apply_direct(int dtype, const qmg_stencil_desc* d, const void* gauge, int Ls, double mass_re, double mass_im, double wilson_coeff, double M5,
                            double b5, double c5, int op, void* lhs, const void* rhs, unsigned pieces, int nrhs, size_t vec_stride, unsigned mask,
                            void* stream);
/* What qmg_mobius_apply_direct launches: the answer of the one host function it switches on.  Host only, no HIP call.  Writes 8 ints in the
 * layout of qmg_dwf_eo_plan and -1 into the rest of plan_out:
 *   family  0 unsupported, 1 k_mobius_load (op 0), 2 success with nothing launched, 3 invalid, 4 k_mobius_result (op 1)
 *   lps     lanes per site: Ls
 *   block   threads per block: 256 for op 0, Ls floor(256 / Ls) for op 1 (whole sites: the exchange is in LDS)
 *   gx, gy  gx blocks cover the Ls Lx/2 lanes of a half row, gy = min(2 Ly, 65535) blocks walk the (parity, y) rows
 *   flags   qmg_dwf_plan's: 1 both parities overwritten, 2 more than one system, 4 complex<float>
 *   lds     bytes of LDS per block: 0 for op 0, two buffers of one chunk per lane for op 1
 *   nk      the systems served
 * QMG_ERR_INVALID: plan_out missing or plan_len below 8. */
int qmg_mobius_plan(int dtype, int Lx, int Ly, int Ls, int op, unsigned pieces, int n_active, int inplace, int* plan_out, int plan_len);

/* ---------------- the even-odd Schur complement of the Moebius operator and its dagger, from the links (csrc/qmg_mobius_eo.hip) ----------------
 * D = A + H B with A, B site-local and the same at every site of a parity: alpha_p = alpha + shift +- eo_shift (+ even, - odd), A_p = alpha_p +
 * kappa L.  With p the parity of the system:
 *   M_p        = A_p - H_{p,1-p} B A_{1-p}^-1 H_{1-p,p} B
 *   M_p^dagger = Gamma5 [A'_p - B' H_{p,1-p} A'_{1-p}^-1 B' H_{1-p,p}] Gamma5         ': conj(m) and conjugated shifts
 *   prepare      b'_p    = b_p - H_{p,1-p} B A_{1-p}^-1 b_{1-p}
 *   reconstruct  x_{1-p} = A_{1-p}^-1 (b_{1-p} - H_{1-p,p} B x_p)
 * Gamma5 M Gamma5 is not M^dagger here (B does not commute with H).  L^Ls = -m on sigma 0, so every function of L is a twisted circulant of Ls
 * coefficients: (L^k h)(s) = h(s-k) for s >= k, -m h(s-k+Ls) below; sigma 1 mirrored under s -> Ls-1-s.  The tables are formed on the host in
 * long double, rounded once and passed by value:  A_p^-1: f_k = r^k / (alpha_p (1 + m r^Ls)), r = -kappa / alpha_p;  A_p^-1 B: g_k = b5 f_k +
 * c5 f_{k-1}, g_0 = b5 f_0 - m c5 f_{Ls-1}.  The kernels exchange a site's chunks along s through LDS and apply a table in 2 Ls complex FMAs.
 * Common to the three entries: d, M5, b5, c5 as in qmg_mobius_apply_direct and its validity rules; mask as in qmg_stencil_apply_batch.
 * Refused before anything is launched:  dof_shift != 0 -- QMG_ERR_UNSUPPORTED;  |kappa| >= |alpha_p| for a parity whose A is inverted --
 * QMG_ERR_UNSUPPORTED (the powers of r would not decay);  alpha_p == 0 or 1 + m r^Ls == 0 for such a parity, or any coefficient (mass,
 * wilson_coeff, M5, b5, c5, shifts, scale, a table entry) not finite -- QMG_ERR_INVALID. */
enum { QMG_MOBIUS_S_ONE = 0, QMG_MOBIUS_S_AINV = 1, QMG_MOBIUS_S_AINV_B = 2 };   /* `table`: the site matrix S applied through LDS */
enum { QMG_MOBIUS_R_ONE = 0, QMG_MOBIUS_R_B = 1 };                               /* `source`: the site matrix R applied to the hop source on the load */
/* lhs_p = scale S rhs_p on the parities named by QMG_P_CLOVER_E / QMG_P_CLOVER_O (any other bit: QMG_ERR_UNSUPPORTED); table: QMG_MOBIUS_S_AINV
 * or QMG_MOBIUS_S_AINV_B (QMG_ERR_INVALID otherwise); overwrites; lhs == rhs is allowed. */
int qmg_mobius_inv5(int dtype, const qmg_stencil_desc* d, int Ls, double mass_re, double mass_im, double wilson_coeff, double M5, double b5, double c5, void* lhs,
                    const void* rhs, unsigned pieces, int table, double scale_re, double scale_im, int nrhs, size_t vec_stride, unsigned mask, void* stream);
/* lhs_p = (QMG_P_ZERO_p ? 0 : lhs_p) + scale S H_{p,1-p} (R [Gamma5] rhs_{1-p}): stage 1 of M (S = A^-1, R = B) and of M^dagger (S = A^-1 B, R = 1,
 * QMG_DWF_G5_IN, called with conj(m) and conjugated shifts), prepare (S = 1, R = B) and reconstruct (S = A^-1, R = B).  pieces, flags and the
 * lhs == rhs rule are those of qmg_dwf_hops_inv5; a table or source outside the enums: QMG_ERR_INVALID. */
int qmg_mobius_hops_inv5(int dtype, const qmg_stencil_desc* d, const void* gauge, int Ls, double mass_re, double mass_im, double wilson_coeff, double M5, double b5,
                         double c5, void* lhs, const void* rhs, unsigned pieces, int table, int source, double scale_re, double scale_im, unsigned flags, int nrhs,
                         size_t vec_stride, unsigned mask, void* stream);
/* lhs_p = M_p rhs_p (op 0) or M_p^dagger rhs_p (op 1), p = parity (0 even, 1 odd).  Two launches either way; no Gamma5 pass and no copy.
 *   op 0:  tmp_o = -A_o^-1 H (B rhs_p),  then  lhs_p = A_p rhs_p + H (B tmp_o)             (B on the load in both; no LDS in the second)
 *   op 1:  tmp_o = -(A'_o^-1 B') H (Gamma5 rhs_p),  then  lhs_p = Gamma5 [A'_p Gamma5 rhs_p + B' (H tmp_o)]   (B' on the hop sum through LDS)
 * Only the 1-p half of tmp is written; the 1-p halves of lhs and rhs are not touched.  lhs, rhs and tmp are three different arrays and op is
 * 0 or 1 (QMG_ERR_INVALID otherwise). */
int qmg_mobius_schur_apply(int dtype, const qmg_stencil_desc* d, const void* gauge, int Ls, double mass_re, double mass_im, double wilson_coeff, double M5,
                           double b5, double c5, void* lhs, const void* rhs, void* tmp, int parity, int op, int nrhs, size_t vec_stride, unsigned mask,
                           void* stream);
/* What the three entries launch: the answer of the one host function they switch on.  Host only, no HIP call.
 * kernel: 0 qmg_mobius_inv5, 1 qmg_mobius_hops_inv5, 2 the second stage of M, 3 the second stage of M^dagger (pieces of 2 and 3:
 * QMG_P_CLOVER_p | the four hops of p | QMG_P_SHIFT_p | QMG_P_ZERO_p of exactly one parity; table and source as the entries take them, ignored
 * by kernels 2 and 3).  Writes 8 ints in the layout of qmg_dwf_eo_plan and -1 into the rest of plan_out:
 *   family  0 unsupported, 1 k_mobius_eo_mix with the hops, 2 success with nothing launched, 3 invalid, 4 k_mobius_eo_mix on the own chunk,
 *           5 k_mobius_eo_schur2, 6 k_mobius_eo_schur2_dagger
 *   lps     lanes per site: Ls
 *   block   threads per block: Ls floor(256 / Ls) (whole sites: the exchange is in LDS); 256 for family 5
 *   gx, gy  gx blocks cover the Ls Lx/2 lanes of a half row, gy = min(rows, 65535) blocks walk the (parity, y) rows
 *   flags   qmg_dwf_plan's (1 every processed parity overwritten, 2 more than one system, 4 complex<float>) | 8 the hop source is mixed by B
 *   lds     bytes of LDS per block: two buffers of one chunk per lane; 0 for family 5
 *   nk      the systems served
 * QMG_ERR_INVALID: plan_out missing or plan_len below 8. */
int qmg_mobius_eo_plan(int dtype, int Lx, int Ly, int Ls, int kernel, unsigned pieces, int table, int source, int n_active, int inplace, int* plan_out,
                       int plan_len);

/* ---------------- domain-wall measurements: wall source, wall / midpoint projection, slice norms (csrc/qmg_dwf_meas.hip) ----------------
 * A 5D vector has nc = 2 Ls components per site (c = 2 s + sigma), a 4D one nc = 2 (sigma); sigma = 0 is the P_+ component (the one that crosses
 * the wall as out(0, 0) += m psi(Ls-1, 0)), sigma = 1 P_-.  Whole lattice only.  Common to the three entries: dtype QMG_C64 / QMG_C32, Ls in
 * 2 .. 32, nsys in 1 .. 16 systems `stride` elements apart (ignored for nsys == 1; at least a vector, and even for QMG_C32), 16-byte aligned
 * vectors; anything else is QMG_ERR_INVALID before a launch.  Input and output must not overlap.
 * psi5 = the wall source of eta4, every element of psi5 overwritten:  psi5(x; 0, 0) = eta4(x, 0),  psi5(x; Ls-1, 1) = eta4(x, 1),  0 elsewhere. */
int qmg_dwf_wall_source(int dtype, int Lx, int Ly, int Ls, void* psi5, const void* eta4, int nsys, size_t stride5, size_t stride4, void* stream);
/* which = 0, the physical quark field:  q4(x, 0) = psi5(x; Ls-1, 0),  q4(x, 1) = psi5(x; 0, 1);
 * which = 1, the midpoint field:        q4(x, 0) = psi5(x; Ls/2-1, 0),  q4(x, 1) = psi5(x; Ls/2, 1) -- odd Ls: QMG_ERR_UNSUPPORTED.
 * Any other `which`: QMG_ERR_INVALID.  Only the two half chunks of a site that are needed are read. */
int qmg_dwf_wall_project(int dtype, int Lx, int Ly, int Ls, void* q4, const void* psi5, int which, int nsys, size_t stride4, size_t stride5, void* stream);
/* out[sys][y][s][sigma] = sum_x |psi5(x, y; s, sigma)|^2 -- 2 Ls Ly doubles per system, accumulated in fp64 for both dtypes, in one pass over the
 * vector (32 Ls B/site in fp64) plus a small second launch that adds per-block partials in a fixed order: no atomics, the same bits on every
 * run.  out_dev (device) and / or out_host (host; the stream is then synchronised) as in qmg_norm2sq_cv_timeslice: at least one.  The partials
 * live in a device buffer of the calling thread that grows on demand and is held until qmg_shutdown. */
int qmg_dwf_slice_norms(int dtype, int Lx, int Ly, int Ls, const void* psi5, int nsys, size_t stride5, double* out_dev, double* out_host, void* stream);
/* What the three entries launch: the answer of the one host function they switch on.  Host only, no HIP call.
 * kernel: 0 wall source, 1 wall projection, 2 midpoint projection, 3 slice norms.  Writes 8 ints and -1 into the rest of plan_out:
 *   family  0 unsupported (midpoint with odd Ls), 1 k_dwf_wall_source, 2 k_dwf_wall_project, 3 invalid, 4 k_dwf_slice_norms + k_dwf_slice_sum
 *   lps     lanes per site: Ls (source, norms: a lane owns one (site, s) pair with its two spin components), 2 (projections)
 *   block   threads per block: 256; for the norms Ls floor(256 / Ls), so that a lane that strides by whole blocks keeps its s
 *   gx, gy  the grid: gx blocks over the lps Lx/2 lanes of a half row (norms: gx = pbr), gy = min(2 Ly, 65535) blocks walk the (parity, y)
 *           rows; the systems go over grid.z
 *   pbr     norms: partial sums per (parity, y) row -- min(blocks that cover the half row, 4) blocks stride over it; else 0
 *   lds     bytes of LDS per block (norms: two doubles per lane of the largest block; else 0)
 *   nk      the systems served
 * QMG_ERR_INVALID: plan_out missing or plan_len below 8. */
int qmg_dwf_meas_plan(int dtype, int Lx, int Ly, int Ls, int kernel, int nsys, int* plan_out, int plan_len);

/* ---------------- flavour-singlet loops from diluted Z4 noise on lock-step batches (csrc/qmg_singlet.hip) ----------------
 * Element i = site * nc + c of a vector, site = (y + p Ly) Lx/2 + j (p the parity half).  The noise is a function of (seed, i) and is never
 * stored:  eta_i = i^(h >> 62),  h = splitmix64(seed * 0xD1342543DE82EF95 + 2 i) -- the first hash qmg_gaussian takes for element i -- that is
 * 1, i, -1, -i, of modulus one.  Dilution (nt, spin, eo): nt >= 1 divides Ly, spin and eo are 0 or 1, ncs = spin ? nc : 1, neo = eo ? 2 : 1; the
 * class of an element is d(i) = ((y mod nt) ncs + (spin ? c : 0)) neo + (eo ? p : 0), D = nt ncs neo classes with disjoint supports.  System k
 * of a batch (nrhs <= 16 vectors `stride` complex elements apart, bit k of mask: active) carries class first_class + k.  g(i), the sign of
 * gamma5: g5_mode 0 (Wilson) +1 for c < nc/2 and -1 otherwise, even nc only; g5_mode 1 (staggered epsilon) -1 on the odd half.
 * QMG_ERR_INVALID before any launch: an invalid lattice, nc < 1, nt that does not divide Ly, spin or eo outside {0, 1}, first_class < 0 or
 * first_class + nrhs > D, nrhs outside 1 .. 16, dtype outside QMG_C64 / QMG_C32, a missing or misaligned (16 bytes) vector, nrhs > 1 with
 * stride below Lx Ly nc; for the loops also g5_mode outside {0, 1}, odd nc with g5_mode 0, and both outputs NULL.  No active system: success,
 * nothing launched.
 * eta_i for all n elements (complex<double>). */
int qmg_noise_z4(void* eta, size_t n, unsigned long long seed, void* stream);
/* out_k = the diluted source of class first_class + k for the active systems, ONE launch: every element of an active system is written (the
 * noise value or zero); a frozen system and the padding between Lx Ly nc and stride are neither read nor written. */
int qmg_noise_dilute_batch(int dtype, void* out, int Lx, int Ly, int nc, int nt, int spin, int eo, int first_class, unsigned long long seed, int nrhs,
                           size_t stride, unsigned mask, void* stream);
/* For the active systems, in ONE pass over psi (16 nc B/site per system in fp64, 8 nc in fp32; the noise is regenerated inside the support and
 * never read), with d = first_class + k and every sum accumulated in fp64:
 *   S_k(y) = sum_{i in row y, d(i) = d} conj(eta_i) psi_k(i),   P_k(y) = the same sum of conj(eta_i) g(i) psi_k(i),   N_k(y) = sum_{i in row y} |psi_k(i)|^2
 *   out[(k Ly + y) 5 + {0..4}] = Re S, Im S, Re P, Im P, N      (N over the WHOLE row; S = P = 0 on a row outside the class)
 * Entries of frozen systems are not written; frozen systems and padding are not read.  No atomics, a fixed summation order: a system's five
 * numbers are the same bits on every run, in every batch and under every mask.  out_dev (device) and / or out_host (host; the stream is then
 * synchronised) as in qmg_norm2sq_cv_timeslice.  Without out_dev the results pass through a device buffer of the calling thread that grows on
 * demand and is held until qmg_shutdown. */
int qmg_loops_timeslice_batch(int dtype, const void* psi, int Lx, int Ly, int nc, int nt, int spin, int eo, int first_class, unsigned long long seed,
                              int g5_mode, int nrhs, size_t stride, unsigned mask, double* out_dev, double* out_host, void* stream);
/* What the two entries launch: the answer of the one host function they switch on.  Host only, no HIP call.  Writes 12 ints and -1 into the rest
 * of out, and returns the status the entries return for these arguments:
 *   family   0 invalid, 1 k_loops_timeslice / k_noise_dilute, 2 no active system (success, nothing launched)
 *   block    threads per block of both kernels: 256, whatever the row length (a row of Lx = 2 keeps 2 nc lanes of a block busy)
 *   gx, gy   the loops grid: gx = the active systems, gy = min(Ly, 65535) blocks over the timeslices
 *   walk     timeslices walked per block, ceil(Ly / gy): block b takes y = b, b + gy, ...; 1 unless Ly > 65535
 *   lds      bytes of LDS per block of the loops kernel
 *   doubles  doubles the loops entry writes: 5 Ly per active system
 *   dgx, dgy the dilution grid: dgx blocks of 256 lanes over the Lx Ly nc elements (at most 262144), dgy = the active systems
 *   dwalk    elements walked per lane of the dilution kernel
 *   nk       the active systems
 *   classes  D
 * QMG_ERR_INVALID also where out is missing or n_out below 12. */
int qmg_singlet_plan(int Lx, int Ly, int nc, int nt, int spin, int eo, int first_class, int nrhs, unsigned mask, int* out, int n_out);

/* ---------------- tuning hooks (not part of the reference surface) ---------------- */
/* Dispatch / codegen knobs, all with the defaults the measurements in profiles/ chose; results never depend on them
 * beyond summation order.  Unknown keys, and values a key does not take, return QMG_ERR_INVALID.
 *   "stencil_pair"  0: one site per lane group (kernel A); 2: fp64, both parities of a column on 2 rows per lane group (1 row where
 *                   Ly is odd) (2)
 *   "pair_prefetch" 1: fp64 batches with nc = 1 request system k+1's right-hand side ahead of system k's arithmetic (1)
 *   "blas_nt_mb"    BLAS-1 kernels read their read-only operands non-temporally from vectors of this many MiB upwards, 0 = never (256)
 *   "stencil_mfma"  1: multi-rhs coarse applies (nc in 8,12,16,24,32; >= 4-5 systems) on the f64 matrix cores, 2-MFMA
 *                   packing for <= 8 systems; 2: plain 4-MFMA products; 0: vector-FMA kernel B only (1)
 *   "stencil_site"  nc = 2 through the site kernel (csrc/qmg_site.hip): bit 0 fp64 where it is the faster one (hops-only,
 *                   one system), bit 1 fp32, bit 2 fp64 always (A/B measurements) (3)
 *   "wilson_pair"   the full Wilson operator from the links: 0 = one site per lane group (kernel W), 1 = both parities of a column
 *                   (kernel W2), 2 = W2 on two rows per lane group for one system on an even run of rows, else as 1 (2)
 *   "setup_fused"   1: block-local setup kernels (block orthonormalisation in LDS, Galerkin build as per-block products);
 *                   0: the full-lattice restrict / prolong / probe passes of the reference's formulation (1)
 *   "malloc_poison" 1: qmg_malloc fills every allocation with 0xFF bytes (NaNs in every storage precision): a buffer read before
 *                   it is written then shows deterministically.  The same holds for qmg_poison_scratch, through which the facade's
 *                   pools (VecPool, ArrayStorageMG) poison every block they hand out, recycled ones included, and for these buffers of
 *                   the library where they are created or grown: the reduction partials (batch reductions, the apply's fused norms, the
 *                   plaquette sums), the epilogue partials, both buffers of the deflation workspace, and the per-thread scratch fields
 *                   of the smearing, flow and dwf_meas entries.  Not filled: the result and MR slots of the reduction workspace (created
 *                   as zeros, which the MR slot's contract is) and the temporaries of the pass-by-pass setup fallbacks
 *                   (csrc/qmg_transfer.hip), which are zeroed or fully written before every use (0)
 *   "reduce_spin"   1: the host picks the results of the batch reductions (qmg_batch_reduce*, qmg_batch_multidot*) up by polling a sequence
 *                   number the final stage's last block publishes in coherent host memory behind them; the stream is NOT synchronised by
 *                   these calls then (later launches are ordered behind the kernel anyway).  0: hipStreamSynchronize, as before (1) */
/* (QMG_TUNING="key=value,key=value" in the environment applies the same settings inside qmg_init -- for A/B runs of programs that do not call this.) */
int qmg_set_tuning(const char* key, int value);

#ifdef __cplusplus
}
#endif
#endif /* QMG_HIP_H */
