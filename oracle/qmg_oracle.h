/* qmg_oracle.h -- CPU ORACLE for the quantum-mg multigrid hot path.
 *
 * TEST INFRASTRUCTURE ONLY.  This library is a plain, single-threaded CPU
 * restatement of the reference algorithm (weinbe2/quantum-mg) for the path
 * named in BASELINE.json.  Only tests/, __graft_entry__.smoke() and the
 * cpu_baseline leg of bench.py may link or call it -- as the checker, never
 * as the thing shipped or measured.  The product path (libqmg_hip.so) never
 * includes or links anything from this directory.
 *
 * PINNING STATUS.  The reference cannot be compiled in this image: every one
 * of its translation units includes blas/generic_vector.h & friends from
 * weinbe2/quantum-linalg (unpinned, absent, no network), and writing stand-in
 * headers to force a build is not allowed.  The reference stores no expected
 * output files.  The oracle is therefore pinned by
 *   (1) the reference's own known-answer test n02 (free Laplace point source:
 *       self 4+m^2, neighbours -1; applied twice: 20.0801, -8.02, 1;
 *       tests/n02_free_laplace_test/free_laplace.cpp:64-100),
 *   (2) the reference's own input fixtures tests/common_cfgs_u1/ (.dat files) read in
 *       its documented order (u1/u1_utils.h:53-63),
 *   (3) an independent coordinate-space construction of each operator from the
 *       formulas printed in operators/{wilson,staggered,gaugedlaplace}.h
 *       (tests/test_oracle_known_answers.py builds the matrix from (x,y)
 *       coordinates in numpy, with no even-odd index algebra shared with this
 *       file), and
 *   (4) the identities the reference tests print (n00 shift round trip, n05
 *       P^dag P = 1, n08 Galerkin, n17 <y,Mx> = <M^dag y,x>, n18/n21 Schur).
 * The BLAS leaves and Krylov solvers (quantum-linalg) have no stored outputs
 * anywhere: for those, "parity unpinned" -- semantics inferred from call sites.
 *
 * All complex data are interleaved (re,im) doubles == std::complex<double>.
 * Layouts follow the reference README.md:4-11:
 *   vector  (eo,y,x,c)            index nc*i + c
 *   matrix  (eo,y,x,c1,c2)        index nc*(nc*i + c1) + c2     (c1 = row)
 *   hopping (mu,eo,y,x,c1,c2)     mu in {+x,+y,-x,-y}
 *   site    i = (y + p*Ly)*Lx/2 + x/2,  p = (x+y)&1   (lattice/lattice.h:75-81)
 */
#ifndef QMG_ORACLE_H
#define QMG_ORACLE_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- enums mirrored from the reference (values identical) ---- */
/* cshift/cshift_2d.h:13-36 */
enum { QO_CSHIFT_FROM_0 = 1, QO_CSHIFT_FROM_XP1 = 2, QO_CSHIFT_FROM_YP1 = 3,
       QO_CSHIFT_FROM_XM1 = 4, QO_CSHIFT_FROM_YM1 = 5 };
enum { QO_EO_FROM_EVEN = 1, QO_EO_FROM_ODD = 2, QO_EO_FROM_EVENODD = 3 };
/* stencil/stencil_2d.h:25-40 */
enum { QO_DIR_XP1 = 0, QO_DIR_YP1 = 1, QO_DIR_XM1 = 2, QO_DIR_YM1 = 3 };

/* Piece mask for qo_stencil_apply (same bit meaning as include/qmg_hip.h). */
enum {
  QO_P_CLOVER_E = 1u << 0,  QO_P_CLOVER_O = 1u << 1,
  QO_P_EO_XP1 = 1u << 2, QO_P_EO_YP1 = 1u << 3, QO_P_EO_XM1 = 1u << 4, QO_P_EO_YM1 = 1u << 5,
  QO_P_OE_XP1 = 1u << 6, QO_P_OE_YP1 = 1u << 7, QO_P_OE_XM1 = 1u << 8, QO_P_OE_YM1 = 1u << 9,
  QO_P_SHIFT_E = 1u << 10, QO_P_SHIFT_O = 1u << 11,
  QO_P_ZERO_E = 1u << 12,  QO_P_ZERO_O = 1u << 13,
  QO_P_CLOVER = 3u, QO_P_EO = 0xFu << 2, QO_P_OE = 0xFu << 6, QO_P_HOPPING = 0xFFu << 2,
  QO_P_SHIFT = 3u << 10, QO_P_ZERO = 3u << 12,
  QO_P_ALL = 0xFFFu                     /* apply_M: clover + hopping + shift, accumulate */
};

typedef struct {
  int Lx, Ly, nc;
  const double* clover;    /* size_cm complex, or NULL  */
  const double* hopping;   /* 4*size_cm complex, or NULL */
  double shift[2], eo_shift[2], dof_shift[2];
} qo_stencil_desc;

/* ---- lattice/lattice.h ---- */
int  qo_coord_to_index(int Lx, int Ly, int x, int y);            /* :75-81  */
void qo_index_to_coord(int Lx, int Ly, int i, int* x, int* y);   /* :199-205 */

/* ---- cshift/cshift_2d.h:45-236 ---- */
int qo_cshift(double* lhs, const double* rhs, int cdir, int eo, int dof, int Lx, int Ly);

/* ---- stencil/stencil_2d.h:666-936 : lhs (+)= pieces * rhs, reference pass structure ---- */
int qo_stencil_apply(const qo_stencil_desc* d, double* lhs, const double* rhs, unsigned pieces);

/* ---- operator fills; gauge is the nc=1 LatticeGauge (mu,eo,y,x) ---- */
int qo_wilson_fill(double* clover, double* hopping, const double* gauge, int Lx, int Ly, double wilson_coeff); /* wilson.h:153-209 */
int qo_staggered_fill(double* hopping, const double* gauge, int Lx, int Ly);                                  /* staggered.h:50-72 */
int qo_laplace_fill(double* clover, double* hopping, const double* gauge, int Lx, int Ly);                    /* gaugedlaplace.h:45-68 */
int qo_free_laplace_fill(double* clover, double* hopping, int Lx, int Ly);                                    /* tests/n02.../free_laplace.h:39-41 */

/* ---- u1/u1_utils.h:38-67,172-181 ---- */
int qo_read_gauge_u1(double* gauge, int Lx, int Ly, const char* path);
int qo_phases_to_gauge_u1(double* gauge, const double* phases_file_order, int Lx, int Ly);
int qo_unit_gauge_u1(double* gauge, int Lx, int Ly);

/* ---- stencil variants: stencil_2d.h:1080-1139, 1452-1601, 1989-2060 ---- */
int qo_build_dagger(double* dclover, double* dhopping, const double* clover, const double* hopping, int Lx, int Ly, int nc);
int qo_build_rbjacobi(double* cinv, double* rclover, double* rhopping, const qo_stencil_desc* d);
int qo_build_rbj_dagger(double* dcinv, double* dclover, double* dhopping,
                        const double* cinv, const double* rclover, const double* rhopping, int Lx, int Ly, int nc);

/* ---- global reductions (quantum-linalg leaves; semantics from call sites) ---- */
double qo_norm2sq(const double* x, long n);
void   qo_dot(const double* x, const double* y, long n, double out[2]);   /* sum conj(x)*y */
double qo_diffnorm2sq(const double* x, const double* y, long n);
double qo_norminf(const double* x, long n);
/* reductions/reductions.h:24-87 */
void qo_norm2sq_cv_timeslice(double* sum, const double* cv, int Lx, int Ly, int nc);
void qo_dot_cv_timeslice(double* sum /*2*Ly*/, const double* a, const double* b, int Lx, int Ly, int nc);
void qo_redot_cv_timeslice(double* sum /*Ly*/, const double* a, const double* b, int Lx, int Ly, int nc);   /* :47-66 */
/* reductions/reductions.h:90-162; the draw of element i is the counter-based normal keyed by (seed, i) (the reference's std::mt19937 +
 * std::normal_distribution stream is not portable); returns -1 (and leaves cv untouched) for timeslice >= Ly or color >= nc */
int qo_gaussian_wall_source(double* cv, int Lx, int Ly, int nc, int timeslice, int color, unsigned long long seed, double deviation, double mean);

/* ---- transfer/transfer.h ---- */
/* coarse_map[i][j], ascending fine cv indices; returns fine_sites_per_coarse (transfer.h:386-448) */
int qo_transfer_build_map(int* map, int fLx, int fLy, int fnc, int cLx, int cLy);
/* fine += sum_d null[d] * coarse[i,d] (transfer.h:455-480); nullvecs = nvec contiguous fine vectors */
int qo_prolong(const double* nullvecs, int nvec, const double* coarse, double* fine,
               int fLx, int fLy, int fnc, int cLx, int cLy, int cnc);
/* coarse[i,d] += sum_k conj(null[d][k]) fine[k] (transfer.h:487-511) */
int qo_restrict(const double* nullvecs, int nvec, const double* fine, double* coarse,
                int fLx, int fLy, int fnc, int cLx, int cLy, int cnc);
/* in-place block Gram-Schmidt, one pass (transfer.h:514-607); cholesky may be NULL */
int qo_block_orthonormalize(double* nullvecs, int nvec, int fLx, int fLy, int fnc, int cLx, int cLy, double* cholesky);

/* in-place block bi-orthonormalisation, one pass (transfer.h:610-769); L, U may be NULL */
int qo_block_bi_orthonormalize(double* pvecs, double* rvecs, int nvec, int fLx, int fLy, int fnc, int cLx, int cLy, double* block_L, double* block_U);

/* ---- operators/coarse.h:90-444 : Galerkin coarse stencil by 9*nc probes ---- */
int qo_coarse_build(double* cclover, double* chopping, const qo_stencil_desc* fine,
                    const double* nullvecs, const double* restrict_vecs /*or NULL*/,
                    int cLx, int cLy, int cnc);

/* ---- K-cycle (oracle/qmg_oracle_kcycle.cpp): multigrid/stateful_multigrid.h:734-1060 driven as
 *      tests/n13_wilson_kcycle/wilson_kcycle.cpp:86-122,459-471 and tests/n19_wilson_kcycle_precond.  Krylov drivers: parity unpinned. ---- */
/* operator types, stencil/stencil_2d.h QMGStencilType */
enum { QO_MATVEC_ORIGINAL = 0, QO_MATVEC_DAGGER = 1, QO_MATVEC_RIGHT_JACOBI = 2, QO_MATVEC_RIGHT_SCHUR = 3, QO_MATVEC_M_MDAGGER = 4,
       QO_MATVEC_MDAGGER_M = 5, QO_MATVEC_RBJ_DAGGER = 6, QO_MATVEC_RBJ_M_MDAGGER = 7, QO_MATVEC_RBJ_MDAGGER_M = 8 };
typedef struct {
  int L; double mass; int n_refine, coarse_dof;   /* L x L Wilson, n_refine 4x4 coarsenings to coarse_dof colours */
  double tol; int max_iter, restart;              /* outer flexible GCR */
  double inner_tol, coarsest_tol; int n_smooth;   /* intermediate / coarsest tolerances (1000 iterations, restart 32); MR steps */
  int level_type;      /* ORIGINAL (n13 hierarchy), RIGHT_JACOBI or RIGHT_SCHUR (n19: Galerkin from the rbjacobi stencil): outer solve and every level */
  int coarsest_type;   /* level_type (restarted GCR), or one of the normal forms of that hierarchy (restarted CG) */
  int cgne;            /* CGNE smoothers (ignored on RIGHT_SCHUR levels) */
  double normal_shift; /* added to a normal coarsest operator */
} qo_kcycle_params;
/* gauge: nc=1 LatticeGauge; nullvecs[l]: coarse_dof vectors of level-l size, NOT yet block-orthonormalised; b: right-hand side of the
 * ORIGINAL system, x_out its reconstructed solution.  Returns outer iterations (negative: not converged; < -100000: bad input);
 * fills true_res (ORIGINAL operator), ops[level], its[level]; hist / chist (may be NULL) receive the outer relative residual per
 * iteration and the iteration count of every coarsest solve (negative: hit its cap), *nhist_out / *nchist_out their lengths. */
int qo_kcycle(const qo_kcycle_params* p, const double* gauge, const double* const* nullvecs, const double* b, double* x_out, double* true_res,
              long* ops, long* its, double* hist, int nhist, int* nhist_out, long* chist, int nchist, int* nchist_out);
/* the n13 shape (ORIGINAL, MR, GCR coarsest solve) */
int qo_wilson_kcycle(int L, double mass, int n_refine, int coarse_dof, const double* gauge, const double* const* nullvecs, const double* b,
                     double tol, int max_iter, int restart, double inner_tol, double coarsest_tol, int n_smooth, double* x_out,
                     double* true_res, long* ops, long* its);

/* the same solve with the outer residual history and the iteration count of every coarsest solve (negative: hit its cap) */
int qo_wilson_kcycle_history(int L, double mass, int n_refine, int coarse_dof, const double* gauge, const double* const* nullvecs, const double* b,
                             double tol, int max_iter, int restart, double inner_tol, double coarsest_tol, int n_smooth, double* x_out,
                             double* true_res, long* ops, long* its, double* hist, int nhist, int* nhist_out, long* chist, int nchist, int* nchist_out);
/* CPU twins of the Krylov drivers on a stencil operator (kind 0 CG, 1 BiCGStab-L, 2 Richardson, 3 MR, 4 restarted GCR;
 * op 0: M, 1: M^dagger M with `dag` the dagger stencil).  Returns 1 converged / 0 not / -1 bad kind.  See qmg_oracle_kcycle.cpp. */
int qo_krylov_solve(int kind, const qo_stencil_desc* d, const qo_stencil_desc* dag, int op, double* x, const double* b, int max_iter, double tol,
                    int param_i, double param_d, int* iters, double* res_sq, double* hist, int nhist);

/* ---- timing helper for bench.py's cpu_baseline leg ---- */
double qo_time_apply(const qo_stencil_desc* d, double* lhs, const double* rhs, unsigned pieces, int reps);

#ifdef __cplusplus
}
#endif
#endif
