// multigrid.hpp -- ArrayStorageMG, MultigridMG and StatefulMultigridMG (with the K-cycle
// `mg_preconditioner`) on device vectors.  Reference: storage/array_storage.h:23-155,
// multigrid/multigrid.h:54-600, multigrid/stateful_multigrid.h:43-1062.  Coarsest-level deflation (stateful_multigrid.h:611-712,
// 893-907) takes its eigenpairs from the GPU thick-restart Lanczos of eigen.hpp, not ARPACK (deflate_coarsest is defined there).
#ifndef QMG_MULTIGRID_HPP
#define QMG_MULTIGRID_HPP

#include <map>
#include <string>
#include <vector>

#include "coarse.hpp"
#include "krylov.hpp"

using std::vector;
using std::to_string;

// ---------------- device-vector pool (array_storage.h) ----------------
template <typename T>
class ArrayStorageMG {
 private:
  ArrayStorageMG(ArrayStorageMG const&);
  ArrayStorageMG& operator=(ArrayStorageMG const&);
  const long array_length;
  int allocated_arrays;
  vector<bool> is_checked_out;
  int n_checked;
  vector<T*> arrays;

 public:
  ArrayStorageMG(const long length, const int n_prealloc = 1) : array_length(length), allocated_arrays(n_prealloc), n_checked(0) {
    if (n_prealloc < 1) std::cout << "[QMG-ERROR]: ArrayStorageMG cannot preallocate less than one vector.\n";
    for (int i = 0; i < n_prealloc; i++) { arrays.push_back(allocate_vector<T>(array_length)); is_checked_out.push_back(false); }
  }
  ~ArrayStorageMG() { for (int i = 0; i < allocated_arrays; i++) deallocate_vector(&arrays[i]); }
  T* check_out() {
    for (int i = 0; i < allocated_arrays; i++)
      if (!is_checked_out[i]) {
        is_checked_out[i] = true; n_checked++;
        // "malloc_poison": a vector that leaves the pool again holds 0xFF like a fresh one, not what its last user left (the key off: no launch)
        qmg::ok(qmg_poison_scratch(arrays[i], (size_t)array_length * sizeof(T), qmg::current_stream()), "qmg_poison_scratch");
        return arrays[i];
      }
    arrays.push_back(allocate_vector<T>(array_length));
    is_checked_out.push_back(true);
    n_checked++;
    return arrays[allocated_arrays++];
  }
  void check_in(T* arr) {
    for (int i = 0; i < allocated_arrays; i++)
      if (arrays[i] == arr) {
        if (is_checked_out[i]) { is_checked_out[i] = false; n_checked--; }
        else cout << "[QMG_WARNING]: Returned array that wasn't checked out.\n";
        return;
      }
    cout << "[QMG_WARNING]: Returned array that doesn't live in library.\n";
  }
  int get_number_allocated() { return allocated_arrays; }
  int get_number_checked() { return n_checked; }
  void consolidate(int minimum = 1) {   // :128-154 (the reference also decrements n_checked for a free array; not repeated)
    for (int i = allocated_arrays - 1; i > 0; i--) {
      if (allocated_arrays <= minimum) break;
      if (!is_checked_out[i]) {
        deallocate_vector(&arrays[i]);
        arrays.erase(arrays.begin() + i);
        is_checked_out.erase(is_checked_out.begin() + i);
        allocated_arrays--;
      }
    }
  }
};

// ---------------- level bookkeeping (multigrid.h) ----------------
class MultigridMG {
 protected:
  MultigridMG(MultigridMG const&);
  MultigridMG& operator=(MultigridMG const&);
  int num_levels;
  vector<Lattice2D*> lattice_list;
  vector<TransferMG*> transfer_list;
  vector<Stencil2D*> stencil_list;
  vector<bool> is_stencil_managed;
  vector<ArrayStorageMG<complex<double>>*> storage_list;
  vector<complex<double>**> global_null_vectors;

  complex<double>** copy_global(complex<double>** nvecs, int n, Lattice2D* fine) {
    if (nvecs == 0) return 0;
    complex<double>** out = new complex<double>*[n];
    for (int j = 0; j < n; j++) {
      out[j] = 0;
      if (nvecs[j] != 0) { out[j] = allocate_vector<complex<double>>(fine->get_size_cv_l()); copy_vector(out[j], nvecs[j], fine->get_size_cv_l()); }
    }
    return out;
  }
  void free_global(int level_fine) {
    if (global_null_vectors[level_fine] == 0) return;
    const int n = lattice_list[level_fine + 1]->get_nc();
    for (int j = 0; j < n; j++) if (global_null_vectors[level_fine][j] != 0) deallocate_vector(&global_null_vectors[level_fine][j]);
    delete[] global_null_vectors[level_fine];
    global_null_vectors[level_fine] = 0;
  }

 public:
  // Storage precision of the Galerkin coarse operators (not in the reference, which is fp64 throughout): with it ON every coarse
  // operator built from now on keeps a complex<float> copy of its matrices and streams that in ORIGINAL-operator applies
  // (Stencil2D::enable_f32_matrices) -- half the bytes of an HBM-bound apply.  Vectors, shifts, arithmetic and the Galerkin
  // builds stay fp64; an apply then equals the fp64 apply of the ROUNDED matrices (relative 6e-8 per entry).
  //   -1 (default): ON for a StatefulMultigridMG -- a hierarchy that only PRECONDITIONS a flexible fp64 outer solve, whose true
  //      residual still reaches its fp64 tolerance (C3: the same 13 outer iterations, 1e-10) -- and OFF for a plain MultigridMG,
  //      whose coarse operators are used as operators (Galerkin identity R A P to 1e-15: n08);
  //    0 / 1: off / on for both (drivers: QMG_COARSE_F32=0 / 1);
  //    2: ON with complex<half> copies (Stencil2D::enable_f32_matrices(16): a quarter of the fp64 stream; levels whose nc or value range
  //       does not allow it keep complex<float>) -- opt-in (drivers: QMG_COARSE_BITS=16).
  static int& coarse_f32_storage() { static int f = -1; return f; }
  virtual bool coarse_f32_default() const { return false; }
  // (nc = 1, 2, 4 have no fp32-stored kernel; y-slabs stream the narrow copies like a whole lattice: qmg_stencil_apply_slab with QMG_SLAB_M32 / _M16)
  bool coarse_f32_wanted(int nc) const {
    if (nc == 1 || nc == 2 || nc == 4) return false;
    const int f = coarse_f32_storage();
    return f < 0 ? coarse_f32_default() : f != 0;
  }
  // true if any level of this hierarchy streams complex<float> Galerkin matrices (drivers print it)
  bool any_coarse_f32(int bits = 0) {   // bits = 16: ... in that width
    for (int i = 1; i < num_levels; i++) {
      if (!stencil_list[i]) continue;
      const Stencil2D::NarrowCopies& storage = stencil_list[i]->narrow[Stencil2D::QMG_NARROW_STORAGE];
      if (storage.on && (bits == 0 || storage.bits == bits)) return true;
    }
    return false;
  }
  bool any_coarse_f16() { return any_coarse_f32(16); }
  // drivers: QMG_COARSE_F32=0 / 1 and QMG_COARSE_BITS=64 / 32 / 16 (the latter wins)
  static void coarse_storage_from_env() {
    if (getenv("QMG_COARSE_F32")) coarse_f32_storage() = atoi(getenv("QMG_COARSE_F32")) != 0 ? 1 : 0;
    if (getenv("QMG_COARSE_BITS")) { const int b = atoi(getenv("QMG_COARSE_BITS")); coarse_f32_storage() = (b == 16) ? 2 : (b == 32) ? 1 : 0; }
  }

  enum QMGMultigridPrecondStencil { QMG_MULTIGRID_PRECOND_ORIGINAL = 0, QMG_MULTIGRID_PRECOND_RIGHT_BLOCK_JACOBI = 1 };

  MultigridMG(Lattice2D* in_lat, Stencil2D* in_stencil) {
    num_levels = 1;
    lattice_list.push_back(in_lat);
    storage_list.push_back(new ArrayStorageMG<complex<double>>(in_lat->get_size_cv_l(), 6));
    stencil_list.push_back(in_stencil);
    is_stencil_managed.push_back(false);
  }
  virtual ~MultigridMG() {
    for (int i = 0; i < num_levels; i++) {
      if (storage_list[i] != 0) delete storage_list[i];
      if (is_stencil_managed[i] && stencil_list[i] != 0) delete stencil_list[i];
    }
    for (int i = 0; i < num_levels - 1; i++) free_global(i);
  }

  int get_num_levels() { return num_levels; }
  Lattice2D* get_lattice(int i) { if (i >= 0 && i < num_levels) return lattice_list[i]; cout << "[QMG-ERROR]: Out of range: Lattice2D level " << i << " does not exist in MultigridMG object.\n"; return 0; }
  TransferMG* get_transfer(int i) { if (i >= 0 && i < num_levels - 1) return transfer_list[i]; cout << "[QMG-ERROR]: Out of range: TransferMG level " << i << " does not exist in MultigridMG object.\n"; return 0; }
  Stencil2D* get_stencil(int i) { if (i >= 0 && i < num_levels) return stencil_list[i]; cout << "[QMG-ERROR]: Out of range: Stencil2D level " << i << " does not exist in MultigridMG object.\n"; return 0; }
  ArrayStorageMG<complex<double>>* get_storage(int i) { if (i >= 0 && i < num_levels) return storage_list[i]; cout << "[QMG-ERROR]: Out of range: ArrayStorageMG level " << i << " does not exist in MultigridMG object.\n"; return 0; }
  complex<double>** get_global_null_vectors(int i) { if (i >= 0 && i < num_levels - 1) return global_null_vectors[i]; cout << "[QMG-ERROR]: Out of range: global null vectors level " << i << " does not exist in MultigridMG object.\n"; return 0; }

  // multigrid.h:257-302
  void push_level(Lattice2D* new_lat, TransferMG* new_transfer, bool build_stencil, bool is_chiral, QMGMultigridPrecondStencil build_stencil_from,
                  CoarseOperator2D::QMGCoarseBuildStencil build_extra, complex<double>** nvecs = 0) {
    num_levels++;
    lattice_list.push_back(new_lat);
    transfer_list.push_back(new_transfer);
    storage_list.push_back(new ArrayStorageMG<complex<double>>(new_lat->get_size_cv_l(), 6));
    if (build_stencil) {
      stencil_list.push_back(new CoarseOperator2D(new_lat, stencil_list[num_levels - 2], lattice_list[num_levels - 2], new_transfer, is_chiral,
                                                  build_stencil_from != QMG_MULTIGRID_PRECOND_ORIGINAL, build_extra));
      if (coarse_f32_wanted(new_lat->get_nc())) { stencil_list.back()->enable_f32_matrices(coarse_f32_storage() == 2 ? 16 : 32); new_transfer->enable_narrow_precond(); }
      is_stencil_managed.push_back(true);
    } else {
      stencil_list.push_back(0);
      is_stencil_managed.push_back(false);
    }
    global_null_vectors.push_back(copy_global(nvecs, new_lat->get_nc(), lattice_list[num_levels - 2]));
  }
  void push_level(Lattice2D* new_lat, TransferMG* new_transfer, bool build_stencil = false, bool is_chiral = false,
                  QMGMultigridPrecondStencil build_stencil_from = QMG_MULTIGRID_PRECOND_ORIGINAL, complex<double>** nvecs = 0) {
    push_level(new_lat, new_transfer, build_stencil, is_chiral, build_stencil_from, CoarseOperator2D::QMG_COARSE_BUILD_ORIGINAL, nvecs);
  }
  void push_level(Lattice2D* new_lat, TransferMG* new_transfer, complex<double>** nvecs) {
    push_level(new_lat, new_transfer, false, false, QMG_MULTIGRID_PRECOND_ORIGINAL, CoarseOperator2D::QMG_COARSE_BUILD_ORIGINAL, nvecs);
  }

  void pop_level() {   // :324-372
    if (num_levels == 1) { std::cout << "[QMG-ERROR]: In MultigridMG::pop_level, cannot pop when there is only one level.\n"; return; }
    const int i = num_levels - 1;
    if (storage_list[i] != 0) delete storage_list[i];
    storage_list.pop_back();
    if (is_stencil_managed[i] && stencil_list[i] != 0) delete stencil_list[i];
    stencil_list.pop_back();
    is_stencil_managed.pop_back();
    free_global(i - 1);
    global_null_vectors.pop_back();
    transfer_list.pop_back();
    lattice_list.pop_back();
    num_levels--;
  }

  void update_level(int level, Lattice2D* new_lat, TransferMG* new_transfer, bool build_stencil, bool is_chiral,
                    QMGMultigridPrecondStencil build_stencil_from, CoarseOperator2D::QMGCoarseBuildStencil build_extra, complex<double>** nvecs = 0) {   // :375-450
    if (level < 1 || level >= num_levels) {
      std::cout << "[QMG-ERROR]: In MultigridMG::update_level, cannot update level " << level << " as it does not exist yet anyway.\n";
      return;
    }
    if (storage_list[level] != 0) delete storage_list[level];
    if (is_stencil_managed[level] && stencil_list[level] != 0) delete stencil_list[level];
    free_global(level - 1);
    lattice_list[level] = new_lat;
    transfer_list[level - 1] = new_transfer;
    storage_list[level] = new ArrayStorageMG<complex<double>>(new_lat->get_size_cv_l(), 6);
    if (build_stencil) {
      stencil_list[level] = new CoarseOperator2D(new_lat, stencil_list[level - 1], lattice_list[level - 1], new_transfer, is_chiral,
                                                 build_stencil_from != QMG_MULTIGRID_PRECOND_ORIGINAL, build_extra);
      if (coarse_f32_wanted(new_lat->get_nc())) { stencil_list[level]->enable_f32_matrices(coarse_f32_storage() == 2 ? 16 : 32); new_transfer->enable_narrow_precond(); }
      is_stencil_managed[level] = true;
    } else {
      stencil_list[level] = 0;
      is_stencil_managed[level] = false;
    }
    global_null_vectors[level - 1] = copy_global(nvecs, new_lat->get_nc(), lattice_list[level - 1]);
  }
  void update_level(int level, Lattice2D* new_lat, TransferMG* new_transfer, bool build_stencil = false, bool is_chiral = false,
                    QMGMultigridPrecondStencil build_stencil_from = QMG_MULTIGRID_PRECOND_ORIGINAL, complex<double>** nvecs = 0) {
    update_level(level, new_lat, new_transfer, build_stencil, is_chiral, build_stencil_from, CoarseOperator2D::QMG_COARSE_BUILD_ORIGINAL, nvecs);
  }

  // lhs += A_i rhs; a level whose stencil was not built is emulated as R A_{i-1} P (:465-512)
  void apply_stencil(complex<double>* lhs, complex<double>* rhs, int i, QMGStencilType app_type = QMG_MATVEC_ORIGINAL) {
    if (i < 0 || i >= num_levels) { cout << "[QMG-ERROR]: Out of range: Cannot apply stencil at level " << i << "\n"; return; }
    if (stencil_list[i] != 0) { stencil_list[i]->apply_M(lhs, rhs, app_type); return; }
    if (app_type != QMG_MATVEC_ORIGINAL) { std::cout << "[QMG-ERROR]: In MultigridMG::apply_stencil, the emulated operator must be QMG_MATVEC_ORIGINAL.\n"; return; }
    complex<double>* pro_rhs = storage_list[i - 1]->check_out();
    complex<double>* Apro_rhs = storage_list[i - 1]->check_out();
    zero_vector(pro_rhs, lattice_list[i - 1]->get_size_cv_l());
    zero_vector(Apro_rhs, lattice_list[i - 1]->get_size_cv_l());
    transfer_list[i - 1]->prolong_c2f(rhs, pro_rhs);
    apply_stencil(Apro_rhs, pro_rhs, i - 1);
    transfer_list[i - 1]->restrict_f2c(Apro_rhs, lhs);
    storage_list[i - 1]->check_in(pro_rhs);
    storage_list[i - 1]->check_in(Apro_rhs);
  }
  void prolong_c2f(complex<double>* coarse_cv, complex<double>* fine_cv, int i) {
    if (i >= 0 && i < num_levels - 1) transfer_list[i]->prolong_c2f(coarse_cv, fine_cv);
    else cout << "[QMG-ERROR]: Out of range: Cannot apply prolong at level " << i << "\n";
  }
  void restrict_f2c(complex<double>* fine_cv, complex<double>* coarse_cv, int i) {
    if (i >= 0 && i < num_levels - 1) transfer_list[i]->restrict_f2c(fine_cv, coarse_cv);
    else cout << "[QMG-ERROR]: Out of range: Cannot apply prolong at level " << i << "\n";
  }
  complex<double>* check_out(int i) { if (i >= 0 && i < num_levels) return storage_list[i]->check_out(); cout << "[QMG-ERROR]: Out of range: Cannot check out vector at level " << i << ".\n"; return 0; }
  void check_in(complex<double>* vec, int i) { if (i >= 0 && i < num_levels) storage_list[i]->check_in(vec); else cout << "[QMG-ERROR]: Out of range: Cannot check in vector at level " << i << ".\n"; }
  int get_storage_number_allocated(int i) { if (i >= 0 && i < num_levels) return storage_list[i]->get_number_allocated(); cout << "[QMG-ERROR]: Out of range: Cannot query number of allocated arrays at level " << i << ".\n"; return -1; }
  int get_storage_number_checked(int i) { if (i >= 0 && i < num_levels) return storage_list[i]->get_number_checked(); cout << "[QMG-ERROR]: Out of range: Cannot query number of checked out arrays at level " << i << ".\n"; return -1; }
};

// ---------------- solve state + K-cycle (stateful_multigrid.h) ----------------
enum QMGDslashType { QMG_DSLASH_TYPE_NULLVEC = 0, QMG_DSLASH_TYPE_KRYLOV = 1, QMG_DSLASH_TYPE_PRESMOOTH = 2, QMG_DSLASH_TYPE_POSTSMOOTH = 3 };

class StatefulMultigridMG : public MultigridMG {
 private:
  StatefulMultigridMG(StatefulMultigridMG const&);
  StatefulMultigridMG& operator=(StatefulMultigridMG const&);
  int current_level;

 public:
  struct LevelSolveMG {   // :62-114
    QMGStencilType fine_stencil_app;
    double intermediate_tol; int intermediate_iters; int intermediate_restart_freq;
    double pre_tol; int pre_iters; bool pre_cgne;
    double post_tol; int post_iters; bool post_cgne;
    LevelSolveMG() : fine_stencil_app(QMG_MATVEC_ORIGINAL), intermediate_tol(1e-20), intermediate_iters(10000000), intermediate_restart_freq(32),
                     pre_tol(1e-20), pre_iters(1000000), pre_cgne(false), post_tol(1e-20), post_iters(1000000), post_cgne(false) {}
  };

  class DslashTrackerMG {   // :118-200
    std::map<QMGDslashType, int> tracker;
    int iterations, total;
   public:
    DslashTrackerMG() { reset_tracker(); }
    void add_tracker_count(QMGDslashType type, int accum) { tracker[type] += accum; total += accum; }
    void add_iterations_count(int accum) { iterations += accum; }
    void shift_all_to_nullvec() {
      tracker[QMG_DSLASH_TYPE_NULLVEC] += tracker[QMG_DSLASH_TYPE_KRYLOV] + tracker[QMG_DSLASH_TYPE_PRESMOOTH] + tracker[QMG_DSLASH_TYPE_POSTSMOOTH];
      tracker[QMG_DSLASH_TYPE_KRYLOV] = tracker[QMG_DSLASH_TYPE_PRESMOOTH] = tracker[QMG_DSLASH_TYPE_POSTSMOOTH] = 0;
      iterations = 0;
    }
    int get_tracker_count(QMGDslashType type) { return tracker[type]; }
    int get_total_count() { return total; }
    int get_iterations_count() { return iterations; }
    void reset_tracker() {
      tracker[QMG_DSLASH_TYPE_NULLVEC] = tracker[QMG_DSLASH_TYPE_KRYLOV] = tracker[QMG_DSLASH_TYPE_PRESMOOTH] = tracker[QMG_DSLASH_TYPE_POSTSMOOTH] = 0;
      total = 0; iterations = 0;
    }
  };

  struct CoarsestSolveMG {   // :204-241
    QMGStencilType coarsest_stencil_app;
    double coarsest_tol; int coarsest_iters; int coarsest_restart_freq;
    bool deflate;   // deflate a normal-equation coarsest solve once deflate_coarsest has computed eigenpairs; ignored otherwise
    double normal_shift;
    CoarsestSolveMG() : coarsest_stencil_app(QMG_MATVEC_ORIGINAL), coarsest_tol(1e-20), coarsest_iters(100000000), coarsest_restart_freq(32), deflate(true), normal_shift(0.0) {}
  };

 protected:
  vector<LevelSolveMG*> level_solve_list;
  vector<DslashTrackerMG*> dslash_tracker_list;
  CoarsestSolveMG* coarsest_solve;
  // coarsest-level deflation (deflate_coarsest): nev eigenpairs of the coarsest normal operator; the eigenvectors are one contiguous
  // device block (coarsest_evecs points into it), with 1 / lambda on the device and, for the fp32 K-cycle, a complex<float> copy
  unsigned int coarsest_deflated;
  complex<double>* coarsest_evals;
  complex<double>** coarsest_evecs;
  complex<double>* evec_block;
  complex<float>* evec_block32;
  double* inv_lambda_dev;
  int deflate_restarts, deflate_applies;
  void free_coarsest_deflation(const char* why) {
    if (coarsest_deflated == 0 && coarsest_evals == 0 && coarsest_evecs == 0) return;
    if (why) std::cout << "[QMG-INFO]: coarsest-level eigenpairs freed (" << why << ")\n";
    delete[] coarsest_evals; delete[] coarsest_evecs;
    deallocate_vector(&evec_block); deallocate_vector(&evec_block32); deallocate_vector(&inv_lambda_dev);
    coarsest_evals = 0; coarsest_evecs = 0; coarsest_deflated = 0;
  }

  static bool valid_fine_app(LevelSolveMG* s) {
    return s->fine_stencil_app == QMG_MATVEC_ORIGINAL || s->fine_stencil_app == QMG_MATVEC_RIGHT_JACOBI || s->fine_stencil_app == QMG_MATVEC_RIGHT_SCHUR;
  }

 public:
  StatefulMultigridMG(Lattice2D* in_lat, Stencil2D* in_stencil, CoarsestSolveMG* in_coarsest_solve)
      : MultigridMG(in_lat, in_stencil), current_level(0), coarsest_solve(in_coarsest_solve), coarsest_deflated(0), coarsest_evals(0), coarsest_evecs(0),
        evec_block(0), evec_block32(0), inv_lambda_dev(0), deflate_restarts(0), deflate_applies(0) {
    dslash_tracker_list.push_back(new DslashTrackerMG());
  }
  ~StatefulMultigridMG() { free_coarsest_deflation(0); for (size_t i = 0; i < dslash_tracker_list.size(); i++) delete dslash_tracker_list[i]; }
  virtual bool coarse_f32_default() const { return true; }   // this hierarchy is a preconditioner (mg_preconditioner)

  void set_multigrid_level(int level) {
    if (level >= 0 && level < get_num_levels()) current_level = level;
    else cout << "[QMG-ERROR]: Out of range: StatefulMultigridMG->current_level " << level << " is outside of [0,max_level-1].\n";
  }
  void go_finer() { if (current_level > 0) current_level--; else cout << "[QMG-ERROR]: Out of range: Cannot go finer than the top level in StatefulMultigridMG.\n"; }
  void go_coarser() { if (current_level < get_num_levels() - 2) current_level++; else cout << "[QMG-ERROR]: Out of range: Cannot go coarser than the second-coarsest level in StatefulMultigridMG.\n"; }
  int get_multigrid_level() { return current_level; }
  LevelSolveMG* get_level_solve(int i) {
    if (i >= 0 && i < get_num_levels() - 1 && level_solve_list[i] != 0) return level_solve_list[i];
    cout << "[QMG-ERROR]: Out of range: LevelSolveMG level " << i << " does not exist in StatefulMultigridMG object.\n";
    return 0;
  }
  LevelSolveMG* get_level_solve() { return get_level_solve(current_level); }
  CoarsestSolveMG* get_coarsest_solve() { return coarsest_solve; }

  // the six push_level flavours (:374-445)
  void push_level(Lattice2D* l, TransferMG* t, bool build_stencil, bool is_chiral, QMGMultigridPrecondStencil from, CoarseOperator2D::QMGCoarseBuildStencil extra, complex<double>** nvecs = 0) {
    MultigridMG::push_level(l, t, build_stencil, is_chiral, from, extra, nvecs);
    level_solve_list.push_back(0);
    dslash_tracker_list.push_back(new DslashTrackerMG());
  }
  void push_level(Lattice2D* l, TransferMG* t, bool build_stencil = false, bool is_chiral = false, QMGMultigridPrecondStencil from = QMG_MULTIGRID_PRECOND_ORIGINAL, complex<double>** nvecs = 0) {
    push_level(l, t, build_stencil, is_chiral, from, CoarseOperator2D::QMG_COARSE_BUILD_ORIGINAL, nvecs);
  }
  void push_level(Lattice2D* l, TransferMG* t, complex<double>** nvecs) { push_level(l, t, false, false, QMG_MULTIGRID_PRECOND_ORIGINAL, CoarseOperator2D::QMG_COARSE_BUILD_ORIGINAL, nvecs); }
  void push_level(Lattice2D* l, TransferMG* t, LevelSolveMG* in_solve, bool build_stencil, bool is_chiral, QMGMultigridPrecondStencil from, CoarseOperator2D::QMGCoarseBuildStencil extra, complex<double>** nvecs = 0) {
    MultigridMG::push_level(l, t, build_stencil, is_chiral, from, extra, nvecs);
    if (!valid_fine_app(in_solve)) std::cout << "[QMG-ERROR]: In StatefulMultigridMG:;push_level, LevelSolveMG::fine_stencil_app should only be original, right jacobi, or schur.\n";
    level_solve_list.push_back(in_solve);
    dslash_tracker_list.push_back(new DslashTrackerMG());
  }
  void push_level(Lattice2D* l, TransferMG* t, LevelSolveMG* in_solve, bool build_stencil = false, bool is_chiral = false, QMGMultigridPrecondStencil from = QMG_MULTIGRID_PRECOND_ORIGINAL, complex<double>** nvecs = 0) {
    push_level(l, t, in_solve, build_stencil, is_chiral, from, CoarseOperator2D::QMG_COARSE_BUILD_ORIGINAL, nvecs);
  }
  void push_level(Lattice2D* l, TransferMG* t, LevelSolveMG* in_solve, complex<double>** nvecs) {
    push_level(l, t, in_solve, false, false, QMG_MULTIGRID_PRECOND_ORIGINAL, CoarseOperator2D::QMG_COARSE_BUILD_ORIGINAL, nvecs);
  }
  void pop_level() {
    free_coarsest_deflation("the coarsest level was popped");
    level_solve_list.pop_back();
    delete dslash_tracker_list.back();
    dslash_tracker_list.pop_back();
    MultigridMG::pop_level();
  }
  void update_level(int level, Lattice2D* l, TransferMG* t, LevelSolveMG* in_solve, bool build_stencil, bool is_chiral, QMGMultigridPrecondStencil from, CoarseOperator2D::QMGCoarseBuildStencil extra, complex<double>** nvecs = 0) {
    if (!valid_fine_app(in_solve)) { std::cout << "[QMG-ERROR]: In StatefulMultigridMG:;update_level, LevelSolveMG::fine_stencil_app should only be original, right jacobi, or schur.\n"; return; }
    free_coarsest_deflation("a level was updated: the coarsest operator changes");
    MultigridMG::update_level(level, l, t, build_stencil, is_chiral, from, extra, nvecs);
    level_solve_list[level - 1] = in_solve;
  }
  void update_level(int level, Lattice2D* l, TransferMG* t, LevelSolveMG* in_solve, bool build_stencil = false, bool is_chiral = false, QMGMultigridPrecondStencil from = QMG_MULTIGRID_PRECOND_ORIGINAL, complex<double>** nvecs = 0) {
    update_level(level, l, t, in_solve, build_stencil, is_chiral, from, CoarseOperator2D::QMG_COARSE_BUILD_ORIGINAL, nvecs);
  }

  // trackers (:500-609)
  bool in_range(int i, const char* what) { if (i >= 0 && i < num_levels) return true; cout << "[QMG-ERROR]: Out of range: Cannot " << what << " at level " << i << ".\n"; return false; }
  void add_tracker_count(QMGDslashType type, int accum, int i) { if (in_range(i, "update tracker")) dslash_tracker_list[i]->add_tracker_count(type, accum); }
  void add_iterations_count(int accum, int i) { if (in_range(i, "update tracker")) dslash_tracker_list[i]->add_iterations_count(accum); }
  void shift_all_to_nullvec(int i) { if (in_range(i, "shift to null vectors")) dslash_tracker_list[i]->shift_all_to_nullvec(); }
  int get_tracker_count(QMGDslashType type, int i) { return in_range(i, "query tracker") ? dslash_tracker_list[i]->get_tracker_count(type) : -1; }
  int get_total_count(int i) { return in_range(i, "query tracker") ? dslash_tracker_list[i]->get_total_count() : -1; }
  int get_iterations_count(int i) { return in_range(i, "query tracker") ? dslash_tracker_list[i]->get_iterations_count() : -1; }
  std::vector<double> query_average_iterations() {
    std::vector<double> avg(num_levels);
    avg[0] = dslash_tracker_list[0]->get_iterations_count();
    for (int i = 1; i < num_levels; i++) avg[i] = ((double)dslash_tracker_list[i]->get_iterations_count()) / ((double)dslash_tracker_list[i - 1]->get_iterations_count());
    return avg;
  }
  void reset_tracker(int i = -1) {
    if (i == -1) { for (int j = 0; j < num_levels; j++) dslash_tracker_list[j]->reset_tracker(); }
    else if (in_range(i, "reset tracker")) dslash_tracker_list[i]->reset_tracker();
  }

  // coarsest-level deflation (:611-712): the num_low lowest and num_high highest eigenpairs of the coarsest normal operator, by the
  // thick-restart Lanczos of eigen.hpp (defined there); print_evals prints them as [QMG-COARSEST-EVALS] lines
  void deflate_coarsest(int num_low, int num_high, bool print_evals = false);
  unsigned int get_coarsest_deflated() { return coarsest_deflated; }
  complex<double>* get_coarsest_evals() { return coarsest_evals; }
  complex<double>** get_coarsest_evecs() { return coarsest_evecs; }
  // not in the reference: what the K-cycle's deflated guess streams (qmg_batch_deflate_t) and what the eigensolver cost
  const void* deflation_basis() { return evec_block; }
  const void* deflation_basis_f32();
  const double* deflation_inv_lambda() { return inv_lambda_dev; }
  int get_deflation_restarts() { return deflate_restarts; }
  int get_deflation_applies() { return deflate_applies; }

  // One K-cycle application, lhs ~= A^-1 rhs (stateful_multigrid.h:734-1060): mg_preconditioner_batch on a batch of one system,
  // defined at the end of batch.hpp.
  static void mg_preconditioner(complex<double>* lhs, complex<double>* rhs, int size, void* extra_data, inversion_verbose_struct* verb);
};

#endif
