/*
 * baspacho_amd.h -- C ABI of the MI355X-native supernodal sparse Cholesky.
 *
 * Plain C boundary (pointers + sizes, no C++/torch types) that a foreign-function binding
 * (ctypes, pybind, cgo, JNI ...) binds instead of the reference's C++ classes.  Each entry
 * point names the reference interface it stands for (paths relative to
 * /root/reference/baspacho/baspacho/).
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; bsp_last_error() returns the
 *     message of the last failure on the calling thread (reference: BASPACHO_CHECK_* throw
 *     std::runtime_error, DebugMacros.h:17-50 / Utils.cpp:33-37);
 *   - index arrays are int64_t as in the reference (CoalescedBlockMatrix.h:88-110);
 *   - numeric data pointers are DEVICE pointers (Solver.h:184-188: GPU engines expect device
 *     memory); the caller owns them; factor works in place;
 *   - `stream` is a hipStream_t (NULL = default stream);
 *   - one factor()/solve() at a time per solver (Solver is not re-entrant).
 */
#ifndef BASPACHO_AMD_H_
#define BASPACHO_AMD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bsp_solver bsp_solver;

/* Solver.h:189-218  (BackendType, AddFillPolicy, Settings) */
enum { BSP_BACKEND_REF = 0, BSP_BACKEND_FAST = 1, BSP_BACKEND_CUDA = 2, BSP_BACKEND_HIP = 3 };
enum {
  BSP_FILL_COMPLETE = 0,
  BSP_FILL_FOR_AUTO_ELIMS = 1,
  BSP_FILL_FOR_GIVEN_ELIMS = 2,
  BSP_FILL_NONE = 3
};

typedef struct bsp_settings {
  int32_t find_sparse_elimination_ranges; /* default 1 */
  int32_t num_threads;                    /* ignored by the HIP engine */
  int32_t backend;                        /* BSP_BACKEND_HIP (CUDA accepted as alias) */
  int32_t add_fill_policy;                /* BSP_FILL_COMPLETE */
  /* optional cost model of the supernode-merge heuristic (ComputationModel.h:56-109):
     potrf[4], trsm[6], syge[6], asmbl[4]; NULL = built-in MI355X model */
  const double* computation_model;
} bsp_settings;

/* Extension (no counterpart in the reference): the schedule switches of the MI355X backend
   (csrc/backend_options.h).  Every field: a negative value (NaN for the doubles) = the library's
   default; a zeroed struct is NOT "all defaults" -- start from bsp_hip_options_default().  The
   environment variables of the same names (BSP_TAIL_BLOCKS, BSP_SOLVE_SWEEP, ...) still override what
   is passed here: they exist for A/B scripts. */
typedef struct bsp_hip_options {
  int32_t lookahead;         /* 0: lookahead units in line */
  int32_t due_stream;        /* 0: one auxiliary stream */
  int32_t split_k;           /* 0: no split-K tile lists */
  int32_t gather_max_pairs;  /* pairs per sparse-elimination gather item */
  int32_t gather_overlap;    /* ignored (kept for ABI stability) */
  int32_t sub_batch_min;     /* batches of at least this many as concurrent sub-batches; 0: never */
  int32_t sub_batches;       /* ... this many parts */
  int32_t tail_blocks;       /* outer blocks of a wide root lump for the persistent tail launch; 0: off */
  int32_t lazy_plan;         /* 1: no eager device plan when the solver is created */
  int32_t block_solve;       /* 0: wide lumps solved panel by panel */
  int32_t solve_inv;         /* 0: substitution instead of inverted diagonal blocks */
  int32_t solve_sweep;       /* 0: no persistent solve sweeps */
  int32_t sweep_min_width;   /* narrowest run of columns a sweep takes */
  int32_t solve_wide;        /* 0: no right-hand-sides-across-the-lanes backward elimination pass */
  int32_t chain_contraction; /* 0: no contraction of pivot chains before the ordering */
  int32_t dense_merge;       /* 0: no "rows >= 90 % of the parent's column" merge rule */
  int32_t expected_batch;    /* matrices per factor() call the supernode-merge model plans for (default 1) */
  double lookahead_min_gf;   /* GF per fork below which lookahead units stay in line */
  double bulk_ahead;         /* share of the next block's chain handed out as optional lookahead units */
  double level_cost_us;      /* supernode merges: cost of one level on the critical path (default 28 us) */
} bsp_hip_options;
void bsp_hip_options_default(bsp_hip_options* out);

const char* bsp_last_error(void);
const char* bsp_version(void);

/* createSolver(settings, paramSizes, SparseStructure{ptrs,inds}, sparseElimRanges, elimLastIds)
   Solver.h:235-237, Solver.cpp:611-752.  ptrs/inds: block CSR of the LOWER triangle incl.
   diagonal.  Symbolic analysis only: does not touch the GPU. */
int bsp_create_solver(const bsp_settings* settings, int64_t num_params, const int64_t* param_sizes,
                      const int64_t* ptrs, const int64_t* inds, int64_t num_elim_ranges,
                      const int64_t* elim_ranges, int64_t num_elim_last, const int64_t* elim_last,
                      bsp_solver** out);

/* ... the same with the backend's switches (NULL = bsp_create_solver) */
int bsp_create_solver_opts(const bsp_settings* settings, const bsp_hip_options* options,
                           int64_t num_params, const int64_t* param_sizes, const int64_t* ptrs,
                           const int64_t* inds, int64_t num_elim_ranges, const int64_t* elim_ranges,
                           int64_t num_elim_last, const int64_t* elim_last, bsp_solver** out);

/* Solver::Solver(CoalescedBlockMatrixSkel&&, sparseElimRanges, permutation, ops)
   Solver.h:37-38 -- solver from a RAW skeleton, as the reference's tests build it
   (tests/FactorTest.cpp:43-65).  col_ptr/row_ind: per-lump sorted row spans (csc). */
int bsp_create_solver_from_skeleton(int64_t num_spans, const int64_t* span_start,
                                    int64_t num_lumps, const int64_t* lump_to_span,
                                    const int64_t* col_ptr, const int64_t* row_ind,
                                    int64_t num_elim_ranges, const int64_t* elim_ranges,
                                    bsp_solver** out);

void bsp_destroy_solver(bsp_solver* s);

/* Solver::order / dataSize / canFactorUpToSpan, skel().numSpans()/numLumps()  Solver.h:111-131 */
int64_t bsp_order(const bsp_solver* s);
int64_t bsp_data_size(const bsp_solver* s);
int64_t bsp_num_spans(const bsp_solver* s);
int64_t bsp_num_lumps(const bsp_solver* s);
int64_t bsp_can_factor_up_to_span(const bsp_solver* s);
int64_t bsp_span_vector_offset(const bsp_solver* s, int64_t span);
int64_t bsp_span_matrix_offset(const bsp_solver* s, int64_t span, int64_t* out);

/* Skeleton arrays (CoalescedBlockMatrix.h:88-110); pointer stays valid while the solver lives */
enum {
  BSP_SKEL_SPAN_START = 0,
  BSP_SKEL_SPAN_TO_LUMP = 1,
  BSP_SKEL_LUMP_START = 2,
  BSP_SKEL_LUMP_TO_SPAN = 3,
  BSP_SKEL_SPAN_OFFSET_IN_LUMP = 4,
  BSP_SKEL_CHAIN_COL_PTR = 5,
  BSP_SKEL_CHAIN_ROW_SPAN = 6,
  BSP_SKEL_CHAIN_DATA = 7,
  BSP_SKEL_CHAIN_ROWS_TILL_END = 8,
  BSP_SKEL_BOARD_COL_PTR = 9,
  BSP_SKEL_BOARD_ROW_LUMP = 10,
  BSP_SKEL_BOARD_CHAIN_COL_ORD = 11,
  BSP_SKEL_BOARD_ROW_PTR = 12,
  BSP_SKEL_BOARD_COL_LUMP = 13,
  BSP_SKEL_BOARD_COL_ORD = 14,
  BSP_SKEL_PARAM_TO_SPAN = 15,     /* Solver::paramToSpan()            Solver.h:136-137 */
  BSP_SKEL_SPARSE_ELIM_RANGES = 16 /* Solver::sparseEliminationRanges  Solver.h:133-134 */
};
int bsp_skeleton_array(const bsp_solver* s, int which, const int64_t** data, int64_t* len);

/* PermutedCoalescedAccessor::blockOffset / diagBlockOffset  Accessor.h:145-166
   (param indices in USER order; flipped = stored block is the transpose).  Fails when the
   block is not part of the factor structure. */
int bsp_block_offset(const bsp_solver* s, int64_t row_param, int64_t col_param, int64_t* offset,
                     int64_t* stride, int32_t* flipped);
int bsp_diag_block_offset(const bsp_solver* s, int64_t param, int64_t* offset, int64_t* stride);

/* Solver::deviceAccessor()  Solver.h:47-48 / MatOpsCuda.cu:85-92: the 8 device arrays
   (spanStart, spanToLump, lumpStart, spanOffsetInLump, chainColPtr, chainRowSpan, chainData,
   permutation), in that order, for use inside a caller's HIP kernel. */
int bsp_device_accessor(bsp_solver* s, const int64_t* out_device_arrays[8]);

void bsp_set_stream(bsp_solver* s, void* stream);

/* Buffer edges, for every bsp_factor_*, bsp_solve_*, bsp_add_mv_from_*, bsp_pseudo_factor_from_* and
   bsp_selected_inverse_* entry below, as for the gradient entries further down (DESIGN.md section 5,
   "Buffer edges"; tests/test_buffer_edges_gpu.py):
   - the strictly-upper elements of the square diagonal blocks of a matrix operand are ignored on input,
     whatever they hold (NaN and Inf included).  A factor leaves them unspecified; bsp_selected_inverse_*
     writes them (the diagonal blocks of Z are full);
   - an operand declared const (dev_mat of the solves and of addMvFrom, dev_in) is only read;
   - a vector block is read and written on its first `order` rows of each of the nrhs columns only: the
     rows from `order` to `stride` of a column are neither read nor written;
   - nothing outside the dataSize() elements of a matrix operand and the (nrhs - 1) * stride + order
     elements of a vector block is read or written, and a pointer needs the alignment of one element only. */
/* Solver::factor<double|float>  Solver.h:60-61, Solver.cpp:149-151 */
int bsp_factor_f64(bsp_solver* s, double* dev_data);
int bsp_factor_f32(bsp_solver* s, float* dev_data);
/* Solver::factor<std::vector<T*>>  (batched, identical structure)  Solver.cpp:459-460;
   dev_ptrs is a HOST array of `batch` device pointers */
int bsp_factor_batched_f64(bsp_solver* s, double* const* dev_ptrs, int32_t batch);
int bsp_factor_batched_f32(bsp_solver* s, float* const* dev_ptrs, int32_t batch);
/* Solver::factorUpTo / factorFrom  Solver.h:75-76, 96-97 */
int bsp_factor_up_to_f64(bsp_solver* s, double* dev_data, int64_t span_index);
int bsp_factor_from_f64(bsp_solver* s, double* dev_data, int64_t span_index);
int bsp_factor_up_to_f32(bsp_solver* s, float* dev_data, int64_t span_index);
int bsp_factor_from_f32(bsp_solver* s, float* dev_data, int64_t span_index);
/* TESTING: Solver::factor driven op by op through the reference's NumericCtx boundary
   (potrf / trsm / saveSyrkGemm / prepareAssemble / assemble / doElimination, MatOps.h:113-136)
   in the reference's call order (Solver.cpp:164-219) instead of the fused path */
int bsp_factor_per_op_f64(bsp_solver* s, double* dev_data);
int bsp_factor_per_op_f32(bsp_solver* s, float* dev_data);
/* Solver::enableStats + the per-op stat callbacks of the reference (Utils.h:100-119) as bench -Z
   uses them (benchmarking/Bench.cpp:72-124): while on, every potrf / trsm / saveSyrkGemm / assemble
   call of the per-op boundary is timed (HIP events around its launches) and kept as one sample
   {size0, size1, size2, seconds}: which = 0 potrf {n}, 1 trsm {n, k}, 2 syrk/gemm {m, n, k},
   3 assemble {blockRows, blockCols}.  bsp_read_op_stats copies up to `capacity` samples (4 doubles
   each) and reports how many exist.  Input of the cost-model fit (tools/fit_computation_model.py,
   examples/OptimizeCompModel.cpp:64-275 in the reference). */
int bsp_collect_op_stats(bsp_solver* s, int32_t on);
int bsp_read_op_stats(bsp_solver* s, int32_t which, double* out, int64_t capacity, int64_t* count);
/* TESTING: while on, factor / solve* / addMvFrom of this solver are driven op by op through the
   reference's NumericCtx / SolveCtx boundary (MatOps.h:113-184) in the reference's call order
   (Solver.cpp:164-219, 270-397, 400-449) -- sparseElimSolveL/Lt, symm, solveL, gemv, assembleVec,
   solveLt, gemvT, assembleVecT, fragmentedMV/SolveL/SolveLt -- instead of the fused paths */
int bsp_force_per_op(bsp_solver* s, int32_t on);
/* Level table of the full-range factor plan (host only; the level schedule replaces the host-serial
 * per-lump loop of Solver.cpp:198-218): 8 values per level -- {sparse-elimination range or -1, panels,
 * widest panel, most rows below a panel, trsm row tiles, update tiles, lookahead tiles, rows below
 * summed over the panels}.  Returns the number of values (call with out = NULL to size), -1 on error. */
int64_t bsp_plan_levels(bsp_solver* s, int64_t* out, int64_t capacity);
/* TESTING hook of the reference: numCtx->doElimination(solver.internalGetElimCtx(i), ...)
   (Solver.h:139-145, tests/FactorTest.cpp:158-160) */
int bsp_do_elimination_f64(bsp_solver* s, double* dev_data, int64_t elim_range_index);
int bsp_do_elimination_f32(bsp_solver* s, float* dev_data, int64_t elim_range_index);

/* Solver::solve / solveL / solveLt  Solver.h:64-73 (vectors in internal order, column-major
   order x nRHS with leading dimension `stride` >= order; dev_mat is only read, its strictly-upper
   diagonal-block elements are ignored, the rows order .. stride of every column are left alone) */
int bsp_solve_f64(bsp_solver* s, const double* dev_mat, double* dev_vec, int64_t stride,
                  int32_t nrhs);
int bsp_solve_l_f64(bsp_solver* s, const double* dev_mat, double* dev_vec, int64_t stride,
                    int32_t nrhs);
int bsp_solve_lt_f64(bsp_solver* s, const double* dev_mat, double* dev_vec, int64_t stride,
                     int32_t nrhs);
int bsp_solve_f32(bsp_solver* s, const float* dev_mat, float* dev_vec, int64_t stride,
                  int32_t nrhs);
int bsp_solve_l_f32(bsp_solver* s, const float* dev_mat, float* dev_vec, int64_t stride,
                    int32_t nrhs);
int bsp_solve_lt_f32(bsp_solver* s, const float* dev_mat, float* dev_vec, int64_t stride,
                     int32_t nrhs);
/* Solver::solveLUpTo / solveLtUpTo / solveLFrom / solveLtFrom  Solver.h:79-108 (span_index must
   be a lump boundary).  which: 0 = LUpTo, 1 = LtUpTo, 2 = LFrom, 3 = LtFrom */
int bsp_solve_partial_f64(bsp_solver* s, const double* dev_mat, double* dev_vec, int64_t stride,
                          int32_t nrhs, int32_t which, int64_t span_index);
int bsp_solve_partial_f32(bsp_solver* s, const float* dev_mat, float* dev_vec, int64_t stride,
                          int32_t nrhs, int32_t which, int64_t span_index);
/* Solver::addMvFrom  Solver.h:89-91: out += alpha * A * in on the symmetric block from span_index
   (a lump boundary) to the end; vectors hold `order` rows, column-major, nRHS columns */
int bsp_add_mv_from_f64(bsp_solver* s, const double* dev_mat, int64_t span_index,
                        const double* dev_in, int64_t in_stride, double* dev_out,
                        int64_t out_stride, int32_t nrhs, double alpha);
int bsp_add_mv_from_f32(bsp_solver* s, const float* dev_mat, int64_t span_index, const float* dev_in,
                        int64_t in_stride, float* dev_out, int64_t out_stride, int32_t nrhs,
                        float alpha);
/* Solver::pseudoFactorFrom  Solver.h:92-94: Cholesky of the diagonal block of every span from
   span_index on, the rows below it divided by the factor (any span width, MatOpsCuda.cu:188-233) */
int bsp_pseudo_factor_from_f64(bsp_solver* s, double* dev_data, int64_t span_index);
int bsp_pseudo_factor_from_f32(bsp_solver* s, float* dev_data, int64_t span_index);
/* Extension (no counterpart in the reference): selected inversion, the marginal covariances of a
   least-squares problem.  Precondition: dev_data holds a complete factor() of this solver (a solver
   that can only factor up to a span, AddFillForGivenElims, is refused).  In place, Z = A^-1
   restricted to the block pattern of L overwrites L in the factor's layout: every lump's diagonal
   block is written full and symmetric (both triangles), every off-diagonal block keeps its stored
   orientation, so bsp_diag_block_offset / bsp_block_offset (and its `flipped` flag) read Z as they
   read L.  Entries of A^-1 outside the pattern are not computed here (bsp_inverse_blocks_* does).
   The strictly-upper elements of L's diagonal blocks are ignored on input (they are overwritten by
   Z).  Runs on the bsp_set_stream stream, no host synchronisation (the first call builds the plan);
   the result is bitwise reproducible.  No GPU or a NULL dev_data: non-zero return, bsp_last_error()
   says why. */
int bsp_selected_inverse_f64(bsp_solver* s, double* dev_data);
int bsp_selected_inverse_f32(bsp_solver* s, float* dev_data);
/* Solver::selectedInverse<std::vector<T*>>: the same for `batch` complete factors of this solver
   (dev_ptrs is a HOST array of distinct device pointers).  Member q is bitwise equal to
   bsp_selected_inverse_* of dev_ptrs[q].  The batch runs in chunks, one after the other on the
   execution stream: each chunk takes one pass over the levels for all its matrices, with scratch
   for each of them.  A chunk holds at most 65535 matrices and what half the free device memory
   holds in scratch (at least one); the grown scratch stays with the solver until it is destroyed.
   A batch <= 0, a NULL dev_ptrs, a NULL member or two equal members: non-zero return before any
   device work, bsp_last_error() says why. */
int bsp_selected_inverse_batched_f64(bsp_solver* s, double* const* dev_ptrs, int32_t batch);
int bsp_selected_inverse_batched_f32(bsp_solver* s, float* const* dev_ptrs, int32_t batch);
/* Extension (no counterpart in the reference): blocks of A^-1 anywhere, on or off the pattern of L, by
   reach solves.  (A^-1)_ij = (L^-1 e_i) . (L^-1 e_j), and L^-1 e_i is nonzero only
   on the lumps reachable from i's lump through the rows of L: a forward solve visits those alone.
   dev_l holds a complete factor() of this solver and is only read; params are the CALLER's param ids in
   a HOST array (repeats allowed).  Both run on the bsp_set_stream stream and are bitwise reproducible.
   They do not synchronise with the host, with two exceptions, both at the beginning of a call, before
   it queues anything: a call whose work tables (reach lists, groups, Gram row ranges) are larger than
   those of any earlier call on this solver waits for the device and allocates its staging slots anew
   (32 pinned host slots and 32 device slots of the largest tables seen stay with the solver), and so
   does a bsp_inverse_blocks_* call that needs a larger workspace than any before.  A solver that
   cannot factor completely (AddFillForGivenElims), a NULL pointer or an id out of range: non-zero
   return before any device work.
   bsp_reach_solve_l_*: dev_w = L^-1 E, E the unit columns of the params stacked in the order given, m
   columns in all: m x bsp_order values, column-major with leading dimension bsp_order, rows in
   internal order, every element written.
   bsp_inverse_blocks_*: block k = A^-1[row_params[k], col_params[k]], row-major at dev_out +
   out_offsets[k] (HOST array of num_pairs + 1 ascending offsets; block k must fit before
   out_offsets[k + 1]).  L^-1 E of the distinct params goes to a workspace kept with the solver
   (distinct columns x bsp_order values; growing it waits for the device). */
int bsp_reach_solve_l_f64(bsp_solver* s, const double* dev_l, int64_t num_params, const int64_t* params,
                          double* dev_w);
int bsp_reach_solve_l_f32(bsp_solver* s, const float* dev_l, int64_t num_params, const int64_t* params,
                          float* dev_w);
int bsp_inverse_blocks_f64(bsp_solver* s, const double* dev_l, int64_t num_pairs, const int64_t* row_params,
                           const int64_t* col_params, double* dev_out, const int64_t* out_offsets);
int bsp_inverse_blocks_f32(bsp_solver* s, const float* dev_l, int64_t num_pairs, const int64_t* row_params,
                           const int64_t* col_params, float* dev_out, const int64_t* out_offsets);
/* Extension (no counterpart in the reference): products with the factor.
   dev_out = L dev_in (which = 0) or L^T dev_in (which = 1), L the lower triangle of dev_l: a buffer in
   this solver's numeric layout of which only the stored elements i >= j are read (the strictly-upper
   elements of the diagonal blocks never are); it need not hold a factor.  dev_in and dev_out are
   bsp_order x nrhs, column-major with leading dimensions in_stride and out_stride, in internal order,
   as for bsp_solve_*.  dev_l and dev_in are only read; every element of dev_out is written exactly
   once and none is read (no memset needed; the padding between columns is left alone).  Every sum runs
   in an order fixed by the structure, without atomics: two runs are bitwise equal, column k of a call
   is bitwise the call on that column alone, member q of a batch is bitwise the single call.  Runs on
   the bsp_set_stream stream without host synchronisation; the first call builds and uploads the plan,
   and a y = L^T x call that needs more room for partial sums than any before waits for the device.
   Batched forms: HOST arrays of `batch` device pointers.  Non-zero return before any device work: a
   NULL pointer, an empty batch, which not 0 or 1, nrhs < 1 (or > 65535), a stride below bsp_order, an
   output that overlaps an input (dev_in == dev_out included) or another output. */
int bsp_factor_product_f64(bsp_solver* s, const double* dev_l, int32_t which, const double* dev_in, int64_t in_stride,
                           double* dev_out, int64_t out_stride, int32_t nrhs);
int bsp_factor_product_f32(bsp_solver* s, const float* dev_l, int32_t which, const float* dev_in, int64_t in_stride,
                           float* dev_out, int64_t out_stride, int32_t nrhs);
int bsp_factor_product_batched_f64(bsp_solver* s, const double* const* dev_l, int32_t which,
                                   const double* const* dev_in, int64_t in_stride, double* const* dev_out,
                                   int64_t out_stride, int32_t nrhs, int32_t batch);
int bsp_factor_product_batched_f32(bsp_solver* s, const float* const* dev_l, int32_t which,
                                   const float* const* dev_in, int64_t in_stride, float* const* dev_out,
                                   int64_t out_stride, int32_t nrhs, int32_t batch);
/* Extension (no counterpart in the reference): gradients on the block pattern of L, for autograd
   (DESIGN.md section 13).  Data is this solver's numeric layout and vectors are in its internal order,
   as for bsp_solve_*.  A(d) is the symmetric matrix with A_ij = A_ji = d_e for every stored element
   e = (i, j): all elements of the off-diagonal chain blocks and i >= j inside the diagonal blocks (the
   strictly-upper elements of the diagonal blocks are not read).  All of them run on the bsp_set_stream
   stream without host synchronisation (the first call builds the work lists); results are bitwise
   reproducible and batch member q is bitwise the single call.  A solver that cannot factor completely
   (AddFillForGivenElims), an empty batch, a NULL pointer or nrhs < 1: non-zero return before any
   device work, bsp_last_error() says why.
   bsp_log_det_*: dev_out[0] = log det A = 2 sum_i log L_ii of a complete factor() (accumulated in fp64
   for both types; a non-positive or NaN pivot gives -inf or NaN, it does not fail).  The batched form
   writes dev_out[q] for dev_factors[q] (a HOST array of device pointers), q < batch. */
int bsp_log_det_f64(bsp_solver* s, const double* dev_factor, double* dev_out);
int bsp_log_det_f32(bsp_solver* s, const float* dev_factor, float* dev_out);
int bsp_log_det_batched_f64(bsp_solver* s, const double* const* dev_factors, double* dev_out, int32_t batch);
int bsp_log_det_batched_f32(bsp_solver* s, const float* const* dev_factors, float* dev_out, int32_t batch);
/* Extension (no counterpart in the reference): the status of a factor and damping of the diagonal, on
   the device.  Both walk the stored diagonal elements of the internal scalars of
   the spans [span_begin, span_end), 0 <= span_begin <= span_end <= numSpans.  The range need not sit on
   a lump boundary: [0, numSpans) after factor(), [0, span) after factorUpTo(span), [span, numSpans)
   after factorFrom(span).  They run on the bsp_set_stream stream without host synchronisation (the first
   call uploads the work list).  A NULL pointer, an empty batch or a range outside the spans: non-zero
   return before any device work, bsp_last_error() says why.
   bsp_factor_status_*: a diagonal d is GOOD when d > 0 and d is finite in its type, BAD otherwise (NaN,
   +-Inf, 0, -0, negative).  dev_out holds four 8-byte words per matrix:
     w[0]  the lowest bad internal scalar of the range, -1 when there is none
     w[1]  the number of bad diagonals of the range
     w[2]  the bit pattern of the double minimum over the good diagonals, +inf when there is none
     w[3]  the bit pattern of the double maximum over the good diagonals, 0.0 when there is none
   (float widens exactly; an empty range gives {-1, 0, +inf, 0.0}).  dev_data is only read and nothing but
   dev_out is written; the record is exact and batch member q (dev_out + 4 q, dev_data a HOST array of
   device pointers) is bitwise the single call.  The contract of w[0]:
     1. it is the lowest internal scalar whose stored diagonal is not finite and positive;
     2. the columns that precede k in the internal order do not depend on A_kk;
     3. so after a factor() whose first failing pivot is column k, w[0] = k.
   The scan only reads diagonals, so on an UNFACTORED matrix it gives the range of diag(A), and a
   necessary condition: a matrix with a bad diagonal cannot factor. */
int bsp_factor_status_f64(bsp_solver* s, const double* dev_data, int64_t span_begin, int64_t span_end,
                          int64_t* dev_out);
int bsp_factor_status_f32(bsp_solver* s, const float* dev_data, int64_t span_begin, int64_t span_end,
                          int64_t* dev_out);
int bsp_factor_status_batched_f64(bsp_solver* s, const double* const* dev_data, int64_t span_begin,
                                  int64_t span_end, int64_t* dev_out, int32_t batch);
int bsp_factor_status_batched_f32(bsp_solver* s, const float* const* dev_data, int64_t span_begin,
                                  int64_t span_end, int64_t* dev_out, int32_t batch);
/* bsp_damp_*: d <- (d * (1 + alpha)) + beta on those diagonals, in place, with three roundings in the
   data's type (t = 1 + alpha; d = d * t; d = d + beta; no fused multiply-add): bitwise the numpy statement
   on scalars of that type.  alpha = dev_alpha_beta[0] and beta = dev_alpha_beta[1] are DEVICE values,
   so a loop can chain calls without synchronising; no other element of the buffer is touched.  The
   batched form takes dev_alpha_beta[2 q], dev_alpha_beta[2 q + 1] for member q; members whose buffers
   overlap are refused. */
int bsp_damp_f64(bsp_solver* s, double* dev_data, int64_t span_begin, int64_t span_end,
                 const double* dev_alpha_beta);
int bsp_damp_f32(bsp_solver* s, float* dev_data, int64_t span_begin, int64_t span_end,
                 const float* dev_alpha_beta);
int bsp_damp_batched_f64(bsp_solver* s, double* const* dev_data, int64_t span_begin, int64_t span_end,
                         const double* dev_alpha_beta, int32_t batch);
int bsp_damp_batched_f32(bsp_solver* s, float* const* dev_data, int64_t span_begin, int64_t span_end,
                         const float* dev_alpha_beta, int32_t batch);
/* bsp_pattern_grad_*: a write-only pass (dev_out is never read) over every stored element e = (i, j):
     i > j:  out_e = s 2 Z_e + alpha sum_k (U_ik V_jk + V_ik U_jk)
     i = j:  out_e = s Z_e   + alpha sum_k U_ik V_ik
     strictly-upper elements of the diagonal blocks:  out_e = 0
   with s = dev_z_scale[0], a DEVICE value.  dev_z NULL: no Z term (dev_z_scale unused); dev_u and
   dev_v NULL together: no rank-2k term (nrhs unused), else U, V are order x nrhs column-major with
   leading dimension `stride` (>= order) and nrhs >= 1.  One of the two terms must be given.  Solve's
   backward: U = A^-1 g_x, V = x, alpha = -1; logdet's backward: Z = bsp_selected_inverse_* of the
   factor, s = the incoming gradient.  The batched form takes HOST arrays of `batch` device pointers
   (dev_z / dev_u / dev_v may be NULL as above) and dev_z_scale[q] for member q. */
int bsp_pattern_grad_f64(bsp_solver* s, const double* dev_z, const double* dev_z_scale, const double* dev_u,
                         const double* dev_v, int64_t stride, int32_t nrhs, double alpha, double* dev_out);
int bsp_pattern_grad_f32(bsp_solver* s, const float* dev_z, const float* dev_z_scale, const float* dev_u,
                         const float* dev_v, int64_t stride, int32_t nrhs, float alpha, float* dev_out);
int bsp_pattern_grad_batched_f64(bsp_solver* s, const double* const* dev_z, const double* dev_z_scale,
                                 const double* const* dev_u, const double* const* dev_v, int64_t stride,
                                 int32_t nrhs, double alpha, double* const* dev_out, int32_t batch);
int bsp_pattern_grad_batched_f32(bsp_solver* s, const float* const* dev_z, const float* dev_z_scale,
                                 const float* const* dev_u, const float* const* dev_v, int64_t stride,
                                 int32_t nrhs, float alpha, float* const* dev_out, int32_t batch);
/* bsp_pattern_outer_*: the non-symmetric rank-k projection (write-only, dev_out is never read):
     i >= j: out_e = alpha sum_k U_ik V_jk
     strictly-upper elements of the diagonal blocks:  out_e = 0
   U, V order x nrhs column-major with leading dimension `stride` (>= order), nrhs >= 1, both required.
   The backward of y = L^-1 b is Lbar = -(L^-T g_y) y^T (U = L^-T g_y, V = y, alpha = -1); that of
   x = L^-T b is Lbar = -x (L^-1 g_x)^T (U = x, V = L^-1 g_x, alpha = -1).  An
   output buffer that overlaps another member's output or any U / V: non-zero return before any
   device work.  The batched form takes HOST arrays of `batch` device pointers. */
int bsp_pattern_outer_f64(bsp_solver* s, const double* dev_u, const double* dev_v, int64_t stride, int32_t nrhs,
                          double alpha, double* dev_out);
int bsp_pattern_outer_f32(bsp_solver* s, const float* dev_u, const float* dev_v, int64_t stride, int32_t nrhs,
                          float alpha, float* dev_out);
int bsp_pattern_outer_batched_f64(bsp_solver* s, const double* const* dev_u, const double* const* dev_v,
                                  int64_t stride, int32_t nrhs, double alpha, double* const* dev_out, int32_t batch);
int bsp_pattern_outer_batched_f32(bsp_solver* s, const float* const* dev_u, const float* const* dev_v,
                                  int64_t stride, int32_t nrhs, float alpha, float* const* dev_out, int32_t batch);
/* bsp_factor_adjoint_*: the reverse-mode sweep of bsp_factor_* (DESIGN.md section 15).  dev_l holds a
   complete factor() of A(d) and is only read.  dev_grad holds Lbar = df/dL on entry, for every stored
   element with i >= j (the strictly-upper elements of the diagonal blocks are ignored), and df/dd on
   return in bsp_pattern_grad_*'s convention: G_ij + G_ji for i > j, G_ii for i = j, 0 on the
   strictly-upper elements, for the dense symmetric gradient G = df/dA.  The cost is about that of
   bsp_selected_inverse_*, whose plan and scratch it shares.  The batched form takes HOST arrays of
   `batch` device pointers, runs in chunks as bsp_selected_inverse_batched_* does, and member q is
   bitwise the single call.  dev_grad == dev_l, gradient buffers that overlap each other or any factor,
   a NULL pointer, batch <= 0 or a solver that cannot factor completely: non-zero return before any
   device work. */
int bsp_factor_adjoint_f64(bsp_solver* s, const double* dev_l, double* dev_grad);
int bsp_factor_adjoint_f32(bsp_solver* s, const float* dev_l, float* dev_grad);
int bsp_factor_adjoint_batched_f64(bsp_solver* s, const double* const* dev_l, double* const* dev_grad,
                                   int32_t batch);
int bsp_factor_adjoint_batched_f32(bsp_solver* s, const float* const* dev_l, float* const* dev_grad,
                                   int32_t batch);
/* bsp_selected_inverse_adjoint_*: the reverse mode of bsp_selected_inverse_* (DESIGN.md section 19).  dev_l
   holds a complete factor(), dev_z what bsp_selected_inverse_* wrote over a copy of it; both are only
   read.  dev_grad holds df/d(slot) on entry for EVERY slot of the layout as bsp_selected_inverse_* writes
   it -- the strictly-upper elements of the diagonal blocks hold Z_ji and are slots of their own -- and
   Lbar = df/dL on return: the stored elements with i >= j, exactly 0 on the strictly-upper elements.
   That is the input of bsp_factor_adjoint_*; the two in a row give the projection of -Z S Z in
   bsp_pattern_grad_*'s convention, S the symmetrised slot weights (S_ij = S_ji = half the sum of dev_grad
   over the slots holding Z_ij or Z_ji, S_ii the diagonal slot).  Plan, scratch and chunks of
   bsp_selected_inverse_*; the cost is one to two times its cost.  The sweep adds into shared slots with
   native float atomics: results are close, NOT bitwise, from run to run, and a batch member is close
   to, not bitwise, the single call.  The batched form takes HOST arrays of `batch` device pointers.
   dev_grad overlapping a dev_l, a dev_z or another member's dev_grad, a NULL pointer, batch <= 0 or a
   solver that cannot factor completely: non-zero return before any device work. */
int bsp_selected_inverse_adjoint_f64(bsp_solver* s, const double* dev_l, const double* dev_z, double* dev_grad);
int bsp_selected_inverse_adjoint_f32(bsp_solver* s, const float* dev_l, const float* dev_z, float* dev_grad);
int bsp_selected_inverse_adjoint_batched_f64(bsp_solver* s, const double* const* dev_l, const double* const* dev_z,
                                             double* const* dev_grad, int32_t batch);
int bsp_selected_inverse_adjoint_batched_f32(bsp_solver* s, const float* const* dev_l, const float* const* dev_z,
                                             float* const* dev_grad, int32_t batch);
/* bsp_factor_adjoint_up_to_*: the reverse-mode sweep of bsp_factor_up_to_* (DESIGN.md section 16).  dev_p
   holds factorUpTo(span) of A(d) -- the factor L11, L21 on the columns before the cut and the Schur
   complement S = A22 - A21 A11^-1 A12 behind it -- and is only read.  dev_grad holds df/dP_e on entry
   for every stored element with i >= j (Lbar before the cut, Sbar behind it; the strictly-upper
   elements of the diagonal blocks are ignored) and df/dd on return, in bsp_pattern_grad_*'s
   convention.  Only the lumps before the cut are swept (a plan of their own, cached per cut; the
   scratch is shared with bsp_selected_inverse_*).  span == bsp_num_spans is bsp_factor_adjoint_*, bit
   for bit; span == 0 returns the input with the strictly-upper elements zeroed.  Batched form as
   bsp_factor_adjoint_batched_*.  Non-zero return before any device work, buffers untouched: a span that
   bsp_factor_up_to_* refuses (inside a lump, cutting a sparse-elimination range, out of range),
   dev_grad == dev_p or overlapping buffers, a NULL pointer, batch <= 0, a solver that cannot factor
   completely. */
int bsp_factor_adjoint_up_to_f64(bsp_solver* s, const double* dev_p, double* dev_grad, int64_t span);
int bsp_factor_adjoint_up_to_f32(bsp_solver* s, const float* dev_p, float* dev_grad, int64_t span);
int bsp_factor_adjoint_up_to_batched_f64(bsp_solver* s, const double* const* dev_p, double* const* dev_grad,
                                         int32_t batch, int64_t span);
int bsp_factor_adjoint_up_to_batched_f32(bsp_solver* s, const float* const* dev_p, float* const* dev_grad,
                                         int32_t batch, int64_t span);
/* bsp_schur_to_dense_*: the trailing block of a layout buffer (rows and columns from `span` on; m = order
   - first scalar of span) as a dense symmetric m x m matrix, row-major: dev_out[dest[i] * m + dest[j]] for
   trailing scalars i, j counted from the cut; zero where the pattern has no block.  All m * m elements
   are written, none is read.  dev_dest: DEVICE int32[m], a permutation of 0 .. m-1, or NULL (identity).
   bsp_schur_from_dense_*: its adjoint in bsp_pattern_grad_*'s convention.  EVERY element of dev_grad
   (data size) is written: g[i, j] + g[j, i] below the diagonal of the trailing block, g[i, i] on it, 0 on
   the strictly-upper elements and on every column before the cut; dev_grad_dense need not be symmetric.
   Span checks and batched forms (HOST arrays of `batch` device pointers, one dev_dest for all) as
   bsp_factor_adjoint_up_to_*; span == bsp_num_spans (m = 0) is refused. */
int bsp_schur_to_dense_f64(bsp_solver* s, const double* dev_p, int64_t span, double* dev_out, const int32_t* dev_dest);
int bsp_schur_to_dense_f32(bsp_solver* s, const float* dev_p, int64_t span, float* dev_out, const int32_t* dev_dest);
int bsp_schur_to_dense_batched_f64(bsp_solver* s, const double* const* dev_p, int64_t span, double* const* dev_out,
                                   const int32_t* dev_dest, int32_t batch);
int bsp_schur_to_dense_batched_f32(bsp_solver* s, const float* const* dev_p, int64_t span, float* const* dev_out,
                                   const int32_t* dev_dest, int32_t batch);
int bsp_schur_from_dense_f64(bsp_solver* s, const double* dev_grad_dense, int64_t span, double* dev_grad,
                             const int32_t* dev_dest);
int bsp_schur_from_dense_f32(bsp_solver* s, const float* dev_grad_dense, int64_t span, float* dev_grad,
                             const int32_t* dev_dest);
int bsp_schur_from_dense_batched_f64(bsp_solver* s, const double* const* dev_grad_dense, int64_t span,
                                     double* const* dev_grad, const int32_t* dev_dest, int32_t batch);
int bsp_schur_from_dense_batched_f32(bsp_solver* s, const float* const* dev_grad_dense, int64_t span,
                                     float* const* dev_grad, const int32_t* dev_dest, int32_t batch);
/* Extension (no counterpart in the reference): assembly of a symmetric matrix given as coordinate
   entries (rows[k], cols[k], values[k]) in the caller's scalar order into this solver's layout, and its
   adjoint.
   - Scalar index i belongs to param p at local position r, from the prefix sums of the param sizes in
     param order.  Indices are int64 in [0, order); 0 <= nnz < 2^31 (nnz = 0: a zero matrix).
   - triangle BSP_TRIANGLE_LOWER: every entry must have row >= col.  BSP_TRIANGLE_FULL: entries with
     row < col are skipped (never read, gradient 0); the caller asserts the matrix is symmetric.  In
     both modes A_ij = A_ji = sum of the values of the entries at (i, j), i >= j.
   - Every kept entry must land on a stored element of the factor (an original block or fill-in): the
     stored lower element, through the permuted block's `flipped` flag (bsp_block_offset) and
     (r, c) -> (c, r) inside a diagonal block.  Anything else makes bsp_assembly_create fail;
     bsp_last_error() names the first offending entry index and its (row, col).
   bsp_assembly_create builds the map once on the host (no device work); the first assemble or adjoint
   call uploads it, and it stays on the device until bsp_assembly_destroy.  An assembly belongs to the
   solver it was built on and must be destroyed before that solver. */
#define BSP_TRIANGLE_LOWER 0
#define BSP_TRIANGLE_FULL 1
typedef struct bsp_assembly bsp_assembly;
int bsp_assembly_create(bsp_solver* s, int64_t nnz, const int64_t* rows, const int64_t* cols, int32_t triangle,
                        bsp_assembly** out);
void bsp_assembly_destroy(bsp_assembly* a);
/* host copy of the map: out[k] = layout offset of entry k, -1 for a skipped entry (nnz values) */
int bsp_assembly_entry_offsets(const bsp_assembly* a, int64_t* out);
/* figures of the map: out[0] nnz, [1] kept entries, [2] distinct elements written by entries, [3] most
   entries summed into one element, [4] elements summed by a whole wave (runs > 64), [5] tiles of the
   assemble kernel, [6] device bytes of the map once uploaded */
int bsp_assembly_info(const bsp_assembly* a, int64_t out[7]);
/* bsp_assemble_*: writes EVERY element of dev_data (its previous contents never matter): the sum of the
   values of the entries mapped to it, in ascending entry index in the value type starting from +0
   (bitwise np.add.at(zeros(dataSize), offsets, values)), and 0 where no entry maps (fill-in, the
   strictly-upper elements of the diagonal blocks).  bsp_assemble_adjoint_*: dev_grad_values[k] =
   dev_grad_data[offset[k]], 0 for skipped entries; with section 13's convention for the gradient of the
   data this is the exact gradient of the entry values, the same for every duplicate.  Both run on the
   bsp_set_stream stream without host synchronisation, with no atomics; results are bitwise
   reproducible and batch member q (HOST arrays of `batch` device pointers) is bitwise the single call.
   An empty batch, a NULL array or member (the nnz-sized side may be NULL when nnz = 0), a repeated
   output pointer or an assembly built on another solver: non-zero return before any device work. */
int bsp_assemble_f64(bsp_solver* s, const bsp_assembly* a, const double* dev_values, double* dev_data);
int bsp_assemble_f32(bsp_solver* s, const bsp_assembly* a, const float* dev_values, float* dev_data);
int bsp_assemble_batched_f64(bsp_solver* s, const bsp_assembly* a, const double* const* dev_values,
                             double* const* dev_data, int32_t batch);
int bsp_assemble_batched_f32(bsp_solver* s, const bsp_assembly* a, const float* const* dev_values,
                             float* const* dev_data, int32_t batch);
int bsp_assemble_adjoint_f64(bsp_solver* s, const bsp_assembly* a, const double* dev_grad_data,
                             double* dev_grad_values);
int bsp_assemble_adjoint_f32(bsp_solver* s, const bsp_assembly* a, const float* dev_grad_data,
                             float* dev_grad_values);
int bsp_assemble_adjoint_batched_f64(bsp_solver* s, const bsp_assembly* a, const double* const* dev_grad_data,
                                     double* const* dev_grad_values, int32_t batch);
int bsp_assemble_adjoint_batched_f32(bsp_solver* s, const bsp_assembly* a, const float* const* dev_grad_data,
                                     float* const* dev_grad_values, int32_t batch);
/* Extension (no counterpart in the reference): the normal equations of a sparse Jacobian J, m x order(),
   given as entries (rows[k], cols[k], values[k]) in the caller's scalar order.
   - No (row, col) may repeat; empty rows and columns are fine; nnz, m and the pair count P = sum over
     rows of d (d + 1) / 2 (d: entries of the row) must be in [0, 2^31).
   - Every unordered pair of entries of one row, self-pairs included, is a pair (ka, kb) with cols[ka] >=
     cols[kb]; it adds values[ka] * values[kb] to the stored lower element of (cols[ka], cols[kb]), found
     as the assembly finds it.  That element must be stored by the solver.
   bsp_normal_eq_create builds the map once on the host (no device work) and fails, with bsp_last_error()
   naming the first offending entry and its (row, col), on an index out of range, a repeated position
   or a pair outside the stored pattern, and stating P when P >= 2^31.  The map has three parts, each
   uploaded by the first call that needs it (forward: hessian; adjoint: hessian_adjoint; vector lists:
   jt_vec / j_vec) and kept until bsp_normal_eq_destroy.  A map belongs to the solver it was built on and
   must be destroyed before that solver. */
typedef struct bsp_normal_eq bsp_normal_eq;
int bsp_normal_eq_create(bsp_solver* s, int64_t m, int64_t nnz, const int64_t* rows, const int64_t* cols,
                         bsp_normal_eq** out);
void bsp_normal_eq_destroy(bsp_normal_eq* e);
/* figures of the map: out[0] nnz, [1] pairs P, [2] distinct elements written by pairs, [3] most pairs summed
   into one element, [4] elements summed by a whole wave (runs > 64), [5] tiles of the hessian kernel,
   [6] / [7] / [8] device bytes of the forward / adjoint / vector parts once uploaded, [9] adjoint terms (2 P) */
int bsp_normal_eq_info(const bsp_normal_eq* e, int64_t out[10]);
/* host copy of the forward map in run order (P values each): pair x is (ka[x], kb[x]) and lands on
   layout offset offset[x]; ascending offset, ascending ka inside one offset */
int bsp_normal_eq_pair_table(const bsp_normal_eq* e, int32_t* ka, int32_t* kb, int64_t* offset);
/* bsp_normal_eq_hessian_*: writes EVERY element of dev_data (its previous contents never matter): the sum of
   the products of its pairs in ascending ka, each product rounded in the value type, added one by one from
   +0 (bitwise np.add.at(zeros(dataSize), offset, values[ka] * values[kb])), 0 where no pair lands.
   bsp_normal_eq_hessian_adjoint_*: dev_grad_values[k] = sum of dev_grad_data[offset of the pair] *
   dev_values[partner] over the pairs that hold k, in ascending partner index, the self-pair twice; with
   section 13's convention for the gradient of the data this is the exact gradient of the entry values.
   bsp_normal_eq_jt_vec_*: dev_out[c, j] = sum over the entries of column c, ascending k, of values[k] *
   dev_r[rows[k], j]  (dev_r [m, q], dev_out [order, q], row-major, q >= 1 vectors).
   bsp_normal_eq_j_vec_*: dev_out[i, j] = sum over the entries of row i, ascending k, of values[k] *
   dev_v[cols[k], j]  (dev_v [order, q], dev_out [m, q]).
   All run on the stream of bsp_set_stream without atomics or host synchronisation; results are bitwise
   reproducible and batch member b (HOST arrays of `batch` device pointers) is bitwise the single call.
   An empty batch, a NULL array or member (a side of size 0 may be NULL), a repeated output pointer, an
   output that aliases an input, or a map built on another solver: non-zero return before any device work. */
int bsp_normal_eq_hessian_f64(bsp_solver* s, const bsp_normal_eq* e, const double* dev_values, double* dev_data);
int bsp_normal_eq_hessian_batched_f64(bsp_solver* s, const bsp_normal_eq* e, const double* const* dev_values,
                                      double* const* dev_data, int32_t batch);
int bsp_normal_eq_hessian_adjoint_f64(bsp_solver* s, const bsp_normal_eq* e, const double* dev_values,
                                      const double* dev_grad_data, double* dev_grad_values);
int bsp_normal_eq_hessian_adjoint_batched_f64(bsp_solver* s, const bsp_normal_eq* e, const double* const* dev_values,
                                              const double* const* dev_grad_data, double* const* dev_grad_values,
                                              int32_t batch);
int bsp_normal_eq_jt_vec_f64(bsp_solver* s, const bsp_normal_eq* e, const double* dev_values, const double* dev_r,
                             int64_t q, double* dev_out);
int bsp_normal_eq_jt_vec_batched_f64(bsp_solver* s, const bsp_normal_eq* e, const double* const* dev_values,
                                     const double* const* dev_r, int64_t q, double* const* dev_out, int32_t batch);
int bsp_normal_eq_j_vec_f64(bsp_solver* s, const bsp_normal_eq* e, const double* dev_values, const double* dev_v,
                            int64_t q, double* dev_out);
int bsp_normal_eq_j_vec_batched_f64(bsp_solver* s, const bsp_normal_eq* e, const double* const* dev_values,
                                    const double* const* dev_v, int64_t q, double* const* dev_out, int32_t batch);
int bsp_normal_eq_hessian_f32(bsp_solver* s, const bsp_normal_eq* e, const float* dev_values, float* dev_data);
int bsp_normal_eq_hessian_batched_f32(bsp_solver* s, const bsp_normal_eq* e, const float* const* dev_values,
                                      float* const* dev_data, int32_t batch);
int bsp_normal_eq_hessian_adjoint_f32(bsp_solver* s, const bsp_normal_eq* e, const float* dev_values,
                                      const float* dev_grad_data, float* dev_grad_values);
int bsp_normal_eq_hessian_adjoint_batched_f32(bsp_solver* s, const bsp_normal_eq* e, const float* const* dev_values,
                                              const float* const* dev_grad_data, float* const* dev_grad_values,
                                              int32_t batch);
int bsp_normal_eq_jt_vec_f32(bsp_solver* s, const bsp_normal_eq* e, const float* dev_values, const float* dev_r,
                             int64_t q, float* dev_out);
int bsp_normal_eq_jt_vec_batched_f32(bsp_solver* s, const bsp_normal_eq* e, const float* const* dev_values,
                                     const float* const* dev_r, int64_t q, float* const* dev_out, int32_t batch);
int bsp_normal_eq_j_vec_f32(bsp_solver* s, const bsp_normal_eq* e, const float* dev_values, const float* dev_v,
                            int64_t q, float* dev_out);
int bsp_normal_eq_j_vec_batched_f32(bsp_solver* s, const bsp_normal_eq* e, const float* const* dev_values,
                                    const float* const* dev_v, int64_t q, float* const* dev_out, int32_t batch);
/* Extension (no counterpart in the reference): products with the symmetric matrix A given as coordinate
   entries (rows[k], cols[k], values[k]) in the caller's scalar order, taken straight from the entries:
   the solver's layout is never built.
   - `triangle` and the index rules are those of bsp_assembly_create: an index outside [0, order) is
     refused, BSP_TRIANGLE_LOWER refuses row < col and BSP_TRIANGLE_FULL skips it, so A is the matrix the
     assembly builds: A_ij = A_ji = sum of the values of the kept entries at (i, j), i >= j.  Whether the
     solver stores the element does not matter here.
   - The term list of scalar i holds, in ascending k, (k, cols[k]) for every kept entry with rows[k] == i
     and (k, rows[k]) for every kept entry with cols[k] == i and rows[k] != i; duplicates stay separate
     terms.  0 <= nnz < 2^31 and the term count must be below 2^31.
   bsp_sym_product_create builds the map once on the host (no device work) and fails, with
   bsp_last_error() naming the first offending entry and its (row, col), or stating the term count when it
   is too large.  The map has two parts, each uploaded by the first call that needs it (row lists: mv;
   entry lists: outer) and kept until bsp_sym_product_destroy.  A map belongs to the solver it was built
   on and must be destroyed before that solver. */
typedef struct bsp_sym_product bsp_sym_product;
int bsp_sym_product_create(bsp_solver* s, int64_t nnz, const int64_t* rows, const int64_t* cols, int32_t triangle,
                           bsp_sym_product** out);
void bsp_sym_product_destroy(bsp_sym_product* p);
/* figures of the map: out[0] nnz, [1] kept entries, [2] terms, [3] most terms in one row, [4] rows summed by
   a whole wave (more than 64 terms), [5] device bytes of both parts once uploaded */
int bsp_sym_product_info(const bsp_sym_product* p, int64_t out[6]);
/* host copy of the term lists: the terms of row i are (entry[t], index[t]), t in [row_start[i],
   row_start[i + 1]) (order + 1 starts; out[2] values in entry and in index) */
int bsp_sym_product_row_table(const bsp_sym_product* p, int32_t* row_start, int32_t* entry, int32_t* index);
/* bsp_sym_product_mv_*: dev_out = A dev_x, both [order, q] row-major, q >= 1 vectors.  dev_out[i, j] = the
   terms (k, idx) of row i folded in list order from +0: s = s + dev_values[k] * dev_x[idx, j], the product
   rounded in the value type before it is added.  EVERY element of dev_out is written exactly once (+0 for
   a row without terms); dev_out is never read.
   bsp_sym_product_outer_*: dev_grad_values[k] = sum over j ascending of t_j, t_j = dev_g[r, j] * dev_x[c, j]
   (+ dev_g[c, j] * dev_x[r, j] when r != c), (r, c) = (rows[k], cols[k]); 0 for a skipped entry.  This is
   the gradient of the entry values of sum(dev_g * (A dev_x)), the same for every duplicate (the convention
   of bsp_assemble_adjoint_*).  dev_g and dev_x are [order, q].
   All run on the stream of bsp_set_stream without atomics, memsets or host synchronisation; results are
   bitwise reproducible and batch member b (HOST arrays of `batch` device pointers) is bitwise the single
   call.  Operands need the alignment of their element type only.  An empty batch, a NULL array or member (a
   side of size 0 may be NULL), q < 1, a repeated output pointer, an output that aliases an input, or a map
   built on another solver: non-zero return before any device work. */
int bsp_sym_product_mv_f64(bsp_solver* s, const bsp_sym_product* p, const double* dev_values, const double* dev_x,
                           int64_t q, double* dev_out);
int bsp_sym_product_mv_batched_f64(bsp_solver* s, const bsp_sym_product* p, const double* const* dev_values,
                                   const double* const* dev_x, int64_t q, double* const* dev_out, int32_t batch);
int bsp_sym_product_outer_f64(bsp_solver* s, const bsp_sym_product* p, const double* dev_g, const double* dev_x,
                              int64_t q, double* dev_grad_values);
int bsp_sym_product_outer_batched_f64(bsp_solver* s, const bsp_sym_product* p, const double* const* dev_g,
                                      const double* const* dev_x, int64_t q, double* const* dev_grad_values,
                                      int32_t batch);
int bsp_sym_product_mv_f32(bsp_solver* s, const bsp_sym_product* p, const float* dev_values, const float* dev_x,
                           int64_t q, float* dev_out);
int bsp_sym_product_mv_batched_f32(bsp_solver* s, const bsp_sym_product* p, const float* const* dev_values,
                                   const float* const* dev_x, int64_t q, float* const* dev_out, int32_t batch);
int bsp_sym_product_outer_f32(bsp_solver* s, const bsp_sym_product* p, const float* dev_g, const float* dev_x,
                              int64_t q, float* dev_grad_values);
int bsp_sym_product_outer_batched_f32(bsp_solver* s, const bsp_sym_product* p, const float* const* dev_g,
                                      const float* const* dev_x, int64_t q, float* const* dev_grad_values,
                                      int32_t batch);
/* EXTENSIONS without a counterpart in the reference: error bounds on the device.
   All run on the stream of bsp_set_stream without atomics or memsets, and without host synchronisation after
   the first call of a size (the map's upload, the partials of bsp_max_ratio_* / bsp_col_max_*); member b of a
   batched call is bitwise the single call.  Refused before any device work, non-zero return: a NULL
   solver, map, array or member (a side of size 0 may be NULL), an empty batch, q < 1, a repeated output
   pointer, an output that aliases an input or another output, a map built on another solver.

   bsp_sym_product_residual_*: over the row lists of bsp_sym_product_mv_*, in ONE pass with two
   accumulators: dev_r[i, j] = dev_b[i, j] + (-s), s the terms dev_values[k] * dev_x[idx, j] of row i folded
   in list order from +0 (bitwise dev_b - mv); dev_d[i, j] = |dev_b[i, j]| + t, t the terms |dev_values[k]| *
   |dev_x[idx, j]| folded the same way: (|A| |x| + |b|)_i, the Oettli-Prager denominator, duplicates as
   separate terms.  Every product is rounded before it is added.  dev_x, dev_b, dev_r, dev_d are [order, q]
   row-major; every element of dev_r and dev_d is written exactly once, neither is read.
   bsp_sym_product_abs_mv_*: dev_out = |A| |dev_x| alone, the same kernel without dev_b. */
int bsp_sym_product_residual_f64(bsp_solver* s, const bsp_sym_product* p, const double* dev_values,
                                 const double* dev_x, const double* dev_b, int64_t q, double* dev_r, double* dev_d);
int bsp_sym_product_residual_batched_f64(bsp_solver* s, const bsp_sym_product* p, const double* const* dev_values,
                                         const double* const* dev_x, const double* const* dev_b, int64_t q,
                                         double* const* dev_r, double* const* dev_d, int32_t batch);
int bsp_sym_product_abs_mv_f64(bsp_solver* s, const bsp_sym_product* p, const double* dev_values, const double* dev_x,
                               int64_t q, double* dev_out);
int bsp_sym_product_abs_mv_batched_f64(bsp_solver* s, const bsp_sym_product* p, const double* const* dev_values,
                                       const double* const* dev_x, int64_t q, double* const* dev_out, int32_t batch);
int bsp_sym_product_residual_f32(bsp_solver* s, const bsp_sym_product* p, const float* dev_values, const float* dev_x,
                                 const float* dev_b, int64_t q, float* dev_r, float* dev_d);
int bsp_sym_product_residual_batched_f32(bsp_solver* s, const bsp_sym_product* p, const float* const* dev_values,
                                         const float* const* dev_x, const float* const* dev_b, int64_t q,
                                         float* const* dev_r, float* const* dev_d, int32_t batch);
int bsp_sym_product_abs_mv_f32(bsp_solver* s, const bsp_sym_product* p, const float* dev_values, const float* dev_x,
                               int64_t q, float* dev_out);
int bsp_sym_product_abs_mv_batched_f32(bsp_solver* s, const bsp_sym_product* p, const float* const* dev_values,
                                       const float* const* dev_x, int64_t q, float* const* dev_out, int32_t batch);
/* bsp_max_ratio_*: dev_out[j] (double, [q]; [batch, q] batched) = max over i < n of ratio(|dev_r[i, j]|,
   dev_d[i, j]) computed in double for both precisions: 0 when r == 0, +inf when d == 0 and r != 0, the
   quotient otherwise; a NaN in either operand (or inf / inf) makes the column's result NaN; 0 for n == 0.
   bsp_col_max_*: dev_out[j] = max over i < n of dev_a[i, j] as a double, NaN if any is; -inf for n == 0.
   Arrays are [n, q] row-major and only read.  Two passes (partials per workgroup kept with the solver, then
   one workgroup per result); max does not depend on the order, so results are bitwise the numpy
   statement.  The partials take 16 bytes per 1024 rows, column and member of a chunk; a call that needs more
   of them than any call before on this solver allocates them, which WAITS FOR THE DEVICE (and cannot be part
   of a stream capture); every later call of that size or below runs without host synchronisation. */
int bsp_max_ratio_f64(bsp_solver* s, const double* dev_r, const double* dev_d, int64_t n, int64_t q, double* dev_out);
int bsp_max_ratio_batched_f64(bsp_solver* s, const double* const* dev_r, const double* const* dev_d, int64_t n,
                              int64_t q, double* dev_out, int32_t batch);
int bsp_col_max_f64(bsp_solver* s, const double* dev_a, int64_t n, int64_t q, double* dev_out);
int bsp_col_max_batched_f64(bsp_solver* s, const double* const* dev_a, int64_t n, int64_t q, double* dev_out,
                            int32_t batch);
int bsp_max_ratio_f32(bsp_solver* s, const float* dev_r, const float* dev_d, int64_t n, int64_t q, double* dev_out);
int bsp_max_ratio_batched_f32(bsp_solver* s, const float* const* dev_r, const float* const* dev_d, int64_t n,
                              int64_t q, double* dev_out, int32_t batch);
int bsp_col_max_f32(bsp_solver* s, const float* dev_a, int64_t n, int64_t q, double* dev_out);
int bsp_col_max_batched_f32(bsp_solver* s, const float* const* dev_a, int64_t n, int64_t q, double* dev_out,
                            int32_t batch);
/* bsp_inv_norm1_*: dev_out[m] (double) = an estimate of ||A^-1||_1 for the matrix whose complete bsp_factor is
   dev_L (a lower bound, almost always within a factor 3); with dev_D (order values in internal order per
   member; NULL: none) of ||D A^-1 D||_1.  Hager's estimator in Higham's form on a fixed schedule of 10
   bsp_solve calls with one right-hand side; nothing is read back.  dev_state receives 12 8-byte words per
   matrix: [0] bits of the estimate (double), [1] the last j, [2] vectors measured (1 .. 5), [3] stop reason
   (0 none, 1 order 1, 2 repeated sign vector, 3 no increase, 4 pass limit, 5 same column again, 6 a
   non-finite vector), [4] 1 when the alternating vector's value won, [5 .. 9] the j chosen after pass
   1 .. 5 (-1: none), [10] bits of the alternating vector's value, [11] 0.
   WORKSPACE, LAPACK style: dev_work is the caller's, 16-byte aligned, bsp_inv_norm1_work_bytes_* bytes per
   member (two vectors of order values, rounded up to 16 bytes, plus 16 bytes per 1024 scalars of the order,
   at least 16), members one after the other.  Nothing is allocated inside the call.  Also refused: a solver
   that can only factor up to a span, order 0, a workspace that is NULL, misaligned or aliases an operand. */
int bsp_inv_norm1_work_bytes_f64(const bsp_solver* s, int64_t* out);
int bsp_inv_norm1_work_bytes_f32(const bsp_solver* s, int64_t* out);
int bsp_inv_norm1_f64(bsp_solver* s, const double* dev_L, const double* dev_D, void* dev_work, int64_t* dev_state,
                      double* dev_out);
int bsp_inv_norm1_batched_f64(bsp_solver* s, const double* const* dev_L, const double* const* dev_D, void* dev_work,
                              int64_t* dev_state, double* dev_out, int32_t batch);
int bsp_inv_norm1_f32(bsp_solver* s, const float* dev_L, const float* dev_D, void* dev_work, int64_t* dev_state,
                      double* dev_out);
int bsp_inv_norm1_batched_f32(bsp_solver* s, const float* const* dev_L, const float* const* dev_D, void* dev_work,
                              int64_t* dev_state, double* dev_out, int32_t batch);
/* EXTENSION without a counterpart in the reference's library (its examples/PCG.cpp is caller-side): the
   pieces of a preconditioned conjugate gradient whose scalars stay on the device.
   One problem per (matrix, right-hand side): vectors are [n, q] row-major, dev_state holds
   bsp_cg_state_words = 12 8-byte words per problem, problem j of member m at (m q + j) 12: [0] iterations,
   [1] stop reason (0 running, 1 converged: rr <= tol^2 bb, 2 step limit, 3 breakdown: p.Ap or r.z not > 0,
   4 a non-finite sum, 5 zero right-hand side), then the doubles [2] rz, [3] pAp, [4] rr, [5] bb = b.b,
   [6] alpha, [7] beta, [8] tol^2, then [9] the step limit, [10], [11] 0.  Every piece reads its scalars from
   the records and leaves x, r, p, z and the record of a stopped problem bitwise unchanged; nothing is read
   back by the library, so the caller may queue any number of iterations and look at the stop words when it
   likes.  One iteration is: Ap = A p (the caller's: bsp_sym_product_mv_* or any operator); alpha; update;
   precond; direction (with plain = 1, no preconditioner: alpha; update; direction with dev_z = dev_r).
     init:       dev_x holds the start, dev_r = b - A x for it (both the caller's): the records are reset,
                 bb and rr taken, the problems of a zero b cleared (x = r = 0).  Then precond and direction
                 (plain: direction alone) give the first p.
     alpha:      pAp = p.Ap, alpha = rz / pAp
     update:     x += alpha p, r -= alpha Ap and rr = r.r of the new r in one pass; the iteration is counted
                 and the stop test made
     precond:    kind 0: dev_z is the caller's M^-1 r and only read; kind 1 (Jacobi) and 2 (block-Jacobi over
                 the solver's params, at most 32 scalars each): dev_z = M^-1 dev_r from dev_minv, which
                 bsp_cg_precond_build_* wrote.  With rz = r.z of the same pass: beta = rz / rz(old)
     direction:  p = z + beta p
     precond_build: dev_minv (bsp_cg_precond_info's third figure elements per member) from the entry values:
                 the diagonal blocks summed in ascending entry index, factored and inverted in double, stored
                 in the data type.  dev_status receives 2 words per member: the caller's scalar of the lowest
                 bad pivot (not positive and finite) or -1, and the number of bad blocks; a bad block's
                 inverse is the zero matrix.
   Dot products are taken in double for both precisions, in the two-pass order of bsp_max_ratio_* with every
   product rounded before it is added; the vector updates round every product in the data type.  No
   atomics; member b of a batched call is bitwise the single call.  WORKSPACE: dev_work is the caller's,
   16-byte aligned, bsp_cg_work_bytes bytes per member (16 bytes per 1024 rows and right-hand side, at least
   16 per right-hand side, plus 4 bytes per row rounded up to 16), members one after the other; nothing is
   allocated inside a call (the first use of a built-in preconditioner uploads its tables).  Refused before any
   device work: NULL arguments, an empty batch, n or q out of range, a misaligned workspace, a map of another
   solver or order, and a written operand that overlaps any other operand, workspace and records included.
   bsp_cg_precond_info: out = {blocks, items, elements of the inverse, widest block};
   bsp_cg_precond_table: the plan's tables (host only): block_start [blocks + 1], item_start [blocks + 1],
   and per item its entry and its position (i - s) w + (j - s) inside its block.
   KIND 3, THE FACTORISED SPARSE APPROXIMATE INVERSE: M^-1 = G^T G, G lower triangular
   on the pattern of the lower triangle of A, at most 32 scalars per row (the row's own and the 31 largest
   before it); every row comes from its own dense system A[S_i, S_i], so nothing depends on anything else.
     bsp_cg_precond_info(p, 3, out): out = {rows, items, elements of G, widest row};
     bsp_cg_precond_build_*(.., 3, ..): dev_minv receives the values of G (out[2] elements per member); a row
                 whose local Cholesky meets a pivot that is not positive and finite is written as zeros, and
                 dev_status = {the lowest caller's scalar of such a pivot or -1, the number of such rows};
     bsp_fsai_apply_*: takes precond's place in the iteration: dev_t = G dev_r (dev_t is the caller's
                 scratch, [n, q]), dev_z = G^T dev_t, rz and beta.  Sums in double, every product rounded, row
                 and column terms in ascending scalar order; bsp_cg_precond_* refuses kind 3 and names this entry;
     bsp_fsai_table: the plan's tables (host only): row_start [n + 1] and cols [elements of G]; item_start
                 [n + 1] and per item its entry and its position la w + lb in the row's local matrix;
                 col_start [n + 1] and per column term its position in G and its row; long_cols, the columns of
                 more than 64 terms, ascending (room for n of them; their number is what col_start says);
     bsp_fsai_check_sizes: the plan's size check alone: refuses an element or item count outside [0, 2^31)
                 and states it. */
int bsp_cg_state_words(int64_t* out);
int bsp_cg_work_bytes(const bsp_solver* s, int64_t n, int64_t q, int64_t* out);
int bsp_cg_precond_info(const bsp_sym_product* p, int32_t kind, int64_t out[4]);
int bsp_cg_precond_table(const bsp_sym_product* p, int32_t kind, int32_t* block_start, int32_t* item_start,
                         int32_t* entry, int32_t* pos);
int bsp_fsai_table(const bsp_sym_product* p, int32_t* row_start, int32_t* cols, int32_t* item_start, int32_t* entry,
                      int32_t* pos, int32_t* col_start, int32_t* col_pos, int32_t* col_row, int32_t* long_cols);
int bsp_fsai_check_sizes(int64_t elems, int64_t items);
int bsp_fsai_apply_f64(bsp_solver* s, const bsp_sym_product* p, int64_t n, int64_t q, const double* dev_g,
                          const double* dev_r, double* dev_t, double* dev_z, void* dev_work, int64_t* dev_state);
int bsp_fsai_apply_batched_f64(bsp_solver* s, const bsp_sym_product* p, int64_t n, int64_t q,
                                  const double* const* dev_g, const double* const* dev_r, double* const* dev_t,
                                  double* const* dev_z, void* dev_work, int64_t* dev_state, int32_t batch);
int bsp_fsai_apply_f32(bsp_solver* s, const bsp_sym_product* p, int64_t n, int64_t q, const float* dev_g,
                          const float* dev_r, float* dev_t, float* dev_z, void* dev_work, int64_t* dev_state);
int bsp_fsai_apply_batched_f32(bsp_solver* s, const bsp_sym_product* p, int64_t n, int64_t q,
                                  const float* const* dev_g, const float* const* dev_r, float* const* dev_t,
                                  float* const* dev_z, void* dev_work, int64_t* dev_state, int32_t batch);
int bsp_cg_init_f64(bsp_solver* s, int64_t n, int64_t q, const double* dev_b, double* dev_x, double* dev_r, double tol,
                    int64_t max_steps, int32_t plain, void* dev_work, int64_t* dev_state);
int bsp_cg_init_batched_f64(bsp_solver* s, int64_t n, int64_t q, const double* const* dev_b, double* const* dev_x,
                            double* const* dev_r, double tol, int64_t max_steps, int32_t plain, void* dev_work,
                            int64_t* dev_state, int32_t batch);
int bsp_cg_alpha_f64(bsp_solver* s, int64_t n, int64_t q, const double* dev_p, const double* dev_ap, void* dev_work,
                     int64_t* dev_state);
int bsp_cg_alpha_batched_f64(bsp_solver* s, int64_t n, int64_t q, const double* const* dev_p,
                             const double* const* dev_ap, void* dev_work, int64_t* dev_state, int32_t batch);
int bsp_cg_update_f64(bsp_solver* s, int64_t n, int64_t q, const double* dev_p, const double* dev_ap, double* dev_x,
                      double* dev_r, int32_t plain, void* dev_work, int64_t* dev_state);
int bsp_cg_update_batched_f64(bsp_solver* s, int64_t n, int64_t q, const double* const* dev_p,
                              const double* const* dev_ap, double* const* dev_x, double* const* dev_r, int32_t plain,
                              void* dev_work, int64_t* dev_state, int32_t batch);
int bsp_cg_precond_f64(bsp_solver* s, const bsp_sym_product* p, int32_t kind, int64_t n, int64_t q,
                       const double* dev_minv, const double* dev_r, double* dev_z, void* dev_work, int64_t* dev_state);
int bsp_cg_precond_batched_f64(bsp_solver* s, const bsp_sym_product* p, int32_t kind, int64_t n, int64_t q,
                               const double* const* dev_minv, const double* const* dev_r, double* const* dev_z,
                               void* dev_work, int64_t* dev_state, int32_t batch);
int bsp_cg_direction_f64(bsp_solver* s, int64_t n, int64_t q, const double* dev_z, double* dev_p, int32_t plain,
                         void* dev_work, int64_t* dev_state);
int bsp_cg_direction_batched_f64(bsp_solver* s, int64_t n, int64_t q, const double* const* dev_z, double* const* dev_p,
                                 int32_t plain, void* dev_work, int64_t* dev_state, int32_t batch);
int bsp_cg_precond_build_f64(bsp_solver* s, const bsp_sym_product* p, int32_t kind, const double* dev_values,
                             double* dev_minv, void* dev_work, int64_t* dev_status);
int bsp_cg_precond_build_batched_f64(bsp_solver* s, const bsp_sym_product* p, int32_t kind,
                                     const double* const* dev_values, double* const* dev_minv, void* dev_work,
                                     int64_t* dev_status, int32_t batch);
int bsp_cg_init_f32(bsp_solver* s, int64_t n, int64_t q, const float* dev_b, float* dev_x, float* dev_r, double tol,
                    int64_t max_steps, int32_t plain, void* dev_work, int64_t* dev_state);
int bsp_cg_init_batched_f32(bsp_solver* s, int64_t n, int64_t q, const float* const* dev_b, float* const* dev_x,
                            float* const* dev_r, double tol, int64_t max_steps, int32_t plain, void* dev_work,
                            int64_t* dev_state, int32_t batch);
int bsp_cg_alpha_f32(bsp_solver* s, int64_t n, int64_t q, const float* dev_p, const float* dev_ap, void* dev_work,
                     int64_t* dev_state);
int bsp_cg_alpha_batched_f32(bsp_solver* s, int64_t n, int64_t q, const float* const* dev_p,
                             const float* const* dev_ap, void* dev_work, int64_t* dev_state, int32_t batch);
int bsp_cg_update_f32(bsp_solver* s, int64_t n, int64_t q, const float* dev_p, const float* dev_ap, float* dev_x,
                      float* dev_r, int32_t plain, void* dev_work, int64_t* dev_state);
int bsp_cg_update_batched_f32(bsp_solver* s, int64_t n, int64_t q, const float* const* dev_p,
                              const float* const* dev_ap, float* const* dev_x, float* const* dev_r, int32_t plain,
                              void* dev_work, int64_t* dev_state, int32_t batch);
int bsp_cg_precond_f32(bsp_solver* s, const bsp_sym_product* p, int32_t kind, int64_t n, int64_t q,
                       const float* dev_minv, const float* dev_r, float* dev_z, void* dev_work, int64_t* dev_state);
int bsp_cg_precond_batched_f32(bsp_solver* s, const bsp_sym_product* p, int32_t kind, int64_t n, int64_t q,
                               const float* const* dev_minv, const float* const* dev_r, float* const* dev_z,
                               void* dev_work, int64_t* dev_state, int32_t batch);
int bsp_cg_direction_f32(bsp_solver* s, int64_t n, int64_t q, const float* dev_z, float* dev_p, int32_t plain,
                         void* dev_work, int64_t* dev_state);
int bsp_cg_direction_batched_f32(bsp_solver* s, int64_t n, int64_t q, const float* const* dev_z, float* const* dev_p,
                                 int32_t plain, void* dev_work, int64_t* dev_state, int32_t batch);
int bsp_cg_precond_build_f32(bsp_solver* s, const bsp_sym_product* p, int32_t kind, const float* dev_values,
                             float* dev_minv, void* dev_work, int64_t* dev_status);
int bsp_cg_precond_build_batched_f32(bsp_solver* s, const bsp_sym_product* p, int32_t kind,
                                     const float* const* dev_values, float* const* dev_minv, void* dev_work,
                                     int64_t* dev_status, int32_t batch);
/* EXTENSION without a counterpart in the reference: matrix-free least squares from the entries of a sparse
   Jacobian J, m x order(), given as (rows[k], cols[k], values[k]) in the caller's scalar order (DESIGN.md
   section 28): products with J and J^T, and the pieces of CGLS for (J^T J + D) x = J^T r + c, D = diag(d),
   d_i = alpha colsq_i + beta, colsq_i the squared norm of column i.  No layout, no pair list, no factor.
   bsp_jac_product_create builds the map once on the host (no device work): the entries of every row and of
   every column in ascending k, each with the list of its runs of more than 64 terms, which a whole wave sums
   in the same sequential order.  The solver gives the order, the stream and the params; its layout is never
   touched.  It fails, with bsp_last_error() naming the first offending entry and its (row, col), on an index
   out of range or a repeated position; nnz and m must be in [0, 2^31).  Nothing of the size of the pair count
   of bsp_normal_eq_create is built.  Each part (rows, columns, blocks) is uploaded by the first call that
   needs it and kept until bsp_jac_product_destroy; the map must be destroyed before its solver.
   bsp_jac_product_info: out[0] nnz, [1] m, [2] n, [3] / [4] the longest row and the rows of more than 64
   entries, [5] / [6] the same for columns, [7] / [8] device bytes of the row and of the column lists.
   bsp_cgls_precond_info: kind 1 (Jacobi) or 2 (block-Jacobi over the solver's params; one wider than 32
   scalars is refused by name, and so is an item count outside [0, 2^31), stated, before anything of that
   size is allocated -- bsp_jac_product_check_items is that check alone): out = {blocks, items, elements of the
   inverse, widest block, device bytes of the plan}.  The items of a block are the pairs (ka, kb) of entries of
   one Jacobian row with both columns in the block, cols[ka] >= cols[kb], self-pairs included, at position
   (cols[ka] - s) w + (cols[kb] - s); they come in ascending Jacobian row.
   bsp_jac_product_table: host copies for tests.  part 0 (rows) and 1 (columns): t0 = start [runs + 1], t1 =
   entry, t2 = the gathered index [nnz each], t3 = the long runs, t4 unused; part 2 (blocks): t0 = block_start,
   t1 = item_start [blocks + 1 each], t2 = ka, t3 = kb, t4 = position [items each].
   PRODUCTS.  jv: dev_out[i, j] = sum over the entries of row i, ascending k, of values[k] * dev_v[cols[k], j];
   jtv: dev_out[c, j] = sum over the entries of column c of values[k] * dev_u[rows[k], j]; every product
   rounded in the value type and added one by one from +0: bitwise bsp_normal_eq_j_vec_* / _jt_vec_*.
     residual: dev_res = dev_r - J dev_x, the subtraction by the thread that holds the sum (dev_r NULL: -J x);
     normal:   dev_out = (J^T dev_res - dev_d * dev_x) + dev_c in this order; dev_d (with dev_x) and dev_c may
               each be NULL, and an absent operand's step is omitted, not added as a zero.
     Both take dev_state (NULL: every column; else the columns of stopped problems are skipped).
   THE ITERATION.  The state record, its stop codes and the frozen-column rule are those of the bsp_cg_* pieces,
   with rz = s.z, pAp = delta = |J p|^2 + p^T D p, rr = s.s and bb = |J^T r + c|^2; the direction is
   bsp_cg_direction_*.  x, p, s, z are [n, q], res and t [m, q], d [n], colsq [n] doubles.
     colsq:   the fold over the column's entries, ascending k from +0, of double(v) * double(v)
     damp:    d_i = T(alpha * colsq_i + beta), in double
     init:    dev_b = J^T r + c (the caller's, by normal): the records reset, bb, x = 0 and stop 5 for a zero b
     delta:   the partials of t.t over the chunks of m, then (dev_d given) those of (p_i * p_i) * d_i over the
              chunks of n, folded as ONE list; not finite stops with 4, not > 0 with 3; alpha = rz / delta
     update:  x += alpha p and res -= alpha t in one launch
     apply:   kind 0: dev_z is the caller's M^-1 s and only read (s itself without a preconditioner); kinds 1,
              2: dev_z = M^-1 dev_s from dev_minv.  The same pass takes s.s and s.z; one fold counts the
              iteration (not with start = 1), tests s.s (non-finite: 4; <= tol^2 bb: 1; step limit: 2), then
              gamma = s.z (non-finite: 4; not > 0: 3) and sets beta = gamma / gamma(old)
     precond_build: kind 1: inv_i = T(1 / (colsq_i + double(d_i))) (dev_values may be NULL); kind 2: the block's
              items summed in ascending Jacobian row in double, double(d) added to the diagonal last, then
              bsp_cg_precond_build_*'s factorisation and inverse (dev_colsq may be NULL).  dev_d NULL: no
              damping.  dev_status as for bsp_cg_precond_build_*.
   One iteration is: t = J p (jv); delta; update; s (normal); apply; direction.
     iterate: that whole iteration in ONE call, queued on dev_p, dev_t, dev_x, dev_res, dev_s, dev_z (with
              dev_values, dev_d, dev_c, dev_minv as above).  The fold of delta rides in the update's launch (every
              workgroup folds the column's partials in the fold's order and takes the same decision), so it is 7
              launches for the pieces' 8, with the same sums in the same order: the same bits as the six calls.
              phase 0: all of it (kind 0 with dev_z == dev_s: no preconditioner); phase 1: up to and including s,
              for a caller that then writes its own z = M^-1 s; phase 2: apply and direction alone.
   Sums in double in the two-pass
   order of the bsp_cg_* pieces; no atomics, no memset; member b of a batched call is bitwise the single call.
   WORKSPACE: the caller's, 16-byte aligned, bsp_cgls_work_bytes bytes per member.  Refused before any device
   work: NULL arguments that the piece needs, an empty batch, q out of range, a misaligned workspace, a map of
   another solver.  A written operand of a piece must not overlap another operand of it (with kind 0, dev_z may be
   dev_s: it is only read); overlaps are the caller's to avoid and are not checked.
   bsp_jac_product_check_items exists for the tests alone: it is the item-count check of the block plan, which no
   test can reach through a map of 2^31 items. */
typedef struct bsp_jac_product bsp_jac_product;
int bsp_jac_product_create(bsp_solver* s, int64_t m, int64_t nnz, const int64_t* rows, const int64_t* cols,
                           bsp_jac_product** out);
void bsp_jac_product_destroy(bsp_jac_product* p);
int bsp_jac_product_info(const bsp_jac_product* p, int64_t out[9]);
int bsp_jac_product_check_items(int64_t items);
int bsp_jac_product_table(const bsp_jac_product* p, int32_t part, int32_t* t0, int32_t* t1, int32_t* t2, int32_t* t3,
                          int32_t* t4);
int bsp_cgls_precond_info(const bsp_jac_product* p, int32_t kind, int64_t out[5]);
int bsp_cgls_work_bytes(const bsp_solver* s, const bsp_jac_product* p, int64_t q, int64_t* out);
int bsp_jac_product_jv_f64(bsp_solver* s, const bsp_jac_product* p, const double* dev_values, const double* dev_v, int64_t q,
                           double* dev_out);
int bsp_jac_product_jv_batched_f64(bsp_solver* s, const bsp_jac_product* p, const double* const* dev_values,
                                   const double* const* dev_v, int64_t q, double* const* dev_out, int32_t batch);
int bsp_jac_product_jtv_f64(bsp_solver* s, const bsp_jac_product* p, const double* dev_values, const double* dev_u, int64_t q,
                            double* dev_out);
int bsp_jac_product_jtv_batched_f64(bsp_solver* s, const bsp_jac_product* p, const double* const* dev_values,
                                    const double* const* dev_u, int64_t q, double* const* dev_out, int32_t batch);
int bsp_cgls_residual_f64(bsp_solver* s, const bsp_jac_product* p, const double* dev_values, const double* dev_x, const double* dev_r,
                          int64_t q, double* dev_res, int64_t* dev_state);
int bsp_cgls_residual_batched_f64(bsp_solver* s, const bsp_jac_product* p, const double* const* dev_values,
                                  const double* const* dev_x, const double* const* dev_r, int64_t q, double* const* dev_res,
                                  int64_t* dev_state, int32_t batch);
int bsp_cgls_normal_f64(bsp_solver* s, const bsp_jac_product* p, const double* dev_values, const double* dev_res, const double* dev_d,
                        const double* dev_x, const double* dev_c, int64_t q, double* dev_out, int64_t* dev_state);
int bsp_cgls_normal_batched_f64(bsp_solver* s, const bsp_jac_product* p, const double* const* dev_values,
                                const double* const* dev_res, const double* const* dev_d, const double* const* dev_x,
                                const double* const* dev_c, int64_t q, double* const* dev_out, int64_t* dev_state, int32_t batch);
int bsp_cgls_colsq_f64(bsp_solver* s, const bsp_jac_product* p, const double* dev_values, double* dev_colsq);
int bsp_cgls_colsq_batched_f64(bsp_solver* s, const bsp_jac_product* p, const double* const* dev_values,
                               double* const* dev_colsq, int32_t batch);
int bsp_cgls_damp_f64(bsp_solver* s, const bsp_jac_product* p, const double* dev_colsq, double alpha, double beta,
                      double* dev_d);
int bsp_cgls_damp_batched_f64(bsp_solver* s, const bsp_jac_product* p, const double* const* dev_colsq, double alpha,
                              double beta, double* const* dev_d, int32_t batch);
int bsp_cgls_init_f64(bsp_solver* s, const bsp_jac_product* p, int64_t q, const double* dev_b, double* dev_x, double tol,
                      int64_t max_steps, void* dev_work, int64_t* dev_state);
int bsp_cgls_init_batched_f64(bsp_solver* s, const bsp_jac_product* p, int64_t q, const double* const* dev_b,
                              double* const* dev_x, double tol, int64_t max_steps, void* dev_work, int64_t* dev_state,
                              int32_t batch);
int bsp_cgls_delta_f64(bsp_solver* s, const bsp_jac_product* p, int64_t q, const double* dev_t, const double* dev_p,
                       const double* dev_d, void* dev_work, int64_t* dev_state);
int bsp_cgls_delta_batched_f64(bsp_solver* s, const bsp_jac_product* p, int64_t q, const double* const* dev_t,
                               const double* const* dev_p, const double* const* dev_d, void* dev_work, int64_t* dev_state,
                               int32_t batch);
int bsp_cgls_update_f64(bsp_solver* s, const bsp_jac_product* p, int64_t q, const double* dev_p, const double* dev_t, double* dev_x,
                        double* dev_res, int64_t* dev_state);
int bsp_cgls_update_batched_f64(bsp_solver* s, const bsp_jac_product* p, int64_t q, const double* const* dev_p,
                                const double* const* dev_t, double* const* dev_x, double* const* dev_res, int64_t* dev_state,
                                int32_t batch);
int bsp_cgls_apply_f64(bsp_solver* s, const bsp_jac_product* p, int32_t kind, int64_t q, const double* dev_minv,
                       const double* dev_s, double* dev_z, int32_t start, void* dev_work, int64_t* dev_state);
int bsp_cgls_apply_batched_f64(bsp_solver* s, const bsp_jac_product* p, int32_t kind, int64_t q,
                               const double* const* dev_minv, const double* const* dev_s, double* const* dev_z, int32_t start,
                               void* dev_work, int64_t* dev_state, int32_t batch);
int bsp_cgls_iterate_f64(bsp_solver* s, const bsp_jac_product* p, int32_t kind, int32_t phase, int64_t q,
                         const double* dev_values, const double* dev_d, const double* dev_c, const double* dev_minv, double* dev_p, double* dev_t,
                         double* dev_x, double* dev_res, double* dev_s, double* dev_z, void* dev_work, int64_t* dev_state);
int bsp_cgls_iterate_batched_f64(bsp_solver* s, const bsp_jac_product* p, int32_t kind, int32_t phase, int64_t q,
                                 const double* const* dev_values, const double* const* dev_d, const double* const* dev_c,
                                 const double* const* dev_minv, double* const* dev_p, double* const* dev_t, double* const* dev_x,
                                 double* const* dev_res, double* const* dev_s, double* const* dev_z, void* dev_work,
                                 int64_t* dev_state, int32_t batch);
int bsp_cgls_precond_build_f64(bsp_solver* s, const bsp_jac_product* p, int32_t kind, const double* dev_values,
                               const double* dev_colsq, const double* dev_d, double* dev_minv, void* dev_work,
                               int64_t* dev_status);
int bsp_cgls_precond_build_batched_f64(bsp_solver* s, const bsp_jac_product* p, int32_t kind,
                                       const double* const* dev_values, const double* const* dev_colsq,
                                       const double* const* dev_d, double* const* dev_minv, void* dev_work, int64_t* dev_status,
                                       int32_t batch);
int bsp_jac_product_jv_f32(bsp_solver* s, const bsp_jac_product* p, const float* dev_values, const float* dev_v, int64_t q,
                           float* dev_out);
int bsp_jac_product_jv_batched_f32(bsp_solver* s, const bsp_jac_product* p, const float* const* dev_values,
                                   const float* const* dev_v, int64_t q, float* const* dev_out, int32_t batch);
int bsp_jac_product_jtv_f32(bsp_solver* s, const bsp_jac_product* p, const float* dev_values, const float* dev_u, int64_t q,
                            float* dev_out);
int bsp_jac_product_jtv_batched_f32(bsp_solver* s, const bsp_jac_product* p, const float* const* dev_values,
                                    const float* const* dev_u, int64_t q, float* const* dev_out, int32_t batch);
int bsp_cgls_residual_f32(bsp_solver* s, const bsp_jac_product* p, const float* dev_values, const float* dev_x, const float* dev_r,
                          int64_t q, float* dev_res, int64_t* dev_state);
int bsp_cgls_residual_batched_f32(bsp_solver* s, const bsp_jac_product* p, const float* const* dev_values,
                                  const float* const* dev_x, const float* const* dev_r, int64_t q, float* const* dev_res,
                                  int64_t* dev_state, int32_t batch);
int bsp_cgls_normal_f32(bsp_solver* s, const bsp_jac_product* p, const float* dev_values, const float* dev_res, const float* dev_d,
                        const float* dev_x, const float* dev_c, int64_t q, float* dev_out, int64_t* dev_state);
int bsp_cgls_normal_batched_f32(bsp_solver* s, const bsp_jac_product* p, const float* const* dev_values,
                                const float* const* dev_res, const float* const* dev_d, const float* const* dev_x,
                                const float* const* dev_c, int64_t q, float* const* dev_out, int64_t* dev_state, int32_t batch);
int bsp_cgls_colsq_f32(bsp_solver* s, const bsp_jac_product* p, const float* dev_values, double* dev_colsq);
int bsp_cgls_colsq_batched_f32(bsp_solver* s, const bsp_jac_product* p, const float* const* dev_values,
                               double* const* dev_colsq, int32_t batch);
int bsp_cgls_damp_f32(bsp_solver* s, const bsp_jac_product* p, const double* dev_colsq, double alpha, double beta,
                      float* dev_d);
int bsp_cgls_damp_batched_f32(bsp_solver* s, const bsp_jac_product* p, const double* const* dev_colsq, double alpha,
                              double beta, float* const* dev_d, int32_t batch);
int bsp_cgls_init_f32(bsp_solver* s, const bsp_jac_product* p, int64_t q, const float* dev_b, float* dev_x, double tol,
                      int64_t max_steps, void* dev_work, int64_t* dev_state);
int bsp_cgls_init_batched_f32(bsp_solver* s, const bsp_jac_product* p, int64_t q, const float* const* dev_b,
                              float* const* dev_x, double tol, int64_t max_steps, void* dev_work, int64_t* dev_state,
                              int32_t batch);
int bsp_cgls_delta_f32(bsp_solver* s, const bsp_jac_product* p, int64_t q, const float* dev_t, const float* dev_p,
                       const float* dev_d, void* dev_work, int64_t* dev_state);
int bsp_cgls_delta_batched_f32(bsp_solver* s, const bsp_jac_product* p, int64_t q, const float* const* dev_t,
                               const float* const* dev_p, const float* const* dev_d, void* dev_work, int64_t* dev_state,
                               int32_t batch);
int bsp_cgls_update_f32(bsp_solver* s, const bsp_jac_product* p, int64_t q, const float* dev_p, const float* dev_t, float* dev_x,
                        float* dev_res, int64_t* dev_state);
int bsp_cgls_update_batched_f32(bsp_solver* s, const bsp_jac_product* p, int64_t q, const float* const* dev_p,
                                const float* const* dev_t, float* const* dev_x, float* const* dev_res, int64_t* dev_state,
                                int32_t batch);
int bsp_cgls_apply_f32(bsp_solver* s, const bsp_jac_product* p, int32_t kind, int64_t q, const float* dev_minv,
                       const float* dev_s, float* dev_z, int32_t start, void* dev_work, int64_t* dev_state);
int bsp_cgls_apply_batched_f32(bsp_solver* s, const bsp_jac_product* p, int32_t kind, int64_t q,
                               const float* const* dev_minv, const float* const* dev_s, float* const* dev_z, int32_t start,
                               void* dev_work, int64_t* dev_state, int32_t batch);
int bsp_cgls_iterate_f32(bsp_solver* s, const bsp_jac_product* p, int32_t kind, int32_t phase, int64_t q,
                         const float* dev_values, const float* dev_d, const float* dev_c, const float* dev_minv, float* dev_p, float* dev_t,
                         float* dev_x, float* dev_res, float* dev_s, float* dev_z, void* dev_work, int64_t* dev_state);
int bsp_cgls_iterate_batched_f32(bsp_solver* s, const bsp_jac_product* p, int32_t kind, int32_t phase, int64_t q,
                                 const float* const* dev_values, const float* const* dev_d, const float* const* dev_c,
                                 const float* const* dev_minv, float* const* dev_p, float* const* dev_t, float* const* dev_x,
                                 float* const* dev_res, float* const* dev_s, float* const* dev_z, void* dev_work,
                                 int64_t* dev_state, int32_t batch);
int bsp_cgls_precond_build_f32(bsp_solver* s, const bsp_jac_product* p, int32_t kind, const float* dev_values,
                               const double* dev_colsq, const float* dev_d, float* dev_minv, void* dev_work,
                               int64_t* dev_status);
int bsp_cgls_precond_build_batched_f32(bsp_solver* s, const bsp_jac_product* p, int32_t kind,
                                       const float* const* dev_values, const double* const* dev_colsq,
                                       const float* const* dev_d, float* const* dev_minv, void* dev_work, int64_t* dev_status,
                                       int32_t batch);
/* EXTENSION without a counterpart in the reference's library as a device entry (the method is the implicit
   Schur complement of Ceres' ITERATIVE_SCHUR; Agarwal, Snavely, Seitz, Szeliski, "Bundle adjustment in the
   large", ECCV 2010): implicit Schur elimination for the matrix-free least squares.  The
   params of the solver are split into eliminated and kept ones; no Jacobian row may touch two eliminated params,
   and an eliminated param has at most 8 scalars.  With N = J^T J + D = [B F; F^T C] in that split, the reduced
   matrix is S = C - F^T B^-1 F; only the inverses of the diagonal blocks of B (binv) and products with vectors
   are formed.  bsp_jac_schur_create builds the host map over a bsp_jac_product, which must outlive it
   (eliminate: param indices in any order, taken in ascending order); it refuses an empty list, an index out of
   range or given twice, an eliminated param wider than 8 scalars, nothing kept, and a row with entries in two
   eliminated params.  The kept scalars are numbered 0 .. nK - 1 and the eliminated ones 0 .. nE - 1 in ascending
   caller's scalar.
     info:   {nnz, m, n, nK, nE, eliminated params, rows of no group, widest eliminated param, most rows in a
             group, kept entries, eliminated entries, long runs of the four lists (rows kept, rows eliminated,
             columns eliminated, columns kept), items of the blocks of B, elements of binv, device bytes of the
             map, device bytes of the block plan, rows in groups}
     table:  part 0 .. 3: (start, entry, index, long runs) of the kept entries by row, the eliminated entries by
             row, the eliminated scalars' entries and the kept columns' entries; 4: (kept scalar, eliminated
             scalar, first eliminated scalar of each eliminated param, its param index); 5: (group start, group
             rows, rows of no group); 6: (block start, block width, item start); 7: (item a, item b, item pos);
             8, 9: as 6 and 7 for the diagonal blocks of C over the kept params (8 also gives their param indices)
     build:  binv from the values and the damping vector dev_d [n] (may be NULL): the blocks of
             bsp_cgls_precond_build_* (kind 2) of the eliminated params, bit for bit; dev_work and dev_status as
             there (bsp_cgls_work_bytes(q = 1) per member); a bad block gets a zero inverse and is counted
     mv:     dev_out [nK, q] = S dev_p; dev_t [m, q] is scratch; dev_state (may be NULL) holds the records of a
             bsp_cg_* iteration, whose stopped columns are skipped
     reduce: dev_out [nK, q] = g_k - F^T B^-1 g_e for the full right-hand side dev_g [n, q]
     back:   dev_out [n, q], caller's order: the kept scalars from dev_xk and x_e = B^-1 (g_e - F x_k)
     precond_info / precond_build / precond_apply: the built-in preconditioners of S on the kept scalars, kind 1
             (Jacobi, 1 / (colsq_c + d_c), from dev_colsq [n]) or 2 (block-Jacobi: the inverses of the diagonal
             blocks of C over the kept params, bsp_cgls_precond_build_*'s sums; a kept param wider than 32 is
             refused by name).  info = {blocks, items, inverse elements, widest block, device bytes}; build takes
             dev_work and dev_status as `build`; apply is the preconditioner piece of bsp_cg_* on [nK, q] vectors
             (z = M^-1 r, r.z, beta) with that iteration's dev_work and dev_state
   Every sum runs in a fixed order with every product rounded before it is added (DESIGN.md section 29 states the
   orders); no atomics; member b of a batched call is bitwise the single call. */
typedef struct bsp_jac_schur bsp_jac_schur;
int bsp_jac_schur_create(const bsp_jac_product* p, int64_t num_eliminate, const int64_t* eliminate, bsp_jac_schur** out);
void bsp_jac_schur_destroy(bsp_jac_schur* h);
int bsp_jac_schur_info(const bsp_jac_schur* h, int64_t out[20]);
int bsp_jac_schur_table(const bsp_jac_schur* h, int32_t part, int32_t* t0, int32_t* t1, int32_t* t2, int32_t* t3);
int bsp_jac_schur_precond_info(const bsp_jac_schur* h, int32_t kind, int64_t out[5]);
int bsp_jac_schur_build_f64(bsp_solver* s, const bsp_jac_schur* h, const double* dev_values, const double* dev_d, double* dev_binv,
                            void* dev_work, int64_t* dev_status);
int bsp_jac_schur_build_batched_f64(bsp_solver* s, const bsp_jac_schur* h, const double* const* dev_values,
                                    const double* const* dev_d, double* const* dev_binv, void* dev_work, int64_t* dev_status,
                                    int32_t batch);
int bsp_jac_schur_mv_f64(bsp_solver* s, const bsp_jac_schur* h, int64_t q, const double* dev_values, const double* dev_binv,
                         const double* dev_d, const double* dev_p, double* dev_t, double* dev_out, const int64_t* dev_state);
int bsp_jac_schur_mv_batched_f64(bsp_solver* s, const bsp_jac_schur* h, int64_t q, const double* const* dev_values,
                                 const double* const* dev_binv, const double* const* dev_d, const double* const* dev_p,
                                 double* const* dev_t, double* const* dev_out, const int64_t* dev_state, int32_t batch);
int bsp_jac_schur_reduce_f64(bsp_solver* s, const bsp_jac_schur* h, int64_t q, const double* dev_values, const double* dev_binv,
                             const double* dev_g, double* dev_t, double* dev_out);
int bsp_jac_schur_reduce_batched_f64(bsp_solver* s, const bsp_jac_schur* h, int64_t q, const double* const* dev_values,
                                     const double* const* dev_binv, const double* const* dev_g, double* const* dev_t,
                                     double* const* dev_out, int32_t batch);
int bsp_jac_schur_back_f64(bsp_solver* s, const bsp_jac_schur* h, int64_t q, const double* dev_values, const double* dev_binv,
                           const double* dev_g, const double* dev_xk, double* dev_t, double* dev_out);
int bsp_jac_schur_back_batched_f64(bsp_solver* s, const bsp_jac_schur* h, int64_t q, const double* const* dev_values,
                                   const double* const* dev_binv, const double* const* dev_g, const double* const* dev_xk,
                                   double* const* dev_t, double* const* dev_out, int32_t batch);
int bsp_jac_schur_precond_build_f64(bsp_solver* s, const bsp_jac_schur* h, int32_t kind, const double* dev_values,
                                    const double* dev_colsq, const double* dev_d, double* dev_minv, void* dev_work,
                                    int64_t* dev_status);
int bsp_jac_schur_precond_build_batched_f64(bsp_solver* s, const bsp_jac_schur* h, int32_t kind,
                                            const double* const* dev_values, const double* const* dev_colsq,
                                            const double* const* dev_d, double* const* dev_minv, void* dev_work,
                                            int64_t* dev_status, int32_t batch);
int bsp_jac_schur_precond_apply_f64(bsp_solver* s, const bsp_jac_schur* h, int32_t kind, int64_t q, const double* dev_minv,
                                    const double* dev_r, double* dev_z, void* dev_work, int64_t* dev_state);
int bsp_jac_schur_precond_apply_batched_f64(bsp_solver* s, const bsp_jac_schur* h, int32_t kind, int64_t q,
                                            const double* const* dev_minv, const double* const* dev_r, double* const* dev_z,
                                            void* dev_work, int64_t* dev_state, int32_t batch);
int bsp_jac_schur_build_f32(bsp_solver* s, const bsp_jac_schur* h, const float* dev_values, const float* dev_d, float* dev_binv,
                            void* dev_work, int64_t* dev_status);
int bsp_jac_schur_build_batched_f32(bsp_solver* s, const bsp_jac_schur* h, const float* const* dev_values,
                                    const float* const* dev_d, float* const* dev_binv, void* dev_work, int64_t* dev_status,
                                    int32_t batch);
int bsp_jac_schur_mv_f32(bsp_solver* s, const bsp_jac_schur* h, int64_t q, const float* dev_values, const float* dev_binv,
                         const float* dev_d, const float* dev_p, float* dev_t, float* dev_out, const int64_t* dev_state);
int bsp_jac_schur_mv_batched_f32(bsp_solver* s, const bsp_jac_schur* h, int64_t q, const float* const* dev_values,
                                 const float* const* dev_binv, const float* const* dev_d, const float* const* dev_p,
                                 float* const* dev_t, float* const* dev_out, const int64_t* dev_state, int32_t batch);
int bsp_jac_schur_reduce_f32(bsp_solver* s, const bsp_jac_schur* h, int64_t q, const float* dev_values, const float* dev_binv,
                             const float* dev_g, float* dev_t, float* dev_out);
int bsp_jac_schur_reduce_batched_f32(bsp_solver* s, const bsp_jac_schur* h, int64_t q, const float* const* dev_values,
                                     const float* const* dev_binv, const float* const* dev_g, float* const* dev_t,
                                     float* const* dev_out, int32_t batch);
int bsp_jac_schur_back_f32(bsp_solver* s, const bsp_jac_schur* h, int64_t q, const float* dev_values, const float* dev_binv,
                           const float* dev_g, const float* dev_xk, float* dev_t, float* dev_out);
int bsp_jac_schur_back_batched_f32(bsp_solver* s, const bsp_jac_schur* h, int64_t q, const float* const* dev_values,
                                   const float* const* dev_binv, const float* const* dev_g, const float* const* dev_xk,
                                   float* const* dev_t, float* const* dev_out, int32_t batch);
int bsp_jac_schur_precond_build_f32(bsp_solver* s, const bsp_jac_schur* h, int32_t kind, const float* dev_values,
                                    const double* dev_colsq, const float* dev_d, float* dev_minv, void* dev_work,
                                    int64_t* dev_status);
int bsp_jac_schur_precond_build_batched_f32(bsp_solver* s, const bsp_jac_schur* h, int32_t kind,
                                            const float* const* dev_values, const double* const* dev_colsq,
                                            const float* const* dev_d, float* const* dev_minv, void* dev_work,
                                            int64_t* dev_status, int32_t batch);
int bsp_jac_schur_precond_apply_f32(bsp_solver* s, const bsp_jac_schur* h, int32_t kind, int64_t q, const float* dev_minv,
                                    const float* dev_r, float* dev_z, void* dev_work, int64_t* dev_state);
int bsp_jac_schur_precond_apply_batched_f32(bsp_solver* s, const bsp_jac_schur* h, int32_t kind, int64_t q,
                                            const float* const* dev_minv, const float* const* dev_r, float* const* dev_z,
                                            void* dev_work, int64_t* dev_state, int32_t batch);
/* EXTENSION without a counterpart in the reference's library: the block diagonal of the reduced matrix S itself as
   the preconditioner of the implicit Schur iteration ("schur_jacobi").  With e an eliminated
   param, b a kept one (at most 32 scalars: a wider one is refused by name), S_bb = D_bb + sum over the free rows of
   J_ib^T J_ib + sum over e of (G_eb - F_eb^T Binv_e F_eb); M^-1 = blockdiag(S_bb^-1), block b row-major at the
   offsets of the kept blocks of kind 2 above.  The host plan is built by the first call from the map's lists
   (counting sorts; never the item plan of kind 2): a pair (e, b) exists when a row of group e has an entry in a
   column of b; the free rows that touch b are cut into pseudo-pairs of at most 64 rows; the pairs of b (real ones
   in ascending e, then the pseudo-pairs) are cut into chunks of at most 64.
     sjacobi_info:  {blocks, real pairs, pseudo-pairs, pair rows, chunks, inverse elements, partial elements per
                    matrix, device bytes}
     sjacobi_table: part 0: (first pair [blocks + 1], first chunk [blocks + 1], width [blocks]; t3: first inverse
                    element [blocks + 1]); 1: (first pair [chunks + 1], block [chunks]; t3: first partial element
                    [chunks + 1]); 2: (eliminated param or -1 [pairs], first pair row [pairs + 1], first record
                    entry [pairs + 1]); 3: (Jacobian row [pair rows], records: per pair row the entry index at every
                    scalar of b, then of e, or -1).  An unknown part is refused by number
     kept_plan_built: 1 when the item plan of kind 2 over the kept params exists on the host, else 0
     sjacobi_build: dev_minv from the values, dev_binv of bsp_jac_schur_build_* and dev_d [n] (may be NULL), in two
                    launches: one wave per (chunk, matrix) writes the lower triangle of its partial sum to
                    dev_partials (partial elements doubles per member), one wave per (block, matrix) folds them,
                    adds d and inverts; dev_work and dev_status as bsp_jac_schur_precond_build_*; a bad block gets
                    a zero inverse and is counted
     sjacobi_apply: bsp_jac_schur_precond_apply_* of kind 2 on dev_minv, without the item plan
   All block arithmetic is in double for both types, every product rounded before it is added, in the orders of
   DESIGN.md section 30; no atomics; member b of a batched call is bitwise the single call. */
int bsp_jac_schur_sjacobi_info(const bsp_jac_schur* h, int64_t out[8]);
int bsp_jac_schur_sjacobi_table(const bsp_jac_schur* h, int32_t part, int32_t* t0, int32_t* t1, int32_t* t2, int64_t* t3);
int bsp_jac_schur_kept_plan_built(const bsp_jac_schur* h, int32_t* out);
int bsp_jac_schur_sjacobi_build_f64(bsp_solver* s, const bsp_jac_schur* h, const double* dev_values, const double* dev_binv,
                                    const double* dev_d, double* dev_partials, double* dev_minv, void* dev_work,
                                    int64_t* dev_status);
int bsp_jac_schur_sjacobi_build_batched_f64(bsp_solver* s, const bsp_jac_schur* h, const double* const* dev_values,
                                            const double* const* dev_binv, const double* const* dev_d,
                                            double* const* dev_partials, double* const* dev_minv, void* dev_work,
                                            int64_t* dev_status, int32_t batch);
int bsp_jac_schur_sjacobi_apply_f64(bsp_solver* s, const bsp_jac_schur* h, int64_t q, const double* dev_minv,
                                    const double* dev_r, double* dev_z, void* dev_work, int64_t* dev_state);
int bsp_jac_schur_sjacobi_apply_batched_f64(bsp_solver* s, const bsp_jac_schur* h, int64_t q, const double* const* dev_minv,
                                            const double* const* dev_r, double* const* dev_z, void* dev_work,
                                            int64_t* dev_state, int32_t batch);
int bsp_jac_schur_sjacobi_build_f32(bsp_solver* s, const bsp_jac_schur* h, const float* dev_values, const float* dev_binv,
                                    const float* dev_d, double* dev_partials, float* dev_minv, void* dev_work,
                                    int64_t* dev_status);
int bsp_jac_schur_sjacobi_build_batched_f32(bsp_solver* s, const bsp_jac_schur* h, const float* const* dev_values,
                                            const float* const* dev_binv, const float* const* dev_d,
                                            double* const* dev_partials, float* const* dev_minv, void* dev_work,
                                            int64_t* dev_status, int32_t batch);
int bsp_jac_schur_sjacobi_apply_f32(bsp_solver* s, const bsp_jac_schur* h, int64_t q, const float* dev_minv,
                                    const float* dev_r, float* dev_z, void* dev_work, int64_t* dev_state);
int bsp_jac_schur_sjacobi_apply_batched_f32(bsp_solver* s, const bsp_jac_schur* h, int64_t q, const float* const* dev_minv,
                                            const float* const* dev_r, float* const* dev_z, void* dev_work,
                                            int64_t* dev_state, int32_t batch);
/* EXTENSION without a counterpart in the reference's library: the pieces of the Lanczos recurrence with its
   scalars on the device, for extreme eigenvalues, a 2-norm condition estimate and
   stochastic Lanczos quadrature (log-determinants) without a factor.  One problem per (matrix, start vector):
   vectors are [n, q] row-major; dev_basis is one array per member whose slot s is the [n, q] vector at
   dev_basis + s slot_stride elements (slot_stride >= n q), `slots` of them; dev_state holds
   bsp_lanczos_state_words = 12 8-byte words per problem, problem c of member m at (m q + c) 12: [0] steps done,
   [1] stop reason (0 running, 2 step limit, 3 invariant subspace: ww <= breakdown^2 (alpha^2 + beta_prev^2),
   4 a non-finite sum, 5 zero start vector; 1 is unused, the shared codes are bsp_cg_*'s), then the doubles
   [2] vv = v0.v0, [3] alpha, [4] beta, [5] ww, [6] breakdown^2, then [7] kmax, [8] .. [11] 0; dev_coef holds 2 kmax
   doubles per problem, alpha_0 .. alpha_{kmax-1} then beta_0 .. beta_{kmax-1}, zeroed by the caller: step j
   writes entry j of both.  Every piece reads its scalars from the records and leaves the basis, dev_coef and
   the record of a stopped problem bitwise unchanged; nothing is read back by the library, so the caller may
   queue any number of steps and look at the stop words when it likes.  Step j is: w = A v_j (the caller's:
   bsp_sym_product_mv_* or any operator); alpha; update; [project; subtract] twice for full
   reorthogonalisation; normalize (not after the last step, kmax - 1: every problem has stopped).
     init:       the records are reset (kmax, breakdown), vv = v0.v0 taken, slot `slot` = v0 T(1 / sqrt(vv));
                 a zero v0 stops with reason 5 and writes no slot
     alpha:      alpha_j = v_j . w, v_j = slot `slot`
     update:     w = (w - T(alpha_j) v_j) - T(beta_{j-1}) v_{j-1}, v_{j-1} = slot `prev` (not read at step 0),
                 with the partials of ww = w.w of the same pass
     project:    c_i = v_i . w for the slots i = 0 .. count - 1, in one pass over w and the slots
     subtract:   w = w - T(c_i) v_i, i = 0 .. count - 1 in this order, with the partials of ww
     normalize:  slot `slot` = w T(1 / beta_j)
   update and subtract take `fold`: non-zero on the last piece of the step that writes w, which then ends the
   step: alpha_j and beta_j = sqrt(ww) stored in the record and dev_coef, the step counted, then stop 4 if
   alpha_j or ww is not finite, stop 3 if ww <= breakdown^2 (alpha_j^2 + beta_{j-1}^2), stop 2 at kmax steps.
   Dot products are taken in double for both precisions, in the two-pass order of bsp_cg_* with every product
   rounded before it is added; the vector updates round every product in the data type.  No atomics; member
   b of a batched call is bitwise the single call.  WORKSPACE: dev_work is the caller's, 16-byte aligned,
   bsp_lanczos_work_bytes bytes per member (16 bytes per 1024 rows, start vector and step of kmax, plus 8
   bytes per start vector and step, rounded up to 16), members one after the other; nothing is allocated
   inside a call.  Refused before any device work: NULL arguments, an empty batch or a NULL member, n < 0,
   q < 1, kmax < 1, a slot or count outside the basis (count also above kmax), a slot stride below n q, a
   misaligned workspace. */
int bsp_lanczos_state_words(int64_t* out);
int bsp_lanczos_work_bytes(const bsp_solver* s, int64_t n, int64_t q, int64_t kmax, int64_t* out);
int bsp_lanczos_init_f64(bsp_solver* s, int64_t n, int64_t q, int64_t kmax, const double* dev_v0, double* dev_basis,
                         int64_t slot_stride, int64_t slots, int64_t slot, double breakdown, void* dev_work,
                         int64_t* dev_state);
int bsp_lanczos_init_batched_f64(bsp_solver* s, int64_t n, int64_t q, int64_t kmax, const double* const* dev_v0,
                                 double* const* dev_basis, int64_t slot_stride, int64_t slots, int64_t slot, double
                                 breakdown, void* dev_work, int64_t* dev_state, int32_t batch);
int bsp_lanczos_alpha_f64(bsp_solver* s, int64_t n, int64_t q, int64_t kmax, const double* dev_w,
                          const double* dev_basis, int64_t slot_stride, int64_t slots, int64_t slot, void* dev_work,
                          int64_t* dev_state);
int bsp_lanczos_alpha_batched_f64(bsp_solver* s, int64_t n, int64_t q, int64_t kmax, const double* const* dev_w,
                                  const double* const* dev_basis, int64_t slot_stride, int64_t slots, int64_t slot,
                                  void* dev_work, int64_t* dev_state, int32_t batch);
int bsp_lanczos_update_f64(bsp_solver* s, int64_t n, int64_t q, int64_t kmax, double* dev_w, const double* dev_basis,
                           int64_t slot_stride, int64_t slots, int64_t slot, int64_t prev, int32_t fold,
                           double* dev_coef, void* dev_work, int64_t* dev_state);
int bsp_lanczos_update_batched_f64(bsp_solver* s, int64_t n, int64_t q, int64_t kmax, double* const* dev_w,
                                   const double* const* dev_basis, int64_t slot_stride, int64_t slots, int64_t slot,
                                   int64_t prev, int32_t fold, double* dev_coef, void* dev_work, int64_t* dev_state,
                                   int32_t batch);
int bsp_lanczos_project_f64(bsp_solver* s, int64_t n, int64_t q, int64_t kmax, const double* dev_w,
                            const double* dev_basis, int64_t slot_stride, int64_t slots, int64_t count, void* dev_work,
                            int64_t* dev_state);
int bsp_lanczos_project_batched_f64(bsp_solver* s, int64_t n, int64_t q, int64_t kmax, const double* const* dev_w,
                                    const double* const* dev_basis, int64_t slot_stride, int64_t slots, int64_t count,
                                    void* dev_work, int64_t* dev_state, int32_t batch);
int bsp_lanczos_subtract_f64(bsp_solver* s, int64_t n, int64_t q, int64_t kmax, double* dev_w,
                             const double* dev_basis, int64_t slot_stride, int64_t slots, int64_t count, int32_t fold,
                             double* dev_coef, void* dev_work, int64_t* dev_state);
int bsp_lanczos_subtract_batched_f64(bsp_solver* s, int64_t n, int64_t q, int64_t kmax, double* const* dev_w,
                                     const double* const* dev_basis, int64_t slot_stride, int64_t slots, int64_t count,
                                     int32_t fold, double* dev_coef, void* dev_work, int64_t* dev_state,
                                     int32_t batch);
int bsp_lanczos_normalize_f64(bsp_solver* s, int64_t n, int64_t q, int64_t kmax, const double* dev_w,
                              double* dev_basis, int64_t slot_stride, int64_t slots, int64_t slot, void* dev_work,
                              int64_t* dev_state);
int bsp_lanczos_normalize_batched_f64(bsp_solver* s, int64_t n, int64_t q, int64_t kmax, const double* const* dev_w,
                                      double* const* dev_basis, int64_t slot_stride, int64_t slots, int64_t slot,
                                      void* dev_work, int64_t* dev_state, int32_t batch);
int bsp_lanczos_init_f32(bsp_solver* s, int64_t n, int64_t q, int64_t kmax, const float* dev_v0, float* dev_basis,
                         int64_t slot_stride, int64_t slots, int64_t slot, double breakdown, void* dev_work,
                         int64_t* dev_state);
int bsp_lanczos_init_batched_f32(bsp_solver* s, int64_t n, int64_t q, int64_t kmax, const float* const* dev_v0,
                                 float* const* dev_basis, int64_t slot_stride, int64_t slots, int64_t slot,
                                 double breakdown, void* dev_work, int64_t* dev_state, int32_t batch);
int bsp_lanczos_alpha_f32(bsp_solver* s, int64_t n, int64_t q, int64_t kmax, const float* dev_w,
                          const float* dev_basis, int64_t slot_stride, int64_t slots, int64_t slot, void* dev_work,
                          int64_t* dev_state);
int bsp_lanczos_alpha_batched_f32(bsp_solver* s, int64_t n, int64_t q, int64_t kmax, const float* const* dev_w,
                                  const float* const* dev_basis, int64_t slot_stride, int64_t slots, int64_t slot,
                                  void* dev_work, int64_t* dev_state, int32_t batch);
int bsp_lanczos_update_f32(bsp_solver* s, int64_t n, int64_t q, int64_t kmax, float* dev_w, const float* dev_basis,
                           int64_t slot_stride, int64_t slots, int64_t slot, int64_t prev, int32_t fold,
                           double* dev_coef, void* dev_work, int64_t* dev_state);
int bsp_lanczos_update_batched_f32(bsp_solver* s, int64_t n, int64_t q, int64_t kmax, float* const* dev_w,
                                   const float* const* dev_basis, int64_t slot_stride, int64_t slots, int64_t slot,
                                   int64_t prev, int32_t fold, double* dev_coef, void* dev_work, int64_t* dev_state,
                                   int32_t batch);
int bsp_lanczos_project_f32(bsp_solver* s, int64_t n, int64_t q, int64_t kmax, const float* dev_w,
                            const float* dev_basis, int64_t slot_stride, int64_t slots, int64_t count, void* dev_work,
                            int64_t* dev_state);
int bsp_lanczos_project_batched_f32(bsp_solver* s, int64_t n, int64_t q, int64_t kmax, const float* const* dev_w,
                                    const float* const* dev_basis, int64_t slot_stride, int64_t slots, int64_t count,
                                    void* dev_work, int64_t* dev_state, int32_t batch);
int bsp_lanczos_subtract_f32(bsp_solver* s, int64_t n, int64_t q, int64_t kmax, float* dev_w, const float* dev_basis,
                             int64_t slot_stride, int64_t slots, int64_t count, int32_t fold, double* dev_coef,
                             void* dev_work, int64_t* dev_state);
int bsp_lanczos_subtract_batched_f32(bsp_solver* s, int64_t n, int64_t q, int64_t kmax, float* const* dev_w,
                                     const float* const* dev_basis, int64_t slot_stride, int64_t slots, int64_t count,
                                     int32_t fold, double* dev_coef, void* dev_work, int64_t* dev_state,
                                     int32_t batch);
int bsp_lanczos_normalize_f32(bsp_solver* s, int64_t n, int64_t q, int64_t kmax, const float* dev_w, float* dev_basis,
                              int64_t slot_stride, int64_t slots, int64_t slot, void* dev_work, int64_t* dev_state);
int bsp_lanczos_normalize_batched_f32(bsp_solver* s, int64_t n, int64_t q, int64_t kmax, const float* const* dev_w,
                                      float* const* dev_basis, int64_t slot_stride, int64_t slots, int64_t slot,
                                      void* dev_work, int64_t* dev_state, int32_t batch);
/* EXTENSION without a counterpart in the reference's library: combinations of the vectors of a basis (DESIGN.md
   section 26), the tall-skinny product behind f(A) v ~ |v0| V f(T_k) e_1 from a Lanczos basis.  For each output
   f < nf and each column c < q of every member
     out_f[:, c] = (accumulate ? out_f[:, c] : +0) + sum_i T(y[c, f, i]) slot (slot + i)[:, c],
   i = 0 .. count - 1 in ascending order, the arithmetic in the data type T with every product rounded before
   it is added (the convention of bsp_lanczos_subtract_*).  Term i has the Lanczos index first + i: it is skipped,
   and its slot not read, when first + i >= dev_limit[c].  The order is fixed so that the bits of a result do not
   depend on how the terms are split over calls: a chain of calls with accumulate != 0 over consecutive ranges
   gives the bits of one call over all of them.  dev_basis, slot_stride and slots are those of bsp_lanczos_*
   (slot s is the [n, q] row-major vector at dev_basis + s slot_stride); dev_y holds doubles [q, nf, ldy], the
   coefficient of (c, f, i) at (c nf + f) ldy + i, and for a batch [batch, q, nf, ldy], one array; dev_limit
   holds int64 [q], for a batch [batch, q], one array; output f of a member is the [n, q] array at dev_out +
   f out_stride.  A column with no term taken gets +0 (accumulate == 0) or is left as it is.  Every slot is read
   once for all nf outputs: min(count, limit - first) n q sizeof(T) bytes read, nf n q sizeof(T) written.  No
   atomics, no workspace; member b of a batched call is bitwise the single call.  Refused before any device
   work: NULL arguments, an empty batch or a NULL member, n < 0, q < 1, nf outside 1 .. 4, count < 1, first < 0,
   slot < 0, slot + count > slots, slot_stride < n q, out_stride < n q, ldy < count.  n == 0 succeeds without a
   launch. */
int bsp_krylov_combine_f64(bsp_solver* s, int64_t n, int64_t q, int32_t nf, const double* dev_basis,
                           int64_t slot_stride, int64_t slots, int64_t slot, int64_t count, int64_t first,
                           const double* dev_y, int64_t ldy, const int64_t* dev_limit, double* dev_out,
                           int64_t out_stride, int32_t accumulate);
int bsp_krylov_combine_batched_f64(bsp_solver* s, int64_t n, int64_t q, int32_t nf, const double* const* dev_basis,
                                   int64_t slot_stride, int64_t slots, int64_t slot, int64_t count, int64_t first,
                                   const double* dev_y, int64_t ldy, const int64_t* dev_limit,
                                   double* const* dev_out, int64_t out_stride, int32_t accumulate, int32_t batch);
int bsp_krylov_combine_f32(bsp_solver* s, int64_t n, int64_t q, int32_t nf, const float* dev_basis,
                           int64_t slot_stride, int64_t slots, int64_t slot, int64_t count, int64_t first,
                           const double* dev_y, int64_t ldy, const int64_t* dev_limit, float* dev_out,
                           int64_t out_stride, int32_t accumulate);
int bsp_krylov_combine_batched_f32(bsp_solver* s, int64_t n, int64_t q, int32_t nf, const float* const* dev_basis,
                                   int64_t slot_stride, int64_t slots, int64_t slot, int64_t count, int64_t first,
                                   const double* dev_y, int64_t ldy, const int64_t* dev_limit,
                                   float* const* dev_out, int64_t out_stride, int32_t accumulate, int32_t batch);
/* out[i_user] = i_internal (order values): the caller's scalar i in the solver's internal vector order
   (param p at spanStart[paramToSpan[p]], its scalars in order) */
int bsp_scalar_permutation(const bsp_solver* s, int64_t* out);
/* Solver::solve<std::vector<T*>> etc. (Solver.h:64-73 with the batch types of MatOps.h:38-42):
   `batch` factored matrices of the same structure and one block of right-hand sides each
   (host arrays of device pointers).  which: 0 = solve, 1 = solveL, 2 = solveLt */
int bsp_solve_batched_f64(bsp_solver* s, const double* const* dev_mats, double* const* dev_vecs,
                          int32_t batch, int64_t stride, int32_t nrhs, int32_t which);
int bsp_solve_batched_f32(bsp_solver* s, const float* const* dev_mats, float* const* dev_vecs,
                          int32_t batch, int64_t stride, int32_t nrhs, int32_t which);
/* the batch forms of the partial operations (Solver.cpp:491-519 instantiates factorUpTo / factorFrom
   / solveLUpTo / solveLtUpTo for std::vector<T*>; solveLFrom / solveLtFrom come with them here).
   factor: which 0 = factorUpTo, 1 = factorFrom; solve: which as bsp_solve_partial_* */
int bsp_factor_partial_batched_f64(bsp_solver* s, double* const* dev_ptrs, int32_t batch,
                                   int64_t span_index, int32_t which);
int bsp_factor_partial_batched_f32(bsp_solver* s, float* const* dev_ptrs, int32_t batch,
                                   int64_t span_index, int32_t which);
int bsp_solve_partial_batched_f64(bsp_solver* s, const double* const* dev_mats,
                                  double* const* dev_vecs, int32_t batch, int64_t stride,
                                  int32_t nrhs, int32_t which, int64_t span_index);
int bsp_solve_partial_batched_f32(bsp_solver* s, const float* const* dev_mats, float* const* dev_vecs,
                                  int32_t batch, int64_t stride, int32_t nrhs, int32_t which,
                                  int64_t span_index);

/* ---- BAL caller pipeline on the device (benchmarking/BaAtLargeOptimizer.cpp:100-131 computeStep,
   with the 9-parameter cameras of a BAL file: Rodrigues rotation, translation, f, k1, k2).  All
   pointers are device memory.
   bsp_bal_linearize: reprojection residual res[2 nObs] and Jacobians Jc[nObs][2][9] (camera),
   Jp[nObs][2][3] (point) of every observation (obs_xy[nObs][2], cams[nCams][9], pts[nPts][3]).
   bsp_bal_fill_hessian: data += J^T J through Solver::deviceAccessor() -- accessor.diagBlock(pt),
   accessor.diagBlock(cam), accessor.block(cam, pt) per observation -- grad += J^T r (may be NULL),
   then the LM damping d <- d (1 + lambda) + 1e-3 lambda of every diagonal entry.  The caller zeroes
   data / grad first; parameters are numbered points first, cameras after (BaAtLargeBench.cpp:50-57).
   dbg (may be NULL): 7 int64 per observation = what the accessor returned on the device (block
   offset, stride, flipped; camera diag offset, stride; point diag offset, stride). */
int bsp_bal_linearize_f64(int64_t num_obs, const int64_t* obs_cam, const int64_t* obs_pt,
                          const double* obs_xy, const double* cams, const double* pts, double* res,
                          double* Jc, double* Jp, void* stream);
int bsp_bal_fill_hessian_f64(bsp_solver* s, int64_t num_pts, int64_t num_cams, int64_t num_obs,
                             const int64_t* obs_cam, const int64_t* obs_pt, const double* Jc,
                             const double* Jp, const double* res, double lambda, double* dev_data,
                             double* dev_grad, int64_t* dev_dbg, void* stream);
int bsp_bal_fill_hessian_f32(bsp_solver* s, int64_t num_pts, int64_t num_cams, int64_t num_obs,
                             const int64_t* obs_cam, const int64_t* obs_pt, const double* Jc,
                             const double* Jp, const double* res, float lambda, float* dev_data,
                             float* dev_grad, int64_t* dev_dbg, void* stream);

/* The same pipeline in the REFERENCE's parameterisation (benchmarking/BaAtLarge.h:56-150
   Cost::compute_residual, BaAtLargeOptimizer.cpp:24-52,100-131,176-183): cameras are 6-wide blocks,
   the tangent of a left SE(3) perturbation T_W_C <- exp(delta) T_W_C (translation first), calibration
   (f, k1, k2) fixed; Jc[nObs][2][6]; a point with camPt.z > 0.01 gives the residual (25, 0) and zero
   Jacobians.  cams[nCams][9] keeps the BAL storage (Rodrigues rotation, translation, f, k1, k2).
   The solver must have been created with camera blocks of size 6 (checked). */
int bsp_bal_linearize_se3_f64(int64_t num_obs, const int64_t* obs_cam, const int64_t* obs_pt,
                              const double* obs_xy, const double* cams, const double* pts,
                              double* res, double* Jc, double* Jp, void* stream);
int bsp_bal_fill_hessian_se3_f64(bsp_solver* s, int64_t num_pts, int64_t num_cams, int64_t num_obs,
                                 const int64_t* obs_cam, const int64_t* obs_pt, const double* Jc,
                                 const double* Jp, const double* res, double lambda, double* dev_data,
                                 double* dev_grad, void* stream);
int bsp_bal_fill_hessian_se3_f32(bsp_solver* s, int64_t num_pts, int64_t num_cams, int64_t num_obs,
                                 const int64_t* obs_cam, const int64_t* obs_pt, const double* Jc,
                                 const double* Jp, const double* res, float lambda, float* dev_data,
                                 float* dev_grad, void* stream);

/* ---- The rest of a Levenberg-Marquardt iteration on the device (BaAtLargeOptimizer.cpp:54-63
   computeCost, :173-184 applyStep, :186-234 optimize; examples/SoftLoss.h and examples/Optimizer.h
   computeSingleGradHess for the robust loss).  All pointers are device memory, everything is fp64; no
   entry uses atomics, synchronises the host or allocates; every launch goes to `stream`.
   bsp_bal_residuals / bsp_bal_residuals_se3: res[2 nObs] alone, what the linearisation writes to res
   (the SE3 form with the same rule: camPt.z > 0.01 gives exactly (25, 0)).
   bsp_bal_loss: per observation s = r0^2 + r1^2, rho[o] = rho(s), w = rho'(s) (SoftLoss.h jet2):
     kind 0 trivial (s, 1);  1 Huber: s > a^2 ? (2 a sqrt(s) - a^2, a / sqrt(s)) : (s, 1);
     2 Cauchy (a^2 log1p(s / a^2), 1 / (1 + s / a^2)).
   With Jc and Jp given (both or neither; cam_size 9 or 6) the observation's 2 residuals and its
   2 x cam_size and 2 x 3 Jacobian rows are multiplied in place by sqrt(w): bsp_bal_fill_hessian then
   accumulates w J^T J and w J^T r (Optimizer.h: H += rho' J^T J, g += rho' J^T r, cost = rho / 2; no
   second-order term).  An observation with w == 1 is not rewritten.  With Jc = Jp = NULL only rho is
   written.  An unknown kind or an `a` that is not finite and positive: non-zero return, nothing launched.
   bsp_bal_sum: out[0] = scale * sum x[0 .. n) in a fixed order (bitwise reproducible; the order is stated
   in csrc/bal_pipeline.h), +0.0 for n == 0.  scratch holds bsp_bal_sum_scratch_len(n) = ceil(n / 2048)
   doubles.
   bsp_bal_apply_step / bsp_bal_apply_step_se3: out of place, cams_out / pts_out must not overlap the
   inputs.  `step` is in the solver's internal order (what bsp_solve leaves in the gradient buffer);
   points first, cameras after.
   pts_out = pts - step; bal9: every camera parameter minus its step; se3: T_W_C <- exp(-step) T_W_C with
   step = (translation part, rotation part) (BaAtLargeOptimizer.cpp:181-182), the rotation returned as an
   axis-angle vector of length <= pi, (f, k1, k2) copied.  A solver whose camera blocks are not 9 (6)
   wide or whose order is not 3 num_pts + 9 (6) num_cams is refused. */
int bsp_bal_residuals_f64(int64_t num_obs, const int64_t* obs_cam, const int64_t* obs_pt,
                          const double* obs_xy, const double* cams, const double* pts, double* res,
                          void* stream);
int bsp_bal_residuals_se3_f64(int64_t num_obs, const int64_t* obs_cam, const int64_t* obs_pt,
                              const double* obs_xy, const double* cams, const double* pts, double* res,
                              void* stream);
int bsp_bal_loss_f64(int64_t num_obs, int32_t cam_size, int32_t kind, double a, double* res, double* Jc,
                     double* Jp, double* rho, void* stream);
int64_t bsp_bal_sum_scratch_len(int64_t n);
int bsp_bal_sum_f64(int64_t n, const double* x, double scale, double* scratch, double* out,
                    void* stream);
int bsp_bal_apply_step_f64(bsp_solver* s, int64_t num_pts, int64_t num_cams, const double* cams,
                           const double* pts, const double* step, double* cams_out, double* pts_out,
                           void* stream);
int bsp_bal_apply_step_se3_f64(bsp_solver* s, int64_t num_pts, int64_t num_cams, const double* cams,
                               const double* pts, const double* step, double* cams_out, double* pts_out,
                               void* stream);

/* ---- Ordered Hessian fill: the contract of the bsp_bal_fill_hessian entries without atomics, so that data
   and grad are the same bits on every run and every device (the summation order is stated in
   csrc/bal_pipeline.h and DESIGN.md section 9).
   bsp_bal_fill_plan_create builds the plan once per problem on the host (no device work) from HOST
   arrays obs_cam / obs_pt of num_obs entries; cam_size is 9 or 6.  An observation whose camera or point
   index is out of range is left out (and counted), as the atomic fill skips it.  It fails, with
   bsp_last_error(), for num_obs >= 2^31, for a solver that does not have num_pts parameters of size 3
   followed by num_cams of size cam_size (order 3 num_pts + cam_size num_cams), and for an observation
   whose block the solver does not store.  A plan belongs to the solver it was built on and must be
   destroyed before it.
   bsp_bal_fill_plan_info: out[12] = kept observations, skipped observations, (point, camera) pairs,
   chunks of the camera lists, chunk length C, lanes per element W, longest point list, longest camera
   list, scratch length (doubles), bytes of the plan on the host, bytes on the device (tables + scratch),
   cam_size.
   bsp_bal_fill_ordered: Jc[nObs][2][cam_size], Jp[nObs][2][3], res[nObs][2] are fp64 device arrays of the
   num_obs observations the plan was built from; data += J^T J, grad += J^T r (grad may be NULL), then the
   damping d <- d (1 + lambda) + 1e-3 lambda of every diagonal entry unless lambda == 0.  Every launch goes
   to `stream`; no atomics, no host synchronisation; the first call with a plan uploads its tables (one
   allocation, one blocking copy), later calls allocate nothing.  The partial sums live in the plan, so one
   plan serves one call at a time.  A NULL solver, plan, data, Jc, Jp or res, or a plan built on another
   solver: non-zero return, nothing launched. */
typedef struct bsp_bal_fill_plan bsp_bal_fill_plan;
int bsp_bal_fill_plan_create(bsp_solver* s, int32_t cam_size, int64_t num_pts, int64_t num_cams, int64_t num_obs,
                             const int64_t* obs_cam, const int64_t* obs_pt, bsp_bal_fill_plan** out);
void bsp_bal_fill_plan_destroy(bsp_bal_fill_plan* p);
int bsp_bal_fill_plan_info(const bsp_bal_fill_plan* p, int64_t out[12]);
int bsp_bal_fill_ordered_f64(bsp_solver* s, const bsp_bal_fill_plan* p, const double* Jc, const double* Jp,
                             const double* res, double lambda, double* dev_data, double* dev_grad,
                             void* stream);
int bsp_bal_fill_ordered_f32(bsp_solver* s, const bsp_bal_fill_plan* p, const double* Jc, const double* Jp,
                             const double* res, float lambda, float* dev_data, float* dev_grad, void* stream);

/* ---- measurement helpers (no reference counterpart; Solver::printStats is the analogue) */
/* algorithmic flops of a full factor: sum over lumps n^3/3 + r n^2 + r^2 n */
double bsp_factor_flops(const bsp_solver* s);

typedef struct bsp_plan_stats {
  double flops, upd_elems, upd_flops, elim_pair_elems, elim_pair_flops, elim_col_elems,
      upd_flops_direct,        /* part of upd_flops launched by the one-panel-level kernels */
      elim_pair_operand_elems, /* values of both source blocks, summed over the pairs */
      elim_target_elems,       /* distinct target elements of the sparse-elimination update */
      trsm_flops, potrf_flops, /* dense panels: rowsBelow*nb^2 and nb^3/3 */
      trsm_flops_merged,       /* ... of which inside chain-step launches (trsm + update + potrf) */
      potrf_flops_fused;       /* ... of which inside the previous level's update launch */
  int64_t num_launches, num_levels, num_panels, num_segs, num_upd_tasks, num_trsm_tasks,
      chain_tab_entries, max_panels_in_level, num_atomic_upd_tasks,
      num_gather_groups, /* always 0 (kept for ABI stability) */
      num_fork_levels;   /* levels that hand lookahead units to the auxiliary streams */
  double deferred_flops; /* flops of those units; the lookahead schedule is used when they are worth
                            the forks (HipPlanHost::lookaheadPays) */
  double tail_upd_flops; /* update flops done inside the persistent tail launch (csrc/hip_tail_kernel.h);
                            not part of upd_flops */
  int64_t num_tail_panels;
} bsp_plan_stats;
int bsp_plan_stats_full(bsp_solver* s, bsp_plan_stats* out);

/* What the calls on this solver actually RAN (cumulative counters; no reference counterpart): a
   test can see that the path it means to test was taken, and a caller can poll for a watchdog
   report of the persistent solve sweeps (hip_sweep_kernels.h) without waiting for the next solve,
   which would throw it. */
typedef struct bsp_run_counters {
  int64_t sweep_launches;       /* persistent solve sweeps launched */
  int64_t sweep_timeouts;       /* ... that ran into their watchdog (reported by a later call) */
  int64_t split_lists_used;     /* update launches that took a split-K tile list */
  int64_t sub_batches_enqueued; /* sub-batches enqueued on a stream of their own */
  int64_t lookahead_forks;      /* lookahead launches handed to the auxiliary streams */
  int64_t sweeps_retired;       /* 1: a time-out retired the sweeps of this solver */
  int64_t sweep_error_pending;  /* 1: a time-out has been raised and not been reported yet */
  int64_t gather_chunks_overlapped; /* always 0 (kept for ABI stability) */
  int64_t tail_launches;        /* persistent tail launches (csrc/hip_tail_kernel.h) */
  int64_t sweep_mfma_launches;  /* ... of sweep_launches: the matrix-core form (several right-hand sides) */
  int64_t solve_wide_launches;  /* backward elimination passes with the right-hand sides across the lanes */
  int64_t inv_reused;           /* backward passes that found the inverted diagonal blocks of their forward pass */
  int64_t potrf_folded_levels;  /* tree levels whose potrf launch was folded into their trsm launch */
  int64_t selinv_launches;      /* kernels enqueued by selected inversion and by its adjoint
                                   (bsp_selected_inverse_adjoint_*), single or batched */
  int64_t selinv_chunks;        /* passes over the selected-inversion levels: 1 per single call, 1 per
                                   chunk of a batched call (the adjoint's passes count here too) */
} bsp_run_counters;
int bsp_run_counters_get(bsp_solver* s, bsp_run_counters* out);

/* kernel classes timed by bsp_factor_profiled_* (HIP events on the execution stream) */
enum {
  BSP_PROF_ELIM_FACTOR = 0,
  BSP_PROF_ELIM_UPDATE = 1,
  BSP_PROF_POTRF = 2,
  BSP_PROF_TRSM = 3,
  BSP_PROF_UPDATE = 4,       /* updateTile: task-list launches, the bulk of the flops */
  BSP_PROF_CHAIN_UPDATE = 5, /* update launches of one-panel levels (next potrf fused in) */
  BSP_PROF_NUM_KINDS = 6
};
int bsp_factor_profiled_f64(bsp_solver* s, double* dev_data, double ms[6], int64_t launches[6]);
/* the same with the real two-stream schedule left on: every launch timed on the stream it runs
   on, i.e. what a kernel takes beside the others (= what a rocprofv3 kernel trace shows) */
int bsp_factor_profiled_insitu_f64(bsp_solver* s, double* dev_data, double ms[6],
                                   int64_t launches[6]);
/* ... and, per class, the time during which at least one of its launches was running (launches of
   one class that go to different streams overlap: their durations add up to more than that) */
int bsp_factor_profiled_busy_f64(bsp_solver* s, double* dev_data, double ms[6], int64_t launches[6],
                                 double busy_ms[6]);

/* sustained v_mfma_f64_16x16x4_f64 rate of the current GPU (TFLOP/s), register-only probe */
int bsp_probe_mfma_f64(double* tflops);

/* Developer aid: in-situ kernel clock records of a library built with BSP_KTRACE=1 (8 values per
 * stamped kernel launch); a normal build reports 0 records. */
int bsp_debug_read_trace(long long* out, int max_records, int* n_records);
/* ... and, for builds with -DBSP_TRACE_TILE as well: per chain-step launch {first workgroup start,
 * last workgroup start, last workgroup end, workgroup-0 end} in 10 ns units; reading resets. */
int bsp_debug_read_extents(unsigned long long* out, int max_launches, int* n);

/* Symbolic plan as one flat int64 buffer, so that rank 0 can analyse once and broadcast it
   (RCCL) to the ranks that factor the other matrices of a batch. */
int bsp_plan_serialize(const bsp_solver* s, int64_t* buf, int64_t capacity, int64_t* needed);
int bsp_create_solver_from_plan(const int64_t* buf, int64_t len, bsp_solver** out);

/* Host-side block-pattern operations of the symbolic phase (SparseStructure.h:34-55), exposed
   for bindings and tests.  `arg`/`flag` per op:
     TRANSPOSE            -                                  SparseStructure::transpose
     CLEAR                flag = clearLower                  SparseStructure::clear
     SYM_PERMUTATION      arg = mapPerm[n], flag = lowerHalf SparseStructure::symmetricPermutation
     INDEP_ELIM_FILL      arg = {start, end}                 addIndependentEliminationFill
     FULL_ELIM_FILL       -                                  addFullEliminationFill
     FILL_REDUCING_PERM   -  (out_inds = perm[n], out_ptrs untouched)  fillReducingPermutation
     EXTRACT_RIGHT_BOTTOM arg = {start}                      extractRightBottom
   out_ptrs needs n+1 entries; the call fails if out_inds (capacity entries) is too small,
   reporting the needed size in *out_nnz. */
enum {
  BSP_SS_TRANSPOSE = 0,
  BSP_SS_CLEAR = 1,
  BSP_SS_SYM_PERMUTATION = 2,
  BSP_SS_INDEP_ELIM_FILL = 3,
  BSP_SS_FULL_ELIM_FILL = 4,
  BSP_SS_FILL_REDUCING_PERM = 5,
  BSP_SS_EXTRACT_RIGHT_BOTTOM = 6
};
int bsp_sparse_structure_op(int op, int64_t n, const int64_t* ptrs, const int64_t* inds,
                            const int64_t* arg, int64_t arg_len, int32_t flag, int64_t* out_ptrs,
                            int64_t* out_inds, int64_t capacity, int64_t* out_n, int64_t* out_nnz);

#ifdef __cplusplus
}
#endif
#endif /* BASPACHO_AMD_H_ */
