// C ABI facade (include/baspacho_amd.h) over the C++ Solver.  Exceptions never cross the
// boundary: they become a non-zero return code + bsp_last_error().
#include "../../include/baspacho_amd.h"

#include <cmath>
#include <cstring>
#include <numeric>
#include <string>
#include <unordered_map>
#include <unordered_set>

#include "assembly.h"
#include "factor_product_plan.h"
#include "jac_product.h"
#include "jac_schur.h"
#include "normal_eq.h"
#include "sym_product.h"
#include "reach.h"
#include "bal_pipeline.h"
#include "../../include/baspacho_amd_testing.h"
#include "computation_model.h"
#include "hip_backend.h"
#include "hip_plan.h"
#include "solver.h"

using namespace BaSpaCho;

struct bsp_solver {
  SolverPtr solver;
  ComputationModel model;  // storage for a user-supplied model
  // BAL layout already validated for (numPts, numCams, camSize): the parameter sizes of a solver
  // never change, so the O(numPts + numCams) walk of checkBalLayout runs once, not per LM iteration
  int64_t balOk[3] = {-1, -1, -1};
};

static thread_local std::string g_lastError;

const char* bsp_last_error(void) { return g_lastError.c_str(); }
const char* bsp_version(void) { return "baspacho_amd 0.1 (gfx950)"; }

#define BSP_TRY try {
#define BSP_CATCH                      \
  }                                    \
  catch (const std::exception& e) {    \
    g_lastError = e.what();            \
    return 1;                          \
  }                                    \
  catch (...) {                        \
    g_lastError = "unknown exception"; \
    return 1;                          \
  }                                    \
  return 0;
// the whole body of an entry that is one statement (the per-dtype macros below)
#define BSP_BODY(...) \
  {                   \
    BSP_TRY           \
    __VA_ARGS__;      \
    BSP_CATCH         \
  }

void bsp_hip_options_default(bsp_hip_options* o) {
  o->lookahead = o->due_stream = o->split_k = o->gather_max_pairs = o->gather_overlap = o->sub_batch_min =
      o->sub_batches = o->tail_blocks = o->lazy_plan = o->block_solve = o->solve_inv = o->solve_sweep =
          o->sweep_min_width = o->solve_wide = o->chain_contraction = o->dense_merge = o->expected_batch = -1;
  o->lookahead_min_gf = o->bulk_ahead = o->level_cost_us = NAN;
}

int bsp_create_solver_opts(const bsp_settings* st, const bsp_hip_options* ho, int64_t numParams,
                           const int64_t* paramSizes, const int64_t* ptrs, const int64_t* inds,
                           int64_t numElimRanges, const int64_t* elimRanges, int64_t numElimLast,
                           const int64_t* elimLast, bsp_solver** out) {
  BSP_TRY
  BASPACHO_CHECK_NOTNULL(out);
  std::unique_ptr<bsp_solver> h(new bsp_solver);
  Settings settings;
  HipBackendOptions options;
  if (ho) {
    options.lookahead = ho->lookahead;
    options.dueStream = ho->due_stream;
    options.splitK = ho->split_k;
    options.gatherMaxPairs = ho->gather_max_pairs;
    options.subBatchMin = ho->sub_batch_min;
    options.subBatches = ho->sub_batches;
    options.tailBlocks = ho->tail_blocks;
    options.lazyPlan = ho->lazy_plan;
    options.blockSolve = ho->block_solve;
    options.solveInv = ho->solve_inv;
    options.solveSweep = ho->solve_sweep;
    options.sweepMinWidth = ho->sweep_min_width;
    options.solveWide = ho->solve_wide;
    options.chainContraction = ho->chain_contraction;
    options.denseMerge = ho->dense_merge;
    options.expectedBatch = ho->expected_batch;
    options.lookaheadMinGF = ho->lookahead_min_gf;
    options.bulkAhead = ho->bulk_ahead;
    options.levelCostUs = ho->level_cost_us;
    settings.hipOptions = &options;
  }
  if (st) {
    settings.findSparseEliminationRanges = st->find_sparse_elimination_ranges != 0;
    settings.numThreads = st->num_threads;
    settings.backend = (BackendType)st->backend;
    settings.addFillPolicy = (AddFillPolicy)st->add_fill_policy;
    if (st->computation_model) {
      const double* p = st->computation_model;
      std::copy(p, p + 4, h->model.potrfParams.begin());
      std::copy(p + 4, p + 10, h->model.trsmParams.begin());
      std::copy(p + 10, p + 16, h->model.sygeParams.begin());
      std::copy(p + 16, p + 20, h->model.asmblParams.begin());
      settings.computationModel = &h->model;
    }
  }
  std::vector<int64_t> sizes(paramSizes, paramSizes + numParams);
  SparseStructure ss(std::vector<int64_t>(ptrs, ptrs + numParams + 1),
                     std::vector<int64_t>(inds, inds + ptrs[numParams]));
  std::vector<int64_t> ranges(elimRanges, elimRanges + (elimRanges ? numElimRanges : 0));
  std::unordered_set<int64_t> last(elimLast, elimLast + (elimLast ? numElimLast : 0));
  h->solver = createSolver(settings, sizes, ss, ranges, last);
  *out = h.release();
  BSP_CATCH
}

int bsp_create_solver(const bsp_settings* st, int64_t numParams, const int64_t* paramSizes,
                      const int64_t* ptrs, const int64_t* inds, int64_t numElimRanges,
                      const int64_t* elimRanges, int64_t numElimLast, const int64_t* elimLast,
                      bsp_solver** out) {
  return bsp_create_solver_opts(st, nullptr, numParams, paramSizes, ptrs, inds, numElimRanges, elimRanges,
                                numElimLast, elimLast, out);
}

int bsp_create_solver_from_skeleton(int64_t numSpans, const int64_t* spanStart, int64_t numLumps,
                                    const int64_t* lumpToSpan, const int64_t* colPtr,
                                    const int64_t* rowInd, int64_t numElimRanges,
                                    const int64_t* elimRanges, bsp_solver** out) {
  BSP_TRY
  BASPACHO_CHECK_NOTNULL(out);
  std::vector<int64_t> ss(spanStart, spanStart + numSpans + 1);
  std::vector<int64_t> l2s(lumpToSpan, lumpToSpan + numLumps + 1);
  std::vector<int64_t> cp(colPtr, colPtr + numLumps + 1);
  std::vector<int64_t> ri(rowInd, rowInd + colPtr[numLumps]);
  std::vector<int64_t> ranges(elimRanges, elimRanges + (elimRanges ? numElimRanges : 0));
  CoalescedBlockMatrixSkel skel(ss, l2s, cp, ri);
  std::unique_ptr<bsp_solver> h(new bsp_solver);
  h->solver.reset(new Solver(std::move(skel), std::move(ranges), {}, hipOps()));
  *out = h.release();
  BSP_CATCH
}

void bsp_destroy_solver(bsp_solver* s) { delete s; }

int64_t bsp_order(const bsp_solver* s) { return s->solver->order(); }
int64_t bsp_data_size(const bsp_solver* s) { return s->solver->dataSize(); }
int64_t bsp_num_spans(const bsp_solver* s) { return s->solver->skel().numSpans(); }
int64_t bsp_num_lumps(const bsp_solver* s) { return s->solver->skel().numLumps(); }
int64_t bsp_can_factor_up_to_span(const bsp_solver* s) { return s->solver->canFactorUpToSpan(); }
int64_t bsp_span_vector_offset(const bsp_solver* s, int64_t span) {
  return s->solver->spanVectorOffset(span);
}
int64_t bsp_span_matrix_offset(const bsp_solver* s, int64_t span, int64_t* out) {
  BSP_TRY
  *out = s->solver->spanMatrixOffset(span);
  BSP_CATCH
}

int bsp_skeleton_array(const bsp_solver* s, int which, const int64_t** data, int64_t* len) {
  BSP_TRY
  const CoalescedBlockMatrixSkel& k = s->solver->skel();
  const std::vector<int64_t>* v = nullptr;
  switch (which) {
    case BSP_SKEL_SPAN_START: v = &k.spanStart; break;
    case BSP_SKEL_SPAN_TO_LUMP: v = &k.spanToLump; break;
    case BSP_SKEL_LUMP_START: v = &k.lumpStart; break;
    case BSP_SKEL_LUMP_TO_SPAN: v = &k.lumpToSpan; break;
    case BSP_SKEL_SPAN_OFFSET_IN_LUMP: v = &k.spanOffsetInLump; break;
    case BSP_SKEL_CHAIN_COL_PTR: v = &k.chainColPtr; break;
    case BSP_SKEL_CHAIN_ROW_SPAN: v = &k.chainRowSpan; break;
    case BSP_SKEL_CHAIN_DATA: v = &k.chainData; break;
    case BSP_SKEL_CHAIN_ROWS_TILL_END: v = &k.chainRowsTillEnd; break;
    case BSP_SKEL_BOARD_COL_PTR: v = &k.boardColPtr; break;
    case BSP_SKEL_BOARD_ROW_LUMP: v = &k.boardRowLump; break;
    case BSP_SKEL_BOARD_CHAIN_COL_ORD: v = &k.boardChainColOrd; break;
    case BSP_SKEL_BOARD_ROW_PTR: v = &k.boardRowPtr; break;
    case BSP_SKEL_BOARD_COL_LUMP: v = &k.boardColLump; break;
    case BSP_SKEL_BOARD_COL_ORD: v = &k.boardColOrd; break;
    case BSP_SKEL_PARAM_TO_SPAN: v = &s->solver->paramToSpan(); break;
    case BSP_SKEL_SPARSE_ELIM_RANGES: v = &s->solver->sparseEliminationRanges(); break;
    default: throw std::runtime_error("bsp_skeleton_array: unknown array id");
  }
  *data = v->data();
  *len = (int64_t)v->size();
  BSP_CATCH
}

int bsp_block_offset(const bsp_solver* s, int64_t rowParam, int64_t colParam, int64_t* offset,
                     int64_t* stride, int32_t* flipped) {
  BSP_TRY
  const int64_t n = s->solver->skel().numSpans();
  BASPACHO_CHECK(rowParam >= 0 && rowParam < n && colParam >= 0 && colParam < n);
  auto acc = s->solver->accessor();
  const int64_t pr = acc.permutation[rowParam], pc = acc.permutation[colParam];
  if (!acc.plainAcc.hasBlock(std::max(pr, pc), std::min(pr, pc))) {
    throw std::runtime_error("bsp_block_offset: block is not in the factor structure");
  }
  auto t = acc.blockOffset(rowParam, colParam);
  *offset = std::get<0>(t);
  *stride = std::get<1>(t);
  *flipped = std::get<2>(t) ? 1 : 0;
  BSP_CATCH
}

int bsp_diag_block_offset(const bsp_solver* s, int64_t param, int64_t* offset, int64_t* stride) {
  BSP_TRY
  BASPACHO_CHECK(param >= 0 && param < s->solver->skel().numSpans());
  auto p = s->solver->accessor().diagBlockOffset(param);
  *offset = p.first;
  *stride = p.second;
  BSP_CATCH
}

int bsp_device_accessor(bsp_solver* s, const int64_t* out[8]) {
  BSP_TRY
  PermutedCoalescedAccessor a = s->solver->deviceAccessor();
  out[0] = a.plainAcc.spanStart;
  out[1] = a.plainAcc.spanToLump;
  out[2] = a.plainAcc.lumpStart;
  out[3] = a.plainAcc.spanOffsetInLump;
  out[4] = a.plainAcc.chainColPtr;
  out[5] = a.plainAcc.chainRowSpan;
  out[6] = a.plainAcc.chainData;
  out[7] = a.permutation;
  BSP_CATCH
}

void bsp_set_stream(bsp_solver* s, void* stream) { s->solver->setStream(stream); }

int bsp_factor_f64(bsp_solver* s, double* d) {
  BSP_TRY
  s->solver->factor(d);
  BSP_CATCH
}
int bsp_factor_f32(bsp_solver* s, float* d) {
  BSP_TRY
  s->solver->factor(d);
  BSP_CATCH
}
int bsp_factor_batched_f64(bsp_solver* s, double* const* ptrs, int32_t batch) {
  BSP_TRY
  std::vector<double*> v(ptrs, ptrs + batch);
  s->solver->factor(&v);
  BSP_CATCH
}
int bsp_factor_batched_f32(bsp_solver* s, float* const* ptrs, int32_t batch) {
  BSP_TRY
  std::vector<float*> v(ptrs, ptrs + batch);
  s->solver->factor(&v);
  BSP_CATCH
}
int bsp_factor_up_to_f64(bsp_solver* s, double* d, int64_t span) {
  BSP_TRY
  s->solver->factorUpTo(d, span);
  BSP_CATCH
}
int bsp_factor_from_f64(bsp_solver* s, double* d, int64_t span) {
  BSP_TRY
  s->solver->factorFrom(d, span);
  BSP_CATCH
}
int bsp_factor_up_to_f32(bsp_solver* s, float* d, int64_t span) {
  BSP_TRY
  s->solver->factorUpTo(d, span);
  BSP_CATCH
}
int bsp_factor_from_f32(bsp_solver* s, float* d, int64_t span) {
  BSP_TRY
  s->solver->factorFrom(d, span);
  BSP_CATCH
}

template <typename T>
static void factorPerOp(bsp_solver* s, T* d) {
  SymbolicCtx& sym = s->solver->internalSymbolicContext();
  hipBackendForcePerOp(sym, true);
  try {
    s->solver->factor(d);
  } catch (...) {
    hipBackendForcePerOp(sym, false);
    throw;
  }
  hipBackendForcePerOp(sym, false);
}
int bsp_factor_per_op_f64(bsp_solver* s, double* d) {
  BSP_TRY
  factorPerOp(s, d);
  BSP_CATCH
}
int bsp_factor_per_op_f32(bsp_solver* s, float* d) {
  BSP_TRY
  factorPerOp(s, d);
  BSP_CATCH
}

int bsp_collect_op_stats(bsp_solver* s, int32_t on) {
  BSP_TRY
  SymbolicCtx& sym = s->solver->internalSymbolicContext();
  s->solver->enableStats(on != 0);
  s->solver->resetStats();
  for (OpStat* st : {&sym.potrfStat, &sym.trsmStat, &sym.sygeStat, &sym.asmblStat}) st->keepSamples = on != 0;
  BSP_CATCH
}
int bsp_read_op_stats(bsp_solver* s, int32_t which, double* out, int64_t capacity, int64_t* count) {
  BSP_TRY
  SymbolicCtx& sym = s->solver->internalSymbolicContext();
  const OpStat* sts[4] = {&sym.potrfStat, &sym.trsmStat, &sym.sygeStat, &sym.asmblStat};
  BASPACHO_CHECK(which >= 0 && which < 4);
  const auto& v = sts[which]->samples;
  *count = (int64_t)v.size();
  for (int64_t i = 0; i < std::min<int64_t>(capacity, (int64_t)v.size()); i++) {
    for (int j = 0; j < 4; j++) out[4 * i + j] = v[i][j];
  }
  BSP_CATCH
}

int bsp_force_per_op(bsp_solver* s, int32_t on) {
  BSP_TRY
  hipBackendForcePerOp(s->solver->internalSymbolicContext(), on != 0);
  BSP_CATCH
}

int bsp_test_read_sweep_trace(bsp_solver* s, long long* out, int32_t max_blocks, int32_t* n_blocks) {
  BSP_TRY
  *n_blocks = hipBackendReadSweepTrace(s->solver->internalSymbolicContext(), out, max_blocks);
  BSP_CATCH
}

int bsp_test_set_fault(bsp_solver* s, int32_t kind) {
  BSP_TRY
  hipBackendSetFault(s->solver->internalSymbolicContext(), kind);
  BSP_CATCH
}

static int selinvPlanRecords(const bsp_solver* s, bool upTo, int64_t span, int64_t* buf, int64_t capacity,
                             int64_t* needed);
int bsp_test_selinv_plan(const bsp_solver* s, int64_t* buf, int64_t capacity, int64_t* needed) {
  return selinvPlanRecords(s, false, 0, buf, capacity, needed);
}
int bsp_test_selinv_plan_up_to(const bsp_solver* s, int64_t span, int64_t* buf, int64_t capacity, int64_t* needed) {
  return selinvPlanRecords(s, true, span, buf, capacity, needed);
}
// the complete plan, or (upTo) the plan of the lumps before the cut at `span`
static int selinvPlanRecords(const bsp_solver* s, bool upTo, int64_t span, int64_t* buf, int64_t capacity,
                             int64_t* needed) {
  BSP_TRY
  const CoalescedBlockMatrixSkel& sk = s->solver->skel();
  const SelInvPlanHost p =
      upTo ? buildSelInvPlan(sk, s->solver->partialCutLump("bsp_test_selinv_plan_up_to", span)) : buildSelInvPlan(sk);
  std::unordered_map<int64_t, int64_t> lumpOfOff;  // data offset of a lump column -> lump
  for (int64_t l = 0; l < sk.numLumps(); l++) lumpOfOff[sk.chainData[sk.chainColPtr[l]]] = l;
  std::vector<int64_t> out = {(int64_t)p.levels.size(), (int64_t)p.smalls.size(), (int64_t)p.nodes.size(),
                              p.linvElems, p.uElems, p.pElems, p.wElems};
  for (int64_t lv = 0; lv < (int64_t)p.levels.size(); lv++) {
    const SelInvLevel& L = p.levels[lv];
    for (int64_t i = L.smallBegin; i < L.smallEnd; i++) {
      const SelInvSmall& q = p.smalls[i];
      out.insert(out.end(), {lumpOfOff.at(q.diagOff), lv, (int64_t)q.n, (int64_t)q.r, (int64_t)q.k});
    }
  }
  for (int64_t lv = 0; lv < (int64_t)p.levels.size(); lv++) {
    const SelInvLevel& L = p.levels[lv];
    for (int64_t i = L.nodeBegin; i < L.nodeEnd; i++) {
      const SelInvNode& q = p.nodes[i];
      out.insert(out.end(), {lumpOfOff.at(q.lumpOff), lv, (int64_t)q.c0, (int64_t)q.w, (int64_t)q.r,
                             (int64_t)q.nRest, (int64_t)q.kChunk, (int64_t)q.nk, (int64_t)q.nTiles,
                             (int64_t)q.tileBase});
    }
  }
  *needed = (int64_t)out.size();
  if (buf != nullptr) std::copy(out.begin(), out.begin() + std::min(capacity, *needed), buf);
  BSP_CATCH
}

static void copyRecords(const std::vector<int64_t>& out, int64_t* buf, int64_t capacity, int64_t* needed) {
  *needed = (int64_t)out.size();
  if (buf != nullptr) std::copy(out.begin(), out.begin() + std::min(capacity, *needed), buf);
}
int bsp_test_launch_tables(const bsp_solver* s, int64_t* buf, int64_t capacity, int64_t* needed) {
  BSP_TRY
  copyRecords(hipBackendLaunchTableRecords(s->solver->internalSymbolicContext()), buf, capacity, needed);
  BSP_CATCH
}
int bsp_test_solve_schedule(const bsp_solver* s, int32_t with_sweeps, int32_t block_solve, int32_t inverses,
                            int32_t sweep_min_width, int64_t* buf, int64_t capacity, int64_t* needed) {
  BSP_TRY
  copyRecords(hipBackendSolveScheduleRecords(s->solver->internalSymbolicContext(), with_sweeps != 0, block_solve != 0,
                                             inverses != 0, sweep_min_width),
              buf, capacity, needed);
  BSP_CATCH
}

template <typename T>
static void doElim(bsp_solver* s, T* d, int64_t idx) {
  const auto& ranges = s->solver->sparseEliminationRanges();
  BASPACHO_CHECK(idx >= 0 && idx + 1 < (int64_t)ranges.size());
  NumericCtxPtr<T> ctx = s->solver->internalSymbolicContext().createNumericCtx<T>(0, d);
  ctx->doElimination(s->solver->internalGetElimCtx((size_t)idx), d, ranges[idx], ranges[idx + 1]);
}
int bsp_do_elimination_f64(bsp_solver* s, double* d, int64_t idx) {
  BSP_TRY
  doElim(s, d, idx);
  BSP_CATCH
}
int bsp_do_elimination_f32(bsp_solver* s, float* d, int64_t idx) {
  BSP_TRY
  doElim(s, d, idx);
  BSP_CATCH
}

int bsp_solve_f64(bsp_solver* s, const double* m, double* v, int64_t stride, int32_t nrhs) {
  BSP_TRY
  s->solver->solve(m, v, stride, nrhs);
  BSP_CATCH
}
int bsp_solve_l_f64(bsp_solver* s, const double* m, double* v, int64_t stride, int32_t nrhs) {
  BSP_TRY
  s->solver->solveL(m, v, stride, nrhs);
  BSP_CATCH
}
int bsp_solve_lt_f64(bsp_solver* s, const double* m, double* v, int64_t stride, int32_t nrhs) {
  BSP_TRY
  s->solver->solveLt(m, v, stride, nrhs);
  BSP_CATCH
}
int bsp_solve_f32(bsp_solver* s, const float* m, float* v, int64_t stride, int32_t nrhs) {
  BSP_TRY
  s->solver->solve(m, v, stride, nrhs);
  BSP_CATCH
}
int bsp_solve_l_f32(bsp_solver* s, const float* m, float* v, int64_t stride, int32_t nrhs) {
  BSP_TRY
  s->solver->solveL(m, v, stride, nrhs);
  BSP_CATCH
}
int bsp_solve_lt_f32(bsp_solver* s, const float* m, float* v, int64_t stride, int32_t nrhs) {
  BSP_TRY
  s->solver->solveLt(m, v, stride, nrhs);
  BSP_CATCH
}

// partial solves: which = 0 solveLUpTo, 1 solveLtUpTo, 2 solveLFrom, 3 solveLtFrom
template <typename T>
static void solvePartial(bsp_solver* s, const T* m, T* v, int64_t stride, int32_t nrhs,
                         int32_t which, int64_t span) {
  if (which == 0) {
    s->solver->solveLUpTo(m, span, v, stride, nrhs);
  } else if (which == 1) {
    s->solver->solveLtUpTo(m, span, v, stride, nrhs);
  } else if (which == 2) {
    s->solver->solveLFrom(m, span, v, stride, nrhs);
  } else if (which == 3) {
    s->solver->solveLtFrom(m, span, v, stride, nrhs);
  } else {
    throw std::runtime_error("bsp_solve_partial: which must be 0..3");
  }
}
int bsp_solve_partial_f64(bsp_solver* s, const double* m, double* v, int64_t stride, int32_t nrhs,
                          int32_t which, int64_t span) {
  BSP_TRY
  solvePartial<double>(s, m, v, stride, nrhs, which, span);
  BSP_CATCH
}
int bsp_solve_partial_f32(bsp_solver* s, const float* m, float* v, int64_t stride, int32_t nrhs,
                          int32_t which, int64_t span) {
  BSP_TRY
  solvePartial<float>(s, m, v, stride, nrhs, which, span);
  BSP_CATCH
}

int bsp_add_mv_from_f64(bsp_solver* s, const double* m, int64_t span, const double* in,
                        int64_t in_stride, double* out, int64_t out_stride, int32_t nrhs,
                        double alpha) {
  BSP_TRY
  s->solver->addMvFrom(m, span, in, in_stride, out, out_stride, nrhs, alpha);
  BSP_CATCH
}
int bsp_add_mv_from_f32(bsp_solver* s, const float* m, int64_t span, const float* in,
                        int64_t in_stride, float* out, int64_t out_stride, int32_t nrhs,
                        float alpha) {
  BSP_TRY
  s->solver->addMvFrom(m, span, in, in_stride, out, out_stride, nrhs, alpha);
  BSP_CATCH
}
// ---- extension operations: single and batched entry of every operation, once per dtype -------------
// the `batch` device pointers of a batched entry as a vector of P (T* or const T*), checked first.
// `name` says which array it is; NULL: the operation's message does not tell its arrays apart
template <typename P, typename T>
static std::vector<P> hostArray(const std::string& what, const char* name, const T* const* p, int32_t batch) {
  if (batch <= 0) throw std::runtime_error(what + ": the batch is empty (batch = " + std::to_string(batch) + ")");
  if (p == nullptr) {
    throw std::runtime_error(what + (name ? std::string(": the array of ") + name + " pointers" : ": an array of pointers") +
                             " is NULL");
  }
  std::vector<P> v(batch);
  for (int32_t q = 0; q < batch; q++) v[q] = const_cast<P>(p[q]);
  return v;
}
template <typename T>
static void selectedInverseBatched(bsp_solver* s, T* const* ptrs, int32_t batch) {
  std::vector<T*> v = hostArray<T*>("selectedInverse", "data", ptrs, batch);
  s->solver->selectedInverse(&v);
}
template <typename T>
static void logDetBatched(bsp_solver* s, const T* const* ptrs, T* out, int32_t batch) {
  s->solver->logDet(hostArray<T*>("logDet", "factor", ptrs, batch), out);
}
template <typename T>
static void patternGradBatched(bsp_solver* s, const T* const* z, const T* zs, const T* const* u,
                               const T* const* v, int64_t stride, int32_t nrhs, T alpha, T* const* out,
                               int32_t batch) {
  const char* what = "patternGrad";
  const std::vector<T*> o = hostArray<T*>(what, "output", out, batch);
  if ((u == nullptr) != (v == nullptr)) throw std::runtime_error("patternGrad: U and V must be given together");
  const auto opt = [&](const char* name, const T* const* p) {  // an array that was not given: no members
    return p ? hostArray<T*>(what, name, p, batch) : std::vector<T*>{};
  };
  s->solver->patternGrad(opt("Z", z), zs, opt("U", u), opt("V", v), stride, nrhs, alpha, o);
}
template <typename T>
static void patternOuterBatched(bsp_solver* s, const T* const* u, const T* const* v, int64_t stride, int32_t nrhs,
                                T alpha, T* const* out, int32_t batch) {
  const char* what = "patternOuter";
  const std::vector<T*> o = hostArray<T*>(what, "output", out, batch);
  s->solver->patternOuter(hostArray<T*>(what, "U", u, batch), hostArray<T*>(what, "V", v, batch), stride, nrhs, alpha,
                          o);
}
template <typename T>
static void factorAdjointBatched(bsp_solver* s, const T* const* l, T* const* grad, int32_t batch) {
  const char* what = "factorAdjoint";
  const std::vector<T*> g = hostArray<T*>(what, "gradient", grad, batch);
  s->solver->factorAdjoint(hostArray<T*>(what, "factor", l, batch), g);
}
template <typename T>
static void selectedInverseAdjointBatched(bsp_solver* s, const T* const* l, const T* const* z, T* const* grad,
                                          int32_t batch) {
  const char* what = "selectedInverseAdjoint";
  const std::vector<T*> g = hostArray<T*>(what, "gradient", grad, batch);
  const std::vector<T*> lv = hostArray<T*>(what, "factor", l, batch);
  s->solver->selectedInverseAdjoint(lv, hostArray<T*>(what, "Z", z, batch), g);
}
template <typename T>
static void factorAdjointUpToBatched(bsp_solver* s, const T* const* p, T* const* grad, int32_t batch, int64_t span) {
  const char* what = "factorAdjointUpTo";
  const std::vector<T*> g = hostArray<T*>(what, "gradient", grad, batch);
  s->solver->factorAdjointUpTo(hostArray<T*>(what, "factor", p, batch), g, span);
}
template <typename T>
static void schurDenseBatched(bsp_solver* s, const T* const* in, int64_t span, T* const* out, const int32_t* dest,
                              int32_t batch, bool toDense) {
  const char* what = toDense ? "schurComplement" : "schurComplementAdjoint";
  const std::vector<T*> o = hostArray<T*>(what, "output", out, batch);
  const std::vector<T*> i = hostArray<T*>(what, "input", in, batch);
  if (toDense) {
    s->solver->schurComplement(i, span, o, dest);
  } else {
    s->solver->schurComplementAdjoint(i, span, o, dest);
  }
}
template <typename T>
static void factorStatusBatched(bsp_solver* s, const T* const* ptrs, int64_t b, int64_t e, int64_t* out, int32_t batch) {
  s->solver->factorStatus(hostArray<T*>("factorStatus", "data", ptrs, batch), b, e, out);
}
template <typename T>
static void dampBatched(bsp_solver* s, T* const* ptrs, int64_t b, int64_t e, const T* ab, int32_t batch) {
  s->solver->dampDiagonal(hostArray<T*>("dampDiagonal", "data", ptrs, batch), b, e, ab);
}
#define BSP_STATUS_API(SFX, T)                                                                                   \
  int bsp_factor_status_##SFX(bsp_solver* s, const T* d, int64_t b, int64_t e, int64_t* out)                     \
      BSP_BODY(s->solver->factorStatus(d, b, e, out))                                                            \
  int bsp_factor_status_batched_##SFX(bsp_solver* s, const T* const* d, int64_t b, int64_t e, int64_t* out,      \
                                      int32_t batch) BSP_BODY(factorStatusBatched(s, d, b, e, out, batch))       \
  int bsp_damp_##SFX(bsp_solver* s, T* d, int64_t b, int64_t e, const T* ab)                                     \
      BSP_BODY(s->solver->dampDiagonal(d, b, e, ab))                                                             \
  int bsp_damp_batched_##SFX(bsp_solver* s, T* const* d, int64_t b, int64_t e, const T* ab, int32_t batch)       \
      BSP_BODY(dampBatched(s, d, b, e, ab, batch))
BSP_STATUS_API(f64, double)
BSP_STATUS_API(f32, float)
#undef BSP_STATUS_API
#define BSP_PATTERN_API(SFX, T)                                                                                  \
  int bsp_selected_inverse_##SFX(bsp_solver* s, T* d) BSP_BODY(s->solver->selectedInverse(d))                    \
  int bsp_selected_inverse_batched_##SFX(bsp_solver* s, T* const* ptrs, int32_t batch)                           \
      BSP_BODY(selectedInverseBatched(s, ptrs, batch))                                                           \
  int bsp_log_det_##SFX(bsp_solver* s, const T* f, T* out) BSP_BODY(s->solver->logDet(f, out))                   \
  int bsp_log_det_batched_##SFX(bsp_solver* s, const T* const* f, T* out, int32_t batch)                         \
      BSP_BODY(logDetBatched(s, f, out, batch))                                                                  \
  int bsp_pattern_grad_##SFX(bsp_solver* s, const T* z, const T* zs, const T* u, const T* v, int64_t stride,     \
                             int32_t nrhs, T alpha, T* out)                                                      \
      BSP_BODY(s->solver->patternGrad(z, zs, u, v, stride, nrhs, alpha, out))                                    \
  int bsp_pattern_grad_batched_##SFX(bsp_solver* s, const T* const* z, const T* zs, const T* const* u,           \
                                     const T* const* v, int64_t stride, int32_t nrhs, T alpha, T* const* out,    \
                                     int32_t batch)                                                              \
      BSP_BODY(patternGradBatched(s, z, zs, u, v, stride, nrhs, alpha, out, batch))                              \
  int bsp_pattern_outer_##SFX(bsp_solver* s, const T* u, const T* v, int64_t stride, int32_t nrhs, T alpha,      \
                              T* out) BSP_BODY(s->solver->patternOuter(u, v, stride, nrhs, alpha, out))          \
  int bsp_pattern_outer_batched_##SFX(bsp_solver* s, const T* const* u, const T* const* v, int64_t stride,       \
                                      int32_t nrhs, T alpha, T* const* out, int32_t batch)                       \
      BSP_BODY(patternOuterBatched(s, u, v, stride, nrhs, alpha, out, batch))                                    \
  int bsp_factor_adjoint_##SFX(bsp_solver* s, const T* l, T* grad) BSP_BODY(s->solver->factorAdjoint(l, grad))   \
  int bsp_factor_adjoint_batched_##SFX(bsp_solver* s, const T* const* l, T* const* grad, int32_t batch)          \
      BSP_BODY(factorAdjointBatched(s, l, grad, batch))                                                          \
  int bsp_selected_inverse_adjoint_##SFX(bsp_solver* s, const T* l, const T* z, T* grad)                         \
      BSP_BODY(s->solver->selectedInverseAdjoint(l, z, grad))                                                    \
  int bsp_selected_inverse_adjoint_batched_##SFX(bsp_solver* s, const T* const* l, const T* const* z,            \
                                                 T* const* grad, int32_t batch)                                  \
      BSP_BODY(selectedInverseAdjointBatched(s, l, z, grad, batch))
BSP_PATTERN_API(f64, double)
BSP_PATTERN_API(f32, float)
#undef BSP_PATTERN_API
// ---- blocks of A^-1 by reach solves ---------------------------------------------------------------
static std::vector<int64_t> hostIds(const char* what, const char* name, const int64_t* p, int64_t n) {
  if (n < 0) throw std::runtime_error(std::string(what) + ": the number of " + name + " is negative");
  if (n > 0 && p == nullptr) throw std::runtime_error(std::string(what) + ": the array of " + name + " is NULL");
  return std::vector<int64_t>(p, p + n);
}
#define BSP_REACH_API(SFX, T)                                                                                    \
  int bsp_reach_solve_l_##SFX(bsp_solver* s, const T* l, int64_t n, const int64_t* params, T* w)                 \
      BSP_BODY(s->solver->reachSolveL(l, hostIds("reachSolveL", "params", params, n), w))                        \
  int bsp_inverse_blocks_##SFX(bsp_solver* s, const T* l, int64_t n, const int64_t* rp, const int64_t* cp,       \
                               T* out, const int64_t* offs)                                                      \
      BSP_BODY(s->solver->inverseBlocks(l, hostIds("inverseBlocks", "row params", rp, n),                        \
                                        hostIds("inverseBlocks", "column params", cp, n), out,                   \
                                        hostIds("inverseBlocks", "output offsets", offs, n < 0 ? n : n + 1)))
BSP_REACH_API(f64, double)
BSP_REACH_API(f32, float)
#undef BSP_REACH_API

// ---- products with the factor -------------------------------------------------------------------------
// which = 0: mulL, 1: mulLt, on one member (L, In, Out pointers) or a batch (vectors of them)
template <typename L, typename In, typename Out>
static void factorProduct(bsp_solver* s, const L& l, int32_t which, const In& in, int64_t inStride, const Out& out,
                          int64_t outStride, int32_t nrhs) {
  if (which == 0) {
    s->solver->mulL(l, in, inStride, out, outStride, nrhs);
  } else if (which == 1) {
    s->solver->mulLt(l, in, inStride, out, outStride, nrhs);
  } else {
    throw std::runtime_error("factorProduct: which = " + std::to_string(which) + " is neither 0 (L x) nor 1 (L^T x)");
  }
}
template <typename T>
static void factorProductBatched(bsp_solver* s, const T* const* l, int32_t which, const T* const* in, int64_t inStride,
                                 T* const* out, int64_t outStride, int32_t nrhs, int32_t batch) {
  const char* what = "factorProduct";
  const std::vector<T*> o = hostArray<T*>(what, "output", out, batch);
  const std::vector<T*> i = hostArray<T*>(what, "input", in, batch);
  factorProduct(s, hostArray<T*>(what, "factor", l, batch), which, i, inStride, o, outStride, nrhs);
}
#define BSP_FACTOR_PRODUCT_API(SFX, T)                                                                           \
  int bsp_factor_product_##SFX(bsp_solver* s, const T* l, int32_t which, const T* in, int64_t in_stride, T* out, \
                               int64_t out_stride, int32_t nrhs)                                                 \
      BSP_BODY(factorProduct(s, l, which, in, in_stride, out, out_stride, nrhs))                                 \
  int bsp_factor_product_batched_##SFX(bsp_solver* s, const T* const* l, int32_t which, const T* const* in,      \
                                       int64_t in_stride, T* const* out, int64_t out_stride, int32_t nrhs,       \
                                       int32_t batch)                                                            \
      BSP_BODY(factorProductBatched<T>(s, l, which, in, in_stride, out, out_stride, nrhs, batch))
BSP_FACTOR_PRODUCT_API(f64, double)
BSP_FACTOR_PRODUCT_API(f32, float)
#undef BSP_FACTOR_PRODUCT_API

int bsp_test_factor_product_plan(const bsp_solver* s, int64_t* buf, int64_t capacity, int64_t* needed) {
  BSP_TRY
  const std::vector<int64_t> out = factorProductPlanRecords(buildFactorProductPlan(s->solver->skel()));
  *needed = (int64_t)out.size();
  if (buf != nullptr) std::copy(out.begin(), out.begin() + std::min(capacity, *needed), buf);
  BSP_CATCH
}

// the reach plan of `params` (caller's ids) with one Gram item per pair i >= j of them
int bsp_test_reach_plan(const bsp_solver* s, int64_t num_params, const int64_t* params, int64_t* buf,
                        int64_t capacity, int64_t* needed) {
  BSP_TRY
  const std::vector<int64_t> prm = hostIds("bsp_test_reach_plan", "params", params, num_params);
  std::vector<int64_t> pr, pc;
  for (int64_t i = 0; i < num_params; i++) {
    for (int64_t j = 0; j <= i; j++) {
      pr.push_back(i);
      pc.push_back(j);
    }
  }
  const ReachPlan p = s->solver->reachPlan("bsp_test_reach_plan", prm, pr, pc);
  std::vector<int64_t> out = {p.cutLump, p.cutSpan, p.numCols, (int64_t)p.querySpan.size(), (int64_t)p.groups.size(),
                              (int64_t)p.items.size(), (int64_t)p.unitCol.size()};
  for (size_t q = 0; q < p.querySpan.size(); q++) {
    out.insert(out.end(), {p.querySpan[q], p.queryLump[q], p.queryCol0[q], p.queryWidth[q],
                           (int64_t)(p.queryListEnd[q] - p.queryListBegin[q])});
    for (int32_t i = p.queryListBegin[q]; i < p.queryListEnd[q]; i++) out.push_back(p.reachLumps[i]);
  }
  for (const ReachGroup& g : p.groups) {
    out.insert(out.end(), {(int64_t)g.query, (int64_t)g.col0, (int64_t)g.k, g.row0, (int64_t)(g.listEnd - g.listBegin),
                           g.listEnd > g.listBegin ? (int64_t)p.reachLumps[g.listBegin] : -1});
  }
  for (size_t k = 0; k < p.items.size(); k++) {
    const GramItem& it = p.items[k];
    out.insert(out.end(), {pr[k], pc[k], (int64_t)it.colP, (int64_t)it.nP, (int64_t)it.colQ, (int64_t)it.nQ, it.outOff,
                           it.rows, (int64_t)(it.rangeEnd - it.rangeBegin)});
    for (int32_t r = it.rangeBegin; r < it.rangeEnd; r++) {
      const int64_t len = (r + 1 < it.rangeEnd ? p.rangePrefix[r + 1] : it.rows) - p.rangePrefix[r];
      out.insert(out.end(), {p.rangeStart[r], p.rangeStart[r] + len});
    }
  }
  for (size_t i = 0; i < p.unitCol.size(); i++) out.insert(out.end(), {p.unitCol[i], p.unitRow[i]});
  *needed = (int64_t)out.size();
  if (buf != nullptr) std::copy(out.begin(), out.begin() + std::min(capacity, *needed), buf);
  BSP_CATCH
}

#define BSP_PARTIAL_ADJOINT_API(SFX, T)                                                                          \
  int bsp_factor_adjoint_up_to_##SFX(bsp_solver* s, const T* p, T* grad, int64_t span)                           \
      BSP_BODY(s->solver->factorAdjointUpTo(p, grad, span))                                                      \
  int bsp_factor_adjoint_up_to_batched_##SFX(bsp_solver* s, const T* const* p, T* const* grad, int32_t batch,    \
                                             int64_t span)                                                       \
      BSP_BODY(factorAdjointUpToBatched(s, p, grad, batch, span))                                                \
  int bsp_schur_to_dense_##SFX(bsp_solver* s, const T* p, int64_t span, T* out, const int32_t* dest)             \
      BSP_BODY(s->solver->schurComplement(p, span, out, dest))                                                   \
  int bsp_schur_to_dense_batched_##SFX(bsp_solver* s, const T* const* p, int64_t span, T* const* out,            \
                                       const int32_t* dest, int32_t batch)                                       \
      BSP_BODY(schurDenseBatched(s, p, span, out, dest, batch, true))                                            \
  int bsp_schur_from_dense_##SFX(bsp_solver* s, const T* gd, int64_t span, T* grad, const int32_t* dest)         \
      BSP_BODY(s->solver->schurComplementAdjoint(gd, span, grad, dest))                                          \
  int bsp_schur_from_dense_batched_##SFX(bsp_solver* s, const T* const* gd, int64_t span, T* const* grad,        \
                                         const int32_t* dest, int32_t batch)                                     \
      BSP_BODY(schurDenseBatched(s, gd, span, grad, dest, batch, false))
BSP_PARTIAL_ADJOINT_API(f64, double)
BSP_PARTIAL_ADJOINT_API(f32, float)
#undef BSP_PARTIAL_ADJOINT_API
struct bsp_assembly {
  std::unique_ptr<AssemblyMap> map;
};

int bsp_assembly_create(bsp_solver* s, int64_t nnz, const int64_t* rows, const int64_t* cols, int32_t triangle,
                        bsp_assembly** out) {
  BSP_TRY
  if (s == nullptr || out == nullptr) throw std::runtime_error("bsp_assembly_create: NULL solver or output");
  std::unique_ptr<bsp_assembly> a(new bsp_assembly);
  a->map = createAssemblyMap(*s->solver, nnz, rows, cols, triangle);
  *out = a.release();
  BSP_CATCH
}
void bsp_assembly_destroy(bsp_assembly* a) { delete a; }
int bsp_assembly_entry_offsets(const bsp_assembly* a, int64_t* out) {
  BSP_TRY
  if (a == nullptr) throw std::runtime_error("bsp_assembly_entry_offsets: the assembly is NULL");
  if (a->map->nnz > 0 && out == nullptr) throw std::runtime_error("bsp_assembly_entry_offsets: out is NULL");
  std::copy(a->map->entryOff.begin(), a->map->entryOff.end(), out);
  BSP_CATCH
}
int bsp_assembly_info(const bsp_assembly* a, int64_t out[7]) {
  BSP_TRY
  if (a == nullptr || out == nullptr) throw std::runtime_error("bsp_assembly_info: NULL argument");
  const AssemblyMap& m = *a->map;
  const int64_t v[7] = {m.nnz, m.numKept(), (int64_t)m.tiles.dest.size(), m.tiles.maxRun,
                        (int64_t)m.tiles.longDest.size(), m.numTiles, m.deviceBytes()};
  std::copy(v, v + 7, out);
  BSP_CATCH
}
static const AssemblyMap& assemblyOf(const bsp_assembly* a) {
  if (a == nullptr) throw std::runtime_error("assemble: the assembly is NULL");
  return *a->map;
}
template <typename T>
static void assembleBatched(bsp_solver* s, const bsp_assembly* a, const T* const* in, T* const* out,
                            int32_t batch, bool adjoint) {
  const char* what = adjoint ? "assembleAdjoint" : "assemble";
  const std::vector<const T*> i = hostArray<const T*>(what, nullptr, in, batch);
  const std::vector<T*> o = hostArray<T*>(what, nullptr, out, batch);
  if (adjoint) {
    s->solver->assembleAdjoint(assemblyOf(a), i, o);
  } else {
    s->solver->assemble(assemblyOf(a), i, o);
  }
}
#define BSP_ASSEMBLY_API(SFX, T)                                                                                 \
  int bsp_assemble_##SFX(bsp_solver* s, const bsp_assembly* a, const T* v, T* d)                                 \
      BSP_BODY(s->solver->assemble(assemblyOf(a), v, d))                                                         \
  int bsp_assemble_batched_##SFX(bsp_solver* s, const bsp_assembly* a, const T* const* v, T* const* d,           \
                                 int32_t batch) BSP_BODY(assembleBatched(s, a, v, d, batch, false))              \
  int bsp_assemble_adjoint_##SFX(bsp_solver* s, const bsp_assembly* a, const T* g, T* gv)                        \
      BSP_BODY(s->solver->assembleAdjoint(assemblyOf(a), g, gv))                                                 \
  int bsp_assemble_adjoint_batched_##SFX(bsp_solver* s, const bsp_assembly* a, const T* const* g, T* const* gv,  \
                                         int32_t batch) BSP_BODY(assembleBatched(s, a, g, gv, batch, true))
BSP_ASSEMBLY_API(f64, double)
BSP_ASSEMBLY_API(f32, float)
#undef BSP_ASSEMBLY_API
struct bsp_normal_eq {
  std::unique_ptr<NormalEqMap> map;
};

int bsp_normal_eq_create(bsp_solver* s, int64_t m, int64_t nnz, const int64_t* rows, const int64_t* cols,
                         bsp_normal_eq** out) {
  BSP_TRY
  if (s == nullptr || out == nullptr) throw std::runtime_error("bsp_normal_eq_create: NULL solver or output");
  std::unique_ptr<bsp_normal_eq> e(new bsp_normal_eq);
  e->map = createNormalEqMap(*s->solver, m, nnz, rows, cols);
  *out = e.release();
  BSP_CATCH
}
void bsp_normal_eq_destroy(bsp_normal_eq* e) { delete e; }
int bsp_normal_eq_info(const bsp_normal_eq* e, int64_t out[10]) {
  BSP_TRY
  if (e == nullptr || out == nullptr) throw std::runtime_error("bsp_normal_eq_info: NULL argument");
  const NormalEqMap& m = *e->map;
  const int64_t v[10] = {m.nnz, m.numPairs, (int64_t)m.tiles.dest.size(), m.tiles.maxRun,
                         (int64_t)m.tiles.longDest.size(), m.numTiles, m.forwardDeviceBytes(), m.adjointDeviceBytes(),
                         m.vectorDeviceBytes(), m.numAdjointTerms()};
  std::copy(v, v + 10, out);
  BSP_CATCH
}
int bsp_normal_eq_pair_table(const bsp_normal_eq* e, int32_t* ka, int32_t* kb, int64_t* offset) {
  BSP_TRY
  if (e == nullptr) throw std::runtime_error("bsp_normal_eq_pair_table: the map is NULL");
  const NormalEqMap& m = *e->map;
  if (m.numPairs > 0 && (ka == nullptr || kb == nullptr || offset == nullptr)) {
    throw std::runtime_error("bsp_normal_eq_pair_table: an output array is NULL");
  }
  std::copy(m.pairA.begin(), m.pairA.end(), ka);
  std::copy(m.pairB.begin(), m.pairB.end(), kb);
  for (size_t u = 0; u < m.tiles.dest.size(); u++) {
    std::fill(offset + m.tiles.runStart[u], offset + m.tiles.runStart[u + 1], m.tiles.dest[u]);
  }
  BSP_CATCH
}
template <typename T>
static void normalEqRun(bsp_solver* s, const bsp_normal_eq* e, int32_t op, const T* const* values, const T* const* x,
                        T* const* out, int64_t q, int32_t batch, bool single) {
  static const char* names[4] = {"normalEqHessian", "normalEqHessianAdjoint", "normalEqJtVec", "normalEqJVec"};
  const std::string what = names[op];
  if (s == nullptr) throw std::runtime_error(what + ": the solver is NULL");
  if (e == nullptr) throw std::runtime_error(what + ": the map is NULL");
  const bool hasX = op != NormalEqHessian;
  const std::vector<const T*> v = hostArray<const T*>(what, nullptr, values, batch);
  const std::vector<T*> o = hostArray<T*>(what, nullptr, out, batch);
  const std::vector<const T*> xs = hasX ? hostArray<const T*>(what, nullptr, x, batch) : std::vector<const T*>{};
  s->solver->normalEq<T>(*e->map, op, v, xs, o, q, single);
}
#define BSP_NORMAL_EQ_API(SFX, T)                                                                                \
  int bsp_normal_eq_hessian_##SFX(bsp_solver* s, const bsp_normal_eq* e, const T* v, T* d)                       \
      BSP_BODY(normalEqRun<T>(s, e, NormalEqHessian, &v, nullptr, &d, 0, 1, true))                               \
  int bsp_normal_eq_hessian_batched_##SFX(bsp_solver* s, const bsp_normal_eq* e, const T* const* v, T* const* d, \
                                          int32_t batch)                                                         \
      BSP_BODY(normalEqRun<T>(s, e, NormalEqHessian, v, nullptr, d, 0, batch, false))                            \
  int bsp_normal_eq_hessian_adjoint_##SFX(bsp_solver* s, const bsp_normal_eq* e, const T* v, const T* g, T* gv)  \
      BSP_BODY(normalEqRun<T>(s, e, NormalEqAdjoint, &v, &g, &gv, 0, 1, true))                                   \
  int bsp_normal_eq_hessian_adjoint_batched_##SFX(bsp_solver* s, const bsp_normal_eq* e, const T* const* v,      \
                                                  const T* const* g, T* const* gv, int32_t batch)                \
      BSP_BODY(normalEqRun<T>(s, e, NormalEqAdjoint, v, g, gv, 0, batch, false))                                 \
  int bsp_normal_eq_jt_vec_##SFX(bsp_solver* s, const bsp_normal_eq* e, const T* v, const T* r, int64_t q,       \
                                 T* out) BSP_BODY(normalEqRun<T>(s, e, NormalEqJtVec, &v, &r, &out, q, 1, true)) \
  int bsp_normal_eq_jt_vec_batched_##SFX(bsp_solver* s, const bsp_normal_eq* e, const T* const* v,               \
                                         const T* const* r, int64_t q, T* const* out, int32_t batch)             \
      BSP_BODY(normalEqRun<T>(s, e, NormalEqJtVec, v, r, out, q, batch, false))                                  \
  int bsp_normal_eq_j_vec_##SFX(bsp_solver* s, const bsp_normal_eq* e, const T* v, const T* x, int64_t q,        \
                                T* out) BSP_BODY(normalEqRun<T>(s, e, NormalEqJVec, &v, &x, &out, q, 1, true))   \
  int bsp_normal_eq_j_vec_batched_##SFX(bsp_solver* s, const bsp_normal_eq* e, const T* const* v,                \
                                        const T* const* x, int64_t q, T* const* out, int32_t batch)              \
      BSP_BODY(normalEqRun<T>(s, e, NormalEqJVec, v, x, out, q, batch, false))
BSP_NORMAL_EQ_API(f64, double)
BSP_NORMAL_EQ_API(f32, float)
#undef BSP_NORMAL_EQ_API
struct bsp_sym_product {
  std::unique_ptr<SymProductMap> map;
};

int bsp_sym_product_create(bsp_solver* s, int64_t nnz, const int64_t* rows, const int64_t* cols, int32_t triangle,
                           bsp_sym_product** out) {
  BSP_TRY
  if (s == nullptr || out == nullptr) throw std::runtime_error("bsp_sym_product_create: NULL solver or output");
  std::unique_ptr<bsp_sym_product> p(new bsp_sym_product);
  p->map = createSymProductMap(*s->solver, nnz, rows, cols, triangle);
  *out = p.release();
  BSP_CATCH
}
void bsp_sym_product_destroy(bsp_sym_product* p) { delete p; }
int bsp_sym_product_info(const bsp_sym_product* p, int64_t out[6]) {
  BSP_TRY
  if (p == nullptr || out == nullptr) throw std::runtime_error("bsp_sym_product_info: NULL argument");
  const SymProductMap& m = *p->map;
  const int64_t v[6] = {m.nnz, m.kept, m.numTerms(), m.rows.maxRun, (int64_t)m.rows.longRuns.size(),
                        m.rowDeviceBytes() + m.entryDeviceBytes()};
  std::copy(v, v + 6, out);
  BSP_CATCH
}
int bsp_sym_product_row_table(const bsp_sym_product* p, int32_t* row_start, int32_t* entry, int32_t* index) {
  BSP_TRY
  if (p == nullptr) throw std::runtime_error("bsp_sym_product_row_table: the map is NULL");
  const SymProductMap& m = *p->map;
  if (row_start == nullptr || (m.numTerms() > 0 && (entry == nullptr || index == nullptr))) {
    throw std::runtime_error("bsp_sym_product_row_table: an output array is NULL");
  }
  std::copy(m.rows.start.begin(), m.rows.start.end(), row_start);
  std::copy(m.rows.entry.begin(), m.rows.entry.end(), entry);
  std::copy(m.rows.idx.begin(), m.rows.idx.end(), index);
  BSP_CATCH
}
template <typename T>
static void symProductRun(bsp_solver* s, const bsp_sym_product* p, int32_t op, const T* const* a, const T* const* x,
                          T* const* out, int64_t q, int32_t batch, bool single) {
  const std::string what = op == SymProductMv ? "symProductMv" : "symProductOuter";
  if (s == nullptr) throw std::runtime_error(what + ": the solver is NULL");
  if (p == nullptr) throw std::runtime_error(what + ": the map is NULL");
  const std::vector<const T*> as = hostArray<const T*>(what, nullptr, a, batch);
  const std::vector<const T*> xs = hostArray<const T*>(what, nullptr, x, batch);
  const std::vector<T*> o = hostArray<T*>(what, nullptr, out, batch);
  s->solver->symProduct<T>(*p->map, op, as, xs, o, q, single);
}
#define BSP_SYM_PRODUCT_API(SFX, T)                                                                              \
  int bsp_sym_product_mv_##SFX(bsp_solver* s, const bsp_sym_product* p, const T* v, const T* x, int64_t q,       \
                               T* out) BSP_BODY(symProductRun<T>(s, p, SymProductMv, &v, &x, &out, q, 1, true))  \
  int bsp_sym_product_mv_batched_##SFX(bsp_solver* s, const bsp_sym_product* p, const T* const* v,               \
                                       const T* const* x, int64_t q, T* const* out, int32_t batch)               \
      BSP_BODY(symProductRun<T>(s, p, SymProductMv, v, x, out, q, batch, false))                                 \
  int bsp_sym_product_outer_##SFX(bsp_solver* s, const bsp_sym_product* p, const T* g, const T* x, int64_t q,    \
                                  T* out)                                                                        \
      BSP_BODY(symProductRun<T>(s, p, SymProductOuter, &g, &x, &out, q, 1, true))                                \
  int bsp_sym_product_outer_batched_##SFX(bsp_solver* s, const bsp_sym_product* p, const T* const* g,            \
                                          const T* const* x, int64_t q, T* const* out, int32_t batch)            \
      BSP_BODY(symProductRun<T>(s, p, SymProductOuter, g, x, out, q, batch, false))
BSP_SYM_PRODUCT_API(f64, double)
BSP_SYM_PRODUCT_API(f32, float)
#undef BSP_SYM_PRODUCT_API

// ---- error bounds --------------------------------------------------------------
// residual (b, r given) or absMv (b, r NULL)
template <typename T>
static void symResidualRun(bsp_solver* s, const bsp_sym_product* p, bool hasB, const T* const* v, const T* const* x,
                           const T* const* b, T* const* r, T* const* d, int64_t q, int32_t batch, bool single) {
  const std::string what = hasB ? "symProductResidual" : "symProductAbsMv";
  if (s == nullptr) throw std::runtime_error(what + ": the solver is NULL");
  if (p == nullptr) throw std::runtime_error(what + ": the map is NULL");
  const std::vector<const T*> vs = hostArray<const T*>(what, nullptr, v, batch);
  const std::vector<const T*> xs = hostArray<const T*>(what, nullptr, x, batch);
  const std::vector<T*> ds = hostArray<T*>(what, nullptr, d, batch);
  std::vector<const T*> bs;
  std::vector<T*> rs;
  if (hasB) {
    bs = hostArray<const T*>(what, nullptr, b, batch);
    rs = hostArray<T*>(what, nullptr, r, batch);
  }
  s->solver->symResidual<T>(*p->map, vs, xs, bs, rs, ds, q, single);
}
// maxRatio (b given) or colMax (b NULL)
template <typename T>
static void colMaxRun(bsp_solver* s, bool ratio, const T* const* a, const T* const* b, int64_t n, int64_t q,
                      double* out, int32_t batch, bool single) {
  const std::string what = ratio ? "maxRatio" : "colMax";
  if (s == nullptr) throw std::runtime_error(what + ": the solver is NULL");
  const std::vector<const T*> as = hostArray<const T*>(what, nullptr, a, batch);
  const std::vector<const T*> bs = ratio ? hostArray<const T*>(what, nullptr, b, batch) : std::vector<const T*>{};
  s->solver->colMax<T>(as, bs, n, q, out, single);
}
template <typename T>
static void invNorm1Run(bsp_solver* s, const T* const* L, const T* const* D, void* work, int64_t* state, double* out,
                        int32_t batch, bool single) {
  const std::string what = "invNorm1Estimate";
  if (s == nullptr) throw std::runtime_error(what + ": the solver is NULL");
  const std::vector<const T*> ls = hostArray<const T*>(what, "factor", L, batch);
  const std::vector<const T*> ds = D ? hostArray<const T*>(what, "scale", D, batch) : std::vector<const T*>{};
  s->solver->invNorm1Estimate<T>(ls, ds, work, state, out, single);
}
#define BSP_ERROR_BOUNDS_API(SFX, T)                                                                             \
  int bsp_sym_product_residual_##SFX(bsp_solver* s, const bsp_sym_product* p, const T* v, const T* x, const T* b, \
                                     int64_t q, T* r, T* d)                                                      \
      BSP_BODY(symResidualRun<T>(s, p, true, &v, &x, &b, &r, &d, q, 1, true))                                    \
  int bsp_sym_product_residual_batched_##SFX(bsp_solver* s, const bsp_sym_product* p, const T* const* v,         \
                                             const T* const* x, const T* const* b, int64_t q, T* const* r,       \
                                             T* const* d, int32_t batch)                                         \
      BSP_BODY(symResidualRun<T>(s, p, true, v, x, b, r, d, q, batch, false))                                    \
  int bsp_sym_product_abs_mv_##SFX(bsp_solver* s, const bsp_sym_product* p, const T* v, const T* x, int64_t q,   \
                                   T* out)                                                                       \
      BSP_BODY(symResidualRun<T>(s, p, false, &v, &x, nullptr, nullptr, &out, q, 1, true))                       \
  int bsp_sym_product_abs_mv_batched_##SFX(bsp_solver* s, const bsp_sym_product* p, const T* const* v,           \
                                           const T* const* x, int64_t q, T* const* out, int32_t batch)           \
      BSP_BODY(symResidualRun<T>(s, p, false, v, x, nullptr, nullptr, out, q, batch, false))                     \
  int bsp_max_ratio_##SFX(bsp_solver* s, const T* r, const T* d, int64_t n, int64_t q, double* out)              \
      BSP_BODY(colMaxRun<T>(s, true, &r, &d, n, q, out, 1, true))                                                \
  int bsp_max_ratio_batched_##SFX(bsp_solver* s, const T* const* r, const T* const* d, int64_t n, int64_t q,     \
                                  double* out, int32_t batch)                                                    \
      BSP_BODY(colMaxRun<T>(s, true, r, d, n, q, out, batch, false))                                             \
  int bsp_col_max_##SFX(bsp_solver* s, const T* a, int64_t n, int64_t q, double* out)                            \
      BSP_BODY(colMaxRun<T>(s, false, &a, nullptr, n, q, out, 1, true))                                          \
  int bsp_col_max_batched_##SFX(bsp_solver* s, const T* const* a, int64_t n, int64_t q, double* out,             \
                                int32_t batch) BSP_BODY(colMaxRun<T>(s, false, a, nullptr, n, q, out, batch, false)) \
  int bsp_inv_norm1_work_bytes_##SFX(const bsp_solver* s, int64_t* out) BSP_BODY({                               \
    if (s == nullptr || out == nullptr) throw std::runtime_error("bsp_inv_norm1_work_bytes: NULL argument");     \
    *out = s->solver->invNorm1WorkBytes<T>();                                                                    \
  })                                                                                                             \
  int bsp_inv_norm1_##SFX(bsp_solver* s, const T* L, const T* D, void* work, int64_t* state, double* out)        \
      BSP_BODY(invNorm1Run<T>(s, &L, D ? &D : nullptr, work, state, out, 1, true))                               \
  int bsp_inv_norm1_batched_##SFX(bsp_solver* s, const T* const* L, const T* const* D, void* work,               \
                                  int64_t* state, double* out, int32_t batch)                                    \
      BSP_BODY(invNorm1Run<T>(s, L, D, work, state, out, batch, false))
BSP_ERROR_BOUNDS_API(f64, double)
BSP_ERROR_BOUNDS_API(f32, float)
#undef BSP_ERROR_BOUNDS_API
// ---- preconditioned conjugate gradient ------------------------------------------
int bsp_cg_state_words(int64_t* out) {
  BSP_TRY
  if (out == nullptr) throw std::runtime_error("bsp_cg_state_words: out is NULL");
  *out = 12;
  BSP_CATCH
}
int bsp_cg_work_bytes(const bsp_solver* s, int64_t n, int64_t q, int64_t* out) {
  BSP_TRY
  if (s == nullptr || out == nullptr) throw std::runtime_error("bsp_cg_work_bytes: NULL argument");
  *out = s->solver->cgWorkBytes(n, q);
  BSP_CATCH
}
int bsp_cg_precond_info(const bsp_sym_product* p, int32_t kind, int64_t out[4]) {
  BSP_TRY
  if (p == nullptr || out == nullptr) throw std::runtime_error("bsp_cg_precond_info: NULL argument");
  if (kind == CgFsai) {
    const CgFsaiPlan& fs = cgFsaiPlan(*p->map);
    const int64_t v[4] = {fs.n, fs.numItems(), fs.elems(), fs.maxWidth};
    std::copy(v, v + 4, out);
    return 0;
  }
  const CgPrecondPlan& pl = cgPrecondPlan(*p->map, kind);
  const int64_t v[4] = {pl.numBlocks, pl.numItems(), pl.inverseElems(), pl.maxWidth};
  std::copy(v, v + 4, out);
  BSP_CATCH
}
int bsp_fsai_table(const bsp_sym_product* p, int32_t* row_start, int32_t* cols, int32_t* item_start, int32_t* entry,
                      int32_t* pos, int32_t* col_start, int32_t* col_pos, int32_t* col_row, int32_t* long_cols) {
  BSP_TRY
  if (p == nullptr) throw std::runtime_error("bsp_fsai_table: the map is NULL");
  const CgFsaiPlan& fs = cgFsaiPlan(*p->map);
  if (row_start == nullptr || item_start == nullptr || col_start == nullptr ||
      (fs.elems() > 0 && (cols == nullptr || col_pos == nullptr || col_row == nullptr || long_cols == nullptr)) ||
      (fs.numItems() > 0 && (entry == nullptr || pos == nullptr))) {
    throw std::runtime_error("bsp_fsai_table: an output array is NULL");
  }
  std::copy(fs.rowStart.begin(), fs.rowStart.end(), row_start);
  std::copy(fs.cols.begin(), fs.cols.end(), cols);
  std::copy(fs.itemStart.begin(), fs.itemStart.end(), item_start);
  std::copy(fs.itemEntry.begin(), fs.itemEntry.end(), entry);
  std::copy(fs.itemPos.begin(), fs.itemPos.end(), pos);
  std::copy(fs.colRuns.start.begin(), fs.colRuns.start.end(), col_start);
  std::copy(fs.colRuns.entry.begin(), fs.colRuns.entry.end(), col_pos);
  std::copy(fs.colRuns.idx.begin(), fs.colRuns.idx.end(), col_row);
  std::copy(fs.colRuns.longRuns.begin(), fs.colRuns.longRuns.end(), long_cols);
  BSP_CATCH
}
int bsp_fsai_check_sizes(int64_t elems, int64_t items) {
  BSP_TRY
  checkCgFsaiSizes(elems, items);
  BSP_CATCH
}
int bsp_cg_precond_table(const bsp_sym_product* p, int32_t kind, int32_t* block_start, int32_t* item_start,
                         int32_t* entry, int32_t* pos) {
  BSP_TRY
  if (p == nullptr) throw std::runtime_error("bsp_cg_precond_table: the map is NULL");
  const CgPrecondPlan& pl = cgPrecondPlan(*p->map, kind);
  if (block_start == nullptr || item_start == nullptr || (pl.numItems() > 0 && (entry == nullptr || pos == nullptr))) {
    throw std::runtime_error("bsp_cg_precond_table: an output array is NULL");
  }
  std::copy(pl.blockStart.begin(), pl.blockStart.end(), block_start);
  std::copy(pl.itemStart.begin(), pl.itemStart.end(), item_start);
  std::copy(pl.itemEntry.begin(), pl.itemEntry.end(), entry);
  std::copy(pl.itemPos.begin(), pl.itemPos.end(), pos);
  BSP_CATCH
}
template <typename T>
static void cgRun(bsp_solver* s, const bsp_sym_product* p, int32_t op, int32_t kind, bool plain, int64_t n, int64_t q,
                  const T* const* in0, const T* const* in1, T* const* out0, T* const* out1, double tol,
                  int64_t maxSteps, void* work, int64_t* state, int64_t* status, int32_t batch, bool single) {
  if (s == nullptr) throw std::runtime_error("cg: the solver is NULL");
  CgArgs<T> a;
  a.op = op;
  a.kind = kind;
  a.plain = plain;
  a.map = p ? p->map.get() : nullptr;
  a.n = op == CgBuild && p ? p->map->n : n;
  a.q = q;
  a.in0 = in0;
  a.in1 = in1;
  a.out0 = out0;
  a.out1 = out1;
  a.tol = tol;
  a.maxSteps = maxSteps;
  a.work = work;
  a.state = state;
  a.status = status;
  s->solver->cg<T>(a, batch, single);
}
#define BSP_CG_API(SFX, T)                                                                                       \
  int bsp_cg_init_##SFX(bsp_solver* s, int64_t n, int64_t q, const T* b, T* x, T* r, double tol,                 \
                        int64_t max_steps, int32_t plain, void* work, int64_t* state)                            \
      BSP_BODY(cgRun<T>(s, nullptr, CgInit, 0, plain != 0, n, q, &b, nullptr, &x, &r, tol, max_steps, work,      \
                        state, nullptr, 1, true))                                                                \
  int bsp_cg_init_batched_##SFX(bsp_solver* s, int64_t n, int64_t q, const T* const* b, T* const* x,             \
                                T* const* r, double tol, int64_t max_steps, int32_t plain, void* work,           \
                                int64_t* state, int32_t batch)                                                   \
      BSP_BODY(cgRun<T>(s, nullptr, CgInit, 0, plain != 0, n, q, b, nullptr, x, r, tol, max_steps, work, state,  \
                        nullptr, batch, false))                                                                  \
  int bsp_cg_alpha_##SFX(bsp_solver* s, int64_t n, int64_t q, const T* p, const T* ap, void* work,               \
                         int64_t* state)                                                                         \
      BSP_BODY(cgRun<T>(s, nullptr, CgAlpha, 0, false, n, q, &p, &ap, nullptr, nullptr, 0, 0, work, state,       \
                        nullptr, 1, true))                                                                       \
  int bsp_cg_alpha_batched_##SFX(bsp_solver* s, int64_t n, int64_t q, const T* const* p, const T* const* ap,     \
                                 void* work, int64_t* state, int32_t batch)                                      \
      BSP_BODY(cgRun<T>(s, nullptr, CgAlpha, 0, false, n, q, p, ap, nullptr, nullptr, 0, 0, work, state,         \
                        nullptr, batch, false))                                                                  \
  int bsp_cg_update_##SFX(bsp_solver* s, int64_t n, int64_t q, const T* p, const T* ap, T* x, T* r,              \
                          int32_t plain, void* work, int64_t* state)                                             \
      BSP_BODY(cgRun<T>(s, nullptr, CgUpdate, 0, plain != 0, n, q, &p, &ap, &x, &r, 0, 0, work, state, nullptr,  \
                        1, true))                                                                                \
  int bsp_cg_update_batched_##SFX(bsp_solver* s, int64_t n, int64_t q, const T* const* p, const T* const* ap,    \
                                  T* const* x, T* const* r, int32_t plain, void* work, int64_t* state,           \
                                  int32_t batch)                                                                 \
      BSP_BODY(cgRun<T>(s, nullptr, CgUpdate, 0, plain != 0, n, q, p, ap, x, r, 0, 0, work, state, nullptr,      \
                        batch, false))                                                                           \
  int bsp_cg_precond_##SFX(bsp_solver* s, const bsp_sym_product* m, int32_t kind, int64_t n, int64_t q,          \
                           const T* minv, const T* r, T* z, void* work, int64_t* state)                          \
      BSP_BODY(cgRun<T>(s, m, CgPrecond, kind, false, n, q, &minv, &r, &z, nullptr, 0, 0, work, state, nullptr,  \
                        1, true))                                                                                \
  int bsp_cg_precond_batched_##SFX(bsp_solver* s, const bsp_sym_product* m, int32_t kind, int64_t n, int64_t q,  \
                                   const T* const* minv, const T* const* r, T* const* z, void* work,             \
                                   int64_t* state, int32_t batch)                                                \
      BSP_BODY(cgRun<T>(s, m, CgPrecond, kind, false, n, q, minv, r, z, nullptr, 0, 0, work, state, nullptr,     \
                        batch, false))                                                                           \
  int bsp_fsai_apply_##SFX(bsp_solver* s, const bsp_sym_product* m, int64_t n, int64_t q, const T* g,         \
                              const T* r, T* t, T* z, void* work, int64_t* state)                               \
      BSP_BODY(cgRun<T>(s, m, CgFsaiApply, CgFsai, false, n, q, &g, &r, &z, &t, 0, 0, work, state, nullptr, 1,   \
                        true))                                                                                   \
  int bsp_fsai_apply_batched_##SFX(bsp_solver* s, const bsp_sym_product* m, int64_t n, int64_t q,             \
                                      const T* const* g, const T* const* r, T* const* t, T* const* z,           \
                                      void* work, int64_t* state, int32_t batch)                                 \
      BSP_BODY(cgRun<T>(s, m, CgFsaiApply, CgFsai, false, n, q, g, r, z, t, 0, 0, work, state, nullptr, batch,   \
                        false))                                                                                  \
  int bsp_cg_direction_##SFX(bsp_solver* s, int64_t n, int64_t q, const T* z, T* p, int32_t plain, void* work,   \
                             int64_t* state)                                                                     \
      BSP_BODY(cgRun<T>(s, nullptr, CgDirection, 0, plain != 0, n, q, &z, nullptr, &p, nullptr, 0, 0, work,      \
                        state, nullptr, 1, true))                                                                \
  int bsp_cg_direction_batched_##SFX(bsp_solver* s, int64_t n, int64_t q, const T* const* z, T* const* p,        \
                                     int32_t plain, void* work, int64_t* state, int32_t batch)                   \
      BSP_BODY(cgRun<T>(s, nullptr, CgDirection, 0, plain != 0, n, q, z, nullptr, p, nullptr, 0, 0, work, state, \
                        nullptr, batch, false))                                                                  \
  int bsp_cg_precond_build_##SFX(bsp_solver* s, const bsp_sym_product* m, int32_t kind, const T* values,         \
                                 T* minv, void* work, int64_t* status)                                           \
      BSP_BODY(cgRun<T>(s, m, CgBuild, kind, false, 0, 1, &values, nullptr, &minv, nullptr, 0, 0, work, nullptr, \
                        status, 1, true))                                                                        \
  int bsp_cg_precond_build_batched_##SFX(bsp_solver* s, const bsp_sym_product* m, int32_t kind,                  \
                                         const T* const* values, T* const* minv, void* work, int64_t* status,    \
                                         int32_t batch)                                                          \
      BSP_BODY(cgRun<T>(s, m, CgBuild, kind, false, 0, 1, values, nullptr, minv, nullptr, 0, 0, work, nullptr,   \
                        status, batch, false))
BSP_CG_API(f64, double)
BSP_CG_API(f32, float)
#undef BSP_CG_API
// ---- matrix-free least squares --------------------------------------------------
struct bsp_jac_product {
  std::unique_ptr<JacobianProductMap> map;
};

int bsp_jac_product_create(bsp_solver* s, int64_t m, int64_t nnz, const int64_t* rows, const int64_t* cols,
                           bsp_jac_product** out) {
  BSP_TRY
  if (s == nullptr || out == nullptr) throw std::runtime_error("bsp_jac_product_create: NULL solver or output");
  std::unique_ptr<bsp_jac_product> p(new bsp_jac_product);
  p->map = createJacobianProductMap(*s->solver, m, nnz, rows, cols);
  *out = p.release();
  BSP_CATCH
}
void bsp_jac_product_destroy(bsp_jac_product* p) { delete p; }
int bsp_jac_product_info(const bsp_jac_product* p, int64_t out[9]) {
  BSP_TRY
  if (p == nullptr || out == nullptr) throw std::runtime_error("bsp_jac_product_info: NULL argument");
  const JacobianProductMap& m = *p->map;
  const int64_t v[9] = {m.nnz, m.m, m.n, m.rows.maxRun, (int64_t)m.rows.longRuns.size(), m.cols.maxRun,
                        (int64_t)m.cols.longRuns.size(), m.rowDeviceBytes(), m.colDeviceBytes()};
  std::copy(v, v + 9, out);
  BSP_CATCH
}
int bsp_jac_product_check_items(int64_t items) {
  BSP_TRY
  checkJacBlockItems(items);
  BSP_CATCH
}
int bsp_cgls_precond_info(const bsp_jac_product* p, int32_t kind, int64_t out[5]) {
  BSP_TRY
  if (p == nullptr || out == nullptr) throw std::runtime_error("bsp_cgls_precond_info: NULL argument");
  if (kind == CgJacobi) {
    const int64_t n = p->map->n, v[5] = {n, 0, n, n > 0 ? 1 : 0, (n + 1) * (int64_t)sizeof(int32_t)};
    std::copy(v, v + 5, out);
    return 0;
  }
  if (kind != CgBlockJacobi) {
    throw std::runtime_error("bsp_cgls_precond_info: unknown kind " + std::to_string(kind) + " (1: jacobi, 2: block_jacobi)");
  }
  const JacBlockPlan& pl = jacBlockPlan(*p->map);
  const int64_t v[5] = {pl.numBlocks, pl.numItems(), pl.inverseElems(), pl.maxWidth, pl.deviceBytes()};
  std::copy(v, v + 5, out);
  BSP_CATCH
}
int bsp_jac_product_table(const bsp_jac_product* p, int32_t part, int32_t* t0, int32_t* t1, int32_t* t2, int32_t* t3,
                          int32_t* t4) {
  BSP_TRY
  if (p == nullptr) throw std::runtime_error("bsp_jac_product_table: the map is NULL");
  const auto put = [](const std::vector<int32_t>& v, int32_t* out) {
    if (!v.empty() && out == nullptr) throw std::runtime_error("bsp_jac_product_table: an output array is NULL");
    std::copy(v.begin(), v.end(), out);
  };
  if (part == 0 || part == 1) {
    const RunList& r = part == 0 ? p->map->rows : p->map->cols;
    put(r.start, t0);
    put(r.entry, t1);
    put(r.idx, t2);
    put(r.longRuns, t3);
  } else if (part == 2) {
    const JacBlockPlan& pl = jacBlockPlan(*p->map);
    put(pl.blockStart, t0);
    put(pl.itemStart, t1);
    put(pl.itemA, t2);
    put(pl.itemB, t3);
    put(pl.itemPos, t4);
  } else {
    throw std::runtime_error("bsp_jac_product_table: unknown part " + std::to_string(part) +
                             " (0: rows, 1: columns, 2: blocks)");
  }
  BSP_CATCH
}
int bsp_cgls_work_bytes(const bsp_solver* s, const bsp_jac_product* p, int64_t q, int64_t* out) {
  BSP_TRY
  if (s == nullptr || p == nullptr || out == nullptr) throw std::runtime_error("bsp_cgls_work_bytes: NULL argument");
  *out = s->solver->cglsWorkBytes(p->map->m, p->map->n, q);
  BSP_CATCH
}
namespace {
// the operands of one piece; the single entries pass the addresses of their pointer arguments
template <typename T>
struct CglsCall {
  CglsArgs<T> a;
  CglsCall(int32_t op, const bsp_jac_product* p, int64_t q = 1) {
    a.op = op;
    a.map = p ? p->map.get() : nullptr;
    a.q = q;
  }
  void run(bsp_solver* s, int32_t batch, bool single) {
    if (s == nullptr) throw std::runtime_error("cgls: the solver is NULL");
    if (a.map == nullptr) throw std::runtime_error("cgls: the map is NULL");
    s->solver->cgls<T>(a, batch, single);
  }
};
// p or NULL as the one-member array of a single call
template <typename P>
P* const* one(P* const& p) {
  return p ? &p : nullptr;
}
}  // namespace
template <typename T>
static void cglsProductRun(bsp_solver* s, const bsp_jac_product* p, int32_t op, int32_t epi, const T* const* v,
                           const T* const* vec, const T* const* addend, const T* const* damp, const T* const* x,
                           int64_t q, T* const* out, int64_t* state, int32_t batch, bool single) {
  CglsCall<T> c(op, p, q);
  c.a.epi = epi;
  c.a.values = v;
  c.a.vec = vec;
  c.a.addend = addend;
  c.a.damp = damp;
  c.a.x = const_cast<T* const*>(x);  // (only read by the epilogue)
  c.a.out = out;
  c.a.state = state;
  c.run(s, batch, single);
}
template <typename T>
static void cglsPieceRun(bsp_solver* s, const bsp_jac_product* p, int32_t op, int32_t kind, bool start, int64_t q,
                         const T* const* values, const T* const* vec, const T* const* addend, const T* const* damp,
                         T* const* x, T* const* out, double* const* colsq, double tol, int64_t maxSteps, double alpha,
                         double beta, void* work, int64_t* state, int64_t* status, int32_t batch, bool single) {
  CglsCall<T> c(op, p, q);
  c.a.kind = kind;
  c.a.start = start;
  c.a.values = values;
  c.a.vec = vec;
  c.a.addend = addend;
  c.a.damp = damp;
  c.a.x = x;
  c.a.out = out;
  c.a.colsq = colsq;
  c.a.tol = tol;
  c.a.maxSteps = maxSteps;
  c.a.alpha = alpha;
  c.a.beta = beta;
  c.a.work = work;
  c.a.state = state;
  c.a.status = status;
  c.run(s, batch, single);
}
template <typename T>
static void cglsIterateRun(bsp_solver* s, const bsp_jac_product* p, int32_t kind, int32_t phase, int64_t q,
                           const T* const* values, const T* const* d, const T* const* c, const T* const* minv,
                           T* const* pv, T* const* t, T* const* x, T* const* res, T* const* sv, T* const* z, void* work,
                           int64_t* state, int32_t batch, bool single) {
  CglsCall<T> call(CglsIterate, p, q);
  call.a.kind = kind;
  call.a.phase = phase;
  call.a.values = values;
  call.a.damp = d;
  call.a.addend = c;
  call.a.minv = minv;
  call.a.p = pv;
  call.a.t = t;
  call.a.x = x;
  call.a.res = res;
  call.a.s = sv;
  call.a.z = z;
  call.a.work = work;
  call.a.state = state;
  call.run(s, batch, single);
}
#define BSP_CC(T, x) const_cast<T* const*>(x)
#define BSP_CD(x) const_cast<double* const*>(x)
#define BSP_CGLS_API(SFX, T)                                                                                     \
  int bsp_jac_product_jv_##SFX(bsp_solver* s, const bsp_jac_product* p, const T* v, const T* x, int64_t q, T* out) \
      BSP_BODY(cglsProductRun<T>(s, p, CglsJv, 0, &v, &x, nullptr, nullptr, nullptr, q, &out, nullptr, 1, true)) \
  int bsp_jac_product_jv_batched_##SFX(bsp_solver* s, const bsp_jac_product* p, const T* const* v,               \
                                       const T* const* x, int64_t q, T* const* out, int32_t batch)               \
      BSP_BODY(cglsProductRun<T>(s, p, CglsJv, 0, v, x, nullptr, nullptr, nullptr, q, out, nullptr, batch, false)) \
  int bsp_jac_product_jtv_##SFX(bsp_solver* s, const bsp_jac_product* p, const T* v, const T* u, int64_t q,      \
                                T* out)                                                                          \
      BSP_BODY(cglsProductRun<T>(s, p, CglsJtv, 0, &v, &u, nullptr, nullptr, nullptr, q, &out, nullptr, 1, true)) \
  int bsp_jac_product_jtv_batched_##SFX(bsp_solver* s, const bsp_jac_product* p, const T* const* v,              \
                                        const T* const* u, int64_t q, T* const* out, int32_t batch)              \
      BSP_BODY(cglsProductRun<T>(s, p, CglsJtv, 0, v, u, nullptr, nullptr, nullptr, q, out, nullptr, batch, false)) \
  int bsp_cgls_residual_##SFX(bsp_solver* s, const bsp_jac_product* p, const T* v, const T* x, const T* r,       \
                              int64_t q, T* res, int64_t* state)                                                 \
      BSP_BODY(cglsProductRun<T>(s, p, CglsJv, 1, &v, &x, one(r), nullptr, nullptr, q, &res, state, 1, true))    \
  int bsp_cgls_residual_batched_##SFX(bsp_solver* s, const bsp_jac_product* p, const T* const* v,                \
                                      const T* const* x, const T* const* r, int64_t q, T* const* res,            \
                                      int64_t* state, int32_t batch)                                             \
      BSP_BODY(cglsProductRun<T>(s, p, CglsJv, 1, v, x, r, nullptr, nullptr, q, res, state, batch, false))       \
  int bsp_cgls_normal_##SFX(bsp_solver* s, const bsp_jac_product* p, const T* v, const T* res, const T* d,       \
                            const T* x, const T* c, int64_t q, T* out, int64_t* state)                           \
      BSP_BODY(cglsProductRun<T>(s, p, CglsJtv, 2, &v, &res, one(c), one(d), one(x), q, &out, state, 1, true))   \
  int bsp_cgls_normal_batched_##SFX(bsp_solver* s, const bsp_jac_product* p, const T* const* v,                  \
                                    const T* const* res, const T* const* d, const T* const* x,                   \
                                    const T* const* c, int64_t q, T* const* out, int64_t* state, int32_t batch)  \
      BSP_BODY(cglsProductRun<T>(s, p, CglsJtv, 2, v, res, c, d, x, q, out, state, batch, false))                \
  int bsp_cgls_colsq_##SFX(bsp_solver* s, const bsp_jac_product* p, const T* v, double* colsq)                   \
      BSP_BODY(cglsPieceRun<T>(s, p, CglsColSq, 0, false, 1, &v, nullptr, nullptr, nullptr, nullptr, nullptr,    \
                               &colsq, 0, 0, 0, 0, nullptr, nullptr, nullptr, 1, true))                          \
  int bsp_cgls_colsq_batched_##SFX(bsp_solver* s, const bsp_jac_product* p, const T* const* v,                   \
                                   double* const* colsq, int32_t batch)                                          \
      BSP_BODY(cglsPieceRun<T>(s, p, CglsColSq, 0, false, 1, v, nullptr, nullptr, nullptr, nullptr, nullptr,     \
                               colsq, 0, 0, 0, 0, nullptr, nullptr, nullptr, batch, false))                      \
  int bsp_cgls_damp_##SFX(bsp_solver* s, const bsp_jac_product* p, const double* colsq, double alpha,            \
                          double beta, T* d)                                                                     \
      BSP_BODY({                                                                                                 \
        double* cs = const_cast<double*>(colsq);                                                                 \
        cglsPieceRun<T>(s, p, CglsDamp, 0, false, 1, nullptr, nullptr, nullptr, nullptr, nullptr, &d, &cs, 0, 0, \
                        alpha, beta, nullptr, nullptr, nullptr, 1, true);                                        \
      })                                                                                                         \
  int bsp_cgls_damp_batched_##SFX(bsp_solver* s, const bsp_jac_product* p, const double* const* colsq,           \
                                  double alpha, double beta, T* const* d, int32_t batch)                         \
      BSP_BODY(cglsPieceRun<T>(s, p, CglsDamp, 0, false, 1, nullptr, nullptr, nullptr, nullptr, nullptr, d,      \
                               BSP_CD(colsq), 0, 0, alpha, beta, nullptr, nullptr, nullptr, batch, false))       \
  int bsp_cgls_init_##SFX(bsp_solver* s, const bsp_jac_product* p, int64_t q, const T* b, T* x, double tol,      \
                          int64_t max_steps, void* work, int64_t* state)                                         \
      BSP_BODY(cglsPieceRun<T>(s, p, CglsInit, 0, false, q, nullptr, &b, nullptr, nullptr, &x, nullptr, nullptr, \
                               tol, max_steps, 0, 0, work, state, nullptr, 1, true))                             \
  int bsp_cgls_init_batched_##SFX(bsp_solver* s, const bsp_jac_product* p, int64_t q, const T* const* b,         \
                                  T* const* x, double tol, int64_t max_steps, void* work, int64_t* state,        \
                                  int32_t batch)                                                                 \
      BSP_BODY(cglsPieceRun<T>(s, p, CglsInit, 0, false, q, nullptr, b, nullptr, nullptr, x, nullptr, nullptr,   \
                               tol, max_steps, 0, 0, work, state, nullptr, batch, false))                        \
  int bsp_cgls_delta_##SFX(bsp_solver* s, const bsp_jac_product* p, int64_t q, const T* t, const T* pv,          \
                           const T* d, void* work, int64_t* state)                                               \
      BSP_BODY({                                                                                                 \
        T* pw = const_cast<T*>(pv);                                                                              \
        cglsPieceRun<T>(s, p, CglsDelta, 0, false, q, nullptr, &t, nullptr, one(d), &pw, nullptr, nullptr, 0, 0, \
                        0, 0, work, state, nullptr, 1, true);                                                    \
      })                                                                                                         \
  int bsp_cgls_delta_batched_##SFX(bsp_solver* s, const bsp_jac_product* p, int64_t q, const T* const* t,        \
                                   const T* const* pv, const T* const* d, void* work, int64_t* state,            \
                                   int32_t batch)                                                                \
      BSP_BODY(cglsPieceRun<T>(s, p, CglsDelta, 0, false, q, nullptr, t, nullptr, d, BSP_CC(T, pv), nullptr,     \
                               nullptr, 0, 0, 0, 0, work, state, nullptr, batch, false))                         \
  int bsp_cgls_update_##SFX(bsp_solver* s, const bsp_jac_product* p, int64_t q, const T* pv, const T* t, T* x,   \
                            T* res, int64_t* state)                                                              \
      BSP_BODY(cglsPieceRun<T>(s, p, CglsUpdate, 0, false, q, nullptr, &pv, &t, nullptr, &x, &res, nullptr, 0,   \
                               0, 0, 0, nullptr, state, nullptr, 1, true))                                       \
  int bsp_cgls_update_batched_##SFX(bsp_solver* s, const bsp_jac_product* p, int64_t q, const T* const* pv,      \
                                    const T* const* t, T* const* x, T* const* res, int64_t* state,               \
                                    int32_t batch)                                                               \
      BSP_BODY(cglsPieceRun<T>(s, p, CglsUpdate, 0, false, q, nullptr, pv, t, nullptr, x, res, nullptr, 0, 0, 0, \
                               0, nullptr, state, nullptr, batch, false))                                        \
  int bsp_cgls_apply_##SFX(bsp_solver* s, const bsp_jac_product* p, int32_t kind, int64_t q, const T* minv,      \
                           const T* sv, T* z, int32_t start, void* work, int64_t* state)                         \
      BSP_BODY(cglsPieceRun<T>(s, p, CglsApply, kind, start != 0, q, nullptr, &sv, nullptr, one(minv), nullptr,  \
                               &z, nullptr, 0, 0, 0, 0, work, state, nullptr, 1, true))                          \
  int bsp_cgls_apply_batched_##SFX(bsp_solver* s, const bsp_jac_product* p, int32_t kind, int64_t q,             \
                                   const T* const* minv, const T* const* sv, T* const* z, int32_t start,         \
                                   void* work, int64_t* state, int32_t batch)                                    \
      BSP_BODY(cglsPieceRun<T>(s, p, CglsApply, kind, start != 0, q, nullptr, sv, nullptr, minv, nullptr, z,     \
                               nullptr, 0, 0, 0, 0, work, state, nullptr, batch, false))                         \
  int bsp_cgls_precond_build_##SFX(bsp_solver* s, const bsp_jac_product* p, int32_t kind, const T* v,            \
                                   const double* colsq, const T* d, T* minv, void* work, int64_t* status)        \
      BSP_BODY({                                                                                                 \
        double* cs = const_cast<double*>(colsq);                                                                 \
        cglsPieceRun<T>(s, p, CglsBuild, kind, false, 1, one(v), nullptr, nullptr, one(d), nullptr, &minv,       \
                        one(cs), 0, 0, 0, 0, work, nullptr, status, 1, true);                                    \
      })                                                                                                         \
  int bsp_cgls_precond_build_batched_##SFX(bsp_solver* s, const bsp_jac_product* p, int32_t kind,                \
                                           const T* const* v, const double* const* colsq, const T* const* d,     \
                                           T* const* minv, void* work, int64_t* status, int32_t batch)           \
      BSP_BODY(cglsPieceRun<T>(s, p, CglsBuild, kind, false, 1, v, nullptr, nullptr, d, nullptr, minv,           \
                               BSP_CD(colsq), 0, 0, 0, 0, work, nullptr, status, batch, false))
#define BSP_CGLS_ITERATE_API(SFX, T)                                                                             \
  int bsp_cgls_iterate_##SFX(bsp_solver* s, const bsp_jac_product* p, int32_t kind, int32_t phase, int64_t q,    \
                             const T* v, const T* d, const T* c, const T* minv, T* pv, T* t, T* x, T* res, T* sv, \
                             T* z, void* work, int64_t* state)                                                   \
      BSP_BODY(cglsIterateRun<T>(s, p, kind, phase, q, one(v), one(d), one(c), one(minv), one(pv), one(t),       \
                                 one(x), one(res), one(sv), one(z), work, state, 1, true))                       \
  int bsp_cgls_iterate_batched_##SFX(bsp_solver* s, const bsp_jac_product* p, int32_t kind, int32_t phase,       \
                                     int64_t q, const T* const* v, const T* const* d, const T* const* c,         \
                                     const T* const* minv, T* const* pv, T* const* t, T* const* x,               \
                                     T* const* res, T* const* sv, T* const* z, void* work, int64_t* state,       \
                                     int32_t batch)                                                              \
      BSP_BODY(cglsIterateRun<T>(s, p, kind, phase, q, v, d, c, minv, pv, t, x, res, sv, z, work, state, batch,  \
                                 false))
BSP_CGLS_ITERATE_API(f64, double)
BSP_CGLS_ITERATE_API(f32, float)
#undef BSP_CGLS_ITERATE_API
BSP_CGLS_API(f64, double)
BSP_CGLS_API(f32, float)
#undef BSP_CGLS_API
// ---- implicit Schur elimination of the matrix-free least squares ----------------
struct bsp_jac_schur {
  std::unique_ptr<JacSchurMap> map;
};

int bsp_jac_schur_create(const bsp_jac_product* p, int64_t num_eliminate, const int64_t* eliminate, bsp_jac_schur** out) {
  BSP_TRY
  if (p == nullptr || out == nullptr) throw std::runtime_error("bsp_jac_schur_create: NULL product or output");
  std::unique_ptr<bsp_jac_schur> h(new bsp_jac_schur);
  h->map = createJacSchurMap(*p->map, num_eliminate, eliminate);
  *out = h.release();
  BSP_CATCH
}
void bsp_jac_schur_destroy(bsp_jac_schur* h) { delete h; }
int bsp_jac_schur_info(const bsp_jac_schur* h, int64_t out[20]) {
  BSP_TRY
  if (h == nullptr || out == nullptr) throw std::runtime_error("bsp_jac_schur_info: NULL argument");
  const JacSchurMap& m = *h->map;
  const JacBlockPlan& pl = *m.elimBlocks;
  const int64_t v[20] = {m.nnz,
                         m.m,
                         m.n,
                         m.nK,
                         m.nE,
                         m.numElim,
                         (int64_t)m.freeRows.size(),
                         m.maxElimWidth,
                         m.maxGroup,
                         (int64_t)m.rowsKept.entry.size(),
                         (int64_t)m.rowsElim.entry.size(),
                         (int64_t)m.rowsKept.longRuns.size(),
                         (int64_t)m.rowsElim.longRuns.size(),
                         (int64_t)m.colsElim.longRuns.size(),
                         (int64_t)m.colsKept.longRuns.size(),
                         pl.numItems(),
                         pl.inverseElems(),
                         m.deviceBytes(),
                         pl.deviceBytes(),
                         (int64_t)m.groupRow.size()};
  std::copy(v, v + 20, out);
  BSP_CATCH
}
int bsp_jac_schur_table(const bsp_jac_schur* h, int32_t part, int32_t* t0, int32_t* t1, int32_t* t2, int32_t* t3) {
  BSP_TRY
  if (h == nullptr) throw std::runtime_error("bsp_jac_schur_table: the map is NULL");
  const auto put = [](const std::vector<int32_t>& v, int32_t* out) {
    if (!v.empty() && out == nullptr) throw std::runtime_error("bsp_jac_schur_table: an output array is NULL");
    std::copy(v.begin(), v.end(), out);
  };
  const JacSchurMap& m = *h->map;
  const JacBlockPlan& pl = *m.elimBlocks;
  if (part >= 0 && part <= 3) {
    const RunList& r = part == 0 ? m.rowsKept : part == 1 ? m.rowsElim : part == 2 ? m.colsElim : m.colsKept;
    put(r.start, t0);
    put(r.entry, t1);
    put(r.idx, t2);
    put(r.longRuns, t3);
  } else if (part == 4) {
    put(m.keptScalar, t0);
    put(m.elimScalar, t1);
    put(m.elimOff, t2);
    put(m.elimParam, t3);
  } else if (part == 5) {
    put(m.groupStart, t0);
    put(m.groupRow, t1);
    put(m.freeRows, t2);
  } else if (part == 6) {
    put(pl.blockStart, t0);
    put(pl.blockWidth, t1);
    put(pl.itemStart, t2);
  } else if (part == 7) {
    put(pl.itemA, t0);
    put(pl.itemB, t1);
    put(pl.itemPos, t2);
  } else if (part == 8) {
    const JacBlockPlan& kp = jacSchurKeptPlan(m);
    put(kp.blockStart, t0);
    put(kp.blockWidth, t1);
    put(kp.itemStart, t2);
    put(m.keptParam, t3);
  } else if (part == 9) {
    const JacBlockPlan& kp = jacSchurKeptPlan(m);
    put(kp.itemA, t0);
    put(kp.itemB, t1);
    put(kp.itemPos, t2);
  } else {
    throw std::runtime_error("bsp_jac_schur_table: unknown part " + std::to_string(part) +
                             " (0 .. 3: the lists, 4: numberings, 5: groups, 6: blocks, 7: items, 8: kept blocks, 9: "
                             "kept items)");
  }
  BSP_CATCH
}
int bsp_jac_schur_precond_info(const bsp_jac_schur* h, int32_t kind, int64_t out[5]) {
  BSP_TRY
  if (h == nullptr || out == nullptr) throw std::runtime_error("bsp_jac_schur_precond_info: NULL argument");
  const JacSchurMap& m = *h->map;
  if (kind == CgJacobi) {
    const int64_t v[5] = {m.nK, 0, m.nK, 1, (int64_t)(m.keptScalar.size() * sizeof(int32_t))};
    std::copy(v, v + 5, out);
    return 0;
  }
  if (kind != CgBlockJacobi) {
    throw std::runtime_error("bsp_jac_schur_precond_info: unknown kind " + std::to_string(kind) +
                             " (1: jacobi, 2: block_jacobi)");
  }
  const JacBlockPlan& pl = jacSchurKeptPlan(m);
  const int64_t v[5] = {pl.numBlocks, pl.numItems(), pl.inverseElems(), pl.maxWidth,
                        pl.deviceBytes() + (int64_t)((m.keptBlockStart.size() + m.keptScalarBlock.size()) * sizeof(int32_t))};
  std::copy(v, v + 5, out);
  BSP_CATCH
}
template <typename T>
static void jacSchurRun(bsp_solver* s, const bsp_jac_schur* h, int32_t op, int64_t q, const T* const* v,
                        const T* const* d, const T* const* binv, const T* const* vec, const T* const* full, T* const* t,
                        T* const* out, void* work, const int64_t* state, int64_t* status, int32_t batch, bool single,
                        int32_t kind = 0, const double* const* colsq = nullptr) {
  if (s == nullptr) throw std::runtime_error("jacobian schur: the solver is NULL");
  if (h == nullptr) throw std::runtime_error("jacobian schur: the map is NULL");
  JacSchurArgs<T> a;
  a.op = op;
  a.q = q;
  a.map = h->map.get();
  a.values = v;
  a.damp = d;
  a.binv = binv;
  a.vec = vec;
  a.full = full;
  a.t = t;
  a.out = out;
  a.work = work;
  a.state = const_cast<int64_t*>(state);  // (written by SchurPrecondApply alone, whose entries take it non-const)
  a.status = status;
  a.kind = kind;
  a.colsq = colsq;
  s->solver->jacSchur<T>(a, batch, single);
}
#define BSP_JAC_SCHUR_API(SFX, T)                                                                                \
  int bsp_jac_schur_build_##SFX(bsp_solver* s, const bsp_jac_schur* h, const T* v, const T* d, T* binv,          \
                                void* work, int64_t* status)                                                     \
      BSP_BODY(jacSchurRun<T>(s, h, SchurBuild, 1, &v, one(d), nullptr, nullptr, nullptr, nullptr, &binv, work,  \
                              nullptr, status, 1, true))                                                         \
  int bsp_jac_schur_build_batched_##SFX(bsp_solver* s, const bsp_jac_schur* h, const T* const* v,                \
                                        const T* const* d, T* const* binv, void* work, int64_t* status,          \
                                        int32_t batch)                                                           \
      BSP_BODY(jacSchurRun<T>(s, h, SchurBuild, 1, v, d, nullptr, nullptr, nullptr, nullptr, binv, work,         \
                              nullptr, status, batch, false))                                                    \
  int bsp_jac_schur_mv_##SFX(bsp_solver* s, const bsp_jac_schur* h, int64_t q, const T* v, const T* binv,        \
                             const T* d, const T* p, T* t, T* out, const int64_t* state)                         \
      BSP_BODY(jacSchurRun<T>(s, h, SchurMv, q, &v, one(d), &binv, &p, nullptr, &t, &out, nullptr, state,        \
                              nullptr, 1, true))                                                                 \
  int bsp_jac_schur_mv_batched_##SFX(bsp_solver* s, const bsp_jac_schur* h, int64_t q, const T* const* v,        \
                                     const T* const* binv, const T* const* d, const T* const* p, T* const* t,    \
                                     T* const* out, const int64_t* state, int32_t batch)                         \
      BSP_BODY(jacSchurRun<T>(s, h, SchurMv, q, v, d, binv, p, nullptr, t, out, nullptr, state, nullptr, batch,  \
                              false))                                                                            \
  int bsp_jac_schur_reduce_##SFX(bsp_solver* s, const bsp_jac_schur* h, int64_t q, const T* v, const T* binv,    \
                                 const T* g, T* t, T* out)                                                       \
      BSP_BODY(jacSchurRun<T>(s, h, SchurReduce, q, &v, nullptr, &binv, nullptr, &g, &t, &out, nullptr, nullptr, \
                              nullptr, 1, true))                                                                 \
  int bsp_jac_schur_reduce_batched_##SFX(bsp_solver* s, const bsp_jac_schur* h, int64_t q, const T* const* v,    \
                                         const T* const* binv, const T* const* g, T* const* t, T* const* out,    \
                                         int32_t batch)                                                          \
      BSP_BODY(jacSchurRun<T>(s, h, SchurReduce, q, v, nullptr, binv, nullptr, g, t, out, nullptr, nullptr,      \
                              nullptr, batch, false))                                                            \
  int bsp_jac_schur_back_##SFX(bsp_solver* s, const bsp_jac_schur* h, int64_t q, const T* v, const T* binv,      \
                               const T* g, const T* xk, T* t, T* out)                                            \
      BSP_BODY(jacSchurRun<T>(s, h, SchurBack, q, &v, nullptr, &binv, &xk, &g, &t, &out, nullptr, nullptr,       \
                              nullptr, 1, true))                                                                 \
  int bsp_jac_schur_back_batched_##SFX(bsp_solver* s, const bsp_jac_schur* h, int64_t q, const T* const* v,      \
                                       const T* const* binv, const T* const* g, const T* const* xk, T* const* t, \
                                       T* const* out, int32_t batch)                                             \
      BSP_BODY(jacSchurRun<T>(s, h, SchurBack, q, v, nullptr, binv, xk, g, t, out, nullptr, nullptr, nullptr,    \
                              batch, false))                                                                     \
  int bsp_jac_schur_precond_build_##SFX(bsp_solver* s, const bsp_jac_schur* h, int32_t kind, const T* v,         \
                                        const double* colsq, const T* d, T* minv, void* work, int64_t* status)   \
      BSP_BODY(jacSchurRun<T>(s, h, SchurPrecondBuild, 1, one(v), one(d), nullptr, nullptr, nullptr, nullptr,    \
                              &minv, work, nullptr, status, 1, true, kind, one(colsq)))                          \
  int bsp_jac_schur_precond_build_batched_##SFX(bsp_solver* s, const bsp_jac_schur* h, int32_t kind,             \
                                                const T* const* v, const double* const* colsq,                   \
                                                const T* const* d, T* const* minv, void* work, int64_t* status,  \
                                                int32_t batch)                                                   \
      BSP_BODY(jacSchurRun<T>(s, h, SchurPrecondBuild, 1, v, d, nullptr, nullptr, nullptr, nullptr, minv, work,  \
                              nullptr, status, batch, false, kind, colsq))                                       \
  int bsp_jac_schur_precond_apply_##SFX(bsp_solver* s, const bsp_jac_schur* h, int32_t kind, int64_t q,          \
                                        const T* minv, const T* r, T* z, void* work, int64_t* state)             \
      BSP_BODY(jacSchurRun<T>(s, h, SchurPrecondApply, q, nullptr, nullptr, &minv, &r, nullptr, nullptr, &z,     \
                              work, state, nullptr, 1, true, kind))                                              \
  int bsp_jac_schur_precond_apply_batched_##SFX(bsp_solver* s, const bsp_jac_schur* h, int32_t kind, int64_t q,  \
                                                const T* const* minv, const T* const* r, T* const* z,            \
                                                void* work, int64_t* state, int32_t batch)                       \
      BSP_BODY(jacSchurRun<T>(s, h, SchurPrecondApply, q, nullptr, nullptr, minv, r, nullptr, nullptr, z, work,  \
                              state, nullptr, batch, false, kind))
BSP_JAC_SCHUR_API(f64, double)
BSP_JAC_SCHUR_API(f32, float)
#undef BSP_JAC_SCHUR_API
// ---- the block diagonal of S as preconditioner of the reduced system -------------
int bsp_jac_schur_sjacobi_info(const bsp_jac_schur* h, int64_t out[8]) {
  BSP_TRY
  if (h == nullptr || out == nullptr) throw std::runtime_error("bsp_jac_schur_sjacobi_info: NULL argument");
  const JacSchurMap& m = *h->map;
  const JacSchurJacobiPlan& pl = jacSchurJacobiPlan(m);
  const int64_t v[8] = {pl.numBlocks,
                        pl.numReal,
                        pl.numPseudo,
                        pl.numPairRows(),
                        pl.numChunks(),
                        pl.inverseElems(),
                        pl.partialElems(),
                        pl.deviceBytes() + (int64_t)((m.keptBlockStart.size() + m.keptScalarBlock.size() +
                                                      m.keptWidth.size() + m.keptFirst.size()) *
                                                     sizeof(int32_t))};
  std::copy(v, v + 8, out);
  BSP_CATCH
}
int bsp_jac_schur_sjacobi_table(const bsp_jac_schur* h, int32_t part, int32_t* t0, int32_t* t1, int32_t* t2,
                                int64_t* t3) {
  BSP_TRY
  if (h == nullptr) throw std::runtime_error("bsp_jac_schur_sjacobi_table: the map is NULL");
  const auto put = [](const auto& v, auto* out) {
    if (!v.empty() && out == nullptr) throw std::runtime_error("bsp_jac_schur_sjacobi_table: an output array is NULL");
    std::copy(v.begin(), v.end(), out);
  };
  const JacSchurMap& m = *h->map;
  if (part < 0 || part > 3) {
    throw std::runtime_error("bsp_jac_schur_sjacobi_table: unknown part " + std::to_string(part) +
                             " (0: blocks, 1: chunks, 2: pairs, 3: pair-rows and records)");
  }
  const JacSchurJacobiPlan& pl = jacSchurJacobiPlan(m);
  if (part == 0) {
    put(pl.blockPair, t0);
    put(pl.blockChunk, t1);
    put(m.keptWidth, t2);
    put(pl.blockOff, t3);
  } else if (part == 1) {
    put(pl.chunkPair, t0);
    put(pl.chunkBlock, t1);
    put(pl.chunkPart, t3);
  } else if (part == 2) {
    put(pl.pairElim, t0);
    put(pl.pairRow, t1);
    put(pl.pairRec, t2);
  } else {
    put(pl.rowOf, t0);
    put(pl.rec, t1);
  }
  BSP_CATCH
}
int bsp_jac_schur_kept_plan_built(const bsp_jac_schur* h, int32_t* out) {
  BSP_TRY
  if (h == nullptr || out == nullptr) throw std::runtime_error("bsp_jac_schur_kept_plan_built: NULL argument");
  *out = h->map->keptBlocks ? 1 : 0;
  BSP_CATCH
}
template <typename T>
static void jacSchurJacobiRun(bsp_solver* s, const bsp_jac_schur* h, int32_t op, int64_t q, const T* const* v,
                              const T* const* binv, const T* const* d, double* const* partials, const T* const* vec,
                              T* const* out, void* work, int64_t* state, int64_t* status, int32_t batch, bool single) {
  if (s == nullptr) throw std::runtime_error("jacobian schur: the solver is NULL");
  if (h == nullptr) throw std::runtime_error("jacobian schur: the map is NULL");
  JacSchurArgs<T> a;
  a.op = op;
  a.q = q;
  a.map = h->map.get();
  a.values = v;
  a.binv = binv;
  a.damp = d;
  a.partials = partials;
  a.vec = vec;
  a.out = out;
  a.work = work;
  a.state = state;
  a.status = status;
  s->solver->jacSchur<T>(a, batch, single);
}
#define BSP_JAC_SCHUR_SJACOBI_API(SFX, T)                                                                         \
  int bsp_jac_schur_sjacobi_build_##SFX(bsp_solver* s, const bsp_jac_schur* h, const T* v, const T* binv,         \
                                        const T* d, double* partials, T* minv, void* work, int64_t* status)      \
      BSP_BODY(jacSchurJacobiRun<T>(s, h, SchurSJacobiBuild, 1, &v, &binv, one(d), &partials, nullptr, &minv,     \
                                    work, nullptr, status, 1, true))                                              \
  int bsp_jac_schur_sjacobi_build_batched_##SFX(bsp_solver* s, const bsp_jac_schur* h, const T* const* v,         \
                                                const T* const* binv, const T* const* d,                          \
                                                double* const* partials, T* const* minv, void* work,              \
                                                int64_t* status, int32_t batch)                                   \
      BSP_BODY(jacSchurJacobiRun<T>(s, h, SchurSJacobiBuild, 1, v, binv, d, partials, nullptr, minv, work,        \
                                    nullptr, status, batch, false))                                               \
  int bsp_jac_schur_sjacobi_apply_##SFX(bsp_solver* s, const bsp_jac_schur* h, int64_t q, const T* minv,          \
                                        const T* r, T* z, void* work, int64_t* state)                             \
      BSP_BODY(jacSchurJacobiRun<T>(s, h, SchurSJacobiApply, q, nullptr, &minv, nullptr, nullptr, &r, &z, work,   \
                                    state, nullptr, 1, true))                                                     \
  int bsp_jac_schur_sjacobi_apply_batched_##SFX(bsp_solver* s, const bsp_jac_schur* h, int64_t q,                 \
                                                const T* const* minv, const T* const* r, T* const* z,             \
                                                void* work, int64_t* state, int32_t batch)                        \
      BSP_BODY(jacSchurJacobiRun<T>(s, h, SchurSJacobiApply, q, nullptr, minv, nullptr, nullptr, r, z, work,      \
                                    state, nullptr, batch, false))
BSP_JAC_SCHUR_SJACOBI_API(f64, double)
BSP_JAC_SCHUR_SJACOBI_API(f32, float)
#undef BSP_JAC_SCHUR_SJACOBI_API
#undef BSP_CC
#undef BSP_CD
// ---- the Lanczos recurrence -----------------------------------------------------
int bsp_lanczos_state_words(int64_t* out) {
  BSP_TRY
  if (out == nullptr) throw std::runtime_error("bsp_lanczos_state_words: out is NULL");
  *out = 12;
  BSP_CATCH
}
int bsp_lanczos_work_bytes(const bsp_solver* s, int64_t n, int64_t q, int64_t kmax, int64_t* out) {
  BSP_TRY
  if (s == nullptr || out == nullptr) throw std::runtime_error("bsp_lanczos_work_bytes: NULL argument");
  *out = s->solver->lanczosWorkBytes(n, q, kmax);
  BSP_CATCH
}
template <typename T>
static void lanczosRun(bsp_solver* s, int32_t op, int64_t n, int64_t q, int64_t kmax, const T* const* vec,
                       T* const* basis, int64_t slotStride, int64_t slots, int64_t slot, int64_t prev, int64_t count,
                       bool fold, double breakdown, double* coef, void* work, int64_t* state, int32_t batch,
                       bool single) {
  if (s == nullptr) throw std::runtime_error("lanczos: the solver is NULL");
  LanczosArgs<T> a;
  a.op = op;
  a.fold = fold;
  a.n = n;
  a.q = q;
  a.kmax = kmax;
  a.slots = slots;
  a.slotStride = slotStride;
  a.slot = slot;
  a.prev = prev;
  a.count = count;
  a.breakdown = breakdown;
  a.vec = const_cast<T* const*>(vec);  // (written by LzUpdate and LzSubtract only, whose entries take T*)
  a.basis = basis;
  a.coef = coef;
  a.work = work;
  a.state = state;
  s->solver->lanczos<T>(a, batch, single);
}
#define BSP_LZ_HEAD bsp_solver *s, int64_t n, int64_t q, int64_t kmax
#define BSP_LZ_BASIS(P) P basis, int64_t slot_stride, int64_t slots
#define BSP_LANCZOS_API(SFX, T)                                                                                   \
  int bsp_lanczos_init_##SFX(BSP_LZ_HEAD, const T* v0, BSP_LZ_BASIS(T*), int64_t slot, double breakdown,           \
                             void* work, int64_t* state)                                                           \
      BSP_BODY(lanczosRun<T>(s, LzInit, n, q, kmax, &v0, &basis, slot_stride, slots, slot, 0, 0, false, breakdown, \
                             nullptr, work, state, 1, true))                                                       \
  int bsp_lanczos_init_batched_##SFX(BSP_LZ_HEAD, const T* const* v0, BSP_LZ_BASIS(T* const*), int64_t slot,       \
                                     double breakdown, void* work, int64_t* state, int32_t batch)                  \
      BSP_BODY(lanczosRun<T>(s, LzInit, n, q, kmax, v0, basis, slot_stride, slots, slot, 0, 0, false, breakdown,   \
                             nullptr, work, state, batch, false))                                                  \
  int bsp_lanczos_alpha_##SFX(BSP_LZ_HEAD, const T* w, BSP_LZ_BASIS(const T*), int64_t slot, void* work,           \
                              int64_t* state) {                                                                    \
    T* bm = const_cast<T*>(basis);                                                                                 \
    BSP_TRY lanczosRun<T>(s, LzAlpha, n, q, kmax, &w, &bm, slot_stride, slots, slot, 0, 0, false, 0, nullptr,      \
                          work, state, 1, true);                                                                   \
    BSP_CATCH                                                                                                      \
  }                                                                                                                \
  int bsp_lanczos_alpha_batched_##SFX(BSP_LZ_HEAD, const T* const* w, BSP_LZ_BASIS(const T* const*), int64_t slot, \
                                      void* work, int64_t* state, int32_t batch)                                   \
      BSP_BODY(lanczosRun<T>(s, LzAlpha, n, q, kmax, w, (T* const*)basis, slot_stride, slots, slot, 0, 0, false,   \
                             0, nullptr, work, state, batch, false))                                               \
  int bsp_lanczos_update_##SFX(BSP_LZ_HEAD, T* w, BSP_LZ_BASIS(const T*), int64_t slot, int64_t prev,              \
                               int32_t fold, double* coef, void* work, int64_t* state) {                           \
    T* bm = const_cast<T*>(basis);                                                                                 \
    const T* wc = w;                                                                                               \
    BSP_TRY lanczosRun<T>(s, LzUpdate, n, q, kmax, &wc, &bm, slot_stride, slots, slot, prev, 0, fold != 0, 0,      \
                          coef, work, state, 1, true);                                                             \
    BSP_CATCH                                                                                                      \
  }                                                                                                                \
  int bsp_lanczos_update_batched_##SFX(BSP_LZ_HEAD, T* const* w, BSP_LZ_BASIS(const T* const*), int64_t slot,      \
                                       int64_t prev, int32_t fold, double* coef, void* work, int64_t* state,       \
                                       int32_t batch)                                                              \
      BSP_BODY(lanczosRun<T>(s, LzUpdate, n, q, kmax, (const T* const*)w, (T* const*)basis, slot_stride, slots,    \
                             slot, prev, 0, fold != 0, 0, coef, work, state, batch, false))                        \
  int bsp_lanczos_project_##SFX(BSP_LZ_HEAD, const T* w, BSP_LZ_BASIS(const T*), int64_t count, void* work,        \
                                int64_t* state) {                                                                  \
    T* bm = const_cast<T*>(basis);                                                                                 \
    BSP_TRY lanczosRun<T>(s, LzProject, n, q, kmax, &w, &bm, slot_stride, slots, 0, 0, count, false, 0, nullptr,   \
                          work, state, 1, true);                                                                   \
    BSP_CATCH                                                                                                      \
  }                                                                                                                \
  int bsp_lanczos_project_batched_##SFX(BSP_LZ_HEAD, const T* const* w, BSP_LZ_BASIS(const T* const*),             \
                                        int64_t count, void* work, int64_t* state, int32_t batch)                  \
      BSP_BODY(lanczosRun<T>(s, LzProject, n, q, kmax, w, (T* const*)basis, slot_stride, slots, 0, 0, count,       \
                             false, 0, nullptr, work, state, batch, false))                                        \
  int bsp_lanczos_subtract_##SFX(BSP_LZ_HEAD, T* w, BSP_LZ_BASIS(const T*), int64_t count, int32_t fold,           \
                                 double* coef, void* work, int64_t* state) {                                       \
    T* bm = const_cast<T*>(basis);                                                                                 \
    const T* wc = w;                                                                                               \
    BSP_TRY lanczosRun<T>(s, LzSubtract, n, q, kmax, &wc, &bm, slot_stride, slots, 0, 0, count, fold != 0, 0,      \
                          coef, work, state, 1, true);                                                             \
    BSP_CATCH                                                                                                      \
  }                                                                                                                \
  int bsp_lanczos_subtract_batched_##SFX(BSP_LZ_HEAD, T* const* w, BSP_LZ_BASIS(const T* const*), int64_t count,   \
                                         int32_t fold, double* coef, void* work, int64_t* state, int32_t batch)    \
      BSP_BODY(lanczosRun<T>(s, LzSubtract, n, q, kmax, (const T* const*)w, (T* const*)basis, slot_stride, slots,  \
                             0, 0, count, fold != 0, 0, coef, work, state, batch, false))                          \
  int bsp_lanczos_normalize_##SFX(BSP_LZ_HEAD, const T* w, BSP_LZ_BASIS(T*), int64_t slot, void* work,             \
                                  int64_t* state)                                                                  \
      BSP_BODY(lanczosRun<T>(s, LzNormalize, n, q, kmax, &w, &basis, slot_stride, slots, slot, 0, 0, false, 0,     \
                             nullptr, work, state, 1, true))                                                       \
  int bsp_lanczos_normalize_batched_##SFX(BSP_LZ_HEAD, const T* const* w, BSP_LZ_BASIS(T* const*), int64_t slot,   \
                                          void* work, int64_t* state, int32_t batch)                               \
      BSP_BODY(lanczosRun<T>(s, LzNormalize, n, q, kmax, w, basis, slot_stride, slots, slot, 0, 0, false, 0,       \
                             nullptr, work, state, batch, false))
BSP_LANCZOS_API(f64, double)
BSP_LANCZOS_API(f32, float)
#undef BSP_LANCZOS_API
#undef BSP_LZ_BASIS
#undef BSP_LZ_HEAD
// ---- combinations of basis vectors ----------------------------------------------
template <typename T>
static void krylovCombineRun(bsp_solver* s, int64_t n, int64_t q, int32_t nf, const T* const* basis,
                             int64_t slotStride, int64_t slots, int64_t slot, int64_t count, int64_t first,
                             const double* y, int64_t ldy, const int64_t* limit, T* const* out, int64_t outStride,
                             int32_t accumulate, int32_t batch, bool single) {
  if (s == nullptr) throw std::runtime_error("krylovCombine: the solver is NULL");
  KrylovCombineArgs<T> a;
  a.n = n;
  a.q = q;
  a.nf = nf;
  a.slots = slots;
  a.slotStride = slotStride;
  a.slot = slot;
  a.count = count;
  a.first = first;
  a.ldy = ldy;
  a.outStride = outStride;
  a.accumulate = accumulate != 0;
  a.basis = basis;
  a.y = y;
  a.limit = limit;
  a.out = out;
  s->solver->krylovCombine<T>(a, batch, single);
}
#define BSP_KV_MID                                                                                            \
  int64_t slot_stride, int64_t slots, int64_t slot, int64_t count, int64_t first, const double *y, int64_t ldy, \
      const int64_t *limit
#define BSP_KRYLOV_API(SFX, T)                                                                                  \
  int bsp_krylov_combine_##SFX(bsp_solver* s, int64_t n, int64_t q, int32_t nf, const T* basis, BSP_KV_MID,     \
                               T* out, int64_t out_stride, int32_t accumulate)                                  \
      BSP_BODY(krylovCombineRun<T>(s, n, q, nf, &basis, slot_stride, slots, slot, count, first, y, ldy, limit,  \
                                   &out, out_stride, accumulate, 1, true))                                      \
  int bsp_krylov_combine_batched_##SFX(bsp_solver* s, int64_t n, int64_t q, int32_t nf, const T* const* basis,  \
                                       BSP_KV_MID, T* const* out, int64_t out_stride, int32_t accumulate,       \
                                       int32_t batch)                                                           \
      BSP_BODY(krylovCombineRun<T>(s, n, q, nf, basis, slot_stride, slots, slot, count, first, y, ldy, limit,   \
                                   out, out_stride, accumulate, batch, false))
BSP_KRYLOV_API(f64, double)
BSP_KRYLOV_API(f32, float)
#undef BSP_KRYLOV_API
#undef BSP_KV_MID
int bsp_scalar_permutation(const bsp_solver* s, int64_t* out) {
  BSP_TRY
  if (out == nullptr) throw std::runtime_error("bsp_scalar_permutation: out is NULL");
  const std::vector<int64_t> p = s->solver->scalarPermutation();
  std::copy(p.begin(), p.end(), out);
  BSP_CATCH
}
int bsp_test_set_selinv_batch_chunk(bsp_solver* s, int32_t max_matrices) {
  BSP_TRY
  if (max_matrices < 0) throw std::runtime_error("bsp_test_set_selinv_batch_chunk: max_matrices < 0");
  hipBackendSetSelInvBatchChunk(s->solver->internalSymbolicContext(), max_matrices);
  BSP_CATCH
}
int bsp_test_ptr_ring_slot_bytes(bsp_solver* s, int64_t* out) {
  BSP_TRY
  if (out == nullptr) throw std::runtime_error("bsp_test_ptr_ring_slot_bytes: out is NULL");
  *out = hipBackendPtrRingSlotBytes(s->solver->internalSymbolicContext());
  BSP_CATCH
}
int bsp_pseudo_factor_from_f64(bsp_solver* s, double* d, int64_t span) {
  BSP_TRY
  s->solver->pseudoFactorFrom(d, span);
  BSP_CATCH
}
int bsp_pseudo_factor_from_f32(bsp_solver* s, float* d, int64_t span) {
  BSP_TRY
  s->solver->pseudoFactorFrom(d, span);
  BSP_CATCH
}

// batched solve: which = 0 solve, 1 solveL, 2 solveLt
template <typename T>
static void solveBatched(bsp_solver* s, const T* const* mats, T* const* vecs, int32_t batch,
                         int64_t stride, int32_t nrhs, int32_t which) {
  std::vector<T*> m(batch), v(vecs, vecs + batch);
  for (int32_t q = 0; q < batch; q++) m[q] = const_cast<T*>(mats[q]);
  if (which == 0) {
    s->solver->solve(&m, &v, stride, nrhs);
  } else if (which == 1) {
    s->solver->solveL(&m, &v, stride, nrhs);
  } else if (which == 2) {
    s->solver->solveLt(&m, &v, stride, nrhs);
  } else {
    throw std::runtime_error("bsp_solve_batched: which must be 0 (solve), 1 (L) or 2 (Lt)");
  }
}
// batched partial factor: which = 0 factorUpTo, 1 factorFrom
template <typename T>
static void factorPartialBatched(bsp_solver* s, T* const* ptrs, int32_t batch, int64_t span,
                                 int32_t which) {
  std::vector<T*> v(ptrs, ptrs + batch);
  if (which == 0) {
    s->solver->factorUpTo(&v, span);
  } else if (which == 1) {
    s->solver->factorFrom(&v, span);
  } else {
    throw std::runtime_error("bsp_factor_partial_batched: which must be 0 (UpTo) or 1 (From)");
  }
}
int bsp_factor_partial_batched_f64(bsp_solver* s, double* const* ptrs, int32_t batch, int64_t span,
                                   int32_t which) {
  BSP_TRY
  factorPartialBatched<double>(s, ptrs, batch, span, which);
  BSP_CATCH
}
int bsp_factor_partial_batched_f32(bsp_solver* s, float* const* ptrs, int32_t batch, int64_t span,
                                   int32_t which) {
  BSP_TRY
  factorPartialBatched<float>(s, ptrs, batch, span, which);
  BSP_CATCH
}
// batched partial solves: which as bsp_solve_partial (0 LUpTo, 1 LtUpTo, 2 LFrom, 3 LtFrom)
template <typename T>
static void solvePartialBatched(bsp_solver* s, const T* const* mats, T* const* vecs, int32_t batch,
                                int64_t stride, int32_t nrhs, int32_t which, int64_t span) {
  std::vector<T*> m(batch), v(vecs, vecs + batch);
  for (int32_t q = 0; q < batch; q++) m[q] = const_cast<T*>(mats[q]);
  if (which == 0) {
    s->solver->solveLUpTo(&m, span, &v, stride, nrhs);
  } else if (which == 1) {
    s->solver->solveLtUpTo(&m, span, &v, stride, nrhs);
  } else if (which == 2) {
    s->solver->solveLFrom(&m, span, &v, stride, nrhs);
  } else if (which == 3) {
    s->solver->solveLtFrom(&m, span, &v, stride, nrhs);
  } else {
    throw std::runtime_error("bsp_solve_partial_batched: which must be 0..3");
  }
}
int bsp_solve_partial_batched_f64(bsp_solver* s, const double* const* mats, double* const* vecs,
                                  int32_t batch, int64_t stride, int32_t nrhs, int32_t which,
                                  int64_t span) {
  BSP_TRY
  solvePartialBatched<double>(s, mats, vecs, batch, stride, nrhs, which, span);
  BSP_CATCH
}
int bsp_solve_partial_batched_f32(bsp_solver* s, const float* const* mats, float* const* vecs,
                                  int32_t batch, int64_t stride, int32_t nrhs, int32_t which,
                                  int64_t span) {
  BSP_TRY
  solvePartialBatched<float>(s, mats, vecs, batch, stride, nrhs, which, span);
  BSP_CATCH
}
int bsp_solve_batched_f64(bsp_solver* s, const double* const* mats, double* const* vecs,
                          int32_t batch, int64_t stride, int32_t nrhs, int32_t which) {
  BSP_TRY
  solveBatched<double>(s, mats, vecs, batch, stride, nrhs, which);
  BSP_CATCH
}
int bsp_solve_batched_f32(bsp_solver* s, const float* const* mats, float* const* vecs,
                          int32_t batch, int64_t stride, int32_t nrhs, int32_t which) {
  BSP_TRY
  solveBatched<float>(s, mats, vecs, batch, stride, nrhs, which);
  BSP_CATCH
}

int bsp_bal_linearize_f64(int64_t numObs, const int64_t* obsCam, const int64_t* obsPt,
                          const double* obsXy, const double* cams, const double* pts, double* res,
                          double* Jc, double* Jp, void* stream) {
  BSP_TRY
  balLinearize(numObs, obsCam, obsPt, obsXy, cams, pts, res, Jc, Jp, stream);
  BSP_CATCH
}
// bsp_bal_fill_hessian_*: the kernels hard-code 3 x 3 point blocks, 9 x 9 camera blocks and 9 x 3
// camera-point blocks, points first -- a solver with any other parameter sizes would send their
// atomics out of bounds, so the layout is checked on the host before the launch
static void checkBalLayout(bsp_solver* s, int64_t numPts, int64_t numCams, int64_t camSize = 9) {
  if (s->balOk[0] == numPts && s->balOk[1] == numCams && s->balOk[2] == camSize) return;
  const BaSpaCho::Solver& solver = *s->solver;
  if (camSize != 9 && camSize != 6) throw std::runtime_error("bsp_bal_fill_hessian: camera size must be 9 or 6");
  BASPACHO_CHECK_GE(numPts, 0);
  BASPACHO_CHECK_GE(numCams, 0);
  BASPACHO_CHECK_EQ(numPts + numCams, solver.skel().numSpans());
  const auto acc = solver.accessor();
  for (int64_t p = 0; p < numPts + numCams; p++) {
    const int64_t want = p < numPts ? 3 : camSize;
    if (acc.paramSize(p) != want) {
      throw std::runtime_error("bsp_bal_fill_hessian: parameter " + std::to_string(p) + " has size " +
                               std::to_string(acc.paramSize(p)) + ", the BAL layout needs " +
                               std::to_string(want) + " (points of size 3 first, then cameras of size " +
                               std::to_string(camSize) + ")");
    }
  }
  s->balOk[0] = numPts;
  s->balOk[1] = numCams;
  s->balOk[2] = camSize;
}

int bsp_bal_fill_hessian_f64(bsp_solver* s, int64_t numPts, int64_t numCams, int64_t numObs,
                             const int64_t* obsCam, const int64_t* obsPt, const double* Jc,
                             const double* Jp, const double* res, double lambda, double* data,
                             double* grad, int64_t* dbg, void* stream) {
  BSP_TRY
  checkBalLayout(s, numPts, numCams);
  balFillHessian<double>(s->solver->deviceAccessor(), 9, numPts, numCams, numObs, obsCam, obsPt, Jc, Jp,
                         res, lambda, data, grad, dbg, stream);
  BSP_CATCH
}
int bsp_bal_fill_hessian_f32(bsp_solver* s, int64_t numPts, int64_t numCams, int64_t numObs,
                             const int64_t* obsCam, const int64_t* obsPt, const double* Jc,
                             const double* Jp, const double* res, float lambda, float* data,
                             float* grad, int64_t* dbg, void* stream) {
  BSP_TRY
  checkBalLayout(s, numPts, numCams);
  balFillHessian<float>(s->solver->deviceAccessor(), 9, numPts, numCams, numObs, obsCam, obsPt, Jc, Jp,
                        res, lambda, data, grad, dbg, stream);
  BSP_CATCH
}

int bsp_bal_linearize_se3_f64(int64_t numObs, const int64_t* obsCam, const int64_t* obsPt,
                              const double* obsXy, const double* cams, const double* pts, double* res,
                              double* Jc, double* Jp, void* stream) {
  BSP_TRY
  balLinearizeSe3(numObs, obsCam, obsPt, obsXy, cams, pts, res, Jc, Jp, stream);
  BSP_CATCH
}
int bsp_bal_fill_hessian_se3_f64(bsp_solver* s, int64_t numPts, int64_t numCams, int64_t numObs,
                                 const int64_t* obsCam, const int64_t* obsPt, const double* Jc,
                                 const double* Jp, const double* res, double lambda, double* data,
                                 double* grad, void* stream) {
  BSP_TRY
  checkBalLayout(s, numPts, numCams, 6);
  balFillHessian<double>(s->solver->deviceAccessor(), 6, numPts, numCams, numObs, obsCam, obsPt, Jc, Jp,
                         res, lambda, data, grad, nullptr, stream);
  BSP_CATCH
}
int bsp_bal_fill_hessian_se3_f32(bsp_solver* s, int64_t numPts, int64_t numCams, int64_t numObs,
                                 const int64_t* obsCam, const int64_t* obsPt, const double* Jc,
                                 const double* Jp, const double* res, float lambda, float* data,
                                 float* grad, void* stream) {
  BSP_TRY
  checkBalLayout(s, numPts, numCams, 6);
  balFillHessian<float>(s->solver->deviceAccessor(), 6, numPts, numCams, numObs, obsCam, obsPt, Jc, Jp,
                        res, lambda, data, grad, nullptr, stream);
  BSP_CATCH
}

// ---- ordered fill (bal_fill_plan.h): a plan per problem, then the fill without atomics
struct bsp_bal_fill_plan {
  std::unique_ptr<BalFillPlan> plan;
};

int bsp_bal_fill_plan_create(bsp_solver* s, int32_t camSize, int64_t numPts, int64_t numCams, int64_t numObs,
                             const int64_t* obsCam, const int64_t* obsPt, bsp_bal_fill_plan** out) {
  BSP_TRY
  if (s == nullptr || out == nullptr) throw std::runtime_error("bsp_bal_fill_plan_create: NULL solver or output");
  std::unique_ptr<bsp_bal_fill_plan> p(new bsp_bal_fill_plan);
  p->plan = createBalFillPlan(*s->solver, camSize, numPts, numCams, numObs, obsCam, obsPt);
  *out = p.release();
  BSP_CATCH
}
void bsp_bal_fill_plan_destroy(bsp_bal_fill_plan* p) { delete p; }
int bsp_bal_fill_plan_info(const bsp_bal_fill_plan* p, int64_t out[12]) {
  BSP_TRY
  if (p == nullptr || out == nullptr) throw std::runtime_error("bsp_bal_fill_plan_info: NULL argument");
  const BalFillPlan& m = *p->plan;
  const int64_t v[12] = {m.numKept,    m.numSkipped, m.numPairs(),   m.numChunks(), kBalFillChunk,    kBalFillLanes,
                         m.maxPtList,  m.maxCamList, m.scratchLen(), m.hostBytes(), m.deviceBytes(), m.camSize};
  std::copy(v, v + 12, out);
  BSP_CATCH
}
template <typename T>
static void balFillOrderedRun(bsp_solver* s, const bsp_bal_fill_plan* p, const double* Jc, const double* Jp,
                              const double* res, T lambda, T* data, T* grad, void* stream) {
  const std::string what = "bsp_bal_fill_ordered: ";
  if (s == nullptr) throw std::runtime_error(what + "the solver is NULL");
  if (p == nullptr) throw std::runtime_error(what + "the plan is NULL");
  const BalFillPlan& m = *p->plan;
  if (m.solver != s->solver.get()) throw std::runtime_error(what + "the plan was built for another solver");
  if (data == nullptr) throw std::runtime_error(what + "data is NULL");
  if (m.numObs > 0 && (Jc == nullptr || Jp == nullptr || res == nullptr)) {
    throw std::runtime_error(what + "Jc, Jp or res is NULL");
  }
  balFillOrdered<T>(m, Jc, Jp, res, lambda, data, grad, stream);
}
int bsp_bal_fill_ordered_f64(bsp_solver* s, const bsp_bal_fill_plan* p, const double* Jc, const double* Jp,
                             const double* res, double lambda, double* data, double* grad, void* stream)
    BSP_BODY(balFillOrderedRun<double>(s, p, Jc, Jp, res, lambda, data, grad, stream))
int bsp_bal_fill_ordered_f32(bsp_solver* s, const bsp_bal_fill_plan* p, const double* Jc, const double* Jp,
                             const double* res, float lambda, float* data, float* grad, void* stream)
    BSP_BODY(balFillOrderedRun<float>(s, p, Jc, Jp, res, lambda, data, grad, stream))

// the plan's tables for the CPU tests (layout: include/baspacho_amd_testing.h)
int bsp_test_bal_fill_plan(const bsp_bal_fill_plan* p, int64_t* buf, int64_t capacity, int64_t* needed) {
  BSP_TRY
  if (p == nullptr || needed == nullptr) throw std::runtime_error("bsp_test_bal_fill_plan: NULL argument");
  const BalFillPlan& m = *p->plan;
  std::vector<int64_t> v = {m.numPts,       m.numCams,     m.camSize,     m.numKept,     m.numSkipped,
                            m.numPairs(),   m.numChunks(), kBalFillChunk, kBalFillLanes, m.scratchLen()};
  auto put = [&v](const auto& a) { v.insert(v.end(), a.begin(), a.end()); };
  put(m.ptPtr);
  put(m.ptObs);
  put(m.pairPtr);
  put(m.pairCam);
  put(m.pairPt);
  put(m.pairOff);
  put(m.pairStride);
  put(m.pairFlip);
  put(m.camPtr);
  put(m.camObs);
  put(m.camChunkPtr);
  put(m.chunkCam);
  put(m.chunkBegin);
  put(m.chunkEnd);
  put(m.ptDiagOff);
  put(m.ptDiagStride);
  put(m.ptStart);
  put(m.camDiagOff);
  put(m.camDiagStride);
  put(m.camStart);
  *needed = (int64_t)v.size();
  if (buf != nullptr) std::copy(v.begin(), v.begin() + std::min<int64_t>(capacity, *needed), buf);
  BSP_CATCH
}

int bsp_bal_residuals_f64(int64_t numObs, const int64_t* obsCam, const int64_t* obsPt,
                          const double* obsXy, const double* cams, const double* pts, double* res,
                          void* stream) {
  BSP_TRY
  balResiduals(numObs, obsCam, obsPt, obsXy, cams, pts, res, stream);
  BSP_CATCH
}
int bsp_bal_residuals_se3_f64(int64_t numObs, const int64_t* obsCam, const int64_t* obsPt,
                              const double* obsXy, const double* cams, const double* pts, double* res,
                              void* stream) {
  BSP_TRY
  balResidualsSe3(numObs, obsCam, obsPt, obsXy, cams, pts, res, stream);
  BSP_CATCH
}
int bsp_bal_loss_f64(int64_t numObs, int32_t camSize, int32_t kind, double a, double* res, double* Jc,
                     double* Jp, double* rho, void* stream) {
  BSP_TRY
  balLoss(numObs, camSize, kind, a, res, Jc, Jp, rho, stream);
  BSP_CATCH
}
int64_t bsp_bal_sum_scratch_len(int64_t n) { return balSumScratchLen(n); }
int bsp_bal_sum_f64(int64_t n, const double* x, double scale, double* scratch, double* out, void* stream) {
  BSP_TRY
  balSum(n, x, scale, scratch, out, stream);
  BSP_CATCH
}
// bsp_bal_apply_step_*: the kernels read 3 (points) and 9 or 6 (cameras) words of `step` at
// paramStart(p), so the layout is checked as for the fill
int bsp_bal_apply_step_f64(bsp_solver* s, int64_t numPts, int64_t numCams, const double* cams,
                           const double* pts, const double* step, double* camsOut, double* ptsOut,
                           void* stream) {
  BSP_TRY
  checkBalLayout(s, numPts, numCams);
  BASPACHO_CHECK_EQ(s->solver->order(), 3 * numPts + 9 * numCams);
  balApplyStep(s->solver->deviceAccessor(), numPts, numCams, cams, pts, step, camsOut, ptsOut, stream);
  BSP_CATCH
}
int bsp_bal_apply_step_se3_f64(bsp_solver* s, int64_t numPts, int64_t numCams, const double* cams,
                               const double* pts, const double* step, double* camsOut, double* ptsOut,
                               void* stream) {
  BSP_TRY
  checkBalLayout(s, numPts, numCams, 6);
  BASPACHO_CHECK_EQ(s->solver->order(), 3 * numPts + 6 * numCams);
  balApplyStepSe3(s->solver->deviceAccessor(), numPts, numCams, cams, pts, step, camsOut, ptsOut, stream);
  BSP_CATCH
}

double bsp_factor_flops(const bsp_solver* s) { return s->solver->factorFlops(); }

int64_t bsp_plan_levels(bsp_solver* s, int64_t* out, int64_t capacity) {
  try {
    std::vector<int64_t> v = hipBackendPlanLevels(s->solver->internalSymbolicContext(), 0,
                                                  s->solver->skel().numLumps());
    const int64_t n = (int64_t)v.size();
    if (out) std::copy(v.begin(), v.begin() + std::min(n, capacity), out);
    return n;
  } catch (const std::exception& e) {
    g_lastError = e.what();
    return -1;
  }
}

int bsp_plan_stats_full(bsp_solver* s, bsp_plan_stats* out) {
  BSP_TRY
  HipPlanStats p = hipBackendPlanStats(s->solver->internalSymbolicContext(), 0,
                                       s->solver->skel().numLumps());
  out->flops = p.flops;
  out->upd_elems = p.updElems;
  out->upd_flops = p.updFlops;
  out->elim_pair_elems = p.elimPairElems;
  out->elim_pair_flops = p.elimPairFlops;
  out->elim_col_elems = p.elimColElems;
  out->upd_flops_direct = p.updFlopsDirect;
  out->elim_pair_operand_elems = p.elimPairOperandElems;
  out->elim_target_elems = p.elimTargetElems;
  out->trsm_flops = p.trsmFlops;
  out->potrf_flops = p.potrfFlops;
  out->trsm_flops_merged = p.trsmFlopsMerged;
  out->potrf_flops_fused = p.potrfFlopsFused;
  out->num_launches = p.numLaunches;
  out->num_levels = p.numLevels;
  out->num_panels = p.numPanels;
  out->num_segs = p.numSegs;
  out->num_upd_tasks = p.numUpdTasks;
  out->num_trsm_tasks = p.numTrsmTasks;
  out->chain_tab_entries = p.chainTabEntries;
  out->max_panels_in_level = p.maxPanelsInLevel;
  out->num_atomic_upd_tasks = p.numAtomicUpdTasks;
  out->num_gather_groups = p.numGatherGroups;
  out->num_fork_levels = p.numForkLevels;
  out->deferred_flops = p.deferredFlops;
  out->tail_upd_flops = p.tailUpdFlops;
  out->num_tail_panels = p.numTailPanels;
  BSP_CATCH
}

int bsp_run_counters_get(bsp_solver* s, bsp_run_counters* out) {
  BSP_TRY
  const HipRunCounters c = hipBackendRunCounters(s->solver->internalSymbolicContext());
  out->sweep_launches = c.sweepLaunches;
  out->sweep_timeouts = c.sweepTimeouts;
  out->split_lists_used = c.splitListsUsed;
  out->sub_batches_enqueued = c.subBatchesEnqueued;
  out->lookahead_forks = c.lookaheadForks;
  out->sweeps_retired = c.sweepsRetired;
  out->sweep_error_pending = c.sweepErrorPending;
  out->gather_chunks_overlapped = 0;
  out->tail_launches = c.tailLaunches;
  out->sweep_mfma_launches = c.sweepMfmaLaunches;
  out->solve_wide_launches = c.solveWideLaunches;
  out->inv_reused = c.invReused;
  out->potrf_folded_levels = c.potrfFoldedLevels;
  out->selinv_launches = c.selinvLaunches;
  out->selinv_chunks = c.selinvChunks;
  BSP_CATCH
}

int bsp_probe_mfma_f64(double* tflops) {
  BSP_TRY
  *tflops = hipBackendMfmaF64ProbeTflops();
  BSP_CATCH
}

int bsp_debug_read_extents(unsigned long long* out, int max_launches, int* n) {
  BSP_TRY
  *n = hipBackendReadExtents(out, max_launches);
  BSP_CATCH
}
int bsp_debug_read_trace(long long* out, int max_records, int* n_records) {
  BSP_TRY
  *n_records = hipBackendReadTrace(out, max_records);
  BSP_CATCH
}

static void factorProfiled(bsp_solver* s, double* d, bool inSitu, double ms[6], int64_t launches[6],
                           double* busy = nullptr) {
  HipKernelProfile prof;
  SymbolicCtx& sym = s->solver->internalSymbolicContext();
  hipBackendSetProfile(sym, &prof, inSitu);
  try {
    s->solver->factor(d);
  } catch (...) {
    hipBackendSetProfile(sym, nullptr);
    throw;
  }
  hipBackendSetProfile(sym, nullptr);
  for (int i = 0; i < kProfNumKinds; i++) {
    ms[i] = prof.ms[i];
    launches[i] = prof.launches[i];
    if (busy) busy[i] = prof.busyMs[i];
  }
}
int bsp_factor_profiled_f64(bsp_solver* s, double* d, double ms[6], int64_t launches[6]) {
  BSP_TRY
  factorProfiled(s, d, false, ms, launches);
  BSP_CATCH
}
int bsp_factor_profiled_insitu_f64(bsp_solver* s, double* d, double ms[6], int64_t launches[6]) {
  BSP_TRY
  factorProfiled(s, d, true, ms, launches);
  BSP_CATCH
}
int bsp_factor_profiled_busy_f64(bsp_solver* s, double* d, double ms[6], int64_t launches[6],
                                 double busy_ms[6]) {
  BSP_TRY
  factorProfiled(s, d, true, ms, launches, busy_ms);
  BSP_CATCH
}

// ---- plan (de)serialisation: [magic, canFactorUpTo, nSpans, nLumps, nRowInd, nRanges,
//      spanStart.., lumpToSpan.., colPtr.., rowInd.., ranges.., permutation..]
static const int64_t kPlanMagic = 0x42535041434d4431LL;  // "BSPACMD1"

int bsp_plan_serialize(const bsp_solver* s, int64_t* buf, int64_t capacity, int64_t* needed) {
  BSP_TRY
  const CoalescedBlockMatrixSkel& k = s->solver->skel();
  const auto& ranges = s->solver->sparseEliminationRanges();
  const auto& perm = s->solver->paramToSpan();
  // column pointers / row indices of the lump columns are exactly chainColPtr / chainRowSpan
  const int64_t nSpans = k.numSpans(), nLumps = k.numLumps();
  const int64_t nRow = (int64_t)k.chainRowSpan.size(), nRanges = (int64_t)ranges.size();
  const int64_t total = 6 + (nSpans + 1) + (nLumps + 1) + (nLumps + 1) + nRow + nRanges + nSpans;
  *needed = total;
  if (!buf || capacity < total) return 0;
  int64_t* p = buf;
  *p++ = kPlanMagic;
  *p++ = s->solver->canFactorUpToSpan();
  *p++ = nSpans;
  *p++ = nLumps;
  *p++ = nRow;
  *p++ = nRanges;
  p = std::copy(k.spanStart.begin(), k.spanStart.end(), p);
  p = std::copy(k.lumpToSpan.begin(), k.lumpToSpan.end(), p);
  p = std::copy(k.chainColPtr.begin(), k.chainColPtr.end(), p);
  p = std::copy(k.chainRowSpan.begin(), k.chainRowSpan.end(), p);
  p = std::copy(ranges.begin(), ranges.end(), p);
  p = std::copy(perm.begin(), perm.end(), p);
  BSP_CATCH
}

int bsp_create_solver_from_plan(const int64_t* buf, int64_t len, bsp_solver** out) {
  BSP_TRY
  BASPACHO_CHECK_NOTNULL(out);
  BASPACHO_CHECK_GE(len, 6);
  BASPACHO_CHECK_EQ(buf[0], kPlanMagic);
  const int64_t canUpTo = buf[1], nSpans = buf[2], nLumps = buf[3], nRow = buf[4],
                nRanges = buf[5];
  const int64_t total = 6 + (nSpans + 1) + (nLumps + 1) + (nLumps + 1) + nRow + nRanges + nSpans;
  BASPACHO_CHECK_EQ(len, total);
  const int64_t* p = buf + 6;
  std::vector<int64_t> spanStart(p, p + nSpans + 1);
  p += nSpans + 1;
  std::vector<int64_t> lumpToSpan(p, p + nLumps + 1);
  p += nLumps + 1;
  std::vector<int64_t> colPtr(p, p + nLumps + 1);
  p += nLumps + 1;
  std::vector<int64_t> rowInd(p, p + nRow);
  p += nRow;
  std::vector<int64_t> ranges(p, p + nRanges);
  p += nRanges;
  std::vector<int64_t> perm(p, p + nSpans);
  CoalescedBlockMatrixSkel skel(spanStart, lumpToSpan, colPtr, rowInd);
  std::unique_ptr<bsp_solver> h(new bsp_solver);
  h->solver.reset(
      new Solver(std::move(skel), std::move(ranges), std::move(perm), hipOps(), canUpTo));
  *out = h.release();
  BSP_CATCH
}

int bsp_sparse_structure_op(int op, int64_t n, const int64_t* ptrs, const int64_t* inds,
                            const int64_t* arg, int64_t argLen, int32_t flag, int64_t* outPtrs,
                            int64_t* outInds, int64_t capacity, int64_t* outN, int64_t* outNnz) {
  BSP_TRY
  SparseStructure ss(std::vector<int64_t>(ptrs, ptrs + n + 1),
                     std::vector<int64_t>(inds, inds + ptrs[n]));
  SparseStructure res;
  switch (op) {
    case BSP_SS_TRANSPOSE: res = ss.transpose(); break;
    case BSP_SS_CLEAR: res = ss.clear(flag != 0); break;
    case BSP_SS_SYM_PERMUTATION: {
      BASPACHO_CHECK_EQ(argLen, n);
      res = ss.symmetricPermutation(std::vector<int64_t>(arg, arg + n), flag != 0);
      break;
    }
    case BSP_SS_INDEP_ELIM_FILL:
      BASPACHO_CHECK_EQ(argLen, 2);
      res = ss.addIndependentEliminationFill(arg[0], arg[1]);
      break;
    case BSP_SS_FULL_ELIM_FILL: res = ss.addFullEliminationFill(); break;
    case BSP_SS_FILL_REDUCING_PERM: {
      std::vector<int64_t> perm = ss.fillReducingPermutation();
      *outN = n;
      *outNnz = (int64_t)perm.size();
      if (capacity < (int64_t)perm.size()) throw std::runtime_error("output capacity too small");
      std::copy(perm.begin(), perm.end(), outInds);
      return 0;
    }
    case BSP_SS_EXTRACT_RIGHT_BOTTOM:
      BASPACHO_CHECK_EQ(argLen, 1);
      res = ss.extractRightBottom(arg[0]);
      break;
    default: throw std::runtime_error("bsp_sparse_structure_op: unknown op");
  }
  *outN = res.order();
  *outNnz = (int64_t)res.inds.size();
  if (capacity < (int64_t)res.inds.size()) throw std::runtime_error("output capacity too small");
  std::copy(res.ptrs.begin(), res.ptrs.end(), outPtrs);
  std::copy(res.inds.begin(), res.inds.end(), outInds);
  BSP_CATCH
}
