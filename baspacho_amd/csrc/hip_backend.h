// Extras of the MI355X backend that sit beside the reference boundary (mat_ops.h):
// per-kernel-class event timing and plan statistics, used by bench.py / the C ABI.
#pragma once

#include <cstdint>
#include <vector>

#include "mat_ops.h"

namespace BaSpaCho {

enum HipProfKind {
  kProfElimFactor = 0,
  kProfElimUpdate = 1,
  kProfPotrf = 2,
  kProfTrsm = 3,
  kProfUpdate = 4,       // updateTile launches (task lists; the bulk of the flops)
  kProfChainUpdate = 5,  // updateTileDirect / updateTileDirectPotrf launches of one-panel levels
  kProfNumKinds = 6
};

struct HipKernelProfile {
  double ms[kProfNumKinds] = {0, 0, 0, 0, 0, 0};
  int64_t launches[kProfNumKinds] = {0, 0, 0, 0, 0, 0};
  // time during which AT LEAST ONE launch of the class was running (launches of one class overlap
  // when they go to different streams: their durations then add up to more than the time the class
  // occupies the device)
  double busyMs[kProfNumKinds] = {0, 0, 0, 0, 0, 0};
};

struct HipPlanStats {
  double flops = 0, updElems = 0, updFlops = 0, elimPairElems = 0, elimPairFlops = 0,
         elimColElems = 0, updFlopsDirect = 0, elimPairOperandElems = 0, elimTargetElems = 0,
         trsmFlops = 0, potrfFlops = 0, trsmFlopsMerged = 0, potrfFlopsFused = 0;
  int64_t numLaunches = 0, numLevels = 0, numPanels = 0, numSegs = 0, numUpdTasks = 0,
          numTrsmTasks = 0, chainTabEntries = 0, maxPanelsInLevel = 0, numAtomicUpdTasks = 0,
          numGatherGroups = 0,  // (always 0 since round 4: the overlapped elimination was removed)
          numForkLevels = 0;
  double deferredFlops = 0;
  double tailUpdFlops = 0;  // update flops done inside persistent tail launches (not part of updFlops)
  int64_t numTailPanels = 0;
};

// while `prof` is non-null every kernel launch of the context is bracketed by HIP events and
// accumulated per kernel class (factor calls then synchronise).  inSitu = false: the launches run
// one after the other on the execution stream (lookahead off: isolated kernel times); inSitu =
// true: the real schedule, side-stream launches timed on the side stream (what a kernel takes
// beside the others -- the number a rocprofv3 kernel trace of the timed steps shows)
void hipBackendSetProfile(SymbolicCtx& sym, HipKernelProfile* prof, bool inSitu = false);

// sustained fp64 MFMA rate of this GPU measured with a register-only probe kernel (TFLOP/s)
double hipBackendMfmaF64ProbeTflops();
// in-situ kernel trace (BSP_KTRACE builds only; returns 0 records otherwise)
int hipBackendReadTrace(long long* out, int maxRecords);
// BSP_KTRACE + BSP_TRACE_TILE builds: per chain-step launch {first start, last start, last end,
// workgroup-0 end} over all its workgroups (wall clock, 100 MHz); resets the table
int hipBackendReadExtents(unsigned long long* out, int maxLaunches);

// TESTING: make factor() take the reference-style per-op loop (potrf/trsm/saveSyrkGemm/
// prepareAssemble/assemble/doElimination virtuals) instead of the fused path
void hipBackendForcePerOp(SymbolicCtx& sym, bool on);

// TESTING, fault injection for the full-size parity tests: kind 1 = factor() does not launch the
// sparse-elimination update (the factor is then wrong and the checks must say so), 0 = off.
// Never read from the environment: a leaked variable cannot corrupt a caller's factor.
void hipBackendSetFault(SymbolicCtx& sym, int kind);

// what the calls on this Solver actually ran (cumulative): lets a test see that the path it means
// to test was taken, and a caller poll for a watchdog report without waiting for the next solve
struct HipRunCounters {
  int64_t sweepLaunches = 0;       // persistent solve sweeps launched (hip_sweep_kernels.h)
  int64_t sweepTimeouts = 0;       // ... that ran into their watchdog (reported by a later call)
  int64_t splitListsUsed = 0;      // update launches that took a split-K tile list
  int64_t subBatchesEnqueued = 0;  // sub-batches enqueued on their own stream
  int64_t lookaheadForks = 0;      // lookahead launches handed to the auxiliary streams
  int64_t tailLaunches = 0;        // persistent tail launches (hip_tail_kernel.h)
  int64_t solveWideLaunches = 0;   // backward elimination passes of hip_solve_wide.h
  int64_t invReused = 0;           // backward passes that reused the inverses of their forward pass
  int64_t potrfFoldedLevels = 0;   // tree levels whose potrf launch was folded into their trsm launch
  int64_t sweepMfmaLaunches = 0;   // ... of sweepLaunches: the matrix-core form for several right-hand sides
  int64_t sweepsRetired = 0;       // 1: a time-out retired the sweeps of this Solver
  int64_t sweepErrorPending = 0;   // 1: a time-out has been raised and not been reported yet
  int64_t selinvLaunches = 0;      // kernels enqueued by selected inversion and its adjoint (single or batched)
  int64_t selinvChunks = 0;        // passes over the selected-inversion levels (one per single call)
};
HipRunCounters hipBackendRunCounters(SymbolicCtx& sym);
// developer aid (BSP_SWEEP_TRACE=1 when the Solver is created): clock stamps {start, operands on chip,
// inputs arrived, x published} (100 MHz) of every spine workgroup of the LAST persistent sweep
int hipBackendReadSweepTrace(SymbolicCtx& sym, long long* out, int maxBlocks);

// per level of the plan (host only): {elimination range or -1, panels, widest panel, most rows below a
// panel, trsm tasks, update tiles, lookahead tiles, rows below summed over the panels}
std::vector<int64_t> hipBackendPlanLevels(SymbolicCtx& sym, int64_t startLump, int64_t upToLump);

// ---- extension operations, on the execution stream --------------------------------------------------
// One shape for all of them: every pointer argument is a HOST array of `batch` device pointers, one per
// member.  single = true: one member (batch = 1), element 0 of each array handed to the kernels
// directly; else the arrays travel to the device through the context's pointer ring and the batch runs
// in chunks of at most 65535 members (gridDim.y), one after the other.  Arguments are checked by the
// caller (solver.cpp), before any device work.
//
// Selected inversion (hip_selinv_kernels.h): data[q] holds a complete factor of this context's skeleton
// and is overwritten by Z = A^-1 on the pattern of L.  Chunks are bounded by device memory as well.
template <typename T>
void hipBackendSelectedInverse(SymbolicCtx& sym, T* const* data, int64_t batch, bool single);
// TESTING: at most `maxMatrices` matrices per chunk of a pass over the selected-inversion levels (0: no cap)
void hipBackendSetSelInvBatchChunk(SymbolicCtx& sym, int64_t maxMatrices);
// TESTING, read-only: bytes of one slot of the pointer ring of batched calls (0 before the first batched call)
int64_t hipBackendPtrRingSlotBytes(SymbolicCtx& sym);

// Gradients on the pattern of L (hip_grad_kernels.h).
// logDet: out[q] = 2 sum_i log L_ii of the complete factor factors[q] (out: device array of `batch`).
template <typename T>
void hipBackendLogDet(SymbolicCtx& sym, const T* const* factors, int64_t batch, bool single, T* out);
// patternGrad: z NULL: no Z term, zScale then unused; u and v NULL: no rank-2k term.  zScale: device
// array of `batch` scales.
template <typename T>
struct HipGradArgs {
  const T* const* z = nullptr;
  const T* zScale = nullptr;
  const T* const* u = nullptr;
  const T* const* v = nullptr;
  int64_t ld = 0;
  int nRHS = 0;
  T alpha = T(0);
  T* const* out = nullptr;
  bool outer = false;  // patternOuter: out_e = alpha sum_k U_ik V_jk for i >= j (z unused)
};
template <typename T>
void hipBackendPatternGrad(SymbolicCtx& sym, const HipGradArgs<T>& a, int64_t batch, bool single);
// Status of a factor and damping of the diagonal (hip_status_kernels.h), over the
// stored diagonals of the internal scalars [spanStart[spanBegin], spanStart[spanEnd]).
// factorStatus: out + 4 q = {lowest bad scalar or -1, bad diagonals, bits of the double min and max over
// the good ones} of data[q], which is only read (out: device array of 4 * batch words).
template <typename T>
void hipBackendFactorStatus(SymbolicCtx& sym, const T* const* data, int64_t batch, bool single, int64_t spanBegin,
                            int64_t spanEnd, int64_t* out);
// dampDiagonal: d <- (d (1 + alpha)) + beta in place, rounded in T after every operation; alphaBeta:
// device array of 2 * batch values, alpha and beta of member q at [2 q] and [2 q + 1].
template <typename T>
void hipBackendDampDiagonal(SymbolicCtx& sym, T* const* data, int64_t batch, bool single, int64_t spanBegin,
                            int64_t spanEnd, const T* alphaBeta);
// Reverse-mode sweep of the factor (hip_chol_adjoint_kernels.h; DESIGN.md sections 15 and 16): P[q] holds
// the factor of the lumps < upToLump with the Schur complement behind them and is only read; grad[q]
// holds Lbar before the cut and Sbar behind it and is overwritten by the data gradient.  upToLump =
// numLumps: the sweep of a complete factor.  The plan of a cut is built on first use and cached; chunks
// are bounded by device memory, as in selected inversion.
template <typename T>
void hipBackendFactorAdjointUpTo(SymbolicCtx& sym, const T* const* P, T* const* grad, int64_t batch, bool single,
                                 int64_t upToLump);
// Reverse mode of selected inversion (hip_selinv_adjoint_kernels.h): L[q] a complete
// factor and Z[q] its selected inverse, both only read; grad[q] holds the gradient of every slot of Z and
// is overwritten by Lbar (0 on the strictly-upper elements).  The complete selected-inversion plan, its
// scratch and its chunks; its launches and passes count in selinvLaunches / selinvChunks.
template <typename T>
void hipBackendSelectedInverseAdjoint(SymbolicCtx& sym, const T* const* L, const T* const* Z, T* const* grad,
                                      int64_t batch, bool single);
// The trailing block of layout buffers (from lump `fromLump` on) to dense symmetric m x m matrices, m =
// order - lumpStart[fromLump] (toDense: in = layout buffers, out = dense, every element written), or the
// adjoint in the data-gradient convention (in = dense gradients, out = layout buffers, written whole).
// dest: device permutation of 0 .. m-1 (dense row / column of trailing scalar k), NULL = identity.
template <typename T>
void hipBackendSchurDense(SymbolicCtx& sym, const T* const* in, T* const* out, int64_t batch, bool single,
                          int64_t fromLump, const int32_t* dest, bool toDense);

// The operations on entry maps (hip_ordered_sum.h).  The tables of a map are kept in map.dev, which is
// freed with the map (hipBackendFreeEntryMap, declared in entry_map.h).
//
// Assembly of coordinate entries into the layout.  The map is uploaded on the
// first call.
// assemble: in = values (nnz each), out = data (dataSize each); adjoint: in = gradients of the data,
// out = gradients of the values.
struct AssemblyMap;
template <typename T>
void hipBackendAssemble(SymbolicCtx& sym, const AssemblyMap& map, const T* const* in, T* const* out,
                        int64_t batch, bool single, bool adjoint);

// Normal equations of a sparse Jacobian.  Each part of the map is uploaded on
// the first call that needs it.
//   NormalEqHessian:  out = data (dataSize each) from values;  x unused
//   NormalEqAdjoint:  out = gradients of the values from values and x = gradients of the data
//   NormalEqJtVec:    out = J^T x ([n, q] each) from values and x ([m, q]);  NormalEqJVec: out = J x
struct NormalEqMap;
enum NormalEqOp : int32_t { NormalEqHessian = 0, NormalEqAdjoint = 1, NormalEqJtVec = 2, NormalEqJVec = 3 };
template <typename T>
void hipBackendNormalEq(SymbolicCtx& sym, const NormalEqMap& map, int32_t op, const T* const* values,
                        const T* const* x, T* const* out, int64_t q, int64_t batch, bool single);

// Products with a symmetric matrix given as entries.  Each part of the map is
// uploaded on the first call that needs it.
//   SymProductMv:     out = A x ([n, q] each) from a = values (nnz) and b = x ([n, q])
//   SymProductOuter:  out = gradient of the values (nnz) from a = g and b = x ([n, q] both)
struct SymProductMap;
enum SymProductOp : int32_t { SymProductMv = 0, SymProductOuter = 1 };
template <typename T>
void hipBackendSymProduct(SymbolicCtx& sym, const SymProductMap& map, int32_t op, const T* const* a,
                          const T* const* b, T* const* out, int64_t q, int64_t batch, bool single);

// Error bounds.
//   symResidual:  r = b - A x and d = |A| |x| + |b| ([n, q] each) over the row lists of SymProductMv, in
//                 one pass; b and r NULL: d = |A| |x| alone
//   colMax:       out[member q + j] (double) = max over the n rows of ratio(|a[i, j]|, b[i, j]), or of
//                 a[i, j] when b is NULL (hip_norm_est_kernels.h)
//   normEstStep:  one step of Solver::invNorm1Estimate on the work areas of `batch` matrices, which sit
//                 normEstWorkBytes apart from `work` on: x (order values of T), xi (order values), then,
//                 normEstPartOffset bytes from x, the partials of the reductions.  D is read by
//                 NormEstScale alone; out by NormEstAltSum alone
template <typename T>
void hipBackendSymResidual(SymbolicCtx& sym, const SymProductMap& map, const T* const* values, const T* const* x,
                           const T* const* b, T* const* r, T* const* d, int64_t q, int64_t batch, bool single);
template <typename T>
void hipBackendColMax(SymbolicCtx& sym, const T* const* a, const T* const* b, int64_t n, int64_t q, double* out,
                      int64_t batch, bool single);
enum NormEstStep : int32_t {
  NormEstStart = 0,      // x = 1 / n, the state record reset
  NormEstUnit = 1,       // x = e_j, j from the record
  NormEstAltVector = 2,  // x = the alternating vector
  NormEstScale = 3,      // x <- D x
  NormEstSum = 4,        // ||x||_1, the sign comparison, xi = x = sgn(x), the decision of the pass
  NormEstArgMax = 5,     // j = argmax |x| (x holding z), the same-column test
  NormEstAltSum = 6      // ||x||_1 of the alternating solve weighed in, the estimate written
};
inline int64_t normEstPartOffset(int64_t order, int64_t elemBytes) { return (2 * order * elemBytes + 15) & ~int64_t(15); }
inline int64_t normEstWorkBytes(int64_t order, int64_t elemBytes) {
  const int64_t parts = (order + 1023) / 1024;
  return normEstPartOffset(order, elemBytes) + (parts > 0 ? parts : 1) * 16;
}
template <typename T>
void hipBackendNormEstStep(SymbolicCtx& sym, int32_t step, void* work, const T* const* D, int64_t* state,
                           double* out, int64_t batch, bool single);

// Preconditioned conjugate gradient (hip_cg_kernels.h): one piece of an iteration on
// `batch` matrices with q right-hand sides each.  Vectors are [n, q] row-major; state holds 12 words per
// (matrix, right-hand side); the work areas sit cgWorkBytes(n, q) apart from `work` on: the partials of
// the dot products, then, cgBadOffset bytes in, the bad-pivot words of a preconditioner build.
//   CgInit:       in0 = b; out0 = x, out1 = r (= b - A x, the caller's): the records reset, bb, rr, the
//                 columns of a zero b cleared; `plain` also starts rz
//   CgAlpha:      in0 = p, in1 = Ap: pAp, alpha
//   CgUpdate:     in0 = p, in1 = Ap; out0 = x, out1 = r: x += alpha p, r -= alpha Ap, rr, the iteration
//                 counted, the stop test; `plain` (no preconditioner) also writes beta
//   CgPrecond:    in0 = the preconditioner's values (kinds 1, 2), in1 = r; out0 = z (kind 0: only read):
//                 z = M^-1 r, rz, beta
//   CgDirection:  in0 = z (r when plain); out0 = p: p = z + beta p
//   CgBuild:      in0 = the entry values; out0 = the preconditioner's values; status: 2 words per matrix
//   CgFsaiApply:  kind CgFsai (section 27): in0 = the values of G, in1 = r; out0 = z, out1 = t (scratch):
//                 t = G r, z = G^T t, rz, beta
enum CgOp : int32_t {
  CgInit = 0,
  CgAlpha = 1,
  CgUpdate = 2,
  CgPrecond = 3,
  CgDirection = 4,
  CgBuild = 5,
  CgFsaiApply = 6
};
template <typename T>
struct CgArgs {
  int32_t op = CgInit, kind = 0;  // kind: CgPrecondKind (sym_product.h)
  bool plain = false;
  int64_t n = 0, q = 1, maxSteps = 0;
  double tol = 0.0;
  const SymProductMap* map = nullptr;  // CgPrecond of kinds 1 and 2, CgBuild, CgFsaiApply
  const T* const* in0 = nullptr;
  const T* const* in1 = nullptr;
  T* const* out0 = nullptr;
  T* const* out1 = nullptr;
  void* work = nullptr;
  int64_t* state = nullptr;
  int64_t* status = nullptr;
};
inline int64_t cgBadOffset(int64_t n, int64_t q) {
  const int64_t parts = (n + 1023) / 1024;
  return q * (parts > 0 ? parts : 1) * 16;
}
inline int64_t cgWorkBytes(int64_t n, int64_t q) { return cgBadOffset(n, q) + ((4 * (n > 0 ? n : 1) + 15) & ~int64_t(15)); }
template <typename T>
void hipBackendCg(SymbolicCtx& sym, const CgArgs<T>& a, int64_t batch, bool single);

// Matrix-free least squares (hip_cgls_kernels.h): one piece of CGLS for (J^T J + D) x =
// J^T r + c on `batch` Jacobians of one map with q columns each.  n-space vectors are [n, q], m-space ones
// [m, q], row-major; d (the damping vector) and colsq hold n values; state holds CgState's 12 words per
// (matrix, column); the work areas sit cglsWorkBytes(m, n, q) apart from `work` on: the partials, then,
// cglsBadOffset bytes in, the bad-pivot words of a build.  An operand that may be absent is NULL.
//   CglsJv:       out = epilogue(J vec), epi CglsPlain or CglsResidual (addend = r, may be absent); state
//                 NULL: every column, else the stopped columns are skipped
//   CglsJtv:      out = epilogue(J^T vec), epi CglsPlain or CglsNormal (damp = d and x, both or neither;
//                 addend = c, may be absent); state as for CglsJv
//   CglsColSq:    colsq (doubles) from the values
//   CglsDamp:     colsq (read); out = d = T(alpha colsq + beta)
//   CglsInit:     vec = b (in n-space); x: the records reset, bb, x = 0 in the columns of a zero b
//   CglsDelta:    vec = t (m-space), x = p, damp = d (may be absent): delta, alpha
//   CglsUpdate:   vec = p, addend = t; x, out = res: x += alpha p, res -= alpha t
//   CglsApply:    kind 0 / 1 / 2 (CgPrecondKind): damp = the preconditioner's values (kinds 1, 2), vec = s; out =
//                 z (kind 0: only read): z = M^-1 s, ss, the iteration counted unless `start`, the stop test,
//                 gamma = s.z, beta
//   CglsBuild:    kind 1 / 2: values, colsq (kind 1), damp = d (may be absent); out = the preconditioner's
//                 values; status: 2 words per matrix
//   CglsIterate:  one whole iteration in one call: CglsJv (t = J p), the partials of CglsDelta, its fold and
//                 CglsUpdate in one launch (cglsAlphaUpdate), CglsJtv (normal epilogue), CglsApply and
//                 cgDirection queued one behind the other on p, t, x, res, s, z with values, damp = d, addend = c
//                 and minv (the preconditioner's values): the same sums in the same order, so the same bits.  phase 0: all of it; 1: up to and including s
//                 (the caller then writes its own z = M^-1 s); 2: apply and direction alone.  kind 0 with z ==
//                 s is the iteration without a preconditioner
struct JacobianProductMap;
enum CglsOp : int32_t {
  CglsJv = 0,
  CglsJtv = 1,
  CglsColSq = 2,
  CglsDamp = 3,
  CglsInit = 4,
  CglsDelta = 5,
  CglsUpdate = 6,
  CglsApply = 7,
  CglsBuild = 8,
  CglsIterate = 9
};
template <typename T>
struct CglsArgs {
  int32_t op = CglsJv, kind = 0, epi = 0, phase = 0;
  bool start = false;
  int64_t q = 1, maxSteps = 0;
  double tol = 0.0, alpha = 0.0, beta = 0.0;
  const JacobianProductMap* map = nullptr;
  const T* const* values = nullptr;
  const T* const* vec = nullptr;
  const T* const* addend = nullptr;
  const T* const* damp = nullptr;
  T* const* x = nullptr;
  T* const* out = nullptr;
  double* const* colsq = nullptr;
  // CglsIterate alone
  T* const* p = nullptr;
  T* const* t = nullptr;
  T* const* res = nullptr;
  T* const* s = nullptr;
  T* const* z = nullptr;
  const T* const* minv = nullptr;
  void* work = nullptr;
  int64_t* state = nullptr;
  int64_t* status = nullptr;
};
inline int64_t cglsBadOffset(int64_t m, int64_t n, int64_t q) {
  const int64_t mp = (m + 1023) / 1024, np = (n + 1023) / 1024;
  const int64_t parts = mp + np > 2 * np ? mp + np : 2 * np;
  return q * (parts > 0 ? parts : 1) * 16;
}
inline int64_t cglsWorkBytes(int64_t m, int64_t n, int64_t q) {
  return cglsBadOffset(m, n, q) + ((4 * (n > 0 ? n : 1) + 15) & ~int64_t(15));
}
template <typename T>
void hipBackendCgls(SymbolicCtx& sym, const CglsArgs<T>& a, int64_t batch, bool single);

// Implicit Schur elimination of the matrix-free least squares (hip_schur_kernels.h): one
// piece on `batch` Jacobians of one structure over a JacSchurMap.  Kept vectors are [nK, q], full ones [n, q], t
// [m, q] is scratch of the caller's; the work area and the status of SchurBuild are those of CglsBuild
// (cglsWorkBytes(m, n, 1) per member).  An operand that may be absent is NULL.
//   SchurBuild:   values, damp = d [n] (may be absent); binv = the inverses of the blocks of B; work, status
//   SchurMv:      values, binv, damp = d (may be absent), vec = p; t; out = S p; state (may be NULL): the
//                 records of a conjugate gradient, whose stopped columns are skipped
//   SchurReduce:  values, binv, full = g; t; out = b_k
//   SchurBack:    values, binv, full = g, vec = x_k; t; out = x [n, q] in the caller's order
//   SchurPrecondBuild:  kind 1 / 2 (CgPrecondKind) of the preconditioner of S on the kept scalars: colsq [n] (kind
//                 1), values (kind 2), damp = d (may be absent); out = its values; work, status as SchurBuild
//   SchurPrecondApply:  CgPrecond of the conjugate gradient on the kept scalars with that preconditioner: binv =
//                 its values, vec = r, out = z; work (cgWorkBytes(nK, q) per member) and state are the iteration's
//   SchurSJacobiBuild:  the block diagonal of S: values, binv, damp = d (may be absent),
//                 partials = the chunk partials (JacSchurJacobiPlan::partialElems() doubles per member); out = the
//                 inverses of the blocks; work, status as SchurBuild
//   SchurSJacobiApply:  SchurPrecondApply of kind 2 on that plan's block offsets (the kept item plan is not built)
struct JacSchurMap;
enum SchurOp : int32_t {
  SchurBuild = 0,
  SchurMv = 1,
  SchurReduce = 2,
  SchurBack = 3,
  SchurPrecondBuild = 4,
  SchurPrecondApply = 5,
  SchurSJacobiBuild = 6,
  SchurSJacobiApply = 7
};
template <typename T>
struct JacSchurArgs {
  int32_t op = SchurBuild, kind = 0;
  int64_t q = 1;
  const JacSchurMap* map = nullptr;
  const T* const* values = nullptr;
  const T* const* damp = nullptr;
  const T* const* binv = nullptr;
  const T* const* vec = nullptr;
  const T* const* full = nullptr;
  T* const* t = nullptr;
  T* const* out = nullptr;
  const double* const* colsq = nullptr;
  double* const* partials = nullptr;
  void* work = nullptr;
  int64_t* state = nullptr;  // (only SchurPrecondApply and SchurSJacobiApply write it)
  int64_t* status = nullptr;
};
template <typename T>
void hipBackendJacSchur(SymbolicCtx& sym, const JacSchurArgs<T>& a, int64_t batch, bool single);

// The Lanczos recurrence (hip_lanczos_kernels.h): one piece of a step on `batch`
// matrices with q start vectors each.  Vectors are [n, q] row-major; slot s of a member's basis is the
// vector at basis + s slotStride; state holds 12 words and coef 2 kmax doubles per (matrix, start vector);
// the work areas sit lanczosWorkBytes(n, q, kmax) apart from `work` on.  `fold` (LzUpdate, LzSubtract): the
// piece is the last that writes w, so the fold of ww that ends the step is queued behind it.
//   LzInit:       vec = v0 (read): the records reset, vv, slot `slot` = v0 / sqrt(vv)
//   LzAlpha:      vec = w (read): alpha = slot `slot` . w
//   LzUpdate:     vec = w: w -= alpha v_j (slot `slot`) + beta v_{j-1} (slot `prev`), the partials of w.w
//   LzProject:    vec = w (read): c_i = slot i . w, i < count
//   LzSubtract:   vec = w: w -= sum_i c_i slot i, i < count ascending, the partials of w.w
//   LzNormalize:  vec = w (read): slot `slot` = w / beta
enum LanczosOp : int32_t { LzInit = 0, LzAlpha = 1, LzUpdate = 2, LzProject = 3, LzSubtract = 4, LzNormalize = 5 };
template <typename T>
struct LanczosArgs {
  int32_t op = LzInit;
  bool fold = false;
  int64_t n = 0, q = 1, kmax = 1, slots = 0, slotStride = 0, slot = 0, prev = 0, count = 0;
  double breakdown = 0.0;
  T* const* vec = nullptr;
  T* const* basis = nullptr;
  double* coef = nullptr;
  void* work = nullptr;
  int64_t* state = nullptr;
};
inline int64_t lanczosProjOffset(int64_t n, int64_t q, int64_t kmax) {
  const int64_t parts = (n + 1023) / 1024;
  return q * kmax * (parts > 0 ? parts : 1) * 16;
}
inline int64_t lanczosWorkBytes(int64_t n, int64_t q, int64_t kmax) {
  return lanczosProjOffset(n, q, kmax) + ((8 * q * kmax + 15) & ~int64_t(15));
}
template <typename T>
void hipBackendLanczos(SymbolicCtx& sym, const LanczosArgs<T>& a, int64_t batch, bool single);

// Combinations of basis vectors (kvCombine, hip_lanczos_kernels.h): for the nf outputs f
// and the q columns c of every member, out_f[:, c] = (accumulate ? out_f[:, c] : +0) + sum_i T(y[c, f, i]) slot
// (slot + i)[:, c], i = 0 .. count - 1 ascending, term i skipped (its slot not read) when first + i >= limit[c].
// The basis is LanczosArgs's; y holds doubles [batch, q, nf, ldy] and limit int64 [batch, q], one array each;
// output f of a member is the [n, q] array at out + f outStride.
template <typename T>
struct KrylovCombineArgs {
  int64_t n = 0, q = 1, nf = 1, slots = 0, slotStride = 0, slot = 0, count = 0, first = 0, ldy = 0, outStride = 0;
  bool accumulate = false;
  const T* const* basis = nullptr;
  const double* y = nullptr;
  const int64_t* limit = nullptr;
  T* const* out = nullptr;
};
template <typename T>
void hipBackendKrylovCombine(SymbolicCtx& sym, const KrylovCombineArgs<T>& a, int64_t batch, bool single);

// Reach solves (hip_reach_kernels.h), one matrix, plan from buildReachPlan (reach.h).
// reachSolveL: W (numCols x order, column-major, leading dimension order) <- the unit columns of the
// queries solved through the lumps of their reach below the plan's cut; the caller then runs
// solveLFrom(cutSpan) over all columns.  L is a complete factor and only read.
// gramBlocks: out + item.outOff <- W_P^T W_Q (row-major) for every item of the plan, written once, W read.
// reachWorkspace: device room for `elems` values kept with the context (inverseBlocks' W); growing it
// waits for the device.  The tables of a call travel through a ring on the execution stream.
struct ReachPlan;
template <typename T>
void hipBackendReachSolveL(SymbolicCtx& sym, const ReachPlan& plan, const T* L, T* W);
template <typename T>
void hipBackendGramBlocks(SymbolicCtx& sym, const ReachPlan& plan, const T* W, T* out);
template <typename T>
T* hipBackendReachWorkspace(SymbolicCtx& sym, int64_t elems);

// Products with the factor (hip_factor_product.h): y[q] = L[q] x[q], or L[q]^T x[q]
// when `transposed`.  L[q] is a buffer in the numeric layout of which the elements i >= j are read; x[q]
// and y[q] are order x nRHS, column-major with leading dimensions ldx and ldy, in internal order.  Every
// element of y is written once, none is read; sums run in an order fixed by the skeleton, without
// atomics.  The plan (factor_product_plan.h) is built and uploaded by the first call.
template <typename T>
void hipBackendFactorProduct(SymbolicCtx& sym, const T* const* L, bool transposed, const T* const* x, int64_t ldx,
                             T* const* y, int64_t ldy, int nRHS, int64_t batch, bool single);

HipPlanStats hipBackendPlanStats(SymbolicCtx& sym, int64_t startLump, int64_t upToLump);

// TESTING (host only): the launch tables (buildLaunchTables, hip_plan.h) and the solve schedule of the
// plan's own levels (buildSolveSchedule) of the plan over every lump, as the flat records of
// include/baspacho_amd_testing.h
std::vector<int64_t> hipBackendLaunchTableRecords(SymbolicCtx& sym);
std::vector<int64_t> hipBackendSolveScheduleRecords(SymbolicCtx& sym, bool withSweeps, bool blockSolve, bool inverses,
                                                    int sweepMinWidth);

}  // namespace BaSpaCho
