// Solver: a symbolic decomposition plus the operations that run on externally allocated
// numeric data.  Public surface mirrors baspacho/baspacho/Solver.h:34-237 (createSolver,
// factor/solve families, accessors, Settings, BackendType, AddFillPolicy) so that callers of
// the reference (bench, BAL_bench, Theseus' baspacho_solver.cpp) compile against it unchanged.
// Numeric data is DEVICE memory: the only engine in this build is the MI355X HIP backend.
#pragma once

#include <memory>
#include <unordered_set>
#include <vector>

#include "backend_options.h"
#include "mat_ops.h"
#include "skeleton.h"
#include "sparse_structure.h"

namespace BaSpaCho {

struct AssemblyMap;
struct NormalEqMap;
struct JacobianProductMap;
struct JacSchurMap;
struct SymProductMap;
template <typename T>
struct CgArgs;
template <typename T>
struct CglsArgs;
template <typename T>
struct JacSchurArgs;
template <typename T>
struct LanczosArgs;
template <typename T>
struct KrylovCombineArgs;
struct ReachPlan;

class Solver {
 public:
  // from a RAW factor skeleton (normally use createSolver)
  Solver(CoalescedBlockMatrixSkel&& factorSkel, std::vector<int64_t>&& sparseElimRanges,
         std::vector<int64_t>&& permutation, OpsPtr&& ops, int64_t canFactorUpTo = -1);

  PermutedCoalescedAccessor accessor() const {
    PermutedCoalescedAccessor acc;
    acc.init(factorSkel.accessor(), permutation.data());
    return acc;
  }

  // accessor whose arrays live in device memory (usable inside a HIP kernel)
  PermutedCoalescedAccessor deviceAccessor() const { return symCtx->deviceAccessor(); }

  void enableStats(bool enabled = true);
  void printStats() const;
  void resetStats();

  // execution stream (hipStream_t) used by every subsequent factor/solve call
  void setStream(void* stream) { symCtx->setStream(stream); }

  template <typename T>
  void factor(T* data, bool verbose = false) const;

  template <typename T>
  void solve(const T* matData, T* vecData, int64_t stride, int nRHS) const;
  template <typename T>
  void solveL(const T* matData, T* vecData, int64_t stride, int nRHS) const;
  template <typename T>
  void solveLt(const T* matData, T* vecData, int64_t stride, int nRHS) const;

  template <typename T>
  void factorUpTo(T* data, int64_t spanIndex, bool verbose = false) const;
  template <typename T>
  void factorFrom(T* data, int64_t spanIndex, bool verbose = false) const;

  template <typename T>
  void solveLUpTo(const T* data, int64_t spanIndex, T* vecData, int64_t stride, int nRHS) const;
  template <typename T>
  void solveLtUpTo(const T* data, int64_t spanIndex, T* vecData, int64_t stride, int nRHS) const;
  template <typename T>
  void solveLFrom(const T* data, int64_t spanIndex, T* vecData, int64_t stride, int nRHS) const;
  template <typename T>
  void solveLtFrom(const T* data, int64_t spanIndex, T* vecData, int64_t stride, int nRHS) const;

  // out += alpha * A * in on the (un-factored) block from spanIndex on   (Solver.h:89-91)
  template <typename T>
  void addMvFrom(const T* matData, int64_t spanIndex, const T* inVecData, int64_t inStride,
                 T* outVecData, int64_t outStride, int nRHS, BaseType<T> alpha = 1.0) const;

  // pseudo-factor: Cholesky of the diagonal block of every span from spanIndex on, rows below
  // divided by it   (Solver.h:92-94; preconditioners of the PCG example)
  template <typename T>
  void pseudoFactorFrom(T* data, int64_t spanIndex, bool verbose = false) const;

  // extension: selected inversion.  `data` holds a complete factor() of this Solver; it is overwritten
  // in place by Z = A^-1 restricted to the block pattern of L, in the factor's layout (diagonal blocks
  // full and symmetric, off-diagonal blocks in their stored orientation).  Runs on the stream of
  // setStream(), without host synchronisation ("Selected inversion").
  // T = std::vector<double*> / std::vector<float*>: a batch of factors of this Solver, as factor(&v);
  // member q comes out bitwise equal to selectedInverse(v[q]).  An empty batch, a NULL member or two
  // members with the same pointer are refused.  The batch runs in chunks bounded by device memory.
  template <typename T>
  void selectedInverse(T* data) const;

  // extension: gradients on the block pattern of L (hip_grad_kernels.h).  Data
  // is this Solver's numeric layout, vectors are in its internal order (as for solve()); A(d) is the
  // symmetric matrix with A_ij = A_ji = d_e for every stored element e = (i, j), i >= j (the
  // strictly-upper elements of the diagonal blocks are not read).  Both run on the stream of
  // setStream(), without host synchronisation, and refuse a Solver that cannot factor completely.
  //
  // logDet: devOut[0] = log det A = 2 sum_i log L_ii of a complete factor() (fp64 accumulation; a
  // non-positive or NaN pivot gives -inf or NaN).  Batch form: devOut[q] for factors[q].
  template <typename T>
  void logDet(const T* factor, T* devOut) const;
  template <typename T>
  void logDet(const std::vector<T*>& factors, T* devOut) const;
  // extension: the status of a factor and damping of the diagonal, on the device (DESIGN.md section 18;
  // hip_status_kernels.h).  Both walk the stored diagonals of the internal scalars of the spans
  // [spanBegin, spanEnd), 0 <= spanBegin <= spanEnd <= numSpans (the range need not sit on a lump
  // boundary: [0, span) after factorUpTo(span), [span, numSpans) after factorFrom(span)), on the stream
  // of setStream() without host synchronisation.  NULL pointers, an empty batch and a range outside
  // the spans are refused before any device work.
  //
  // factorStatus: a diagonal is good when it is positive and finite in T.  devOut[0..3] (8-byte words) =
  // {lowest bad internal scalar or -1, number of bad diagonals, bits of the double minimum over the good
  // ones (+inf: none), bits of the double maximum (0.0: none)}; `data` is only read.  After a factor()
  // whose first failing pivot is column k, devOut[0] = k: the columns before k do not depend on A_kk.
  // Batch form: devOut + 4 q for data[q], bitwise the single call.
  template <typename T>
  void factorStatus(const T* data, int64_t spanBegin, int64_t spanEnd, int64_t* devOut) const;
  template <typename T>
  void factorStatus(const std::vector<T*>& data, int64_t spanBegin, int64_t spanEnd, int64_t* devOut) const;
  // dampDiagonal: d <- (d (1 + alpha)) + beta in place, each operation rounded in T; alpha =
  // devAlphaBeta[0], beta = devAlphaBeta[1] are DEVICE values.  Batch form: devAlphaBeta[2 q], [2 q + 1]
  // for data[q]; members that overlap are refused.
  template <typename T>
  void dampDiagonal(T* data, int64_t spanBegin, int64_t spanEnd, const T* devAlphaBeta) const;
  template <typename T>
  void dampDiagonal(const std::vector<T*>& data, int64_t spanBegin, int64_t spanEnd, const T* devAlphaBeta) const;
  // patternGrad: writes, for every stored element e = (i, j) (out is never read),
  //   i > j: out_e = zScale[0] 2 Z_e + alpha sum_k (U_ik V_jk + V_ik U_jk)
  //   i = j: out_e = zScale[0] Z_e   + alpha sum_k U_ik V_ik
  //   strictly-upper elements of the diagonal blocks: out_e = 0
  // Z (e.g. the output of selectedInverse) NULL: no Z term (zScale unused).  U and V (n x nRHS,
  // column-major, leading dimension `stride`) both NULL: no rank-2k term; else nRHS >= 1.  zScale is a
  // DEVICE value.  Batch form: element q of each vector (Z and U / V may be empty vectors), zScale[q].
  template <typename T>
  void patternGrad(const T* Z, const T* zScale, const T* U, const T* V, int64_t stride, int nRHS, T alpha,
                   T* out) const;
  template <typename T>
  void patternGrad(const std::vector<T*>& Z, const T* zScale, const std::vector<T*>& U,
                   const std::vector<T*>& V, int64_t stride, int nRHS, T alpha,
                   const std::vector<T*>& out) const;
  // patternOuter: the non-symmetric rank-k projection, for every stored element e = (i, j) (out is never
  // read): i >= j: out_e = alpha sum_k U_ik V_jk; strictly-upper elements of the diagonal blocks: 0.
  // U, V as for patternGrad (both required, nRHS >= 1).  Batch form: member q of each vector.  NULL
  // pointers, an empty batch and output buffers that overlap each other or an input are refused.
  template <typename T>
  void patternOuter(const T* U, const T* V, int64_t stride, int nRHS, T alpha, T* out) const;
  template <typename T>
  void patternOuter(const std::vector<T*>& U, const std::vector<T*>& V, int64_t stride, int nRHS, T alpha,
                    const std::vector<T*>& out) const;

  // extension: reverse-mode sweep of factor() (hip_chol_adjoint_kernels.h).  `L`
  // holds a complete factor() of A(d); `grad` holds Lbar = df/dL on entry (every stored element with
  // i >= j; the strictly-upper elements of the diagonal blocks are ignored) and df/dd on return, in
  // patternGrad's convention.  L is only read.  Runs on the stream of setStream() without host
  // synchronisation.  Batch form: member q of each vector, bitwise the single call; the batch runs in
  // chunks bounded by device memory, as selectedInverse does.  NULL pointers, an empty batch, sizes
  // that differ, gradient buffers that overlap each other or a factor, and a Solver that cannot
  // factor completely are refused before any device work.
  template <typename T>
  void factorAdjoint(const T* L, T* grad) const;
  template <typename T>
  void factorAdjoint(const std::vector<T*>& L, const std::vector<T*>& grad) const;

  // extension: reverse mode of selectedInverse() (hip_selinv_adjoint_kernels.h).
  // `L` holds a complete factor(), `Z` what selectedInverse wrote over a copy of it; both are only read.
  // `grad` holds df/d(slot) on entry for EVERY slot of the layout as selectedInverse writes it (the
  // strictly-upper elements of the diagonal blocks are slots of their own) and Lbar = df/dL on return:
  // the elements i >= j, exactly 0 above the diagonal -- the input of factorAdjoint.  Stream, batch form
  // and chunks as factorAdjoint.  The scatter of the sweep adds with float atomics: results are close,
  // not bitwise, from run to run.  Refused before any device work: NULL pointers, an empty batch,
  // gradient buffers that overlap each other, a factor or a Z, a Solver that cannot factor completely.
  template <typename T>
  void selectedInverseAdjoint(const T* L, const T* Z, T* grad) const;
  template <typename T>
  void selectedInverseAdjoint(const std::vector<T*>& L, const std::vector<T*>& Z, const std::vector<T*>& grad) const;

  // extension: reverse-mode sweep of factorUpTo().  `P` holds factorUpTo(spanIndex)
  // of A(d): [L11 0; L21 S], S = A22 - A21 A11^-1 A12 on the spans from spanIndex on; it is only read.
  // `grad` holds df/dP_e on entry for every stored element i >= j (Lbar on the columns before the cut,
  // Sbar behind it; strictly-upper elements ignored) and df/dd on return.  spanIndex = numSpans() is
  // factorAdjoint; spanIndex = 0 returns the input (strictly-upper elements zeroed).  Stream, batch
  // form and chunks as factorAdjoint.  Refused before any device work: a span that factorUpTo refuses
  // (inside a lump, cutting a sparse-elimination range), NULL or overlapping buffers, an empty batch,
  // a Solver that cannot factor completely.
  template <typename T>
  void factorAdjointUpTo(const T* P, T* grad, int64_t spanIndex) const;
  template <typename T>
  void factorAdjointUpTo(const std::vector<T*>& P, const std::vector<T*>& grad, int64_t spanIndex) const;
  // schurComplement: the trailing block of a layout buffer (rows and columns from span spanIndex on, m =
  // order() - spanStart[spanIndex] scalars) as a dense symmetric m x m matrix, row-major: out[dest[i] m +
  // dest[j]] for trailing scalars i, j counted from the cut, zero where the pattern has no block.  Every
  // element of `out` is written, none is read.  dest: DEVICE permutation of 0 .. m-1, NULL = identity.
  // schurComplementAdjoint: its adjoint in patternGrad's convention; every element of gradData is
  // written: gradDense[i, j] + gradDense[j, i] below the diagonal, gradDense[i, i] on it, 0 above it and
  // on every column before the cut.  gradDense need not be symmetric.  Span checks as factorAdjointUpTo.
  template <typename T>
  void schurComplement(const T* P, int64_t spanIndex, T* out, const int32_t* dest = nullptr) const;
  template <typename T>
  void schurComplement(const std::vector<T*>& P, int64_t spanIndex, const std::vector<T*>& out,
                       const int32_t* dest = nullptr) const;
  template <typename T>
  void schurComplementAdjoint(const T* gradDense, int64_t spanIndex, T* gradData,
                              const int32_t* dest = nullptr) const;
  template <typename T>
  void schurComplementAdjoint(const std::vector<T*>& gradDense, int64_t spanIndex,
                              const std::vector<T*>& gradData, const int32_t* dest = nullptr) const;
  // the lump at which a partial factor up to spanIndex ends; throws (prefix `what`) for a span that
  // factorUpTo refuses and for a Solver that cannot factor completely
  int64_t partialCutLump(const char* what, int64_t spanIndex) const;

  // extension: assembly of coordinate entries (row, col, value) into this Solver's layout (DESIGN.md
  // section 14; assembly.h).  `map` comes from createAssemblyMap(*this, ...).  assemble writes every
  // element of `data` (never read): the sum, in ascending entry index from +0, of the values of the
  // entries mapped to it, and 0 where none is.  assembleAdjoint: gradValues[k] = gradData[entryOff[k]],
  // 0 for skipped entries.  Both run on the stream of setStream() without host synchronisation (the
  // first call uploads the map).  Batch forms: member q of each vector, bitwise the single call.  A map
  // of another Solver, an empty batch, a NULL pointer (the nnz-sized side may be NULL when nnz = 0) or
  // a repeated output pointer are refused before any device work.
  template <typename T>
  void assemble(const AssemblyMap& map, const T* values, T* data) const;
  template <typename T>
  void assemble(const AssemblyMap& map, const std::vector<const T*>& values, const std::vector<T*>& data) const;
  template <typename T>
  void assembleAdjoint(const AssemblyMap& map, const T* gradData, T* gradValues) const;
  template <typename T>
  void assembleAdjoint(const AssemblyMap& map, const std::vector<const T*>& gradData,
                       const std::vector<T*>& gradValues) const;
  // extension: normal equations of a sparse Jacobian J (normal_eq.h).  `map` comes
  // from createNormalEqMap(*this, ...); op is a NormalEqOp (hip_backend.h); member b of the batch uses
  // values[b] (nnz), x[b] and out[b]:
  //   NormalEqHessian: out = H = J^T J in this Solver's layout (dataSize, every element written), x empty
  //   NormalEqAdjoint: out = gradient of the values (nnz) from x = gradient of the data (dataSize)
  //   NormalEqJtVec:   out = J^T x ([n, q] row-major) from x ([m, q]);  NormalEqJVec: out = J x ([m, q])
  // single = true: one member handed to the kernels directly (the batch forms go through a pointer
  // array); member b is bitwise the single call either way.  Runs on the stream of setStream() without
  // host synchronisation (the first call of a kind uploads its part of the map).  A map of another
  // Solver, an empty batch, a NULL pointer (a side of size 0 may be NULL), a repeated output pointer or
  // an output that overlaps an input of its member are refused before any device work.
  template <typename T>
  void normalEq(const NormalEqMap& map, int32_t op, const std::vector<const T*>& values,
                const std::vector<const T*>& x, const std::vector<T*>& out, int64_t q, bool single) const;
  // extension: products with the symmetric matrix of coordinate entries, without its layout (DESIGN.md
  // section 21; sym_product.h).  `map` comes from createSymProductMap(*this, ...); op is a SymProductOp
  // (hip_backend.h); member b of the batch uses a[b], x[b] and out[b], x and g [order(), q] row-major:
  //   SymProductMv:    out = A x ([n, q], every element written) from a = values (nnz) and x
  //   SymProductOuter: out[k] = sum_j g[r, j] x[c, j] (+ g[c, j] x[r, j] off the diagonal), (r, c) the
  //                    position of entry k, 0 for a skipped entry, from a = g and x: the gradient of the
  //                    values of sum(g * (A x)), the same for every duplicate
  // single = true: one member handed to the kernels directly; member b is bitwise the single call either
  // way.  Runs on the stream of setStream() without host synchronisation (the first call of a kind
  // uploads its part of the map).  A map of another Solver, an empty batch, q < 1, a NULL pointer (a side
  // of size 0 may be NULL), a repeated output pointer or an output that overlaps an input are refused
  // before any device work.
  template <typename T>
  void symProduct(const SymProductMap& map, int32_t op, const std::vector<const T*>& a,
                  const std::vector<const T*>& x, const std::vector<T*>& out, int64_t q, bool single) const;
  // extension: error bounds (hip_ordered_sum.h, hip_norm_est_kernels.h).  All run on
  // the stream of setStream() without host synchronisation, and refuse before any device work a map of
  // another Solver, an empty batch, q < 1, a NULL pointer, a repeated output pointer and an output that
  // overlaps an input or another output.
  //
  // symResidual: over the row lists of SymProductMv, in one pass, r[i, j] = b[i, j] - s, s the terms
  // values[k] * x[idx, j] of row i folded in list order from +0 (bitwise b - mv(values, x)), and d[i, j] =
  // |b[i, j]| + t, t the terms |values[k]| * |x[idx, j]| folded the same way: (|A| |x| + |b|)_i with
  // duplicates as separate terms.  x, b, r, d are [order(), q] row-major; every element of r and d is
  // written once, neither is read.  With b and r empty: d = |A| |x| alone.
  template <typename T>
  void symResidual(const SymProductMap& map, const std::vector<const T*>& values, const std::vector<const T*>& x,
                   const std::vector<const T*>& b, const std::vector<T*>& r, const std::vector<T*>& d, int64_t q,
                   bool single) const;
  // colMax: devOut[member q + j] = max over i < n of a[i, j] as a double (-inf for n == 0); with b:
  // maxRatio, the max of ratio(|a[i, j]|, b[i, j]) in double (0 for n == 0), where ratio is 0 when a == 0,
  // +inf when b == 0 and a != 0, and a NaN in either operand makes the column's result NaN.  a and b are
  // [n, q] row-major and only read.  The partials of the first pass are kept with the Solver; a call that
  // needs more of them than any before allocates them, which waits for the device.
  template <typename T>
  void colMax(const std::vector<const T*>& a, const std::vector<const T*>& b, int64_t n, int64_t q,
              double* devOut, bool single) const;
  // invNorm1Estimate: devOut[m] = an estimate of ||A^-1||_1 (a lower bound, almost always within a factor
  // 3) for the matrix whose complete factor() is L[m]; with D (one device vector of order() values in
  // internal order per member) of ||D A^-1 D||_1.  Hager's estimator in Higham's form on a fixed schedule
  // of 10 solve() calls with one right-hand side, nothing read back: devState holds the 12-word state
  // record of every matrix (hip_norm_est_kernels.h).  `work` is the caller's: invNorm1WorkBytes<T>() bytes
  // per member, 16-byte aligned, members one after the other; nothing is allocated.  A factor that broke
  // down gives a non-finite estimate.  Refuses a Solver that cannot factor completely and order() == 0.
  template <typename T>
  int64_t invNorm1WorkBytes() const;
  template <typename T>
  void invNorm1Estimate(const std::vector<const T*>& L, const std::vector<const T*>& D, void* work,
                        int64_t* devState, double* devOut, bool single) const;
  // extension: the pieces of a preconditioned conjugate gradient on the device (DESIGN.md section 24;
  // hip_cg_kernels.h).  `a` (CgArgs, hip_backend.h) names the piece (CgOp) and its operands: vectors [n, q]
  // row-major, one pointer per batch member; `state`, 12 words per (member, right-hand side), members one
  // after the other; `work`, the caller's, cgWorkBytes() per member, 16-byte aligned; `status` (CgBuild), 2
  // words per member.  n is the caller's (the operator need not be this Solver's matrix), except for the
  // built-in preconditioners, whose map must be this Solver's and of order n.  The product A p between
  // CgDirection and CgAlpha is the caller's.  Stopped columns are left bitwise unchanged by every piece.
  // CgFsaiApply (kind CgFsai, section 27) takes CgPrecond's place with a scratch vector t of its own.
  // Runs on the stream of setStream(), nothing is allocated (the first use of a preconditioner uploads its
  // plan) and nothing read back.  Refused before any device work: an empty batch, n or q out of range, a NULL
  // or misaligned workspace, a NULL pointer, a map of another Solver or order, a negative or NaN tolerance or
  // step limit, and a written operand (workspace and records included) that overlaps any other operand.
  int64_t cgWorkBytes(int64_t n, int64_t q) const;
  template <typename T>
  void cg(const CgArgs<T>& a, int64_t batch, bool single) const;
  // extension: the pieces of the matrix-free least squares (CGLS) on the device (DESIGN.md section 28;
  // hip_cgls_kernels.h) over a JacobianProductMap of this Solver (jac_product.h).  `a` (CglsArgs,
  // hip_backend.h) names the piece (CglsOp) and its operands, one pointer per batch member; `state`, `work`
  // (cglsWorkBytes() per member, 16-byte aligned) and `status` as for cg().  Runs on the stream of
  // setStream(), nothing is allocated (the first use of a part of the map uploads it) and nothing read back.
  // Refused before any device work: an empty batch, q out of range, a NULL or misaligned workspace, a NULL
  // pointer of an operand the piece needs, a map of another Solver, a negative or NaN tolerance or step limit.
  int64_t cglsWorkBytes(int64_t m, int64_t n, int64_t q) const;
  template <typename T>
  void cgls(const CglsArgs<T>& a, int64_t batch, bool single) const;
  // extension: the pieces of the implicit Schur elimination of the matrix-free least squares (DESIGN.md section
  // 29; hip_schur_kernels.h) over a JacSchurMap (jac_schur.h) of a JacobianProductMap of this Solver.  `a`
  // (JacSchurArgs, hip_backend.h) names the piece (SchurOp) and its operands, one pointer per batch member;
  // `work` (cglsWorkBytes(m, n, 1) per member, 16-byte aligned) and `status` as for cgls()'s build.  Runs on the
  // stream of setStream(), nothing is allocated (the first use of a part of the map uploads it) and nothing read
  // back.  Refused before any device work: an empty batch, q out of range, a NULL or misaligned workspace, a
  // NULL pointer of an operand the piece needs, a map of another Solver.
  template <typename T>
  void jacSchur(const JacSchurArgs<T>& a, int64_t batch, bool single) const;
  // extension: the pieces of the Lanczos recurrence on the device (DESIGN.md section 25;
  // hip_lanczos_kernels.h).  `a` (LanczosArgs, hip_backend.h) names the piece (LanczosOp) and its operands:
  // the vector [n, q] row-major and the basis (slot s at basis + s slotStride elements, `slots` of them), one
  // pointer each per batch member; `state`, 12 words, and `coef`, 2 kmax doubles, per (member, start vector),
  // members one after the other; `work`, the caller's, lanczosWorkBytes() per member, 16-byte aligned.  The
  // product w = A v_j before LzAlpha is the caller's.  Stopped columns are left bitwise unchanged by every
  // piece.  Runs on the stream of setStream(), nothing is allocated and nothing read back.  Refused before any
  // device work: an empty batch, n, q or kmax out of range, a slot or a count outside the basis, a slot
  // stride below n q, a NULL or misaligned workspace, a NULL pointer.
  int64_t lanczosWorkBytes(int64_t n, int64_t q, int64_t kmax) const;
  template <typename T>
  void lanczos(const LanczosArgs<T>& a, int64_t batch, bool single) const;
  // extension: combinations of the vectors of a basis (kvCombine, hip_lanczos_kernels.h):
  // for the nf outputs f and the q columns c of every member, out_f[:, c] = (accumulate ? out_f[:, c] : +0) +
  // sum_i T(y[c, f, i]) slot (slot + i)[:, c] over i = 0 .. count - 1 ascending in T, every product rounded
  // before it is added; term i has the index first + i and is skipped, its slot not read, when first + i >=
  // limit[c].  `a` (KrylovCombineArgs, hip_backend.h): the basis as LanczosArgs's, one pointer per member; y,
  // doubles [batch, q, nf, ldy], and limit, int64 [batch, q], one array each; out, one pointer per member, its
  // output f at out + f outStride.  Runs on the stream of setStream(), nothing is allocated and nothing read
  // back.  Refused before any device work: an empty batch, n, q or nf out of range, a count below 1, a negative
  // first, slots outside the basis, a slot or output stride below n q, ldy below count, a NULL pointer.
  template <typename T>
  void krylovCombine(const KrylovCombineArgs<T>& a, int64_t batch, bool single) const;
  // extension: blocks of A^-1 anywhere, on or off the pattern of L, by reach solves (DESIGN.md section 20;
  // reach.h, hip_reach_kernels.h).  `L` holds a complete factor() and is only read; params are the
  // caller's param ids (repeats allowed).  Both run on the stream of setStream() without host
  // synchronisation and refuse NULL pointers, ids out of range and a Solver that cannot factor completely
  // before any device work.
  //
  // reachSolveL: W = L^-1 E, E the unit columns of the params stacked in the order given (m columns in
  // all); W is m x order(), column-major with leading dimension order(), rows in internal order, every
  // element written.  Only the lumps on each column's reach are visited, then the trailing wide lumps
  // by solveLFrom over all columns.
  template <typename T>
  void reachSolveL(const T* L, const std::vector<int64_t>& params, T* W) const;
  // inverseBlocks: block k = A^-1[rowParams[k], colParams[k]], row-major at out + outOffsets[k]
  // (outOffsets: numPairs + 1 entries, block k inside [outOffsets[k], outOffsets[k + 1])); every block is
  // written once, bitwise reproducibly.  W = L^-1 E of the distinct params lives in a workspace kept with
  // the Solver (distinct columns x order() values; it grows on demand, which waits for the device).
  template <typename T>
  void inverseBlocks(const T* L, const std::vector<int64_t>& rowParams, const std::vector<int64_t>& colParams,
                     T* out, const std::vector<int64_t>& outOffsets) const;
  // the plan reachSolveL / inverseBlocks run for these queries (host only): params as above, pairs as
  // indices into params
  ReachPlan reachPlan(const char* what, const std::vector<int64_t>& params, const std::vector<int64_t>& pairRow,
                      const std::vector<int64_t>& pairCol, const std::vector<int64_t>& outOffsets = {}) const;

  // extension: products with the factor (hip_factor_product.h).  mulL: y = L x,
  // mulLt: y = L^T x, L the lower triangle of `L`: a buffer in this Solver's numeric layout of which only
  // the stored elements i >= j are read (a factor(), or any other data).  x and y are order() x nRHS,
  // column-major with leading dimensions inStride and outStride, in internal order (as for solve()).  x
  // and L are only read; every element of y is written exactly once and none is read.  Sums run in an
  // order fixed by the structure, without atomics: two runs are bitwise equal, column k of a call is
  // bitwise the call on that column alone, member q of a batch is bitwise the single call.  Both run on
  // the stream of setStream() without host synchronisation (the first call uploads the plan).  Refused
  // before any device work: NULL pointers, an empty batch, nRHS < 1, a stride below order(), an output
  // that overlaps an input or another output.
  template <typename T>
  void mulL(const T* L, const T* x, int64_t inStride, T* y, int64_t outStride, int nRHS) const;
  template <typename T>
  void mulL(const std::vector<T*>& L, const std::vector<T*>& x, int64_t inStride, const std::vector<T*>& y,
            int64_t outStride, int nRHS) const;
  template <typename T>
  void mulLt(const T* L, const T* x, int64_t inStride, T* y, int64_t outStride, int nRHS) const;
  template <typename T>
  void mulLt(const std::vector<T*>& L, const std::vector<T*>& x, int64_t inStride, const std::vector<T*>& y,
             int64_t outStride, int nRHS) const;

  // scalarPermutation()[i] = internal index of the caller's scalar i (params in param order, each
  // at the start of its span)
  std::vector<int64_t> scalarPermutation() const;

  int64_t order() const { return factorSkel.order(); }
  int64_t dataSize() const { return factorSkel.dataSize(); }
  int64_t canFactorUpToSpan() const { return canFactorUpTo; }
  int64_t spanVectorOffset(int64_t spanIndex) const {
    return factorSkel.spanVectorOffset(spanIndex);
  }
  int64_t spanMatrixOffset(int64_t spanIndex) const {
    return factorSkel.spanMatrixOffset(spanIndex);
  }
  const CoalescedBlockMatrixSkel& skel() const { return factorSkel; }
  const std::vector<int64_t>& sparseEliminationRanges() const { return sparseElimRanges; }
  const std::vector<int64_t>& paramToSpan() const { return permutation; }

  // algorithmic flops of a full factor: sum over lumps of n^3/3 + r n^2 + r^2 n
  // (n = lump width, r = rows below the diagonal block); SURVEY.md section 8(d)
  double factorFlops() const;

  // TESTING
  SymbolicCtx& internalSymbolicContext() { return *symCtx; }
  SymElimCtx& internalGetElimCtx(size_t i) {
    BASPACHO_CHECK_LT(i, elimCtxs.size());
    return *elimCtxs[i];
  }

 private:
  void initElimination();
  int64_t boardElimTempSize(int64_t lump, int64_t boardIndexInCol) const;

  template <typename T>
  void factorLump(NumericCtx<T>& numCtx, T* data, int64_t lump) const;
  template <typename T>
  void eliminateBoard(NumericCtx<T>& numCtx, T* data, int64_t ptr) const;
  template <typename T>
  void internalFactorRange(T* data, int64_t startSpanIndex, int64_t endSpanIndex,
                           bool verbose = false) const;
  template <typename T>
  void internalSolveLRange(SolveCtx<T>& slvCtx, const T* data, int64_t startSpanIndex,
                           int64_t endSpanIndex, T* vecData, int64_t stride, int nRHS) const;
  template <typename T>
  void internalSolveLtRange(SolveCtx<T>& slvCtx, const T* data, int64_t startSpanIndex,
                            int64_t endSpanIndex, T* vecData, int64_t stride, int nRHS) const;

  CoalescedBlockMatrixSkel factorSkel;
  std::vector<int64_t> sparseElimRanges;
  std::vector<int64_t> permutation;  // on indices: v'[p[i]] = v[i]
  int64_t canFactorUpTo;

  OpsPtr ops;
  SymbolicCtxPtr symCtx;
  std::vector<SymElimCtxPtr> elimCtxs;
  std::vector<int64_t> startElimRowPtr;
  int64_t maxElimTempSize = 0;
};

using SolverPtr = std::unique_ptr<Solver>;

// Engine selection.  BackendHip is the MI355X engine; BackendCuda is accepted as an alias so
// that GPU callers of the reference keep working.  BackendRef / BackendFast (CPU) are not part
// of this build and make createSolver throw.
enum BackendType {
  BackendRef,
  BackendFast,
  BackendCuda,
  BackendHip,
};

enum AddFillPolicy {
  AddFillComplete,       // fill for complete factoring, reorder
  AddFillForAutoElims,   // fill for given+auto elimination ranges, reorder
  AddFillForGivenElims,  // fill for the given elimination ranges, no reorder
  AddFillNone,           // no fill, no reorder
};

struct ComputationModel;

struct Settings {
  bool findSparseEliminationRanges = true;
  int numThreads = 16;  // unused by the HIP engine; kept for source compatibility
  BackendType backend = BackendHip;
  AddFillPolicy addFillPolicy = AddFillComplete;
  const ComputationModel* computationModel = nullptr;
  // extension: schedule switches of the MI355X backend (backend_options.h); null = defaults
  const HipBackendOptions* hipOptions = nullptr;
};

SolverPtr createSolver(const Settings& settings, const std::vector<int64_t>& paramSizes,
                       const SparseStructure& ss, const std::vector<int64_t>& sparseElimRanges = {},
                       const std::unordered_set<int64_t>& elimLastIds = {});

}  // namespace BaSpaCho
