// Solver driver.  Follows the call structure of baspacho/baspacho/Solver.cpp:
//   ctor :22-40, factorLump :42-64, eliminateBoard :66-98, initElimination :117-147,
//   internalFactorRange :164-219, solve family :221-397, createSolver :611-752.
// When the backend advertises a fused path (MI355X HIP backend) the per-op loops below are
// bypassed and the whole range is handed to NumericCtx::factorRange / SolveCtx::solve*Range.
#include "solver.h"

#include <cmath>
#include <algorithm>
#include <iostream>
#include <numeric>
#include <unordered_map>
#include <chrono>
#include <cstdlib>

#include "assembly.h"
#include "jac_product.h"
#include "jac_schur.h"
#include "normal_eq.h"
#include "reach.h"
#include "sym_product.h"
#include "computation_model.h"
#include "elimination_tree.h"
#include "hip_backend.h"

namespace BaSpaCho {

using std::vector;

namespace {

// geometry of one lump column, read off the skeleton
struct ColumnGeom {
  int64_t width;       // lump size
  int64_t diagOffset;  // data offset of the square diagonal block
  int64_t belowOffset; // data offset of the first row below the diagonal block
  int64_t rowsBelow;   // number of rows below the diagonal block
  int64_t firstBelowChain;  // chain index (absolute) of the first below-diagonal chain
  int64_t numBelowChains;
};

ColumnGeom columnGeom(const CoalescedBlockMatrixSkel& sk, int64_t lump) {
  ColumnGeom g;
  g.width = sk.lumpStart[lump + 1] - sk.lumpStart[lump];
  const int64_t c0 = sk.chainColPtr[lump];
  const int64_t nChains = sk.chainColPtr[lump + 1] - c0;
  const int64_t diagChains = sk.boardChainColOrd[sk.boardColPtr[lump] + 1];
  g.diagOffset = sk.chainData[c0];
  g.belowOffset = sk.chainData[c0 + diagChains];
  g.rowsBelow = sk.chainRowsTillEnd[c0 + nChains - 1] - sk.chainRowsTillEnd[c0 + diagChains - 1];
  g.firstBelowChain = c0 + diagChains;
  g.numBelowChains = nChains - diagChains;
  return g;
}

}  // namespace

Solver::Solver(CoalescedBlockMatrixSkel&& factorSkel_, vector<int64_t>&& sparseElimRanges_,
               vector<int64_t>&& permutation_, OpsPtr&& ops_, int64_t canFactorUpTo_)
    : factorSkel(std::move(factorSkel_)),
      sparseElimRanges(std::move(sparseElimRanges_)),
      permutation(std::move(permutation_)),
      canFactorUpTo(canFactorUpTo_ < 0 ? factorSkel.numSpans() : canFactorUpTo_),
      ops(std::move(ops_)) {
  BASPACHO_CHECK_NOTNULL(ops.get());
  BASPACHO_CHECK((int64_t)sparseElimRanges.size() != 1);
  if (permutation.empty()) {  // raw skeleton: identity ordering
    permutation.resize(factorSkel.numSpans());
    std::iota(permutation.begin(), permutation.end(), 0);
  }
  symCtx = ops->createSymbolicCtx(factorSkel, permutation);
  symCtx->setSparseElimRanges(sparseElimRanges);
  for (size_t r = 0; r + 1 < sparseElimRanges.size(); r++) {
    elimCtxs.push_back(symCtx->prepareElimination(sparseElimRanges[r], sparseElimRanges[r + 1]));
  }
  initElimination();
  symCtx->prepareFactor(canFactorUpTo < factorSkel.numSpans() ? factorSkel.spanToLump[canFactorUpTo]
                                                             : factorSkel.numLumps());
}

template <typename T>
void Solver::factorLump(NumericCtx<T>& numCtx, T* data, int64_t lump) const {
  ColumnGeom g = columnGeom(factorSkel, lump);
  numCtx.potrf(g.width, data, g.diagOffset);
  if (g.rowsBelow > 0) numCtx.trsm(g.width, g.rowsBelow, data, g.diagOffset, g.belowOffset);
}

namespace {

// shape of the update produced by board `ord` of column `lump`
struct BoardGeom {
  int64_t firstChain;   // absolute chain index where the board starts
  int64_t rectRowBegin; // rows of the column above the board
  int64_t rowsSub;      // rows of the board itself (m)
  int64_t rowsFull;     // rows from the board to the end of the column (n)
  int64_t numBlockRows, numBlockCols;
  int64_t targetLump;
};

BoardGeom boardGeom(const CoalescedBlockMatrixSkel& sk, int64_t lump, int64_t ord) {
  BoardGeom b;
  const int64_t c0 = sk.chainColPtr[lump];
  const int64_t b0 = sk.boardColPtr[lump], bEnd = sk.boardColPtr[lump + 1];
  const int64_t chFirst = sk.boardChainColOrd[b0 + ord];
  const int64_t chNext = sk.boardChainColOrd[b0 + ord + 1];
  const int64_t chEnd = sk.boardChainColOrd[bEnd - 1];
  b.firstChain = c0 + chFirst;
  b.rectRowBegin = sk.chainRowsTillEnd[c0 + chFirst - 1];
  b.rowsSub = sk.chainRowsTillEnd[c0 + chNext - 1] - b.rectRowBegin;
  b.rowsFull = sk.chainRowsTillEnd[c0 + chEnd - 1] - b.rectRowBegin;
  b.numBlockRows = chEnd - chFirst;
  b.numBlockCols = chNext - chFirst;
  b.targetLump = sk.boardRowLump[b0 + ord];
  return b;
}

}  // namespace

template <typename T>
void Solver::eliminateBoard(NumericCtx<T>& numCtx, T* data, int64_t ptr) const {
  const int64_t srcLump = factorSkel.boardColLump[ptr];
  const int64_t srcWidth = factorSkel.lumpStart[srcLump + 1] - factorSkel.lumpStart[srcLump];
  BoardGeom b = boardGeom(factorSkel, srcLump, factorSkel.boardColOrd[ptr]);

  numCtx.saveSyrkGemm(b.rowsSub, b.rowsFull, srcWidth, data, factorSkel.chainData[b.firstChain]);

  const int64_t targetWidth =
      factorSkel.lumpStart[b.targetLump + 1] - factorSkel.lumpStart[b.targetLump];
  numCtx.assemble(data, b.rectRowBegin, targetWidth, b.firstChain, b.rowsSub, b.numBlockRows,
                  b.numBlockCols);
}

int64_t Solver::boardElimTempSize(int64_t lump, int64_t boardIndexInCol) const {
  BoardGeom b = boardGeom(factorSkel, lump, boardIndexInCol);
  return b.rowsSub * b.rowsFull;
}

void Solver::initElimination() {
  const int64_t denseFrom = sparseElimRanges.empty() ? 0 : sparseElimRanges.back();
  const int64_t nLumps = factorSkel.numLumps();
  startElimRowPtr.assign(nLumps - denseFrom, 0);
  maxElimTempSize = 0;
  for (int64_t l = denseFrom; l < nLumps; l++) {
    // boards of row l, sorted by column lump; skip the sparse-eliminated source columns
    int64_t r = factorSkel.boardRowPtr[l];
    const int64_t rEnd = factorSkel.boardRowPtr[l + 1];
    BASPACHO_CHECK_EQ(factorSkel.boardColLump[rEnd - 1], l);  // last board = diagonal
    while (factorSkel.boardColLump[r] < denseFrom) r++;
    BASPACHO_CHECK_LT(r, rEnd);
    startElimRowPtr[l - denseFrom] = r;
    for (; r < rEnd && factorSkel.boardColLump[r] < l; r++) {
      const int64_t src = factorSkel.boardColLump[r], ord = factorSkel.boardColOrd[r];
      BASPACHO_CHECK_LT(ord, factorSkel.boardColPtr[src + 1] - factorSkel.boardColPtr[src]);
      BASPACHO_CHECK_EQ(l, factorSkel.boardRowLump[factorSkel.boardColPtr[src] + ord]);
      maxElimTempSize = std::max(maxElimTempSize, boardElimTempSize(src, ord));
    }
  }
}

double Solver::factorFlops() const {
  double flops = 0;
  for (int64_t l = 0; l < factorSkel.numLumps(); l++) {
    ColumnGeom g = columnGeom(factorSkel, l);
    double n = double(g.width), r = double(g.rowsBelow);
    flops += n * n * n / 3.0 + r * n * n + r * r * n;
  }
  return flops;
}

template <typename T>
void Solver::factor(T* data, bool verbose) const {
  factorUpTo(data, factorSkel.numSpans(), verbose);
}

template <typename T>
void Solver::factorUpTo(T* data, int64_t spanIndex, bool verbose) const {
  internalFactorRange(data, 0, spanIndex, verbose);
}

template <typename T>
void Solver::factorFrom(T* data, int64_t spanIndex, bool verbose) const {
  internalFactorRange(data, spanIndex, factorSkel.numSpans(), verbose);
}

template <typename T>
void Solver::internalFactorRange(T* data, int64_t startSpanIndex, int64_t endSpanIndex,
                                 bool verbose) const {
  BASPACHO_CHECK_GE(startSpanIndex, 0);
  BASPACHO_CHECK_LE(startSpanIndex, endSpanIndex);
  BASPACHO_CHECK_LT(endSpanIndex, (int64_t)factorSkel.spanOffsetInLump.size());
  BASPACHO_CHECK_EQ(factorSkel.spanOffsetInLump[startSpanIndex], 0);
  BASPACHO_CHECK_EQ(factorSkel.spanOffsetInLump[endSpanIndex], 0);
  BASPACHO_CHECK_LE(endSpanIndex, canFactorUpTo);
  const int64_t startLump = factorSkel.spanToLump[startSpanIndex];
  const int64_t upToLump = factorSkel.spanToLump[endSpanIndex];

  NumericCtxPtr<T> numCtx = symCtx->createNumericCtx<T>(maxElimTempSize, data);

  // a partial range may not cut through a sparse-elimination range
  for (size_t r = 0; r + 1 < sparseElimRanges.size(); r++) {
    const int64_t rb = sparseElimRanges[r], re = sparseElimRanges[r + 1];
    if (re > upToLump) {
      BASPACHO_CHECK_EQ(rb, upToLump);
      break;
    }
    if (startLump > rb) BASPACHO_CHECK_GE(startLump, re);
  }

  if (numCtx->hasFusedFactor()) {
    if (verbose) {
      std::cout << "Fused factor, lumps [" << startLump << ", " << upToLump << ")" << std::endl;
    }
    numCtx->factorRange(data, startLump, upToLump);
    return;
  }

  // ---- reference-style per-op loop (for backends without a fused path)
  for (size_t r = 0; r + 1 < sparseElimRanges.size(); r++) {
    const int64_t rb = sparseElimRanges[r], re = sparseElimRanges[r + 1];
    if (re > upToLump) return;
    if (startLump > rb) continue;
    if (verbose) std::cout << "Elim set: " << r << " (" << rb << ".." << re << ")" << std::endl;
    numCtx->doElimination(*elimCtxs[r], data, rb, re);
  }

  const int64_t denseFrom = sparseElimRanges.empty() ? 0 : sparseElimRanges.back();
  if (verbose) std::cout << "Block-Fact from: " << denseFrom << std::endl;

  for (int64_t l = std::max(startLump, denseFrom); l < factorSkel.numLumps(); l++) {
    numCtx->prepareAssemble(l);
    // off-diagonal boards of row l: one update per source column
    for (int64_t r = startElimRowPtr[l - denseFrom], rEnd = factorSkel.boardRowPtr[l + 1] - 1;
         r < rEnd; r++) {
      const int64_t src = factorSkel.boardColLump[r];
      if (src >= upToLump) break;
      if (src < startLump) continue;
      eliminateBoard(*numCtx, data, r);
    }
    if (l < upToLump) factorLump(*numCtx, data, l);
  }
}

template <typename T>
void Solver::solve(const T* matData, T* vecData, int64_t stride, int nRHS) const {
  SolveCtxPtr<T> slvCtx = symCtx->createSolveCtx<T>(nRHS, matData);
  internalSolveLRange(*slvCtx, matData, 0, factorSkel.numSpans(), vecData, stride, nRHS);
  internalSolveLtRange(*slvCtx, matData, 0, factorSkel.numSpans(), vecData, stride, nRHS);
}

template <typename T>
void Solver::solveL(const T* matData, T* vecData, int64_t stride, int nRHS) const {
  solveLUpTo(matData, factorSkel.numSpans(), vecData, stride, nRHS);
}

template <typename T>
void Solver::solveLt(const T* matData, T* vecData, int64_t stride, int nRHS) const {
  solveLtUpTo(matData, factorSkel.numSpans(), vecData, stride, nRHS);
}

template <typename T>
void Solver::solveLUpTo(const T* matData, int64_t spanIndex, T* vecData, int64_t stride,
                        int nRHS) const {
  SolveCtxPtr<T> slvCtx = symCtx->createSolveCtx<T>(nRHS, matData);
  internalSolveLRange(*slvCtx, matData, 0, spanIndex, vecData, stride, nRHS);
}

template <typename T>
void Solver::solveLtUpTo(const T* matData, int64_t spanIndex, T* vecData, int64_t stride,
                         int nRHS) const {
  SolveCtxPtr<T> slvCtx = symCtx->createSolveCtx<T>(nRHS, matData);
  internalSolveLtRange(*slvCtx, matData, 0, spanIndex, vecData, stride, nRHS);
}

template <typename T>
void Solver::solveLFrom(const T* matData, int64_t spanIndex, T* vecData, int64_t stride,
                        int nRHS) const {
  SolveCtxPtr<T> slvCtx = symCtx->createSolveCtx<T>(nRHS, matData);
  internalSolveLRange(*slvCtx, matData, spanIndex, factorSkel.numSpans(), vecData, stride, nRHS);
}

template <typename T>
void Solver::solveLtFrom(const T* matData, int64_t spanIndex, T* vecData, int64_t stride,
                         int nRHS) const {
  SolveCtxPtr<T> slvCtx = symCtx->createSolveCtx<T>(nRHS, matData);
  internalSolveLtRange(*slvCtx, matData, spanIndex, factorSkel.numSpans(), vecData, stride, nRHS);
}

template <typename T>
void Solver::internalSolveLRange(SolveCtx<T>& slvCtx, const T* matData, int64_t startSpanIndex,
                                 int64_t endSpanIndex, T* vecData, int64_t stride,
                                 int nRHS) const {
  BASPACHO_CHECK_GE(startSpanIndex, 0);
  BASPACHO_CHECK_LE(startSpanIndex, endSpanIndex);
  BASPACHO_CHECK_LT(endSpanIndex, (int64_t)factorSkel.spanOffsetInLump.size());
  BASPACHO_CHECK_EQ(factorSkel.spanOffsetInLump[startSpanIndex], 0);
  BASPACHO_CHECK_EQ(factorSkel.spanOffsetInLump[endSpanIndex], 0);
  const int64_t startLump = factorSkel.spanToLump[startSpanIndex];
  const int64_t upToLump = factorSkel.spanToLump[endSpanIndex];

  if (slvCtx.hasFusedSolve()) {
    // (the same range checks as the op-by-op loop below makes on its way: Solver.cpp:281-290)
    for (size_t r = 0; r + 1 < sparseElimRanges.size(); r++) {
      const int64_t rb = sparseElimRanges[r], re = sparseElimRanges[r + 1];
      if (re > upToLump) {
        BASPACHO_CHECK_EQ(rb, upToLump);
        break;
      }
      if (startLump > rb) BASPACHO_CHECK_GE(startLump, re);
    }
    slvCtx.solveLRange(matData, startLump, upToLump, vecData, stride);
    return;
  }

  for (size_t r = 0; r + 1 < sparseElimRanges.size(); r++) {
    const int64_t rb = sparseElimRanges[r], re = sparseElimRanges[r + 1];
    if (re > upToLump) {
      BASPACHO_CHECK_EQ(rb, upToLump);
      return;
    }
    if (startLump > rb) {
      BASPACHO_CHECK_GE(startLump, re);
      continue;
    }
    slvCtx.sparseElimSolveL(*elimCtxs[r], matData, rb, re, vecData, stride);
  }
  const int64_t denseFrom =
      std::max(startLump, sparseElimRanges.empty() ? int64_t(0) : sparseElimRanges.back());

  if (factorSkel.numSpans() == factorSkel.numLumps() && slvCtx.hasFragmentedOps() && nRHS == 1) {
    slvCtx.fragmentedSolveL(matData, denseFrom, upToLump, vecData);
    return;
  }
  for (int64_t l = denseFrom; l < upToLump; l++) {
    ColumnGeom g = columnGeom(factorSkel, l);
    const int64_t vecOff = factorSkel.lumpStart[l];
    slvCtx.solveL(matData, g.diagOffset, g.width, vecData, vecOff, stride);
    if (g.rowsBelow == 0) continue;
    slvCtx.gemv(matData, g.belowOffset, g.rowsBelow, g.width, vecData, vecOff, stride, -1.0);
    slvCtx.assembleVec(g.firstBelowChain, g.numBelowChains, vecData, stride);
  }
}

template <typename T>
void Solver::internalSolveLtRange(SolveCtx<T>& slvCtx, const T* matData, int64_t startSpanIndex,
                                  int64_t endSpanIndex, T* vecData, int64_t stride,
                                  int nRHS) const {
  BASPACHO_CHECK_GE(startSpanIndex, 0);
  BASPACHO_CHECK_LE(startSpanIndex, endSpanIndex);
  BASPACHO_CHECK_LT(endSpanIndex, (int64_t)factorSkel.spanOffsetInLump.size());
  BASPACHO_CHECK_EQ(factorSkel.spanOffsetInLump[startSpanIndex], 0);
  BASPACHO_CHECK_EQ(factorSkel.spanOffsetInLump[endSpanIndex], 0);
  const int64_t startLump = factorSkel.spanToLump[startSpanIndex];
  const int64_t upToLump = factorSkel.spanToLump[endSpanIndex];

  if (slvCtx.hasFusedSolve()) {
    // (the checks of the op-by-op loop below: Solver.cpp:383-392)
    for (int64_t r = (int64_t)sparseElimRanges.size() - 2; r >= 0; r--) {
      const int64_t rb = sparseElimRanges[r], re = sparseElimRanges[r + 1];
      if (re > upToLump) {
        BASPACHO_CHECK_LE(rb, upToLump);
        continue;
      }
      if (rb < startLump) {
        BASPACHO_CHECK_GE(startLump, re);
        break;
      }
    }
    slvCtx.solveLtRange(matData, startLump, upToLump, vecData, stride);
    return;
  }

  const int64_t denseFrom =
      std::max(startLump, sparseElimRanges.empty() ? int64_t(0) : sparseElimRanges.back());
  const int64_t spansInRange = factorSkel.lumpToSpan[upToLump] - factorSkel.lumpToSpan[denseFrom];
  if (spansInRange == upToLump - denseFrom && slvCtx.hasFragmentedOps() && nRHS == 1) {
    slvCtx.fragmentedSolveLt(matData, denseFrom, upToLump, vecData);
  } else {
    for (int64_t l = upToLump - 1; l >= denseFrom; l--) {
      ColumnGeom g = columnGeom(factorSkel, l);
      const int64_t vecOff = factorSkel.lumpStart[l];
      if (g.rowsBelow > 0) {
        slvCtx.assembleVecT(vecData, stride, g.firstBelowChain, g.numBelowChains);
        slvCtx.gemvT(matData, g.belowOffset, g.rowsBelow, g.width, vecData, vecOff, stride, -1.0);
      }
      slvCtx.solveLt(matData, g.diagOffset, g.width, vecData, vecOff, stride);
    }
  }

  for (int64_t r = (int64_t)sparseElimRanges.size() - 2; r >= 0; r--) {
    const int64_t rb = sparseElimRanges[r], re = sparseElimRanges[r + 1];
    if (re > upToLump) {
      BASPACHO_CHECK_LE(rb, upToLump);
      continue;
    }
    if (rb < startLump) {
      BASPACHO_CHECK_GE(startLump, re);
      return;
    }
    slvCtx.sparseElimSolveLt(*elimCtxs[r], matData, rb, re, vecData, stride);
  }
}

void Solver::printStats() const {
  std::cout << "Matrix stats:\n  data size......: " << factorSkel.dataSize()
            << "\n  solve temp data: " << maxElimTempSize << std::endl;
  for (size_t r = 0; r + 1 < sparseElimRanges.size(); r++) {
    std::cout << "  elim set [" << sparseElimRanges[r] << ".." << sparseElimRanges[r + 1]
              << "]: " << elimCtxs[r]->elimStat.toString() << std::endl;
  }
  std::cout << "Factor timings and call stats:"
            << "\n  largest node size: " << symCtx->potrfBiggestN
            << "\n  potrf: " << symCtx->potrfStat.toString()
            << "\n  trsm: " << symCtx->trsmStat.toString() << "\n  syrk/gemm("
            << symCtx->syrkCalls << "+" << symCtx->gemmCalls
            << "): " << symCtx->sygeStat.toString()
            << "\n  asmbl: " << symCtx->asmblStat.toString() << std::endl;
}

void Solver::enableStats(bool enable) {
  for (auto& e : elimCtxs) e->elimStat.enabled = enable;
  symCtx->potrfStat.enabled = enable;
  symCtx->trsmStat.enabled = enable;
  symCtx->sygeStat.enabled = enable;
  symCtx->asmblStat.enabled = enable;
}

void Solver::resetStats() {
  for (auto& e : elimCtxs) e->elimStat.reset();
  symCtx->potrfBiggestN = 0;
  symCtx->potrfStat.reset();
  symCtx->trsmStat.reset();
  symCtx->syrkCalls = symCtx->gemmCalls = 0;
  symCtx->sygeStat.reset();
  symCtx->asmblStat.reset();
}

template <typename T>
void Solver::addMvFrom(const T* matData, int64_t spanIndex, const T* inVecData, int64_t inStride,
                       T* outVecData, int64_t outStride, int nRHS, BaseType<T> alpha) const {
  SolveCtxPtr<T> slvCtx = symCtx->createSolveCtx<T>(nRHS, matData);
  BASPACHO_CHECK_GE(spanIndex, 0);
  BASPACHO_CHECK_LT(spanIndex, (int64_t)factorSkel.spanOffsetInLump.size());
  BASPACHO_CHECK_EQ(factorSkel.spanOffsetInLump[spanIndex], 0);
  const int64_t startLump = factorSkel.spanToLump[spanIndex];
  const int64_t upToLump = (int64_t)factorSkel.lumpStart.size() - 1;
  if (slvCtx->hasFusedSolve()) {
    // (the reference's symm / gemv / assembleVec sequence below is one fused device kernel here)
    slvCtx->addMvRange(matData, startLump, upToLump, inVecData, inStride, outVecData, outStride,
                       alpha);
    return;
  }
  // op-by-op, as the reference drives it (Solver.cpp:412-448)
  const int64_t spansInRange = factorSkel.lumpToSpan[upToLump] - factorSkel.lumpToSpan[startLump];
  if (spansInRange == upToLump - startLump && slvCtx->hasFragmentedOps() && nRHS == 1) {
    BASPACHO_CHECK_EQ(factorSkel.lumpToSpan[startLump], startLump);
    slvCtx->fragmentedMV(matData, inVecData, startLump, upToLump, outVecData, alpha);
    return;
  }
  for (int64_t l = startLump; l < upToLump; l++) {
    ColumnGeom g = columnGeom(factorSkel, l);
    const int64_t vecOff = factorSkel.lumpStart[l];
    slvCtx->symm(matData, g.diagOffset, g.width, inVecData, vecOff, inStride, outVecData, outStride,
                 alpha);
    if (g.rowsBelow == 0) continue;
    slvCtx->gemv(matData, g.belowOffset, g.rowsBelow, g.width, inVecData, vecOff, inStride, alpha);
    slvCtx->assembleVec(g.firstBelowChain, g.numBelowChains, outVecData, outStride);
    slvCtx->assembleVecT(inVecData, inStride, g.firstBelowChain, g.numBelowChains);
    slvCtx->gemvT(matData, g.belowOffset, g.rowsBelow, g.width, outVecData, vecOff, outStride, alpha);
  }
}

template <typename T>
void Solver::pseudoFactorFrom(T* data, int64_t spanIndex, bool /*verbose*/) const {
  NumericCtxPtr<T> numCtx = symCtx->createNumericCtx<T>(maxElimTempSize, data);
  numCtx->pseudoFactorSpans(data, spanIndex, factorSkel.numSpans());
}

template void Solver::addMvFrom<double>(const double*, int64_t, const double*, int64_t, double*,
                                        int64_t, int, double) const;
template void Solver::addMvFrom<float>(const float*, int64_t, const float*, int64_t, float*,
                                       int64_t, int, float) const;
template void Solver::pseudoFactorFrom<double>(double*, int64_t, bool) const;
template void Solver::pseudoFactorFrom<float>(float*, int64_t, bool) const;

// ---- extension operations on the device --------------------------------------------------------
// Every public method is a pair: one member given by its pointers, or a batch given by vectors.  Both
// go through one run... helper per operation, which checks the arguments before any device work and
// hands host arrays of device pointers to the backend (hip_backend.h).  The checks they share:
static void checkCompleteFactor(const char* what, int64_t canFactorUpTo, int64_t numSpans,
                                const char* who = "it") {
  if (canFactorUpTo < numSpans) {
    throw std::runtime_error(std::string(what) + ": this Solver can only factor up to span " +
                             std::to_string(canFactorUpTo) +
                             " (fill added for the given elimination ranges only); " + who +
                             " needs a complete factor");
  }
}

// outputs (`outBytes` each) must not overlap one another nor any input (`inBytes` each)
template <typename T>
static void checkNoOverlap(const char* what, const std::vector<T*>& outs, size_t outBytes,
                           const std::vector<const T*>& ins, size_t inBytes) {
  struct Range {
    uintptr_t b, e;
    size_t q;
  };
  std::vector<Range> o;
  for (size_t q = 0; q < outs.size(); q++) {
    const uintptr_t b = reinterpret_cast<uintptr_t>(outs[q]);
    o.push_back({b, b + outBytes, q});
  }
  std::sort(o.begin(), o.end(), [](const Range& x, const Range& y) { return x.b < y.b; });
  for (size_t i = 1; i < o.size(); i++) {
    if (o[i].b < o[i - 1].e) {
      throw std::runtime_error(std::string(what) + ": the output buffers of batch members " +
                               std::to_string(o[i - 1].q) + " and " + std::to_string(o[i].q) + " overlap");
    }
  }
  for (size_t q = 0; q < ins.size(); q++) {
    const uintptr_t b = reinterpret_cast<uintptr_t>(ins[q]), e = b + inBytes;
    // the first output that ends past b
    auto it = std::upper_bound(o.begin(), o.end(), b, [](uintptr_t x, const Range& r) { return x < r.e; });
    // outputs are sorted by start and disjoint, so their ends are sorted too
    if (it != o.end() && it->b < e) {
      throw std::runtime_error(std::string(what) + ": the output buffer of batch member " +
                               std::to_string(it->q) + " overlaps input " + std::to_string(q));
    }
  }
}

// `v` names one non-NULL pointer per batch member
template <typename T>
static void checkMembers(const char* what, const char* name, const std::vector<T*>& v, size_t batch) {
  if (v.size() != batch) {
    throw std::runtime_error(std::string(what) + ": " + name + " has " + std::to_string(v.size()) +
                             " pointers for a batch of " + std::to_string(batch));
  }
  for (size_t q = 0; q < v.size(); q++) {
    if (v[q] == nullptr) {
      throw std::runtime_error(std::string(what) + ": the " + name + " pointer of batch member " +
                               std::to_string(q) + " is NULL");
    }
  }
}

// the members as pointers to const: what the backend takes for an argument it only reads
template <typename T>
static std::vector<const T*> constView(const std::vector<T*>& v) {
  return std::vector<const T*>(v.begin(), v.end());
}

// the pointer of a single call as a batch of one
template <typename T>
static std::vector<T*> one(const T* p) {
  return {const_cast<T*>(p)};
}

// ---- selected inversion: distinct factors (two members aliasing one buffer would race) ------------
template <typename T>
static void runSelInv(const Solver& s, SymbolicCtx& sym, bool single, const std::vector<T*>& data) {
  const char* what = "selectedInverse";
  if (data.empty()) throw std::runtime_error("selectedInverse: the batch is empty");
  checkMembers(what, "data", data, data.size());
  std::vector<std::pair<T*, size_t>> sorted;
  for (size_t q = 0; q < data.size(); q++) sorted.emplace_back(data[q], q);
  std::sort(sorted.begin(), sorted.end());
  for (size_t i = 1; i < sorted.size(); i++) {
    if (sorted[i].first == sorted[i - 1].first) {
      throw std::runtime_error("selectedInverse: batch members " + std::to_string(sorted[i - 1].second) +
                               " and " + std::to_string(sorted[i].second) +
                               " are the same pointer (two members must not share a buffer)");
    }
  }
  checkCompleteFactor(what, s.canFactorUpToSpan(), s.skel().numSpans(), "the selected inverse");
  hipBackendSelectedInverse<T>(sym, data.data(), (int64_t)data.size(), single);
}
template <typename T>
static void runSelInv(const Solver& s, SymbolicCtx& sym, T* data) {
  if (data == nullptr) throw std::runtime_error("selectedInverse: the data pointer is NULL");
  runSelInv(s, sym, true, one(data));
}
template <typename T>
static void runSelInv(const Solver& s, SymbolicCtx& sym, std::vector<T*>* data) {
  if (data == nullptr) throw std::runtime_error("selectedInverse: the batch is NULL");
  runSelInv(s, sym, false, *data);
}

template <typename T>
void Solver::selectedInverse(T* data) const {
  runSelInv(*this, *symCtx, data);
}

// ---- gradients on the pattern of L -------------------------------------------------------------
template <typename T>
static void runLogDet(const Solver& s, SymbolicCtx& sym, bool single, const std::vector<T*>& factors, T* devOut) {
  const char* what = "logDet";
  if (factors.empty()) throw std::runtime_error("logDet: the batch is empty");
  checkMembers(what, "factor", factors, factors.size());
  if (devOut == nullptr) throw std::runtime_error("logDet: the output pointer is NULL");
  checkCompleteFactor(what, s.canFactorUpToSpan(), s.skel().numSpans());
  hipBackendLogDet<T>(sym, constView(factors).data(), (int64_t)factors.size(), single, devOut);
}

template <typename T>
void Solver::logDet(const T* factor, T* devOut) const {
  if (factor == nullptr) throw std::runtime_error("logDet: the factor pointer is NULL");
  runLogDet(*this, *symCtx, true, one(factor), devOut);
}

template <typename T>
void Solver::logDet(const std::vector<T*>& factors, T* devOut) const {
  runLogDet(*this, *symCtx, false, factors, devOut);
}

// ---- status of a factor, damping of the diagonal ---------------------------------------------------
static void checkSpanRange(const char* what, int64_t spanBegin, int64_t spanEnd, int64_t numSpans) {
  if (spanBegin < 0 || spanBegin > spanEnd || spanEnd > numSpans) {
    throw std::runtime_error(std::string(what) + ": the span range [" + std::to_string(spanBegin) + ", " +
                             std::to_string(spanEnd) + ") is not inside [0, " + std::to_string(numSpans) + "]");
  }
}

template <typename T>
static void runFactorStatus(const Solver& s, SymbolicCtx& sym, bool single, const std::vector<T*>& data,
                            int64_t spanBegin, int64_t spanEnd, int64_t* devOut) {
  const char* what = "factorStatus";
  if (data.empty()) throw std::runtime_error("factorStatus: the batch is empty");
  checkMembers(what, "data", data, data.size());
  if (devOut == nullptr) throw std::runtime_error("factorStatus: the output pointer is NULL");
  checkSpanRange(what, spanBegin, spanEnd, s.skel().numSpans());
  hipBackendFactorStatus<T>(sym, constView(data).data(), (int64_t)data.size(), single, spanBegin, spanEnd, devOut);
}

template <typename T>
void Solver::factorStatus(const T* data, int64_t spanBegin, int64_t spanEnd, int64_t* devOut) const {
  if (data == nullptr) throw std::runtime_error("factorStatus: the data pointer is NULL");
  runFactorStatus(*this, *symCtx, true, one(data), spanBegin, spanEnd, devOut);
}

template <typename T>
void Solver::factorStatus(const std::vector<T*>& data, int64_t spanBegin, int64_t spanEnd, int64_t* devOut) const {
  runFactorStatus(*this, *symCtx, false, data, spanBegin, spanEnd, devOut);
}

template <typename T>
static void runDampDiagonal(const Solver& s, SymbolicCtx& sym, bool single, const std::vector<T*>& data,
                            int64_t spanBegin, int64_t spanEnd, const T* devAlphaBeta) {
  const char* what = "dampDiagonal";
  if (data.empty()) throw std::runtime_error("dampDiagonal: the batch is empty");
  checkMembers(what, "data", data, data.size());
  if (devAlphaBeta == nullptr) throw std::runtime_error("dampDiagonal: the alpha / beta pointer is NULL");
  checkSpanRange(what, spanBegin, spanEnd, s.skel().numSpans());
  // in place: two members on one buffer would be damped twice, in a race
  checkNoOverlap<T>(what, data, (size_t)s.dataSize() * sizeof(T), {}, 0);
  hipBackendDampDiagonal<T>(sym, data.data(), (int64_t)data.size(), single, spanBegin, spanEnd, devAlphaBeta);
}

template <typename T>
void Solver::dampDiagonal(T* data, int64_t spanBegin, int64_t spanEnd, const T* devAlphaBeta) const {
  if (data == nullptr) throw std::runtime_error("dampDiagonal: the data pointer is NULL");
  runDampDiagonal(*this, *symCtx, true, one(data), spanBegin, spanEnd, devAlphaBeta);
}

template <typename T>
void Solver::dampDiagonal(const std::vector<T*>& data, int64_t spanBegin, int64_t spanEnd,
                          const T* devAlphaBeta) const {
  runDampDiagonal(*this, *symCtx, false, data, spanBegin, spanEnd, devAlphaBeta);
}

// Z and U / V may be empty vectors (not given); the batch is the size of `out`
template <typename T>
static void runPatternGrad(const Solver& s, SymbolicCtx& sym, bool single, const std::vector<T*>& Z,
                           const T* zScale, const std::vector<T*>& U, const std::vector<T*>& V, int64_t stride,
                           int nRHS, T alpha, const std::vector<T*>& out) {
  const char* what = "patternGrad";
  const size_t batch = out.size();
  if (batch == 0) throw std::runtime_error("patternGrad: the batch is empty");
  checkMembers(what, "out", out, batch);
  if (Z.empty() && U.empty() && V.empty()) {
    throw std::runtime_error("patternGrad: neither Z nor U / V given (nothing to compute)");
  }
  if (!Z.empty()) {
    checkMembers(what, "Z", Z, batch);
    if (zScale == nullptr) throw std::runtime_error("patternGrad: Z given without its device scale (NULL)");
  }
  if (U.empty() != V.empty()) throw std::runtime_error("patternGrad: U and V must be given together");
  if (!U.empty()) {
    checkMembers(what, "U", U, batch);
    checkMembers(what, "V", V, batch);
    if (nRHS < 1) throw std::runtime_error("patternGrad: nRHS = " + std::to_string(nRHS) + " < 1");
    if (stride < s.order()) {
      throw std::runtime_error("patternGrad: stride " + std::to_string(stride) + " < order " +
                               std::to_string(s.order()));
    }
  }
  checkCompleteFactor(what, s.canFactorUpToSpan(), s.skel().numSpans());
  const std::vector<const T*> z = constView(Z), u = constView(U), v = constView(V);
  HipGradArgs<T> a;
  a.z = z.empty() ? nullptr : z.data();
  a.zScale = zScale;
  a.u = u.empty() ? nullptr : u.data();
  a.v = v.empty() ? nullptr : v.data();
  a.ld = stride;
  a.nRHS = u.empty() ? 0 : nRHS;
  a.alpha = alpha;
  a.out = out.data();
  hipBackendPatternGrad<T>(sym, a, (int64_t)batch, single);
}

template <typename T>
void Solver::patternGrad(const T* Z, const T* zScale, const T* U, const T* V, int64_t stride, int nRHS,
                         T alpha, T* out) const {
  if (out == nullptr) throw std::runtime_error("patternGrad: the output pointer is NULL");
  if ((U == nullptr) != (V == nullptr)) throw std::runtime_error("patternGrad: U and V must be given together");
  const auto opt = [](const T* p) { return p ? one(p) : std::vector<T*>{}; };
  runPatternGrad(*this, *symCtx, true, opt(Z), zScale, opt(U), opt(V), stride, nRHS, alpha, one(out));
}

template <typename T>
void Solver::patternGrad(const std::vector<T*>& Z, const T* zScale, const std::vector<T*>& U,
                         const std::vector<T*>& V, int64_t stride, int nRHS, T alpha,
                         const std::vector<T*>& out) const {
  runPatternGrad(*this, *symCtx, false, Z, zScale, U, V, stride, nRHS, alpha, out);
}

template <typename T>
static void runPatternOuter(const Solver& s, SymbolicCtx& sym, bool single, const std::vector<T*>& U,
                            const std::vector<T*>& V, int64_t stride, int nRHS, T alpha,
                            const std::vector<T*>& out) {
  const char* what = "patternOuter";
  if (out.empty()) throw std::runtime_error("patternOuter: the batch is empty");
  checkMembers(what, "out", out, out.size());
  checkMembers(what, "U", U, out.size());
  checkMembers(what, "V", V, out.size());
  if (nRHS < 1) throw std::runtime_error("patternOuter: nRHS = " + std::to_string(nRHS) + " < 1");
  if (stride < s.order()) {
    throw std::runtime_error("patternOuter: stride " + std::to_string(stride) + " < order " +
                             std::to_string(s.order()));
  }
  const std::vector<const T*> u = constView(U), v = constView(V);
  std::vector<const T*> in = u;
  in.insert(in.end(), v.begin(), v.end());
  checkNoOverlap(what, out, s.dataSize() * sizeof(T), in, (stride * (nRHS - 1) + s.order()) * sizeof(T));
  checkCompleteFactor(what, s.canFactorUpToSpan(), s.skel().numSpans());
  HipGradArgs<T> a;
  a.u = u.data();
  a.v = v.data();
  a.ld = stride;
  a.nRHS = nRHS;
  a.alpha = alpha;
  a.out = out.data();
  a.outer = true;
  hipBackendPatternGrad<T>(sym, a, (int64_t)out.size(), single);
}

template <typename T>
void Solver::patternOuter(const T* U, const T* V, int64_t stride, int nRHS, T alpha, T* out) const {
  runPatternOuter(*this, *symCtx, true, one(U), one(V), stride, nRHS, alpha, one(out));
}

template <typename T>
void Solver::patternOuter(const std::vector<T*>& U, const std::vector<T*>& V, int64_t stride, int nRHS, T alpha,
                          const std::vector<T*>& out) const {
  runPatternOuter(*this, *symCtx, false, U, V, stride, nRHS, alpha, out);
}

// ---- reverse-mode sweep of the factor, of the partial factor and its dense
// ---- Schur complement (section 16) ----------------------------------------------------------------
// the lump of a span that factorUpTo accepts as its end; anything else throws before any device work
int64_t Solver::partialCutLump(const char* what, int64_t spanIndex) const {
  const int64_t nSpans = factorSkel.numSpans();
  checkCompleteFactor(what, canFactorUpTo, nSpans);
  if (spanIndex < 0 || spanIndex > nSpans) {
    throw std::runtime_error(std::string(what) + ": span " + std::to_string(spanIndex) + " is not in [0, " +
                             std::to_string(nSpans) + "]");
  }
  if (factorSkel.spanOffsetInLump[spanIndex] != 0) {
    throw std::runtime_error(std::string(what) + ": span " + std::to_string(spanIndex) +
                             " lies inside a lump (a partial factor ends at a lump boundary)");
  }
  const int64_t lump = factorSkel.spanToLump[spanIndex];
  for (size_t r = 0; r + 1 < sparseElimRanges.size(); r++) {
    if (sparseElimRanges[r] < lump && lump < sparseElimRanges[r + 1]) {
      throw std::runtime_error(std::string(what) + ": span " + std::to_string(spanIndex) + " (lump " +
                               std::to_string(lump) + ") cuts the sparse-elimination range [" +
                               std::to_string(sparseElimRanges[r]) + ", " +
                               std::to_string(sparseElimRanges[r + 1]) + ")");
    }
  }
  return lump;
}

// the sweep of the factor up to spanIndex; factorAdjoint is the cut behind the last span (`name`: what
// the operation calls its factor argument)
template <typename T>
static void runFactorAdjoint(const Solver& s, SymbolicCtx& sym, const char* what, const char* name, bool single,
                             const std::vector<T*>& P, const std::vector<T*>& grad, int64_t spanIndex) {
  if (grad.empty()) throw std::runtime_error(std::string(what) + ": the batch is empty");
  checkMembers(what, "grad", grad, grad.size());
  checkMembers(what, name, P, grad.size());
  const std::vector<const T*> p = constView(P);
  const size_t bytes = s.dataSize() * sizeof(T);
  checkNoOverlap(what, grad, bytes, p, bytes);
  const int64_t lump = s.partialCutLump(what, spanIndex);
  hipBackendFactorAdjointUpTo<T>(sym, p.data(), grad.data(), (int64_t)grad.size(), single, lump);
}

template <typename T>
void Solver::factorAdjoint(const T* L, T* grad) const {
  runFactorAdjoint(*this, *symCtx, "factorAdjoint", "L", true, one(L), one(grad), factorSkel.numSpans());
}

template <typename T>
void Solver::factorAdjoint(const std::vector<T*>& L, const std::vector<T*>& grad) const {
  runFactorAdjoint(*this, *symCtx, "factorAdjoint", "L", false, L, grad, factorSkel.numSpans());
}

template <typename T>
void Solver::factorAdjointUpTo(const T* P, T* grad, int64_t spanIndex) const {
  runFactorAdjoint(*this, *symCtx, "factorAdjointUpTo", "P", true, one(P), one(grad), spanIndex);
}

template <typename T>
void Solver::factorAdjointUpTo(const std::vector<T*>& P, const std::vector<T*>& grad, int64_t spanIndex) const {
  runFactorAdjoint(*this, *symCtx, "factorAdjointUpTo", "P", false, P, grad, spanIndex);
}

// ---- reverse mode of selected inversion ------------------------------------
template <typename T>
static void runSelInvAdjoint(const Solver& s, SymbolicCtx& sym, bool single, const std::vector<T*>& L,
                             const std::vector<T*>& Z, const std::vector<T*>& grad) {
  const char* what = "selectedInverseAdjoint";
  if (grad.empty()) throw std::runtime_error(std::string(what) + ": the batch is empty");
  checkMembers(what, "grad", grad, grad.size());
  checkMembers(what, "L", L, grad.size());
  checkMembers(what, "Z", Z, grad.size());
  const std::vector<const T*> l = constView(L), z = constView(Z);
  std::vector<const T*> in = l;
  in.insert(in.end(), z.begin(), z.end());
  const size_t bytes = s.dataSize() * sizeof(T);
  checkNoOverlap(what, grad, bytes, in, bytes);
  checkCompleteFactor(what, s.canFactorUpToSpan(), s.skel().numSpans());
  hipBackendSelectedInverseAdjoint<T>(sym, l.data(), z.data(), grad.data(), (int64_t)grad.size(), single);
}

template <typename T>
void Solver::selectedInverseAdjoint(const T* L, const T* Z, T* grad) const {
  runSelInvAdjoint(*this, *symCtx, true, one(L), one(Z), one(grad));
}

template <typename T>
void Solver::selectedInverseAdjoint(const std::vector<T*>& L, const std::vector<T*>& Z,
                                    const std::vector<T*>& grad) const {
  runSelInvAdjoint(*this, *symCtx, false, L, Z, grad);
}

// toDense: in = layout buffers, out = dense m x m; else in = dense gradients, out = layout buffers
template <typename T>
static void runSchurDense(const Solver& s, SymbolicCtx& sym, const char* what, bool single,
                          const std::vector<T*>& in, const std::vector<T*>& out, int64_t spanIndex,
                          const int32_t* dest, bool toDense) {
  if (out.empty()) throw std::runtime_error(std::string(what) + ": the batch is empty");
  checkMembers(what, "out", out, out.size());
  checkMembers(what, "in", in, out.size());
  const int64_t lump = s.partialCutLump(what, spanIndex);
  const int64_t m = s.order() - s.skel().spanStart[spanIndex];
  if (m == 0) throw std::runtime_error(std::string(what) + ": no span behind span " + std::to_string(spanIndex));
  const size_t dataBytes = s.dataSize() * sizeof(T), denseBytes = (size_t)m * m * sizeof(T);
  const std::vector<const T*> i = constView(in);
  checkNoOverlap(what, out, toDense ? denseBytes : dataBytes, i, toDense ? dataBytes : denseBytes);
  hipBackendSchurDense<T>(sym, i.data(), out.data(), (int64_t)out.size(), single, lump, dest, toDense);
}

template <typename T>
void Solver::schurComplement(const T* P, int64_t spanIndex, T* out, const int32_t* dest) const {
  runSchurDense(*this, *symCtx, "schurComplement", true, one(P), one(out), spanIndex, dest, true);
}
template <typename T>
void Solver::schurComplement(const std::vector<T*>& P, int64_t spanIndex, const std::vector<T*>& out,
                             const int32_t* dest) const {
  runSchurDense(*this, *symCtx, "schurComplement", false, P, out, spanIndex, dest, true);
}
template <typename T>
void Solver::schurComplementAdjoint(const T* gradDense, int64_t spanIndex, T* gradData, const int32_t* dest) const {
  runSchurDense(*this, *symCtx, "schurComplementAdjoint", true, one(gradDense), one(gradData), spanIndex, dest, false);
}
template <typename T>
void Solver::schurComplementAdjoint(const std::vector<T*>& gradDense, int64_t spanIndex,
                                    const std::vector<T*>& gradData, const int32_t* dest) const {
  runSchurDense(*this, *symCtx, "schurComplementAdjoint", false, gradDense, gradData, spanIndex, dest, false);
}

// ---- assembly of coordinate entries -----------------------------------------------------------
std::vector<int64_t> Solver::scalarPermutation() const {
  const std::vector<int64_t>& spanStart = factorSkel.spanStart;
  std::vector<int64_t> out;
  out.reserve(order());
  for (int64_t sp : permutation) {
    for (int64_t i = spanStart[sp]; i < spanStart[sp + 1]; i++) out.push_back(i);
  }
  return out;
}

// One side of an operation on an entry map: what its pointers are called in a message about one of them
// (`name`) and about their number (`counted`), one pointer per batch member, the elements behind each
// pointer, and whether the operation writes them (the last side does).  A side of 0 elements is never
// touched and may be NULL.
template <typename T>
struct OpSide {
  const char *name, *counted;
  const T* const* ptrs;
  size_t members;
  int64_t elems;
  bool output;
};

// The argument check of assemble, normalEq and symProduct, before any device work.  Faults are reported
// in this order: a map of another solver; an empty batch; sides of different member counts; `fault`, the
// caller's own finding about its scalar arguments (empty: none); then, member by member, a NULL pointer
// (the sides in the order given) and an output that repeats an earlier member's; then, with `aliasing`,
// member by member, an output that overlaps an input of its member (the inputs in the order given) and
// an input that is the output of any member.
template <typename T>
static void checkOpArguments(const char* what, const char* mapName, bool sameSolver,
                             const std::vector<OpSide<T>>& sides, const std::string& fault, bool aliasing) {
  const auto fail = [what](const std::string& m) { throw std::runtime_error(std::string(what) + ": " + m); };
  const auto pointerOf = [](const OpSide<T>& s, size_t b) {
    return std::string("the ") + s.name + " pointer of batch member " + std::to_string(b);
  };
  const size_t members = sides[0].members;
  const OpSide<T>& out = sides.back();
  if (!sameSolver) fail(std::string("the ") + mapName + " was built on another solver");
  if (members == 0) fail("the batch is empty");
  bool sameCount = true;
  std::string counts;
  for (size_t i = 0; i < sides.size(); i++) {
    sameCount = sameCount && sides[i].members == members;
    counts += (i == 0 ? "" : i + 1 == sides.size() ? " and " : ", ") + std::to_string(sides[i].members) + " " +
              sides[i].counted;
  }
  if (!sameCount) fail("the batch has " + counts);
  if (!fault.empty()) fail(fault);
  std::unordered_set<const T*> seen;
  for (size_t b = 0; b < members; b++) {
    for (const OpSide<T>& s : sides) {
      if (s.ptrs[b] == nullptr && s.elems > 0) fail(pointerOf(s, b) + " is NULL");
    }
    if (out.ptrs[b] != nullptr && !seen.insert(out.ptrs[b]).second) {
      fail(pointerOf(out, b) + " repeats an earlier member's");
    }
  }
  if (!aliasing) return;
  const auto overlap = [](const T* a, int64_t na, const T* b, int64_t nb) {
    return a != nullptr && b != nullptr && na > 0 && nb > 0 && a < b + nb && b < a + na;
  };
  for (size_t b = 0; b < members; b++) {
    for (const OpSide<T>& s : sides) {
      if (!s.output && overlap(out.ptrs[b], out.elems, s.ptrs[b], s.elems)) {
        fail(pointerOf(out, b) + " aliases its " + s.name);
      }
    }
    for (const OpSide<T>& s : sides) {
      if (!s.output && seen.count(s.ptrs[b])) {
        fail("an input pointer of batch member " + std::to_string(b) + " is also an output of the batch");
      }
    }
  }
}

// `in` is values forward and gradData backward, `out` data forward and gradValues backward.  With nnz = 0
// the nnz-sized side may be NULL; the layout side must be given even when the layout is empty.  Aliasing
// is not checked
template <typename T>
static void runAssembly(const char* what, const Solver* self, SymbolicCtx& sym, const AssemblyMap& map,
                        const std::vector<const T*>& in, const std::vector<T*>& out, bool single, bool adjoint) {
  const int64_t nLayout = std::max<int64_t>(map.dataSize, 1);
  checkOpArguments<T>(what, "assembly", map.solver == self,
                      {{adjoint ? "gradient-of-data" : "values", "inputs", in.data(), in.size(),
                        adjoint ? nLayout : map.nnz, false},
                       {adjoint ? "gradient-of-values" : "data", "outputs", out.data(), out.size(),
                        adjoint ? map.nnz : nLayout, true}},
                      "", false);
  hipBackendAssemble<T>(sym, map, in.data(), out.data(), (int64_t)in.size(), single, adjoint);
}

template <typename T>
void Solver::assemble(const AssemblyMap& map, const T* values, T* data) const {
  runAssembly<T>("assemble", this, *symCtx, map, {values}, {data}, true, false);
}
template <typename T>
void Solver::assemble(const AssemblyMap& map, const std::vector<const T*>& values,
                      const std::vector<T*>& data) const {
  runAssembly<T>("assemble", this, *symCtx, map, values, data, false, false);
}
template <typename T>
void Solver::assembleAdjoint(const AssemblyMap& map, const T* gradData, T* gradValues) const {
  runAssembly<T>("assembleAdjoint", this, *symCtx, map, {gradData}, {gradValues}, true, true);
}
template <typename T>
void Solver::assembleAdjoint(const AssemblyMap& map, const std::vector<const T*>& gradData,
                             const std::vector<T*>& gradValues) const {
  runAssembly<T>("assembleAdjoint", this, *symCtx, map, gradData, gradValues, false, true);
}

// ---- normal equations of a sparse Jacobian -------------------------------------------------------
template <typename T>
void Solver::normalEq(const NormalEqMap& map, int32_t op, const std::vector<const T*>& values,
                      const std::vector<const T*>& x, const std::vector<T*>& out, int64_t q, bool single) const {
  static const char* names[4] = {"normalEqHessian", "normalEqHessianAdjoint", "normalEqJtVec", "normalEqJVec"};
  if (op < 0 || op > 3) throw std::runtime_error("normalEq: unknown operation " + std::to_string(op));
  const bool hasX = op != NormalEqHessian, adj = op == NormalEqAdjoint, jt = op == NormalEqJtVec;
  std::vector<OpSide<T>> sides = {{"values", "values", values.data(), values.size(), map.nnz, false}};
  if (hasX) {
    sides.push_back({adj ? "gradient-of-data" : "vector", "inputs", x.data(), x.size(),
                     adj ? map.dataSize : jt ? map.m * q : map.n * q, false});
  }
  sides.push_back({!hasX ? "data" : adj ? "gradient-of-values" : "output", "outputs", out.data(), out.size(),
                   !hasX ? map.dataSize : adj ? map.nnz : jt ? map.n * q : map.m * q, true});
  const bool badQ = hasX && !adj && q < 1;
  checkOpArguments<T>(names[op], "map", map.solver == this, sides,
                      badQ ? "q = " + std::to_string(q) + " vectors; at least one is needed" : "", true);
  hipBackendNormalEq<T>(*symCtx, map, op, values.data(), hasX ? x.data() : nullptr, out.data(), q,
                        (int64_t)values.size(), single);
}
// ---- products with a matrix given as entries (sym_product.h) -------------------
template <typename T>
void Solver::symProduct(const SymProductMap& map, int32_t op, const std::vector<const T*>& a,
                        const std::vector<const T*>& x, const std::vector<T*>& out, int64_t q, bool single) const {
  if (op != SymProductMv && op != SymProductOuter) {
    throw std::runtime_error("symProduct: unknown operation " + std::to_string(op));
  }
  const bool mv = op == SymProductMv;
  const std::string fault = q < 1            ? "q = " + std::to_string(q) + " vectors; at least one is needed"
                            : q >= INT32_MAX ? "q = " + std::to_string(q) + " vectors is outside [1, 2^31 - 1)"
                                             : "";
  checkOpArguments<T>(mv ? "symProductMv" : "symProductOuter", "map", map.solver == this,
                      {{mv ? "values" : "gradient", mv ? "values" : "gradients", a.data(), a.size(),
                        mv ? map.nnz : map.n * q, false},
                       {"vector", "vectors", x.data(), x.size(), map.n * q, false},
                       {mv ? "output" : "gradient-of-values", "outputs", out.data(), out.size(),
                        mv ? map.n * q : map.nnz, true}},
                      fault, true);
  hipBackendSymProduct<T>(*symCtx, map, op, a.data(), x.data(), out.data(), q, (int64_t)a.size(), single);
}
// ---- error bounds -------------------------------------------------------------
static std::string badVectorCount(int64_t q) {
  return q < 1            ? "q = " + std::to_string(q) + " vectors; at least one is needed"
         : q >= INT32_MAX ? "q = " + std::to_string(q) + " vectors is outside [1, 2^31 - 1)"
                          : "";
}

template <typename T>
void Solver::symResidual(const SymProductMap& map, const std::vector<const T*>& values,
                         const std::vector<const T*>& x, const std::vector<const T*>& b, const std::vector<T*>& r,
                         const std::vector<T*>& d, int64_t q, bool single) const {
  const bool hasB = !b.empty() || !r.empty();
  const char* what = hasB ? "symProductResidual" : "symProductAbsMv";
  const std::string fault = badVectorCount(q);
  const int64_t nq = map.n * q;
  std::vector<OpSide<T>> ins = {{"values", "values", values.data(), values.size(), map.nnz, false},
                                {"vector", "vectors", x.data(), x.size(), nq, false}};
  if (hasB) ins.push_back({"right-hand side", "right-hand sides", b.data(), b.size(), nq, false});
  const std::vector<const T*> rc(r.begin(), r.end()), dc(d.begin(), d.end());
  if (hasB) {
    std::vector<OpSide<T>> sides = ins;
    sides.push_back({"scale", "scale outputs", dc.data(), dc.size(), nq, false});
    sides.push_back({"residual", "residual outputs", rc.data(), rc.size(), nq, true});
    checkOpArguments<T>(what, "map", map.solver == this, sides, fault, true);
  }
  // (the second output against the inputs and, as an input of this check, against the first)
  std::vector<OpSide<T>> sides = ins;
  if (hasB) sides.push_back({"residual", "residual outputs", rc.data(), rc.size(), nq, false});
  sides.push_back({hasB ? "scale" : "output", hasB ? "scale outputs" : "outputs", dc.data(), dc.size(), nq, true});
  checkOpArguments<T>(what, "map", map.solver == this, sides, fault, true);
  hipBackendSymResidual<T>(*symCtx, map, values.data(), x.data(), hasB ? b.data() : nullptr,
                           hasB ? r.data() : nullptr, d.data(), q, (int64_t)values.size(), single);
}

template <typename T>
void Solver::colMax(const std::vector<const T*>& a, const std::vector<const T*>& b, int64_t n, int64_t q,
                    double* devOut, bool single) const {
  const bool ratio = !b.empty();
  const std::string what = ratio ? "maxRatio" : "colMax";
  const auto fail = [&](const std::string& m) { throw std::runtime_error(what + ": " + m); };
  if (a.empty()) fail("the batch is empty");
  if (ratio && b.size() != a.size()) {
    fail("the batch has " + std::to_string(a.size()) + " numerators and " + std::to_string(b.size()) + " denominators");
  }
  if (n < 0) fail("n = " + std::to_string(n) + " rows");
  const std::string fault = badVectorCount(q);
  if (!fault.empty()) fail(fault);
  if (devOut == nullptr) fail("the output pointer is NULL");
  const char* o0 = reinterpret_cast<const char*>(devOut);
  const char* o1 = o0 + a.size() * (size_t)q * sizeof(double);
  const auto checkSide = [&](const std::vector<const T*>& v, const char* name) {
    for (size_t m = 0; m < v.size(); m++) {
      if (v[m] == nullptr && n > 0) {
        fail(std::string("the ") + name + " pointer of batch member " + std::to_string(m) + " is NULL");
      }
      const char* p0 = reinterpret_cast<const char*>(v[m]);
      if (n > 0 && p0 < o1 && o0 < p0 + (size_t)(n * q) * sizeof(T)) {
        fail(std::string("the output aliases the ") + name + " of batch member " + std::to_string(m));
      }
    }
  };
  checkSide(a, ratio ? "numerator" : "input");
  checkSide(b, "denominator");
  hipBackendColMax<T>(*symCtx, a.data(), ratio ? b.data() : nullptr, n, q, devOut, (int64_t)a.size(), single);
}

template <typename T>
int64_t Solver::invNorm1WorkBytes() const {
  return normEstWorkBytes(order(), sizeof(T));
}

template <typename T>
void Solver::invNorm1Estimate(const std::vector<const T*>& L, const std::vector<const T*>& D, void* work,
                              int64_t* devState, double* devOut, bool single) const {
  const char* what = "invNorm1Estimate";
  const auto fail = [&](const std::string& m) { throw std::runtime_error(std::string(what) + ": " + m); };
  checkCompleteFactor(what, canFactorUpTo, factorSkel.numSpans());
  const int64_t n = order(), batch = (int64_t)L.size();
  if (batch == 0) fail("the batch is empty");
  if (n < 1) fail("the order is 0");
  const bool scaled = !D.empty();
  if (scaled && D.size() != L.size()) {
    fail("the batch has " + std::to_string(L.size()) + " factors and " + std::to_string(D.size()) + " scale vectors");
  }
  if (work == nullptr) fail("the workspace pointer is NULL");
  if (reinterpret_cast<uintptr_t>(work) % 16 != 0) fail("the workspace is not 16-byte aligned");
  if (devState == nullptr) fail("the state pointer is NULL");
  if (devOut == nullptr) fail("the output pointer is NULL");
  const int64_t stride = invNorm1WorkBytes<T>();
  char* w0 = static_cast<char*>(work);
  const char* w1 = w0 + batch * stride;
  const auto overlapsWork = [&](const void* p, size_t bytes) {
    const char* c = static_cast<const char*>(p);
    return c < w1 && w0 < c + bytes;
  };
  for (int64_t m = 0; m < batch; m++) {
    if (L[m] == nullptr) fail("the factor pointer of batch member " + std::to_string(m) + " is NULL");
    if (scaled && D[m] == nullptr) fail("the scale pointer of batch member " + std::to_string(m) + " is NULL");
    if (overlapsWork(L[m], (size_t)dataSize() * sizeof(T))) {
      fail("the workspace aliases the factor of batch member " + std::to_string(m));
    }
    if (scaled && overlapsWork(D[m], (size_t)n * sizeof(T))) {
      fail("the workspace aliases the scale vector of batch member " + std::to_string(m));
    }
  }
  const size_t stateBytes = (size_t)batch * 12 * sizeof(int64_t), outBytes = (size_t)batch * sizeof(double);
  if (overlapsWork(devState, stateBytes)) fail("the workspace aliases the state");
  if (overlapsWork(devOut, outBytes)) fail("the workspace aliases the output");
  const char* s0 = reinterpret_cast<const char*>(devState);
  const char* o0 = reinterpret_cast<const char*>(devOut);
  if (o0 < s0 + stateBytes && s0 < o0 + outBytes) fail("the output aliases the state");
  // the two outputs against the inputs (the same factor or scale vector in several members is allowed)
  const auto overlapsOutputs = [&](const void* p, size_t bytes) -> const char* {
    const char* c = static_cast<const char*>(p);
    if (c < s0 + stateBytes && s0 < c + bytes) return "state";
    if (c < o0 + outBytes && o0 < c + bytes) return "output";
    return nullptr;
  };
  for (int64_t m = 0; m < batch; m++) {
    if (const char* o = overlapsOutputs(L[m], (size_t)dataSize() * sizeof(T))) {
      fail(std::string("the ") + o + " aliases the factor of batch member " + std::to_string(m));
    }
    if (scaled) {
      if (const char* o = overlapsOutputs(D[m], (size_t)n * sizeof(T))) {
        fail(std::string("the ") + o + " aliases the scale vector of batch member " + std::to_string(m));
      }
    }
  }

  std::vector<T*> mats(batch), vecs(batch);
  for (int64_t m = 0; m < batch; m++) {
    mats[m] = const_cast<T*>(L[m]);
    vecs[m] = reinterpret_cast<T*>(w0 + m * stride);
  }
  const auto step = [&](int32_t s) {
    hipBackendNormEstStep<T>(*symCtx, s, work, scaled ? D.data() : nullptr, devState, devOut, batch, single);
  };
  const auto applyInverse = [&]() {  // x <- [D] A^-1 [D] x
    if (scaled) step(NormEstScale);
    if (single) {
      solve<T>(mats[0], vecs[0], n, 1);
    } else {
      solve(&mats, &vecs, n, 1);
    }
    if (scaled) step(NormEstScale);
  };
  step(NormEstStart);
  applyInverse();
  step(NormEstSum);
  applyInverse();
  step(NormEstArgMax);
  for (int pass = 2; pass <= 5; pass++) {
    step(NormEstUnit);
    applyInverse();
    step(NormEstSum);
    if (pass == 5) break;
    applyInverse();
    step(NormEstArgMax);
  }
  step(NormEstAltVector);
  applyInverse();
  step(NormEstAltSum);
}

// ---- preconditioned conjugate gradient ----------------------------------------
int64_t Solver::cgWorkBytes(int64_t n, int64_t q) const {
  if (n < 0 || n >= (int64_t(1) << 31) || q < 1 || q >= INT32_MAX) {
    throw std::runtime_error("cgWorkBytes: n = " + std::to_string(n) + ", q = " + std::to_string(q) +
                             " is outside [0, 2^31) x [1, 2^31 - 1)");
  }
  return BaSpaCho::cgWorkBytes(n, q);
}

template <typename T>
void Solver::cg(const CgArgs<T>& a, int64_t batch, bool single) const {
  static const char* names[7] = {"cgInit",      "cgAlpha",        "cgUpdate",   "cgPrecond",
                                 "cgDirection", "cgPrecondBuild", "cgFsaiApply"};
  if (a.op < 0 || a.op > CgFsaiApply) throw std::runtime_error("cg: unknown operation " + std::to_string(a.op));
  const std::string what = names[a.op];
  const auto fail = [&](const std::string& m) { throw std::runtime_error(what + ": " + m); };
  const bool builtIn = a.kind == CgJacobi || a.kind == CgBlockJacobi;
  const bool fsai = a.kind == CgFsai && (a.op == CgBuild || a.op == CgFsaiApply);
  const bool usesMap = a.op == CgBuild || (a.op == CgPrecond && builtIn) || a.op == CgFsaiApply;
  if (a.op == CgPrecond && a.kind == CgFsai) {
    fail("kind 3 (fsai) needs the scratch vector t: it is applied by bsp_fsai_apply_*");
  }
  if ((a.op == CgBuild && !builtIn && !fsai) || (a.op == CgPrecond && !builtIn && a.kind != CgGiven) ||
      (a.op == CgFsaiApply && !fsai)) {
    fail("unknown preconditioner kind " + std::to_string(a.kind) +
         " (0: the caller's z, 1: jacobi, 2: block_jacobi, 3: fsai)");
  }
  if (usesMap) {
    if (a.map == nullptr) fail("the map is NULL");
    if (a.map->solver != this) fail("the map was built on another solver");
    if (a.map->n != a.n) {
      fail("n = " + std::to_string(a.n) + ", the map's order is " + std::to_string(a.map->n));
    }
  }
  if (batch < 1) fail("the batch is empty");
  if (a.n < 0 || a.n >= (int64_t(1) << 31)) fail("n = " + std::to_string(a.n) + " is outside [0, 2^31)");
  const std::string fault = badVectorCount(a.q);
  if (!fault.empty()) fail(fault);
  const int64_t nq = a.n * a.q, parts = (a.n + 1023) / 1024;
  if (nq >= (int64_t(1) << 40) || parts * a.q >= INT32_MAX) fail("n q = " + std::to_string(nq) + " is too large");
  if (a.op == CgInit) {
    if (!(a.tol >= 0.0)) fail("tol = " + std::to_string(a.tol) + "; it must be >= 0");
    if (a.maxSteps < 0) fail("max_steps = " + std::to_string(a.maxSteps) + "; it must be >= 0");
  }
  if (a.work == nullptr) fail("the workspace pointer is NULL");
  if (reinterpret_cast<uintptr_t>(a.work) % 16 != 0) fail("the workspace is not 16-byte aligned");
  if (a.op == CgBuild ? a.status == nullptr : a.state == nullptr) {
    fail(a.op == CgBuild ? "the status pointer is NULL" : "the state pointer is NULL");
  }
  // the operands of the piece: (name, pointers, elements, written)
  struct Slot {
    const char* name;
    const T* const* ptrs;
    int64_t elems;
    bool written;
  };
  const int64_t invElems = fsai ? cgFsaiPlan(*a.map).elems() : usesMap ? cgPrecondPlan(*a.map, a.kind).inverseElems() : 0;
  const auto c = [](T* const* p) { return const_cast<const T* const*>(p); };
  std::vector<Slot> slots;
  switch (a.op) {
    case CgInit: slots = {{"right-hand side", a.in0, nq, false}, {"x", c(a.out0), nq, true}, {"r", c(a.out1), nq, true}}; break;
    case CgAlpha: slots = {{"p", a.in0, nq, false}, {"Ap", a.in1, nq, false}}; break;
    case CgUpdate:
      slots = {{"p", a.in0, nq, false}, {"Ap", a.in1, nq, false}, {"x", c(a.out0), nq, true}, {"r", c(a.out1), nq, true}};
      break;
    case CgPrecond:
      if (builtIn) slots.push_back({"preconditioner", a.in0, invElems, false});
      slots.push_back({"r", a.in1, nq, false});
      slots.push_back({"z", c(a.out0), nq, builtIn});
      break;
    case CgDirection: slots = {{a.plain ? "r" : "z", a.in0, nq, false}, {"p", c(a.out0), nq, true}}; break;
    case CgFsaiApply:
      slots = {{"preconditioner", a.in0, invElems, false}, {"r", a.in1, nq, false}, {"t", c(a.out1), nq, true}, {"z", c(a.out0), nq, true}};
      break;
    default: slots = {{"values", a.in0, a.map->nnz, false}, {"preconditioner", c(a.out0), invElems, true}}; break;
  }
  struct Region {
    const char *begin, *end;
    bool written;
    std::string name;
  };
  std::vector<Region> regions;
  for (const Slot& s : slots) {
    if (s.ptrs == nullptr) fail(std::string("the ") + s.name + " pointers are NULL");
    for (int64_t m = 0; m < batch; m++) {
      if (s.elems == 0) continue;
      if (s.ptrs[m] == nullptr) fail(std::string("the ") + s.name + " pointer of batch member " + std::to_string(m) + " is NULL");
      const char* p = reinterpret_cast<const char*>(s.ptrs[m]);
      regions.push_back({p, p + s.elems * (int64_t)sizeof(T), s.written,
                         std::string(s.name) + " of batch member " + std::to_string(m)});
    }
  }
  const char* w0 = static_cast<const char*>(a.work);
  regions.push_back({w0, w0 + batch * BaSpaCho::cgWorkBytes(a.n, a.q), true, "workspace"});
  if (a.op == CgBuild) {
    const char* s0 = reinterpret_cast<const char*>(a.status);
    regions.push_back({s0, s0 + batch * 16, true, "status"});
  } else {
    const char* s0 = reinterpret_cast<const char*>(a.state);
    regions.push_back({s0, s0 + batch * a.q * 96, true, "state"});
  }
  std::sort(regions.begin(), regions.end(), [](const Region& x, const Region& y) { return x.begin < y.begin; });
  const Region *widest = nullptr, *widestWritten = nullptr;  // the regions so far that end last
  for (const Region& r : regions) {
    if (widestWritten != nullptr && r.begin < widestWritten->end) fail("the " + widestWritten->name + " aliases the " + r.name);
    if (r.written && widest != nullptr && r.begin < widest->end) fail("the " + r.name + " aliases the " + widest->name);
    if (widest == nullptr || r.end > widest->end) widest = &r;
    if (r.written && (widestWritten == nullptr || r.end > widestWritten->end)) widestWritten = &r;
  }
  hipBackendCg<T>(*symCtx, a, batch, single);
}

// ---- matrix-free least squares ------------------------------------------------
int64_t Solver::cglsWorkBytes(int64_t m, int64_t n, int64_t q) const {
  const int64_t lim = int64_t(1) << 31;
  if (m < 0 || m >= lim || n < 0 || n >= lim || q < 1 || q >= INT32_MAX) {
    throw std::runtime_error("cglsWorkBytes: m = " + std::to_string(m) + ", n = " + std::to_string(n) + ", q = " +
                             std::to_string(q) + " is outside [0, 2^31) x [0, 2^31) x [1, 2^31 - 1)");
  }
  return BaSpaCho::cglsWorkBytes(m, n, q);
}

template <typename T>
void Solver::cgls(const CglsArgs<T>& a, int64_t batch, bool single) const {
  static const char* names[10] = {"cglsJv",    "cglsJtv",    "cglsColSq", "cglsDamp",  "cglsInit",
                                  "cglsDelta", "cglsUpdate", "cglsApply", "cglsBuild", "cglsIterate"};
  if (a.op < 0 || a.op > CglsIterate) throw std::runtime_error("cgls: unknown operation " + std::to_string(a.op));
  const std::string what = names[a.op];
  const auto fail = [&](const std::string& m) { throw std::runtime_error(what + ": " + m); };
  if (a.map == nullptr) fail("the map is NULL");
  if (a.map->solver != this) fail("the map was built on another solver");
  if (batch < 1) fail("the batch is empty");
  const std::string fault = badVectorCount(a.q);
  if (!fault.empty()) fail(fault);
  const int64_t m = a.map->m, n = a.map->n, q = a.q;
  if ((m + n) * q >= (int64_t(1) << 40) || ((m + 1023) / 1024 + (n + 1023) / 1024) * q >= INT32_MAX) {
    fail("(m + n) q = " + std::to_string((m + n) * q) + " is too large");
  }
  const bool product = a.op == CglsJv || a.op == CglsJtv;
  const bool builtIn = a.kind == CgJacobi || a.kind == CgBlockJacobi;
  if (product && a.epi != 0 && a.epi != (a.op == CglsJv ? 1 : 2)) {
    fail("epilogue " + std::to_string(a.epi) + " (0: none, 1: residual, of J v; 2: normal, of J^T u)");
  }
  if (a.op == CglsIterate && (a.phase < 0 || a.phase > 2)) {
    fail("phase " + std::to_string(a.phase) + " (0: the whole iteration, 1: up to s, 2: apply and direction)");
  }
  if (((a.op == CglsApply || a.op == CglsIterate) && !builtIn && a.kind != CgGiven) || (a.op == CglsBuild && !builtIn)) {
    fail("unknown preconditioner kind " + std::to_string(a.kind) + " (0: the caller's z, 1: jacobi, 2: block_jacobi)");
  }
  if (a.op == CglsInit) {
    if (!(a.tol >= 0.0)) fail("tol = " + std::to_string(a.tol) + "; it must be >= 0");
    if (a.maxSteps < 0) fail("max_steps = " + std::to_string(a.maxSteps) + "; it must be >= 0");
  }
  const bool usesWork = a.op >= CglsInit && a.op != CglsUpdate;
  if (usesWork) {
    if (a.work == nullptr) fail("the workspace pointer is NULL");
    if (reinterpret_cast<uintptr_t>(a.work) % 16 != 0) fail("the workspace is not 16-byte aligned");
  }
  if (a.op == CglsBuild && a.status == nullptr) fail("the status pointer is NULL");
  if (((a.op >= CglsInit && a.op <= CglsApply) || a.op == CglsIterate) && a.state == nullptr) {
    fail("the state pointer is NULL");
  }
  // the operands the piece needs: (name, pointers, elements)
  struct Slot {
    const char* name;
    const void* const* ptrs;
    int64_t elems;
    bool optional;
  };
  const auto p = [](auto ptrs) { return reinterpret_cast<const void* const*>(ptrs); };
  const int64_t nq = n * q, mq = m * q, nnz = a.map->nnz;
  const int64_t invElems = a.kind == CgBlockJacobi && (a.op == CglsApply || a.op == CglsBuild || a.op == CglsIterate)
                               ? jacBlockPlan(*a.map).inverseElems()
                               : n;
  std::vector<Slot> slots;
  switch (a.op) {
    case CglsJv:
      slots = {{"values", p(a.values), nnz, false}, {"vector", p(a.vec), nq, false}, {"r", p(a.addend), mq, true},
               {"output", p(a.out), mq, false}};
      break;
    case CglsJtv:
      slots = {{"values", p(a.values), nnz, false}, {"vector", p(a.vec), mq, false}, {"c", p(a.addend), nq, true},
               {"d", p(a.damp), n, true}, {"x", p(a.x), nq, a.damp == nullptr}, {"output", p(a.out), nq, false}};
      break;
    case CglsColSq: slots = {{"values", p(a.values), nnz, false}, {"colsq", p(a.colsq), n, false}}; break;
    case CglsDamp: slots = {{"colsq", p(a.colsq), n, false}, {"d", p(a.out), n, false}}; break;
    case CglsInit: slots = {{"b", p(a.vec), nq, false}, {"x", p(a.x), nq, false}}; break;
    case CglsDelta: slots = {{"t", p(a.vec), mq, false}, {"p", p(a.x), nq, false}, {"d", p(a.damp), n, true}}; break;
    case CglsUpdate:
      slots = {{"p", p(a.vec), nq, false}, {"t", p(a.addend), mq, false}, {"x", p(a.x), nq, false},
               {"res", p(a.out), mq, false}};
      break;
    case CglsApply:
      slots = {{"preconditioner", p(a.damp), invElems, !builtIn}, {"s", p(a.vec), nq, false}, {"z", p(a.out), nq, false}};
      break;
    case CglsIterate: {
      const bool head = a.phase != 2, tail = a.phase != 1;
      slots = {{"p", p(a.p), nq, false}};
      if (head) {
        slots.insert(slots.end(), {{"values", p(a.values), nnz, false}, {"t", p(a.t), mq, false}, {"d", p(a.damp), n, true},
                                   {"x", p(a.x), nq, false}, {"res", p(a.res), mq, false}, {"c", p(a.addend), nq, true},
                                   {"s", p(a.s), nq, false}});
      }
      if (tail) {
        slots.insert(slots.end(), {{"preconditioner", p(a.minv), invElems, !builtIn}, {"s", p(a.s), nq, false},
                                   {"z", p(a.z), nq, false}});
      }
      break;
    }
    default:
      slots = {{"values", p(a.values), nnz, a.kind == CgJacobi}, {"colsq", p(a.colsq), n, a.kind != CgJacobi},
               {"d", p(a.damp), n, true}, {"preconditioner", p(a.out), invElems, false}};
      break;
  }
  for (const Slot& s : slots) {
    if (s.ptrs == nullptr) {  // (an operand without elements may be NULL altogether)
      if (!s.optional && s.elems > 0) fail(std::string("the ") + s.name + " pointers are NULL");
      continue;
    }
    for (int64_t b = 0; b < batch; b++) {
      if (s.ptrs[b] == nullptr && s.elems > 0) {
        fail(std::string("the ") + s.name + " pointer of batch member " + std::to_string(b) + " is NULL");
      }
    }
  }
  hipBackendCgls<T>(*symCtx, a, batch, single);
}

// ---- implicit Schur elimination of the matrix-free least squares --------------
template <typename T>
void Solver::jacSchur(const JacSchurArgs<T>& a, int64_t batch, bool single) const {
  static const char* names[8] = {"schurBuild",        "schurMv",           "schurReduce",      "schurBack",
                                 "schurPrecondBuild", "schurPrecondApply", "schurJacobiBuild", "schurJacobiApply"};
  if (a.op < 0 || a.op > SchurSJacobiApply) throw std::runtime_error("jacobian schur: unknown operation " + std::to_string(a.op));
  const std::string what = names[a.op];
  const auto fail = [&](const std::string& m) { throw std::runtime_error(what + ": " + m); };
  if (a.map == nullptr) fail("the map is NULL");
  if (a.map->product->solver != this) fail("the map was built on another solver");
  if (batch < 1) fail("the batch is empty");
  const std::string fault = badVectorCount(a.q);
  if (!fault.empty()) fail(fault);
  const int64_t m = a.map->m, n = a.map->n, nK = a.map->nK, q = a.q;
  if ((m + n) * q >= (int64_t(1) << 40)) fail("(m + n) q = " + std::to_string((m + n) * q) + " is too large");
  const bool precond = a.op == SchurPrecondBuild || a.op == SchurPrecondApply;
  const bool sjacobi = a.op == SchurSJacobiBuild || a.op == SchurSJacobiApply;
  const bool applies = a.op == SchurPrecondApply || a.op == SchurSJacobiApply;
  if (precond && a.kind != CgJacobi && a.kind != CgBlockJacobi) {
    fail("unknown preconditioner kind " + std::to_string(a.kind) + " (1: jacobi, 2: block_jacobi)");
  }
  if (a.op == SchurBuild || precond || sjacobi) {
    if (a.work == nullptr) fail("the workspace pointer is NULL");
    if (reinterpret_cast<uintptr_t>(a.work) % 16 != 0) fail("the workspace is not 16-byte aligned");
    if (!applies && a.status == nullptr) fail("the status pointer is NULL");
    if (applies && a.state == nullptr) fail("the state pointer is NULL");
  }
  const int64_t pinv = sjacobi   ? jacSchurJacobiPlan(*a.map).inverseElems()
                       : !precond ? 0
                       : a.kind == CgBlockJacobi ? jacSchurKeptPlan(*a.map).inverseElems()
                                                 : nK;
  struct Slot {
    const char* name;
    const void* const* ptrs;
    int64_t elems;
    bool optional;
  };
  const auto p = [](auto ptrs) { return reinterpret_cast<const void* const*>(ptrs); };
  const int64_t inv = a.map->elimBlocks->inverseElems(), nnz = a.map->nnz;
  std::vector<Slot> slots;
  switch (a.op) {
    case SchurBuild:
      slots = {{"values", p(a.values), nnz, false}, {"d", p(a.damp), n, true}, {"inverses", p(a.out), inv, false}};
      break;
    case SchurMv:
      slots = {{"values", p(a.values), nnz, false}, {"inverses", p(a.binv), inv, false}, {"d", p(a.damp), n, true},
               {"p", p(a.vec), nK * q, false},      {"t", p(a.t), m * q, false},         {"output", p(a.out), nK * q, false}};
      break;
    case SchurReduce:
      slots = {{"values", p(a.values), nnz, false}, {"inverses", p(a.binv), inv, false}, {"g", p(a.full), n * q, false},
               {"t", p(a.t), m * q, false},         {"output", p(a.out), nK * q, false}};
      break;
    case SchurBack:
      slots = {{"values", p(a.values), nnz, false}, {"inverses", p(a.binv), inv, false}, {"g", p(a.full), n * q, false},
               {"x_k", p(a.vec), nK * q, false},    {"t", p(a.t), m * q, false},         {"output", p(a.out), n * q, false}};
      break;
    case SchurPrecondBuild:
      slots = {{"values", p(a.values), nnz, a.kind == CgJacobi}, {"colsq", p(a.colsq), n, a.kind != CgJacobi},
               {"d", p(a.damp), n, true}, {"preconditioner", p(a.out), pinv, false}};
      break;
    case SchurSJacobiBuild:
      slots = {{"values", p(a.values), nnz, false},
               {"inverses", p(a.binv), inv, false},
               {"d", p(a.damp), n, true},
               {"partials", p(a.partials), jacSchurJacobiPlan(*a.map).partialElems(), false},
               {"preconditioner", p(a.out), pinv, false}};
      break;
    default:
      slots = {{"preconditioner", p(a.binv), pinv, false}, {"r", p(a.vec), nK * q, false}, {"z", p(a.out), nK * q, false}};
      break;
  }
  for (const Slot& s : slots) {
    if (s.ptrs == nullptr) {  // (an operand without elements may be NULL altogether)
      if (!s.optional && s.elems > 0) fail(std::string("the ") + s.name + " pointers are NULL");
      continue;
    }
    for (int64_t b = 0; b < batch; b++) {
      if (s.ptrs[b] == nullptr && s.elems > 0) {
        fail(std::string("the ") + s.name + " pointer of batch member " + std::to_string(b) + " is NULL");
      }
    }
  }
  hipBackendJacSchur<T>(*symCtx, a, batch, single);
}

// ---- the Lanczos recurrence ---------------------------------------------------
static void checkLanczosSizes(const std::string& what, int64_t n, int64_t q, int64_t kmax) {
  const auto fail = [&](const std::string& m) { throw std::runtime_error(what + ": " + m); };
  if (n < 0 || n >= (int64_t(1) << 31)) fail("n = " + std::to_string(n) + " is outside [0, 2^31)");
  if (q < 1 || q >= INT32_MAX) fail("q = " + std::to_string(q) + " is outside [1, 2^31 - 1)");
  if (kmax < 1 || kmax > (int64_t(1) << 20)) fail("kmax = " + std::to_string(kmax) + " is outside [1, 2^20]");
  const int64_t parts = (n + 1023) / 1024;
  if (n * q >= (int64_t(1) << 40) || parts * q >= INT32_MAX || kmax * q >= INT32_MAX ||
      (parts > 0 ? parts : 1) * q * kmax >= (int64_t(1) << 40)) {
    fail("n q = " + std::to_string(n * q) + " with kmax = " + std::to_string(kmax) + " is too large");
  }
}

int64_t Solver::lanczosWorkBytes(int64_t n, int64_t q, int64_t kmax) const {
  checkLanczosSizes("lanczosWorkBytes", n, q, kmax);
  return BaSpaCho::lanczosWorkBytes(n, q, kmax);
}

template <typename T>
void Solver::lanczos(const LanczosArgs<T>& a, int64_t batch, bool single) const {
  static const char* names[6] = {"lanczosInit",    "lanczosAlpha",    "lanczosUpdate",
                                 "lanczosProject", "lanczosSubtract", "lanczosNormalize"};
  if (a.op < 0 || a.op > LzNormalize) throw std::runtime_error("lanczos: unknown operation " + std::to_string(a.op));
  const std::string what = names[a.op];
  const auto fail = [&](const std::string& m) { throw std::runtime_error(what + ": " + m); };
  if (batch < 1) fail("the batch is empty");
  checkLanczosSizes(what, a.n, a.q, a.kmax);
  const int64_t nq = a.n * a.q;
  if (a.slots < 1) fail("slots = " + std::to_string(a.slots) + "; the basis needs at least one slot");
  if (a.slotStride < nq) {
    fail("the slot stride " + std::to_string(a.slotStride) + " is below n q = " + std::to_string(nq));
  }
  const auto checkSlot = [&](const char* name, int64_t s) {
    if (s < 0 || s >= a.slots) {
      fail(std::string("the ") + name + " slot " + std::to_string(s) + " is outside the basis of " +
           std::to_string(a.slots) + " slots");
    }
  };
  if (a.op == LzProject || a.op == LzSubtract) {
    if (a.count < 1 || a.count > a.slots || a.count > a.kmax) {
      fail("count = " + std::to_string(a.count) + " is outside [1, min(slots, kmax)] = [1, " +
           std::to_string(std::min(a.slots, a.kmax)) + "]");
    }
  } else {
    checkSlot(a.op == LzInit || a.op == LzNormalize ? "output" : "current", a.slot);
    if (a.op == LzUpdate) checkSlot("previous", a.prev);
  }
  if (a.op == LzInit && !(a.breakdown >= 0.0)) {
    fail("breakdown = " + std::to_string(a.breakdown) + "; it must be >= 0");
  }
  if (a.work == nullptr) fail("the workspace pointer is NULL");
  if (reinterpret_cast<uintptr_t>(a.work) % 16 != 0) fail("the workspace is not 16-byte aligned");
  if (a.state == nullptr) fail("the state pointer is NULL");
  const bool folds = (a.op == LzUpdate || a.op == LzSubtract) && a.fold;
  if (folds && a.coef == nullptr) fail("the coefficient pointer is NULL");
  const char* vecName = a.op == LzInit ? "start vector" : "w";
  if (a.vec == nullptr) fail(std::string("the ") + vecName + " pointers are NULL");
  if (a.basis == nullptr) fail("the basis pointers are NULL");
  for (int64_t m = 0; m < batch; m++) {
    if (nq > 0 && a.vec[m] == nullptr) {
      fail(std::string("the ") + vecName + " pointer of batch member " + std::to_string(m) + " is NULL");
    }
    if (nq > 0 && a.basis[m] == nullptr) fail("the basis pointer of batch member " + std::to_string(m) + " is NULL");
  }
  hipBackendLanczos<T>(*symCtx, a, batch, single);
}

// ---- combinations of basis vectors ---------------------------------------------
template <typename T>
void Solver::krylovCombine(const KrylovCombineArgs<T>& a, int64_t batch, bool single) const {
  const std::string what = "krylovCombine";
  const auto fail = [&](const std::string& m) { throw std::runtime_error(what + ": " + m); };
  if (batch < 1) fail("the batch is empty");
  checkLanczosSizes(what, a.n, a.q, 1);
  if (a.nf < 1 || a.nf > 4) fail("nf = " + std::to_string(a.nf) + " is outside [1, 4]");
  const int64_t nq = a.n * a.q;
  if (a.count < 1) fail("count = " + std::to_string(a.count) + "; a call combines at least one slot");
  if (a.first < 0) fail("first = " + std::to_string(a.first) + " is negative");
  if (a.slot < 0) fail("slot = " + std::to_string(a.slot) + " is negative");
  if (a.slots < 1 || a.count > a.slots || a.slot > a.slots - a.count) {
    fail("the slots " + std::to_string(a.slot) + " .. " + std::to_string(a.slot) + " + " + std::to_string(a.count) +
         " - 1 are outside the basis of " + std::to_string(a.slots) + " slots");
  }
  if (a.count >= INT32_MAX) fail("count = " + std::to_string(a.count) + " is too large");
  if (a.slotStride < nq) {
    fail("the slot stride " + std::to_string(a.slotStride) + " is below n q = " + std::to_string(nq));
  }
  if (a.outStride < nq) {
    fail("the output stride " + std::to_string(a.outStride) + " is below n q = " + std::to_string(nq));
  }
  if (a.ldy < a.count) fail("ldy = " + std::to_string(a.ldy) + " is below count = " + std::to_string(a.count));
  if (a.y == nullptr) fail("the coefficient pointer is NULL");
  if (a.limit == nullptr) fail("the limit pointer is NULL");
  if (a.basis == nullptr) fail("the basis pointers are NULL");
  if (a.out == nullptr) fail("the output pointers are NULL");
  for (int64_t m = 0; m < batch; m++) {
    if (nq > 0 && a.basis[m] == nullptr) fail("the basis pointer of batch member " + std::to_string(m) + " is NULL");
    if (nq > 0 && a.out[m] == nullptr) fail("the output pointer of batch member " + std::to_string(m) + " is NULL");
  }
  if (a.n == 0) return;
  hipBackendKrylovCombine<T>(*symCtx, a, batch, single);
}

// ---- blocks of A^-1 by reach solves (reach.h) --------------------------------
ReachPlan Solver::reachPlan(const char* what, const std::vector<int64_t>& params, const std::vector<int64_t>& pairRow,
                            const std::vector<int64_t>& pairCol, const std::vector<int64_t>& outOffsets) const {
  checkCompleteFactor(what, canFactorUpTo, factorSkel.numSpans(), "a reach solve");
  const int64_t numParams = (int64_t)permutation.size();
  std::vector<int64_t> spans;
  for (size_t i = 0; i < params.size(); i++) {
    if (params[i] < 0 || params[i] >= numParams) {
      throw std::runtime_error(std::string(what) + ": param " + std::to_string(params[i]) + " (position " +
                               std::to_string(i) + ") is not in [0, " + std::to_string(numParams) + ")");
    }
    spans.push_back(permutation[params[i]]);
  }
  try {
    return buildReachPlan(factorSkel, sparseElimRanges, spans, pairRow, pairCol, outOffsets);
  } catch (const std::runtime_error& e) {
    throw std::runtime_error(std::string(what) + ": " + e.what());
  }
}

// W <- L^-1 E for the plan's queries: the reach kernel below the cut, solveLFrom behind it
template <typename T>
static void runReachSolve(const Solver& s, SymbolicCtx& sym, const ReachPlan& plan, const T* L, T* W) {
  hipBackendReachSolveL<T>(sym, plan, L, W);
  if (plan.numCols > 0 && plan.cutLump < s.skel().numLumps()) {
    s.solveLFrom(L, plan.cutSpan, W, s.order(), (int)plan.numCols);
  }
}

template <typename T>
void Solver::reachSolveL(const T* L, const std::vector<int64_t>& params, T* W) const {
  const char* what = "reachSolveL";
  if (L == nullptr) throw std::runtime_error("reachSolveL: the factor pointer is NULL");
  if (W == nullptr) throw std::runtime_error("reachSolveL: the output pointer is NULL");
  const ReachPlan plan = reachPlan(what, params, {}, {});
  runReachSolve(*this, *symCtx, plan, L, W);
}

template <typename T>
void Solver::inverseBlocks(const T* L, const std::vector<int64_t>& rowParams, const std::vector<int64_t>& colParams,
                           T* out, const std::vector<int64_t>& outOffsets) const {
  const char* what = "inverseBlocks";
  if (L == nullptr) throw std::runtime_error("inverseBlocks: the factor pointer is NULL");
  if (out == nullptr) throw std::runtime_error("inverseBlocks: the output pointer is NULL");
  if (rowParams.size() != colParams.size()) {
    throw std::runtime_error("inverseBlocks: " + std::to_string(rowParams.size()) + " row params for " +
                             std::to_string(colParams.size()) + " column params");
  }
  if (outOffsets.size() != rowParams.size() + 1) {
    throw std::runtime_error("inverseBlocks: the output offsets must hold numPairs + 1 entries");
  }
  for (size_t k = 0; k < rowParams.size(); k++) {
    if (outOffsets[k] < 0 || outOffsets[k + 1] < outOffsets[k]) {
      throw std::runtime_error("inverseBlocks: the output offsets must be non-negative and ascending");
    }
  }
  // the distinct params, in the order of their first appearance
  std::vector<int64_t> params, pairRow, pairCol;
  std::unordered_map<int64_t, int64_t> index;
  const auto indexOf = [&](int64_t prm) {
    auto it = index.find(prm);
    if (it == index.end()) {
      it = index.emplace(prm, (int64_t)params.size()).first;
      params.push_back(prm);
    }
    return it->second;
  };
  for (size_t k = 0; k < rowParams.size(); k++) {
    pairRow.push_back(indexOf(rowParams[k]));
    pairCol.push_back(indexOf(colParams[k]));
  }
  const ReachPlan plan = reachPlan(what, params, pairRow, pairCol, outOffsets);
  if (plan.items.empty()) return;
  T* W = hipBackendReachWorkspace<T>(*symCtx, plan.numCols * order());
  runReachSolve(*this, *symCtx, plan, L, W);
  hipBackendGramBlocks<T>(*symCtx, plan, W, out);
}

// ---- products with the factor ------------------------------------------------
template <typename T>
static void runFactorProduct(const Solver& s, SymbolicCtx& sym, bool single, const char* what, bool transposed,
                             const std::vector<T*>& L, const std::vector<T*>& x, int64_t inStride,
                             const std::vector<T*>& y, int64_t outStride, int nRHS) {
  if (y.empty()) throw std::runtime_error(std::string(what) + ": the batch is empty");
  checkMembers(what, "output", y, y.size());
  checkMembers(what, "input", x, y.size());
  checkMembers(what, "factor", L, y.size());
  if (nRHS < 1) throw std::runtime_error(std::string(what) + ": nRHS = " + std::to_string(nRHS) + " < 1");
  if (nRHS > 65535) throw std::runtime_error(std::string(what) + ": nRHS = " + std::to_string(nRHS) + " > 65535");
  if (inStride < s.order() || outStride < s.order()) {
    throw std::runtime_error(std::string(what) + ": stride " + std::to_string(std::min(inStride, outStride)) +
                             " < order " + std::to_string(s.order()));
  }
  const std::vector<const T*> ls = constView(L), xs = constView(x);
  const size_t outBytes = (size_t)(outStride * (nRHS - 1) + s.order()) * sizeof(T);
  checkNoOverlap(what, y, outBytes, xs, (size_t)(inStride * (nRHS - 1) + s.order()) * sizeof(T));
  checkNoOverlap(what, y, outBytes, ls, (size_t)s.dataSize() * sizeof(T));
  hipBackendFactorProduct<T>(sym, ls.data(), transposed, xs.data(), inStride, y.data(), outStride, nRHS,
                             (int64_t)y.size(), single);
}

template <typename T>
void Solver::mulL(const T* L, const T* x, int64_t inStride, T* y, int64_t outStride, int nRHS) const {
  runFactorProduct(*this, *symCtx, true, "mulL", false, one(L), one(x), inStride, one(y), outStride, nRHS);
}
template <typename T>
void Solver::mulL(const std::vector<T*>& L, const std::vector<T*>& x, int64_t inStride, const std::vector<T*>& y,
                  int64_t outStride, int nRHS) const {
  runFactorProduct(*this, *symCtx, false, "mulL", false, L, x, inStride, y, outStride, nRHS);
}
template <typename T>
void Solver::mulLt(const T* L, const T* x, int64_t inStride, T* y, int64_t outStride, int nRHS) const {
  runFactorProduct(*this, *symCtx, true, "mulLt", true, one(L), one(x), inStride, one(y), outStride, nRHS);
}
template <typename T>
void Solver::mulLt(const std::vector<T*>& L, const std::vector<T*>& x, int64_t inStride, const std::vector<T*>& y,
                   int64_t outStride, int nRHS) const {
  runFactorProduct(*this, *symCtx, false, "mulLt", true, L, x, inStride, y, outStride, nRHS);
}

// one single / batch pair per operation
#define BSP_INSTANTIATE_EXTENSIONS(T)                                                                          \
  template void Solver::mulL<T>(const T*, const T*, int64_t, T*, int64_t, int) const;                          \
  template void Solver::mulL<T>(const std::vector<T*>&, const std::vector<T*>&, int64_t,                       \
                                const std::vector<T*>&, int64_t, int) const;                                   \
  template void Solver::mulLt<T>(const T*, const T*, int64_t, T*, int64_t, int) const;                         \
  template void Solver::mulLt<T>(const std::vector<T*>&, const std::vector<T*>&, int64_t,                      \
                                 const std::vector<T*>&, int64_t, int) const;                                  \
  using BspVec_##T = const std::vector<T*>&;                                                                   \
  using BspCVec_##T = const std::vector<const T*>&;                                                            \
  template void Solver::selectedInverse<T>(T*) const;                                                          \
  template void Solver::selectedInverse<std::vector<T*>>(std::vector<T*>*) const;                              \
  template void Solver::logDet<T>(const T*, T*) const;                                                         \
  template void Solver::logDet<T>(BspVec_##T, T*) const;                                                       \
  template void Solver::factorStatus<T>(const T*, int64_t, int64_t, int64_t*) const;                           \
  template void Solver::factorStatus<T>(BspVec_##T, int64_t, int64_t, int64_t*) const;                         \
  template void Solver::dampDiagonal<T>(T*, int64_t, int64_t, const T*) const;                                 \
  template void Solver::dampDiagonal<T>(BspVec_##T, int64_t, int64_t, const T*) const;                         \
  template void Solver::patternGrad<T>(const T*, const T*, const T*, const T*, int64_t, int, T, T*) const;     \
  template void Solver::patternGrad<T>(BspVec_##T, const T*, BspVec_##T, BspVec_##T, int64_t, int, T,          \
                                       BspVec_##T) const;                                                      \
  template void Solver::patternOuter<T>(const T*, const T*, int64_t, int, T, T*) const;                        \
  template void Solver::patternOuter<T>(BspVec_##T, BspVec_##T, int64_t, int, T, BspVec_##T) const;            \
  template void Solver::factorAdjoint<T>(const T*, T*) const;                                                  \
  template void Solver::factorAdjoint<T>(BspVec_##T, BspVec_##T) const;                                        \
  template void Solver::selectedInverseAdjoint<T>(const T*, const T*, T*) const;                               \
  template void Solver::selectedInverseAdjoint<T>(BspVec_##T, BspVec_##T, BspVec_##T) const;                   \
  template void Solver::factorAdjointUpTo<T>(const T*, T*, int64_t) const;                                     \
  template void Solver::factorAdjointUpTo<T>(BspVec_##T, BspVec_##T, int64_t) const;                           \
  template void Solver::schurComplement<T>(const T*, int64_t, T*, const int32_t*) const;                       \
  template void Solver::schurComplement<T>(BspVec_##T, int64_t, BspVec_##T, const int32_t*) const;             \
  template void Solver::schurComplementAdjoint<T>(const T*, int64_t, T*, const int32_t*) const;                \
  template void Solver::schurComplementAdjoint<T>(BspVec_##T, int64_t, BspVec_##T, const int32_t*) const;      \
  template void Solver::assemble<T>(const AssemblyMap&, const T*, T*) const;                                   \
  template void Solver::assemble<T>(const AssemblyMap&, BspCVec_##T, BspVec_##T) const;                        \
  template void Solver::assembleAdjoint<T>(const AssemblyMap&, const T*, T*) const;                            \
  template void Solver::assembleAdjoint<T>(const AssemblyMap&, BspCVec_##T, BspVec_##T) const;                 \
  template void Solver::symProduct<T>(const SymProductMap&, int32_t, BspCVec_##T, BspCVec_##T, BspVec_##T,     \
                                      int64_t, bool) const;                                                    \
  template void Solver::normalEq<T>(const NormalEqMap&, int32_t, BspCVec_##T, BspCVec_##T, BspVec_##T,         \
                                    int64_t, bool) const;                                                      \
  template void Solver::symResidual<T>(const SymProductMap&, BspCVec_##T, BspCVec_##T, BspCVec_##T, BspVec_##T, \
                                       BspVec_##T, int64_t, bool) const;                                       \
  template void Solver::colMax<T>(BspCVec_##T, BspCVec_##T, int64_t, int64_t, double*, bool) const;            \
  template int64_t Solver::invNorm1WorkBytes<T>() const;                                                       \
  template void Solver::invNorm1Estimate<T>(BspCVec_##T, BspCVec_##T, void*, int64_t*, double*, bool) const;   \
  template void Solver::cg<T>(const CgArgs<T>&, int64_t, bool) const;                                          \
  template void Solver::cgls<T>(const CglsArgs<T>&, int64_t, bool) const;                                      \
  template void Solver::jacSchur<T>(const JacSchurArgs<T>&, int64_t, bool) const;                              \
  template void Solver::lanczos<T>(const LanczosArgs<T>&, int64_t, bool) const;                                \
  template void Solver::krylovCombine<T>(const KrylovCombineArgs<T>&, int64_t, bool) const;                    \
  template void Solver::reachSolveL<T>(const T*, const std::vector<int64_t>&, T*) const;                       \
  template void Solver::inverseBlocks<T>(const T*, const std::vector<int64_t>&, const std::vector<int64_t>&,   \
                                         T*, const std::vector<int64_t>&) const;
BSP_INSTANTIATE_EXTENSIONS(double)
BSP_INSTANTIATE_EXTENSIONS(float)
#undef BSP_INSTANTIATE_EXTENSIONS

#define BSP_INSTANTIATE(T)                                                                     \
  template void Solver::factor<T>(T*, bool) const;                                             \
  template void Solver::factorUpTo<T>(T*, int64_t, bool) const;                                \
  template void Solver::factorFrom<T>(T*, int64_t, bool) const;                                \
  template void Solver::solve<T>(const T*, T*, int64_t, int) const;                            \
  template void Solver::solveL<T>(const T*, T*, int64_t, int) const;                           \
  template void Solver::solveLt<T>(const T*, T*, int64_t, int) const;                          \
  template void Solver::solveLUpTo<T>(const T*, int64_t, T*, int64_t, int) const;              \
  template void Solver::solveLtUpTo<T>(const T*, int64_t, T*, int64_t, int) const;             \
  template void Solver::solveLFrom<T>(const T*, int64_t, T*, int64_t, int) const;              \
  template void Solver::solveLtFrom<T>(const T*, int64_t, T*, int64_t, int) const;

BSP_INSTANTIATE(double)
BSP_INSTANTIATE(float)
BSP_INSTANTIATE(std::vector<double*>)
BSP_INSTANTIATE(std::vector<float*>)
#undef BSP_INSTANTIATE

static OpsPtr getBackend(const Settings& settings, const HipBackendOptions& options) {
  if (settings.backend == BackendHip || settings.backend == BackendCuda) return hipOps(&options);
  throw std::runtime_error(
      "baspacho_amd: only the MI355X HIP backend (BackendHip, alias BackendCuda) is part of "
      "this build; the CPU restatement lives under oracle/ as test infrastructure");
}

SolverPtr createSolver(const Settings& settings, const vector<int64_t>& paramSize,
                       const SparseStructure& ssIn, const vector<int64_t>& sparseElimRanges,
                       const std::unordered_set<int64_t>& elimLastIds) {
  BASPACHO_CHECK(settings.addFillPolicy == AddFillComplete || elimLastIds.empty());
  BASPACHO_CHECK((int64_t)sparseElimRanges.size() != 1);
  BASPACHO_CHECK_EQ((int64_t)paramSize.size(), ssIn.order());
  // the backend's switches: the caller's, then the environment on top (A/B scripts), resolved once
  HipBackendOptions options = settings.hipOptions ? *settings.hipOptions : HipBackendOptions();
  options.applyEnv();
  const int64_t nParams = (int64_t)paramSize.size();
  const int64_t givenElimEnd = sparseElimRanges.empty() ? 0 : sparseElimRanges.back();
  if (!sparseElimRanges.empty()) {
    BASPACHO_CHECK(isStrictlyIncreasing(sparseElimRanges, 0, sparseElimRanges.size()));
    BASPACHO_CHECK_LE(givenElimEnd, nParams);
    for (int64_t id : elimLastIds) BASPACHO_CHECK_GE(id, givenElimEnd);
  }

  // fill created by the user-given (un-reordered) elimination ranges
  SparseStructure ss = ssIn;
  if (settings.addFillPolicy != AddFillNone) {
    for (size_t e = 0; e + 1 < sparseElimRanges.size(); e++) {
      ss = ss.addIndependentEliminationFill(sparseElimRanges[e], sparseElimRanges[e + 1]);
    }
  }

  if (settings.addFillPolicy == AddFillNone || settings.addFillPolicy == AddFillForGivenElims) {
    // identity ordering, one lump per parameter
    vector<int64_t> spanStart(paramSize.begin(), paramSize.end());
    spanStart.push_back(0);
    cumSumVec(spanStart);
    vector<int64_t> lumpToSpan(nParams + 1), identity(nParams);
    std::iota(lumpToSpan.begin(), lumpToSpan.end(), 0);
    std::iota(identity.begin(), identity.end(), 0);
    SparseStructure cols = ss.transpose();
    CoalescedBlockMatrixSkel skel(spanStart, lumpToSpan, cols.ptrs, cols.inds);
    vector<int64_t> ranges = sparseElimRanges;
    return SolverPtr(new Solver(std::move(skel), std::move(ranges), std::move(identity),
                                getBackend(settings, options),
                                settings.addFillPolicy == AddFillNone ? 0 : givenElimEnd));
  }

  const bool timing = std::getenv("BSP_TIMING") != nullptr;
  auto tic = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) {
    if (!timing) return;
    auto now = std::chrono::steady_clock::now();
    std::cerr << "[createSolver] " << what << ": "
              << std::chrono::duration<double>(now - tic).count() << " s" << std::endl;
    tic = now;
  };

  // fill-reducing ordering of what is left after the given eliminations
  SparseStructure bottom = ss.extractRightBottom(givenElimEnd);
  lap("elim fill + extract");
  vector<int64_t> perm = bottom.fillReducingPermutation(HipBackendOptions::on(options.chainContraction, true));
  lap("min-degree ordering");
  vector<int64_t> noCrossPoints;
  if (!elimLastIds.empty()) {  // stable partition: "last" ids go to the end
    vector<int64_t> head, tail;
    for (int64_t p : perm) (elimLastIds.count(p + givenElimEnd) ? tail : head).push_back(p);
    noCrossPoints.push_back((int64_t)head.size());
    perm = head;
    perm.insert(perm.end(), tail.begin(), tail.end());
  }
  vector<int64_t> invPerm = inversePermutation(perm);
  SparseStructure sortedBottom = bottom.symmetricPermutation(invPerm, false);

  const int64_t nBottom = nParams - givenElimEnd;
  vector<int64_t> sortedBottomSize(nBottom);
  for (int64_t i = 0; i < nBottom; i++) sortedBottomSize[invPerm[i]] = paramSize[givenElimEnd + i];

  // EXPLICIT merge model of the level-scheduled backend (round 6): time = levels on the critical path x
  // levelCost + batch x (throughput terms of the ops).  A level runs the ops of all its lumps -- and of
  // all matrices of a batch -- in one launch, so an op's own fixed cost is not paid per lump (the
  // built-in model carries none) and what a merge adds in fill is paid once per matrix of the batch,
  // while the levels it saves (elimination_tree.cpp, computeMerges) are saved once per CALL: a batch of
  // 64 wants fewer merges than a single matrix.  expectedBatch scales every coefficient; a caller's own
  // model is taken as it is (its constants included) and scaled the same way.
  ComputationModel adjusted =
      settings.computationModel ? *settings.computationModel : ComputationModel::model_Hip_MI355X;
  {
    const double bs = double(std::max(1, options.expectedBatch));
    for (double& v : adjusted.potrfParams) v *= bs;
    for (double& v : adjusted.trsmParams) v *= bs;
    for (double& v : adjusted.sygeParams) v *= bs;
    for (double& v : adjusted.asmblParams) v *= bs;
  }
  const ComputationModel* model = &adjusted;

  EliminationTree et(sortedBottomSize, sortedBottom, model);
  et.denseMergeRule = HipBackendOptions::on(options.denseMerge, true);
  et.expectedBatch = std::max(1, options.expectedBatch);
  if (!std::isnan(options.levelCostUs)) et.levelCost = 1e-6 * options.levelCostUs;
  et.buildTree();
  lap("etree build");
  et.processTree(settings.findSparseEliminationRanges, noCrossPoints,
                 settings.addFillPolicy == AddFillForAutoElims);
  lap("etree process (ranges + merges)");
  et.computeAggregateStruct(settings.addFillPolicy == AddFillForAutoElims);
  lap("aggregate structure");

  // total ordering: identity on the given-elimination prefix, (etree o AMD) on the rest
  vector<int64_t> bottomInvPerm = composePermutations(et.permInverse, invPerm);
  vector<int64_t> fullInvPerm(nParams);
  std::iota(fullInvPerm.begin(), fullInvPerm.begin() + givenElimEnd, 0);
  for (int64_t i = 0; i < nBottom; i++) fullInvPerm[givenElimEnd + i] = givenElimEnd + bottomInvPerm[i];

  vector<int64_t> fullSpanStart(nParams + 1, 0);
  leftPermute(fullSpanStart.begin(), fullInvPerm, paramSize);
  cumSumVec(fullSpanStart);

  vector<int64_t> fullLumpToSpan(givenElimEnd);
  std::iota(fullLumpToSpan.begin(), fullLumpToSpan.end(), 0);
  shiftConcat(fullLumpToSpan, givenElimEnd, et.lumpToSpan.begin(), et.lumpToSpan.end());
  BASPACHO_CHECK_EQ((int64_t)fullSpanStart.size() - 1, fullLumpToSpan.back());

  // the first columns (given eliminations) come from the un-merged permuted structure
  SparseStructure sortedCols = ss.symmetricPermutation(fullInvPerm, false).transpose();
  const int64_t prefixEntries = sortedCols.ptrs[givenElimEnd];
  vector<int64_t> fullColStart(sortedCols.ptrs.begin(), sortedCols.ptrs.begin() + givenElimEnd);
  shiftConcat(fullColStart, prefixEntries, et.colStart.begin(), et.colStart.end());
  BASPACHO_CHECK_EQ(fullColStart.size(), fullLumpToSpan.size());
  vector<int64_t> fullRowParam(sortedCols.inds.begin(), sortedCols.inds.begin() + prefixEntries);
  shiftConcat(fullRowParam, givenElimEnd, et.rowParam.begin(), et.rowParam.end());
  BASPACHO_CHECK_EQ((int64_t)fullRowParam.size(), fullColStart.back());

  CoalescedBlockMatrixSkel skel(fullSpanStart, fullLumpToSpan, fullColStart, fullRowParam);
  lap("skeleton");

  // given ranges followed by the automatically detected ones (shifted past the prefix)
  vector<int64_t> fullRanges = sparseElimRanges;
  if (!et.sparseElimRanges.empty()) {
    shiftConcat(fullRanges, givenElimEnd,
                et.sparseElimRanges.begin() + (sparseElimRanges.empty() ? 0 : 1),
                et.sparseElimRanges.end());
  }
  if (fullRanges.size() == 1) fullRanges.clear();
  const int64_t fullElimEnd = fullRanges.empty() ? 0 : fullRanges.back();

  return SolverPtr(new Solver(std::move(skel), std::move(fullRanges), std::move(fullInvPerm),
                              getBackend(settings, options),
                              settings.addFillPolicy == AddFillForAutoElims ? fullElimEnd : nParams));
}

}  // namespace BaSpaCho
