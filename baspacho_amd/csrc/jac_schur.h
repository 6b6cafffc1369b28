// Implicit Schur elimination on a sparse Jacobian given as entries: the params are split
// into eliminated and kept ones, no Jacobian row touches two eliminated params, and the conjugate gradient runs
// on the reduced system S x_k = b_k, S = C - F^T B^-1 F, of which only the diagonal blocks of B and products
// with vectors are ever formed.  This file is the host map of that elimination over a JacobianProductMap
// (jac_product.h): counting sorts, no device work; the kernels that use it are in hip_schur_kernels.h.
//
// CONVENTIONS.  Those of jac_product.h.  The eliminated params are taken in ascending param index whatever the
// order they were given in; e counts them.  The kept scalars are numbered c = 0 .. nK - 1 in ascending caller's
// scalar (keptScalar[c]; keptIndex is the inverse, -1 for an eliminated scalar), the eliminated ones l = 0 ..
// nE - 1 likewise (elimScalar[l]); param e holds l in [elimOff[e], elimOff[e + 1]), at most kSchurMaxElimWidth.
// Every list holds its entries in ascending entry index k:
//   rowsKept   run i (Jacobian row): the kept entries of the row, idx = the kept index of their column
//   rowsElim   run i: the eliminated entries of the row, idx = the eliminated scalar l of their column
//   colsElim   run l: the entries of eliminated scalar l, idx = their row
//   colsKept   run c: the entries of kept column c, idx = their row
// each with the list of its runs of more than kAssemblyLongRun entries.  Group e is the rows with an entry in
// eliminated param e, ascending: groupRow[groupStart[e] .. groupStart[e + 1]); freeRows are the rows of no
// group, ascending.  elimBlocks is the plan of the diagonal blocks of B = J_e^T J_e + D_e (createJacBlockPlanOn).
// The kept params, ascending: param keptParam[b] holds the caller's scalars [keptFirst[b], keptFirst[b] +
// keptWidth[b]) and the kept indices [keptBlockStart[b], keptBlockStart[b + 1]); keptScalarBlock[c] = b.  The plan of
// the diagonal blocks of C = J_k^T J_k + D_k over them (jacSchurKeptPlan) is built by the first call that asks.
//
// THE BLOCK DIAGONAL OF S (schur_jacobi; built by jac_schur_jacobi.cpp from the lists above,
// never from the kept item plan).  A pair (e, b) exists when a row of group e has an entry in a column of kept
// param b; its rows are those rows, ascending.  The free rows that touch b are cut, ascending, into pieces of at
// most kSchurJacobiChunk rows: pseudo-pairs (pairElim = -1).  The pairs of b -- real ones in ascending e, then the
// pseudo-pairs -- are [blockPair[b], blockPair[b + 1]) and are cut into chunks of at most kSchurJacobiChunk pairs:
// chunk h of block chunkBlock[h] holds the pairs [chunkPair[h], chunkPair[h + 1]) and writes the w_b (w_b + 1) / 2
// lower-triangle elements of its partial sum (element (a, c), a >= c, at a (a + 1) / 2 + c) from chunkPart[h] on;
// the chunks of b are [blockChunk[b], blockChunk[b + 1]).  Pair p has the pair-rows [pairRow[p], pairRow[p + 1]);
// pair-row x of it (Jacobian row rowOf[pairRow[p] + x]) has a record of w_b + w_e entry indices from
// rec[pairRec[p] + x (w_b + w_e)] on: the entry at (row, scalar a of b) for a < w_b, then the entry at (row,
// scalar l of e), or -1 where the row has none (a pseudo-pair: w_e = 0).  blockOff[b]: the first element of the
// inverse of block b, w_b^2 each, from keptWidth alone.
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

#include "jac_product.h"

namespace BaSpaCho {

constexpr int32_t kSchurMaxElimWidth = 8;  // widest eliminated param
constexpr int32_t kSchurJacobiChunk = 64;  // pairs of a chunk, rows of a pseudo-pair (part of the interface)

struct JacSchurJacobiPlan {
  int64_t numBlocks = 0, numReal = 0, numPseudo = 0;
  std::vector<int64_t> blockOff, chunkPart;
  std::vector<int32_t> blockPair, blockChunk, chunkPair, chunkBlock, pairElim, pairRow, pairRec, rec;
  std::vector<int32_t> rowOf;  // (host only: the kernels read the records)
  int64_t numPairs() const { return (int64_t)pairElim.size(); }
  int64_t numPairRows() const { return (int64_t)rowOf.size(); }
  int64_t numChunks() const { return (int64_t)chunkBlock.size(); }
  int64_t inverseElems() const { return blockOff.empty() ? 0 : blockOff.back(); }
  int64_t partialElems() const { return chunkPart.empty() ? 0 : chunkPart.back(); }
  int64_t deviceBytes() const {
    return (int64_t)((blockOff.size() + chunkPart.size()) * sizeof(int64_t) +
                     (blockPair.size() + blockChunk.size() + chunkPair.size() + chunkBlock.size() + pairElim.size() +
                      pairRow.size() + pairRec.size() + rec.size()) *
                         sizeof(int32_t));
  }
};

struct JacSchurMap {
  const JacobianProductMap* product = nullptr;  // not owned; must outlive the map
  int64_t m = 0, n = 0, nnz = 0, nK = 0, nE = 0, numElim = 0, maxElimWidth = 0, maxGroup = 0;
  std::vector<int32_t> elimParam;  // [numElim] the param index of eliminated param e, ascending
  std::vector<int32_t> elimOff;    // [numElim + 1]
  std::vector<int32_t> keptScalar, keptIndex, elimScalar;
  RunList rowsKept, rowsElim, colsElim, colsKept;
  std::vector<int32_t> groupStart, groupRow, freeRows;
  std::unique_ptr<JacBlockPlan> elimBlocks;
  std::vector<int32_t> keptParam, keptFirst, keptWidth, keptBlockStart, keptScalarBlock;
  mutable std::unique_ptr<JacBlockPlan> keptBlocks;
  mutable std::unique_ptr<JacSchurJacobiPlan> schurJacobi;  // built by the first call that asks (jacSchurJacobiPlan)

  mutable HipEntryMapDevPtr dev;

  int64_t deviceBytes() const {
    return rowsKept.deviceBytes() + rowsElim.deviceBytes() + colsElim.deviceBytes() + colsKept.deviceBytes() +
           (int64_t)((elimOff.size() + keptScalar.size() + elimScalar.size() + groupStart.size() + groupRow.size() +
                      freeRows.size()) * sizeof(int32_t));
  }
};

// Builds the map for the eliminated params `eliminate` (indices into the solver's params, any order).  Throws,
// before anything of the size of the entries is allocated, for: an empty list; an index out of range or given
// twice; an eliminated param wider than kSchurMaxElimWidth; nothing kept; a Jacobian row with entries in two
// eliminated params (the lowest such row is named with both params); an item count of the blocks outside
// [0, 2^31).
std::unique_ptr<JacSchurMap> createJacSchurMap(const JacobianProductMap& product, int64_t numEliminate,
                                               const int64_t* eliminate);

// The plan of the diagonal blocks of C over the kept params, cached in the map.  Throws, naming it, for a kept
// param wider than kCgMaxBlockWidth.
const JacBlockPlan& jacSchurKeptPlan(const JacSchurMap& map);

// The plan of the block diagonal of S (above) from the map's lists: counting sorts only, nothing of the size of the
// kept item plan.  Throws, naming it and before anything of the entries' size is allocated, for a kept param wider
// than kCgMaxBlockWidth and for a table count (pair-rows, record entries) outside [0, 2^31).
std::unique_ptr<JacSchurJacobiPlan> createJacSchurJacobiPlan(const JacSchurMap& map);
// ... cached in the map
const JacSchurJacobiPlan& jacSchurJacobiPlan(const JacSchurMap& map);

}  // namespace BaSpaCho
