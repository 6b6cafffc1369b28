// Reach plans: blocks of A^-1 anywhere, on or off the pattern of L, from forward solves alone
// (DESIGN.md section 20).  (A^-1)_ij = (L^-1 e_i) . (L^-1 e_j), and w_i = L^-1 e_i is nonzero only on
// the reach of i: the lumps reachable from i's lump through "the lump that owns one of my row spans".
// This header and reach.cpp are host code without dependencies beyond the skeleton; the records below
// are also what the kernels of hip_reach_kernels.h read.
#pragma once

#include <cstdint>
#include <vector>

#include "skeleton.h"

namespace BaSpaCho {

constexpr int kReachCols = 16;       // columns of one workgroup of reachSolveL
constexpr int kReachMaxWidth = 64;   // widest lump reachSolveL takes (kPanelWidth): wider ones set the cut

// one workgroup of reachSolveL: k <= kReachCols columns of one query, W columns col0 .. col0 + k - 1,
// the unit entry of column c at internal scalar row0 + c, walking reachLumps[listBegin .. listEnd)
struct ReachGroup {
  int64_t row0;
  int32_t col0, k;
  int32_t listBegin, listEnd;
  int32_t query, pad;
};

// one workgroup of gramBlocks: out[outOff ..] = W_P^T W_Q (nP x nQ, row-major) over the internal scalar
// rows of ranges [rangeBegin, rangeEnd) of the plan, `rows` of them in all
struct GramItem {
  int64_t outOff, rows;
  int32_t colP, nP, colQ, nQ;
  int32_t rangeBegin, rangeEnd;
};

struct ReachPlan {
  int64_t cutLump = 0, cutSpan = 0, cutScalar = 0;
  int64_t numCols = 0;  // m: columns of W, the queries stacked in the order given
  // per query
  std::vector<int64_t> querySpan, queryLump, queryCol0, queryWidth;
  std::vector<int32_t> queryListBegin, queryListEnd;  // its reach in reachLumps, truncated at the cut
  std::vector<int32_t> reachLumps;                    // one sorted list per distinct query lump below the cut
  std::vector<ReachGroup> groups;                     // the queries below the cut, ceil(width / 16) each
  // unit entries of the queries at or beyond the cut (no workgroup): W[unitCol, unitRow] = 1
  std::vector<int64_t> unitCol, unitRow;
  // per requested pair
  std::vector<GramItem> items;
  std::vector<int64_t> rangeStart, rangePrefix;  // per range: first internal scalar, rows of the item before it
  int64_t outSize = 0;
};

// the cut of a skeleton: the first lump wider than kReachMaxWidth, lowered to the beginning of the
// sparse-elimination range that holds it (solveLFrom refuses a start inside a range); numLumps when
// no lump is wide.  elimRanges: consecutive boundaries, as Solver::sparseEliminationRanges()
int64_t reachCutLump(const CoalescedBlockMatrixSkel& skel, const std::vector<int64_t>& elimRanges);

// the lumps < cutLump closed under "lump owning a row span of a lump in the list", from `lump` on, sorted
std::vector<int32_t> reachOfLump(const CoalescedBlockMatrixSkel& skel, int64_t lump, int64_t cutLump);

// spans: the queries, spans in internal order (repeats allowed: their columns repeat).  pairRow /
// pairCol: indices into `spans`, one Gram item each; outOffsets (numPairs + 1, or empty: blocks packed
// one after the other).  Throws std::runtime_error on arguments out of range
ReachPlan buildReachPlan(const CoalescedBlockMatrixSkel& skel, const std::vector<int64_t>& elimRanges,
                         const std::vector<int64_t>& spans, const std::vector<int64_t>& pairRow,
                         const std::vector<int64_t>& pairCol, const std::vector<int64_t>& outOffsets = {});

}  // namespace BaSpaCho
