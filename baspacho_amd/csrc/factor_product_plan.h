// Host plan of the products with the factor, y = L x and y = L^T x (kernels in
// hip_factor_product.h).  No HIP here: the plan is a function of the skeleton alone, built on the host,
// uploaded on the first product and kept with the extension state.
//
// y = L x gathers by row.  The terms of row i (span s) are, chain after chain over the chains whose row
// span is s in ascending column lump, the columns j of the chain's lump with lumpStart + j <= i: the
// span -> chains index below is a counting sort of the chains by chainRowSpan (stable: chains are stored
// by column lump, so ascending chain is ascending lump).  The chain of the span's own lump comes last.
// A span whose longest row has at most kFactorProductLongTerms terms is short: its rows go one per lane.
// Above that its rows go one per wave (longRows), unless the span has at most 64 rows and at least
// kFactorProductHugeChains chains of lumps of at most kFactorProductLaneChain columns (the camera rows of
// BAL: thousands of 3-column blocks): such a span goes to one workgroup of 16 waves (hugeSpans), which
// deals those chains to its waves as whole blocks and takes the wider ones (hugeWide: their positions in
// spanChain) with all waves together.
//
// y = L^T x gathers by column.  Lumps of at most kFactorProductNarrow columns go one column per lane,
// packed (smallColLump / smallCol).  Wider lumps are cut into strips of 64 columns; the rows of a strip
// from its first column on are cut into chunks of about kFactorProductChunkRows rows, one workgroup
// (LtTask) each.  A strip of one chunk writes y; the chunks of a split strip write partial sums that a
// second pass folds in chunk order (LtFold).
#pragma once

#include <cstdint>
#include <vector>

#include "skeleton.h"

namespace BaSpaCho {

constexpr int64_t kFactorProductLongTerms = 128;
constexpr int64_t kFactorProductHugeChains = 256;
constexpr int64_t kFactorProductLaneChain = 16;
constexpr int64_t kFactorProductNarrow = 8;
constexpr int64_t kFactorProductChunkRows = 256;
constexpr int64_t kFactorProductStrip = 64;

// rows [rBeg, rEnd) of columns [c0, c0 + nc) of lump `lump` (w columns, data at dataOff)
struct LtTask {
  int64_t dataOff;
  int32_t lump, w, c0, nc;
  int32_t rBeg, rEnd;
  int32_t chain;  // the chain that holds row rBeg
  int32_t part;   // first slot of the task's 64 partial sums, -1: the task writes y
};

// y[col0 + lane] = the sum over chunks c = 0 .. numChunks - 1, in this order, of part[part0 + 64 c + lane]
struct LtFold {
  int32_t col0, nc, part0, numChunks;
};

struct FactorProductPlan {
  // y = L x
  std::vector<int32_t> spanChainPtr;   // numSpans + 1
  std::vector<int32_t> spanChain;      // chains sorted by row span
  std::vector<int32_t> spanChainLump;  // the column lump of spanChain[p]
  std::vector<int32_t> rowToSpan;      // order
  std::vector<int32_t> spanLong;       // numSpans: 0 = rows one per lane, 1 = one per wave, 2 = the span per workgroup
  std::vector<int32_t> longRows;       // the rows of the spans of kind 1, ascending
  std::vector<int32_t> hugeSpans;      // the spans of kind 2, ascending
  std::vector<int32_t> hugeWidePtr;    // hugeSpans + 1: the wide chains of each in hugeWide
  std::vector<int32_t> hugeWide;       // positions in spanChain, ascending
  // y = L^T x
  std::vector<LtTask> ltTasks;
  std::vector<LtFold> ltFolds;
  std::vector<int32_t> smallColLump, smallCol;  // per packed column: its lump, its internal scalar
  int64_t partElems = 0;                        // partial sums per (matrix, right-hand side)
};

FactorProductPlan buildFactorProductPlan(const CoalescedBlockMatrixSkel& skel);

// the plan as int64 records (include/baspacho_amd_testing.h, bsp_test_factor_product_plan)
std::vector<int64_t> factorProductPlanRecords(const FactorProductPlan& plan);

}  // namespace BaSpaCho
