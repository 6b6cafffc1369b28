// Products with a sparse Jacobian given as entries, without any layout and without the pair lists of the
// normal equations: y = J v, g = J^T u, the squared column norms and the diagonal
// blocks of J^T J, for the matrix-free least squares of hip_cgls_kernels.h.  The map is built once on the
// host (this file, no device work); the kernels that use it are launched by hip_extensions.hip.
//
// CONVENTIONS.  J is m x n (n = the solver's order), given as entries (rows[k], cols[k], values[k]) in the
// caller's scalar order, no (row, col) repeated: normal_eq.h's rules.  The solver is the device context and
// the source of the params; its layout is never touched.  Run i of `rows` holds the entries of Jacobian row
// i in ascending k with their columns, run c of `cols` the entries of column c in ascending k with their
// rows; each has the list of its runs of more than kAssemblyLongRun terms, which a whole wave sums in the
// same sequential order.  Nothing here has the size of the pair count P of section 17.
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

#include "entry_map.h"

namespace BaSpaCho {

// The diagonal blocks of J^T J over the solver's params, in the caller's order, for block-Jacobi: block b
// holds the scalars [blockStart[b], blockStart[b + 1]), at most kCgMaxBlockWidth of them, and its inverse
// the elements [blockOff[b], blockOff[b + 1]) of the preconditioner's values, row-major.  The items of
// block b are (itemA[t], itemB[t], itemPos[t]), t in [itemStart[b], itemStart[b + 1]): every unordered pair
// of entries of one Jacobian row whose columns are both in the block, self-pairs included, cols[itemA] >=
// cols[itemB], at itemPos = (cols[itemA] - s) w + (cols[itemB] - s), s the block's first scalar and w its
// width.  They come in ascending Jacobian row; inside a row the entries x of the block in ascending entry
// index, each paired with the entries up to and including itself.
// A plan over a subset of the params (createJacBlockPlanOn; jac_schur.h) has blockWidth: block b then holds the
// scalars [blockStart[b], blockStart[b] + blockWidth[b]), blockStart[numBlocks] = n, and scalarBlock is -1 outside
// the subset.  blockWidth is empty for a plan over all params.
struct JacBlockPlan {
  int64_t n = 0, numBlocks = 0, maxWidth = 0;
  std::vector<int32_t> blockStart, blockWidth, scalarBlock, itemStart, itemA, itemB, itemPos;
  std::vector<int64_t> blockOff;
  int64_t inverseElems() const { return blockOff.empty() ? 0 : blockOff.back(); }
  int64_t numItems() const { return (int64_t)itemA.size(); }
  int64_t deviceBytes() const {
    return (int64_t)((blockStart.size() + blockWidth.size() + scalarBlock.size() + itemStart.size() + 3 * itemA.size()) *
                         sizeof(int32_t) +
                     blockOff.size() * sizeof(int64_t));
  }
};

struct JacobianProductMap {
  const Solver* solver = nullptr;  // the device context and the params; its layout is never touched
  int64_t m = 0, n = 0, nnz = 0;
  RunList rows, cols;
  std::vector<int32_t> scalarStart;  // 0 .. n: every scalar as a block of its own, for the status of a Jacobi build

  mutable HipEntryMapDevPtr dev;
  mutable std::unique_ptr<JacBlockPlan> blocks;  // built by the first call that asks for it (jacBlockPlan)

  int64_t rowDeviceBytes() const { return rows.deviceBytes(); }
  int64_t colDeviceBytes() const { return cols.deviceBytes(); }
};

// Builds the map of the m x order() Jacobian with entries (rows[k], cols[k]) for `solver`.  Throws, naming
// the first offending entry index and its (row, col), for an index out of range or a repeated (row, col);
// nnz and m must be in [0, 2^31).  Host only: counting sorts, no comparison sort.
std::unique_ptr<JacobianProductMap> createJacobianProductMap(const Solver& solver, int64_t m, int64_t nnz,
                                                             const int64_t* rows, const int64_t* cols);

// The item count of the blocks of `sizes` scalars (they sum to map.n), which must be in [0, 2^31): checked
// (and stated) by checkJacBlockItems before anything of its size is allocated.
void checkJacBlockItems(int64_t items);
// The plan over blocks of `blockSizes` scalars in the caller's order.  Throws for a block wider than
// kCgMaxBlockWidth, naming it.  Host only: stable counting sorts.
std::unique_ptr<JacBlockPlan> createJacBlockPlan(const JacobianProductMap& map, const std::vector<int64_t>& blockSizes);
// The plan over the blocks [first[b], first[b] + width[b]) alone, ascending and disjoint (the caller's check):
// the items of the other scalars are left out.  `maxWidth`: the widest block taken, named in the refusal.
std::unique_ptr<JacBlockPlan> createJacBlockPlanOn(const JacobianProductMap& map, const std::vector<int32_t>& first,
                                                   const std::vector<int32_t>& width);
// ... of the map's solver (its params), cached in the map
const JacBlockPlan& jacBlockPlan(const JacobianProductMap& map);

}  // namespace BaSpaCho
