// Products with a symmetric matrix given as coordinate entries, without its layout (DESIGN.md section
// 21): y = A x straight from the entry values, and the gradient of the values of such a product.  The
// map is built once on the host (this file, no device work); the kernels that use it are in
// hip_ordered_sum.h, launched by hip_extensions.hip.
//
// CONVENTIONS.  A is n x n (n = the solver's order), given as entries (rows[k], cols[k], values[k]) in
// the caller's scalar order, under the index rules of the assembly (assembly.h): an index out of range
// is refused, "lower" refuses row < col and "full" skips it, so A_ij = A_ji = the sum of the values of
// the kept entries at (i, j), i >= j -- the matrix the assembly builds.  Whether the solver stores the
// element does not matter here: nothing is written to a layout.  The term list of scalar i holds, in
// ascending k, (k, cols[k]) for every kept entry with rows[k] == i and (k, rows[k]) for every kept entry
// with cols[k] == i and rows[k] != i; duplicates stay separate terms.  (A x)_i is the sum over the terms
// (k, idx) of row i of values[k] * x[idx], in list order, every product rounded in the value type, added
// one by one from +0.
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

#include "assembly.h"

namespace BaSpaCho {

// The plan of a built-in preconditioner of the conjugate gradient: the diagonal
// blocks of A and the entries that land in each.  CgJacobi: every scalar is a block of width 1.
// CgBlockJacobi: the blocks are the solver's params, in the caller's order.  The items of block b are
// (itemEntry[t], itemPos[t]), t in [itemStart[b], itemStart[b + 1]), in ascending entry index: the kept
// entry k at (i, j), i >= j, both in block b, with itemPos = (i - s) w + (j - s), s the block's first
// scalar and w its width.  The inverse of block b takes the elements [blockOff[b], blockOff[b + 1]) of
// the preconditioner's values, row-major.
enum CgPrecondKind : int32_t { CgGiven = 0, CgJacobi = 1, CgBlockJacobi = 2, CgFsai = 3 };
constexpr int64_t kCgMaxBlockWidth = 32;
constexpr int64_t kCgFsaiMaxRow = 32;  // widest row of the factorised sparse approximate inverse
struct CgPrecondPlan {
  int32_t kind = CgJacobi;
  int64_t n = 0, numBlocks = 0, maxWidth = 0;
  std::vector<int32_t> blockStart, scalarBlock, itemStart, itemEntry, itemPos;
  std::vector<int64_t> blockOff;
  int64_t inverseElems() const { return blockOff.empty() ? 0 : blockOff.back(); }
  int64_t numItems() const { return (int64_t)itemEntry.size(); }
};

// The plan of the factorised sparse approximate inverse M^-1 = G^T G, G lower
// triangular on the pattern of the lower triangle of A.  Row i of G sits on the scalars cols[rowStart[i]
// .. rowStart[i + 1]), ascending: i itself, last, and the scalars j < i with a kept entry at (i, j) (a zero
// value counts, duplicates count once), only the kCgFsaiMaxRow - 1 largest of them when there are more.
// The items of row i are (itemEntry[t], itemPos[t]), t in [itemStart[i], itemStart[i + 1]), in ascending
// entry index: the kept entry k at (a, b), a >= b, both in the row's set, with itemPos = la w + lb, la and
// lb the local indices of a and b and w the row's width.  Column j of G is run j of colRuns: (position in
// the values of G, row) in ascending row, with the list of the columns of more than kAssemblyLongRun terms;
// chunkLongFirst[c] is the first of them at or past scalar 1024 c (the chunks of the dot products).
struct CgFsaiPlan {
  int64_t n = 0, maxWidth = 0;
  std::vector<int32_t> rowStart, cols, itemStart, itemEntry, itemPos, chunkLongFirst;
  RunList colRuns;
  int64_t elems() const { return (int64_t)cols.size(); }
  int64_t numItems() const { return (int64_t)itemEntry.size(); }
};

struct SymProductMap {
  const Solver* solver = nullptr;  // the solver the map was built for (its order, its stream)
  int32_t triangle = AssemblyLower;
  int64_t n = 0, nnz = 0, kept = 0;

  // row lists: the terms of row i in ascending entry index, with the list of the long rows
  RunList rows;

  // entry lists: (entRow[k], entCol[k]) of every entry, entRow[k] = -1 for a skipped one
  std::vector<int32_t> entRow, entCol;

  mutable HipEntryMapDevPtr dev;

  // the preconditioner plans, built by the first call that asks for one (cgPrecondPlan)
  mutable std::unique_ptr<CgPrecondPlan> cgPlans[3];
  mutable std::unique_ptr<CgFsaiPlan> cgFsai;

  int64_t numTerms() const { return (int64_t)rows.entry.size(); }
  // bytes each part takes on the device once uploaded
  int64_t rowDeviceBytes() const { return rows.deviceBytes(); }
  int64_t entryDeviceBytes() const { return (int64_t)((entRow.size() + entCol.size()) * sizeof(int32_t)); }
};

// Builds the map of the entries (rows[k], cols[k]) for a matrix of order n; triangle as for
// createAssemblyMap.  Throws, naming the first offending entry index and its (row, col), for an index
// out of range and, in "lower" mode, for row < col; nnz, n and the term count must be in [0, 2^31): the
// term count is checked (and stated) before anything of its size is allocated.  Host only: counting
// sorts, no comparison sort.
std::unique_ptr<SymProductMap> createSymProductMap(int64_t n, int64_t nnz, const int64_t* rows, const int64_t* cols,
                                                   int32_t triangle);
// ... for `solver`: n = solver.order(), and the map runs on that solver alone
std::unique_ptr<SymProductMap> createSymProductMap(const Solver& solver, int64_t nnz, const int64_t* rows,
                                                   const int64_t* cols, int32_t triangle);

// The plan of `kind` (CgJacobi or CgBlockJacobi) over the entries of `map`, from blocks of `blockSizes`
// scalars in the caller's order (they sum to map.n; ignored for CgJacobi).  Throws for a block wider than
// kCgMaxBlockWidth, naming it.  Host only: one counting sort.
std::unique_ptr<CgPrecondPlan> createCgPrecondPlan(const SymProductMap& map, int32_t kind,
                                                   const std::vector<int64_t>& blockSizes);
// ... of the map's solver (its params), cached in the map
const CgPrecondPlan& cgPrecondPlan(const SymProductMap& map, int32_t kind);

// The plan of CgFsai over the entries of `map`.  The element count of G and the item count must be in [0,
// 2^31): each is checked (and stated) by checkCgFsaiSizes before anything of its size is allocated.  Host
// only: counting sorts, no comparison sort.
void checkCgFsaiSizes(int64_t elems, int64_t items);
std::unique_ptr<CgFsaiPlan> createCgFsaiPlan(const SymProductMap& map);
// ... cached in the map
const CgFsaiPlan& cgFsaiPlan(const SymProductMap& map);

}  // namespace BaSpaCho
