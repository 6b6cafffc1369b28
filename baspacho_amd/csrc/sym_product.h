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

struct SymProductMap {
  const Solver* solver = nullptr;  // the solver the map was built for (its order, its stream)
  int32_t triangle = AssemblyLower;
  int64_t n = 0, nnz = 0, kept = 0;

  // row lists: the terms of row i in ascending entry index, with the list of the long rows
  RunList rows;

  // entry lists: (entRow[k], entCol[k]) of every entry, entRow[k] = -1 for a skipped one
  std::vector<int32_t> entRow, entCol;

  mutable HipEntryMapDevPtr dev;

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

}  // namespace BaSpaCho
