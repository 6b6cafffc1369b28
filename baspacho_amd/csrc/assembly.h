// Assembly of a symmetric matrix given as coordinate entries (row, col, value) in the caller's scalar
// order into a Solver's numeric layout.  The map from entries to layout offsets
// is built once on the host (this file, no device work); the kernels that use it are in
// hip_ordered_sum.h, launched by hip_extensions.hip.
//
// CONVENTIONS.  Scalar index i of the caller belongs to param p at local position r, from the prefix
// sums of the param sizes in param order.  The symmetric matrix is defined by its lower triangle:
// A_ij = A_ji = sum of the values of the entries at (i, j), i >= j.  Triangle `lower`: every entry
// must have row >= col; `full`: entries with row < col are skipped (offset -1, never read, gradient 0).
// Every kept entry must land on a stored element of the factor (an original block or fill-in); the
// element is the stored lower one, through PermutedCoalescedAccessor::blockOffset and its `flipped`
// flag, and (r, c) -> (c, r) inside a diagonal block.  Duplicates are summed in ascending entry index,
// in the value type, starting from +0: bitwise what np.add.at(zeros(dataSize), offsets, values) gives.
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

#include "entry_map.h"

namespace BaSpaCho {

enum AssemblyTriangle : int32_t { AssemblyLower = 0, AssemblyFull = 1 };

struct AssemblyMap {
  const Solver* solver = nullptr;  // the solver whose layout the map targets
  int32_t triangle = AssemblyLower;
  int64_t nnz = 0, dataSize = 0, numTiles = 0;

  std::vector<int64_t> entryOff;  // per entry: layout offset, -1 when skipped

  // destination-sorted form (forward pass): the entries of destination u are runEntry[tiles.runStart[u]
  // .. tiles.runStart[u + 1]), in ascending entry index
  std::vector<int32_t> runEntry;
  TileRuns tiles;

  mutable HipEntryMapDevPtr dev;

  int64_t numKept() const { return (int64_t)runEntry.size(); }
  // bytes the map takes on the device once uploaded
  int64_t deviceBytes() const {
    return (int64_t)(entryOff.size() * sizeof(int64_t) + runEntry.size() * sizeof(int32_t)) + tiles.deviceBytes();
  }
};

// Builds the map of `nnz` entries (rows[k], cols[k]) for `solver`.  Throws, naming the first offending
// entry index and its (row, col), for an index out of [0, order), row < col in `lower` mode, or an
// element that is not stored; nnz must be in [0, 2^31).  Host only, O(nnz + numTiles) after the
// per-entry block lookups (two stable counting-sort passes, no comparison sort).
std::unique_ptr<AssemblyMap> createAssemblyMap(const Solver& solver, int64_t nnz, const int64_t* rows,
                                               const int64_t* cols, int32_t triangle);

}  // namespace BaSpaCho
