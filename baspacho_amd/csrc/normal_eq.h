// Normal equations of a sparse Jacobian, H = J^T J in a Solver's numeric layout, g = J^T r and y = J v
// (DESIGN.md section 17).  The maps from Jacobian entries to the layout are built once on the host
// (this file, no device work); the kernels that use them are in hip_ordered_sum.h, launched by
// hip_extensions.hip.
//
// CONVENTIONS.  J is m x n (n = the solver's order), given as entries (rows[k], cols[k], values[k]) in
// the caller's scalar order, no (row, col) repeated.  Every unordered pair of entries of one Jacobian
// row, self-pairs included, is one pair (ka, kb) with cols[ka] >= cols[kb]; it adds values[ka] *
// values[kb] to the stored lower element of (cols[ka], cols[kb]), found as the assembly finds it
// (entry_map.h).  H[d] is the sum over its pairs in ascending ka, every product rounded in the value
// type, added one by one from +0: bitwise np.add.at(zeros(dataSize), off, v[ka] * v[kb]) with the pairs
// in run order.  g[c] = sum of values[k] * r[rows[k]] over the entries of column c, y[i] = sum of
// values[k] * v[cols[k]] over the entries of row i, both in ascending k with the same rounding.  The
// adjoint of H: gradValues[k] = sum of gradData[d_p] * values[partner] over the pairs p that hold k, in
// ascending partner index, the self-pair listed twice in a row.
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

#include "assembly.h"

namespace BaSpaCho {

struct NormalEqMap {
  const Solver* solver = nullptr;  // the solver whose layout the map targets
  int64_t m = 0, n = 0, nnz = 0, dataSize = 0, numTiles = 0;
  int64_t numPairs = 0;  // P = sum over rows of d (d + 1) / 2

  // forward form, destination-sorted as in AssemblyMap: the pairs of destination u are
  // (pairA[x], pairB[x]), x in [tiles.runStart[u], tiles.runStart[u + 1]), in ascending pairA
  std::vector<int32_t> pairA, pairB;
  TileRuns tiles;

  // adjoint form: the terms of entry k are (adjPartner[t], adjDest[t]), t in [adjStart[k],
  // adjStart[k + 1]), in ascending partner (the self-pair twice); adjLong lists the entries with more
  // than kAssemblyLongRun terms, which a whole wave sums
  std::vector<int64_t> adjStart;
  std::vector<int32_t> adjPartner;
  std::vector<int64_t> adjDest;
  std::vector<int32_t> adjLong;

  // vector lists: the entries of column c in ascending k with their rows (cols), the entries of row i
  // with their columns (rows); neither has a long list: one lane sums a run of any length
  RunList cols, rows;

  mutable HipEntryMapDevPtr dev;

  int64_t numAdjointTerms() const { return (int64_t)adjPartner.size(); }
  // bytes each part takes on the device once uploaded
  int64_t forwardDeviceBytes() const {
    return (int64_t)((pairA.size() + pairB.size()) * sizeof(int32_t)) + tiles.deviceBytes();
  }
  int64_t adjointDeviceBytes() const {
    return (int64_t)((adjStart.size() + adjDest.size()) * sizeof(int64_t) +
                     (adjPartner.size() + adjLong.size()) * sizeof(int32_t));
  }
  int64_t vectorDeviceBytes() const { return cols.deviceBytes() + rows.deviceBytes(); }
};

// Builds the map of the m x order() Jacobian with entries (rows[k], cols[k]) for `solver`.  Throws,
// naming the first offending entry index and its (row, col), for an index out of range, a repeated
// (row, col), or a pair whose element is not stored; nnz and m must be in [0, 2^31), and so must the
// pair count P, which is checked (and stated) before anything of size P is allocated.  Host only:
// counting sorts, no comparison sort.
std::unique_ptr<NormalEqMap> createNormalEqMap(const Solver& solver, int64_t m, int64_t nnz, const int64_t* rows,
                                               const int64_t* cols);

}  // namespace BaSpaCho
