// Host pieces shared by the maps that turn caller-order entries into ordered sums on the device:
// assembly.cpp (coordinate entries), normal_eq.cpp (pairs of Jacobian entries,
// section 17) and sym_product.cpp (row lists, section 21).  The stored lower element of a scalar pair,
// the stable counting sort, the destination-sorted runs with their tile index (TileRuns), items grouped
// into runs by a key (RunList), the checks of the caller's arrays and the handle of a map's device
// copy.  Header only, no device work; the kernels that sum the runs are in hip_ordered_sum.h.
#pragma once

#include <algorithm>
#include <cstdint>
#include <memory>
#include <numeric>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "solver.h"

namespace BaSpaCho {

// layout elements per workgroup of the tile kernel; runs longer than kAssemblyLongRun items are summed
// by a whole wave instead of one lane
constexpr int64_t kAssemblyTile = 2048;
constexpr int32_t kAssemblyLongRun = 64;
constexpr bool isLongRun(int64_t len) { return len > kAssemblyLongRun; }

// a map's tables on the device (hip_extensions.hip), each uploaded by the first call that needs it and
// freed with the map
struct HipEntryMapDev;
void hipBackendFreeEntryMap(HipEntryMapDev* dev);
struct HipEntryMapDevFree {
  void operator()(HipEntryMapDev* dev) const { hipBackendFreeEntryMap(dev); }
};
using HipEntryMapDevPtr = std::unique_ptr<HipEntryMapDev, HipEntryMapDevFree>;

// stable counting sort of idx by key(idx) in [0, numKeys)
template <typename Key>
static void countingSort(const std::vector<int32_t>& in, std::vector<int32_t>& out, int64_t numKeys, Key key) {
  std::vector<int64_t> start(numKeys + 1, 0);
  for (int32_t k : in) start[key(k) + 1]++;
  for (int64_t b = 0; b < numKeys; b++) start[b + 1] += start[b];
  out.resize(in.size());
  for (int32_t k : in) out[start[key(k)]++] = k;
}

// caller's scalar -> (param, local position), params in param order, and the stored lower element of
// a scalar pair (i, j), i >= j: PermutedCoalescedAccessor::blockOffset, its `flipped` flag, and
// (r, c) -> (c, r) inside a diagonal block
struct ScalarLocator {
  PermutedCoalescedAccessor acc;
  const std::vector<int64_t>& perm;
  int64_t n;
  std::vector<int64_t> userStart, paramOf;

  explicit ScalarLocator(const Solver& solver)
      : acc(solver.accessor()), perm(solver.paramToSpan()), n(solver.order()) {
    const std::vector<int64_t>& spanStart = solver.skel().spanStart;
    const int64_t numParams = (int64_t)perm.size();
    userStart.assign(numParams + 1, 0);
    paramOf.resize(n);
    for (int64_t p = 0; p < numParams; p++) {
      const int64_t size = spanStart[perm[p] + 1] - spanStart[perm[p]];
      userStart[p + 1] = userStart[p] + size;
      std::fill(paramOf.begin() + userStart[p], paramOf.begin() + userStart[p + 1], p);
    }
  }

  // layout offset of (i, j), i >= j, both in [0, n); -1 when the block of its params is not stored
  int64_t offset(int64_t i, int64_t j) const {
    const int64_t p = paramOf[i], q = paramOf[j];
    int64_t r = i - userStart[p], c = j - userStart[q];
    const int64_t sp = perm[p], sq = perm[q];
    if (!acc.plainAcc.hasBlock(std::max(sp, sq), std::min(sp, sq))) return -1;
    const auto osf = acc.blockOffset(p, q);
    if (sp == sq && r < c) std::swap(r, c);
    const int64_t off = std::get<0>(osf), stride = std::get<1>(osf);
    return std::get<2>(osf) ? off + c * stride + r : off + r * stride + c;
  }
};

// items by (offset, item index): LSD counting sort, first on the position inside the tile, then on
// the tile, both stable on the order of `items` (consumed)
template <typename Off>
static void sortByOffset(std::vector<int32_t>& items, std::vector<int32_t>& sorted, int64_t numTiles, Off off) {
  std::vector<int32_t> byLocal;
  countingSort(items, byLocal, kAssemblyTile, [off](int32_t k) { return off(k) & (kAssemblyTile - 1); });
  std::vector<int32_t>().swap(items);
  countingSort(byLocal, sorted, numTiles, [off](int32_t k) { return off(k) / kAssemblyTile; });
}

// the destination-sorted form of items sorted by offset: the unique destinations in ascending offset; the
// items of destination u are the sorted items [runStart[u], runStart[u + 1]).  Tile index: destinations
// [tileFirst[t], tileFirst[t + 1]) lie in layout tile t (kAssemblyTile elements); destLocal[u] = dest[u] -
// tile base.  longDest lists the destinations whose runs are longer than kAssemblyLongRun, ascending;
// those of tile t are [tileLongFirst[t], tileLongFirst[t + 1])
struct TileRuns {
  std::vector<int64_t> dest;
  std::vector<int32_t> runStart;
  std::vector<int32_t> tileFirst;
  std::vector<uint16_t> destLocal;
  std::vector<int32_t> longDest;
  std::vector<int32_t> tileLongFirst;
  int64_t maxRun = 0;  // most items summed into one element

  // off(x): offset of the x-th sorted item
  template <typename Off>
  void build(int64_t numSorted, int64_t numTiles, Off off) {
    tileFirst.assign(numTiles + 1, 0);
    tileLongFirst.assign(numTiles + 1, 0);
    for (int64_t x = 0; x < numSorted; x++) {
      const int64_t o = off(x);
      if (x == 0 || o != dest.back()) {
        dest.push_back(o);
        runStart.push_back((int32_t)x);
        destLocal.push_back((uint16_t)(o & (kAssemblyTile - 1)));
        tileFirst[o / kAssemblyTile + 1]++;
      }
    }
    runStart.push_back((int32_t)numSorted);
    const int64_t numDest = (int64_t)dest.size();
    for (int64_t u = 0; u < numDest; u++) {
      const int64_t len = runStart[u + 1] - runStart[u];
      maxRun = std::max(maxRun, len);
      if (isLongRun(len)) {
        longDest.push_back((int32_t)u);
        tileLongFirst[dest[u] / kAssemblyTile + 1]++;
      }
    }
    for (int64_t b = 0; b < numTiles; b++) {
      tileFirst[b + 1] += tileFirst[b];
      tileLongFirst[b + 1] += tileLongFirst[b];
    }
  }
  // bytes on the device once uploaded (dest stays on the host)
  int64_t deviceBytes() const {
    return (int64_t)((runStart.size() + tileFirst.size() + longDest.size() + tileLongFirst.size()) * sizeof(int32_t) +
                     destLocal.size() * sizeof(uint16_t));
  }
};

// items grouped into runs by a key: the items of run u are (entry[t], idx[t]), t in [start[u],
// start[u + 1]), in the order the items were given.  longRuns (when asked for) lists the runs of more
// than kAssemblyLongRun items, which a whole wave sums
struct RunList {
  std::vector<int32_t> start, entry, idx, longRuns;
  int64_t maxRun = 0;  // most items in one run

  // item t in [0, numItems) goes to run key(t) in [0, numKeys) as (entryOf(t), idxOf(t))
  template <typename Key, typename Entry, typename Idx>
  void build(int64_t numItems, int64_t numKeys, Key key, Entry entryOf, Idx idxOf, bool wantLong) {
    std::vector<int32_t> ids(numItems), sorted;
    std::iota(ids.begin(), ids.end(), 0);
    countingSort(ids, sorted, numKeys, key);
    start.assign(numKeys + 1, 0);
    for (int32_t t : ids) start[key(t) + 1]++;
    for (int64_t u = 0; u < numKeys; u++) start[u + 1] += start[u];
    entry.resize(numItems);
    idx.resize(numItems);
    for (int64_t t = 0; t < numItems; t++) {
      entry[t] = (int32_t)entryOf(sorted[t]);
      idx[t] = (int32_t)idxOf(sorted[t]);
    }
    for (int64_t u = 0; u < numKeys; u++) {
      const int64_t len = start[u + 1] - start[u];
      maxRun = std::max(maxRun, len);
      if (wantLong && isLongRun(len)) longRuns.push_back((int32_t)u);
    }
  }
  int64_t deviceBytes() const {
    return (int64_t)((start.size() + entry.size() + idx.size() + longRuns.size()) * sizeof(int32_t));
  }
};

// ---- what every map says about its input: `op` is the map's name in the message
static inline std::string entryName(int64_t k, int64_t i, int64_t j) {
  return "entry " + std::to_string(k) + " at (" + std::to_string(i) + ", " + std::to_string(j) + ")";
}
static inline void checkBelow2p31(const char* op, const char* what, int64_t v) {
  if (v < 0 || v >= (int64_t(1) << 31)) {
    throw std::runtime_error(std::string(op) + ": " + what + " = " + std::to_string(v) + " is outside [0, 2^31)");
  }
}
static inline void checkEntryArrays(const char* op, int64_t nnz, const int64_t* rows, const int64_t* cols) {
  if (nnz > 0 && (rows == nullptr || cols == nullptr)) {
    throw std::runtime_error(std::string(op) + ": the row or column array is NULL");
  }
}
// the entries of an m x n Jacobian: every index in range
static inline void checkJacobianRange(const char* op, int64_t m, int64_t n, int64_t nnz, const int64_t* rows,
                                      const int64_t* cols) {
  for (int64_t k = 0; k < nnz; k++) {
    const int64_t i = rows[k], j = cols[k];
    if (i < 0 || i >= m || j < 0 || j >= n) {
      throw std::runtime_error(std::string(op) + ": " + entryName(k, i, j) + " is out of range [0, " +
                               std::to_string(m) + ") x [0, " + std::to_string(n) + ")");
    }
  }
}
// ... and no (row, col) repeated.  byCol: the entries by (col, k), the `entry` of the column lists; stably by
// row they hold the repeats of one position side by side; the first repeated entry is the smallest
// second-of-a-pair
static inline void checkJacobianRepeats(const char* op, int64_t m, int64_t nnz, const int64_t* rows,
                                        const int64_t* cols, const std::vector<int32_t>& byCol) {
  std::vector<int32_t> byRowCol;
  countingSort(byCol, byRowCol, m, [rows](int32_t k) { return rows[k]; });
  int64_t first = -1, earlier = -1;
  for (int64_t x = 1; x < nnz; x++) {
    const int32_t a = byRowCol[x - 1], b = byRowCol[x];
    if (rows[a] == rows[b] && cols[a] == cols[b] && (first < 0 || b < first)) {
      first = b;
      earlier = a;
    }
  }
  if (first < 0) return;
  // `earlier` is the repeat's predecessor in its group; name the group's first entry
  int64_t k0 = earlier;
  for (int64_t k = 0; k < earlier; k++) {
    if (rows[k] == rows[first] && cols[k] == cols[first]) {
      k0 = k;
      break;
    }
  }
  throw std::runtime_error(std::string(op) + ": " + entryName(first, rows[first], cols[first]) +
                           " repeats the position of entry " + std::to_string(k0) +
                           "; duplicate Jacobian entries are not summed");
}

}  // namespace BaSpaCho
