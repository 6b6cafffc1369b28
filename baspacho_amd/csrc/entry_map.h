// Host pieces shared by the maps that send caller-order scalar pairs to a Solver's numeric layout:
// assembly.cpp (coordinate entries) and normal_eq.cpp (pairs of Jacobian entries,
// section 17).  The stored lower element of a scalar pair, the stable counting sort, and the
// destination-sorted runs with their tile index.  Header only, no device work.
#pragma once

#include <algorithm>
#include <cstdint>
#include <tuple>
#include <vector>

#include "assembly.h"
#include "solver.h"

namespace BaSpaCho {

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

// the destination-sorted form of items sorted by offset (off(x): offset of the x-th sorted item): the
// unique destinations ascending, run starts, the tile index with destLocal and the long-run list
struct TileRuns {
  std::vector<int64_t>& dest;
  std::vector<int32_t>& runStart;
  std::vector<int32_t>& tileFirst;
  std::vector<uint16_t>& destLocal;
  std::vector<int32_t>& longDest;
  std::vector<int32_t>& tileLongFirst;
  int64_t& maxRun;
};
template <typename Off>
static void buildTileRuns(int64_t numSorted, int64_t numTiles, Off off, TileRuns t) {
  t.tileFirst.assign(numTiles + 1, 0);
  t.tileLongFirst.assign(numTiles + 1, 0);
  for (int64_t x = 0; x < numSorted; x++) {
    const int64_t o = off(x);
    if (x == 0 || o != t.dest.back()) {
      t.dest.push_back(o);
      t.runStart.push_back((int32_t)x);
      t.destLocal.push_back((uint16_t)(o & (kAssemblyTile - 1)));
      t.tileFirst[o / kAssemblyTile + 1]++;
    }
  }
  t.runStart.push_back((int32_t)numSorted);
  const int64_t numDest = (int64_t)t.dest.size();
  for (int64_t u = 0; u < numDest; u++) {
    const int64_t len = t.runStart[u + 1] - t.runStart[u];
    t.maxRun = std::max(t.maxRun, len);
    if (len > kAssemblyLongRun) {
      t.longDest.push_back((int32_t)u);
      t.tileLongFirst[t.dest[u] / kAssemblyTile + 1]++;
    }
  }
  for (int64_t b = 0; b < numTiles; b++) {
    t.tileFirst[b + 1] += t.tileFirst[b];
    t.tileLongFirst[b + 1] += t.tileLongFirst[b];
  }
}

}  // namespace BaSpaCho
