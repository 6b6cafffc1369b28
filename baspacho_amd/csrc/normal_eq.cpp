// Host maps of the normal equations of a sparse Jacobian (normal_eq.h).
#include "normal_eq.h"

#include <algorithm>
#include <numeric>
#include <stdexcept>
#include <string>

#include "entry_map.h"
#include "hip_backend.h"
#include "solver.h"

namespace BaSpaCho {

NormalEqMap::~NormalEqMap() {
  if (dev) hipBackendFreeNormalEq(dev);
}

int64_t NormalEqMap::forwardDeviceBytes() const {
  return (int64_t)(runStart.size() * sizeof(int32_t) + pairA.size() * sizeof(int32_t) +
                   pairB.size() * sizeof(int32_t) + tileFirst.size() * sizeof(int32_t) +
                   destLocal.size() * sizeof(uint16_t) + longDest.size() * sizeof(int32_t) +
                   tileLongFirst.size() * sizeof(int32_t));
}

int64_t NormalEqMap::adjointDeviceBytes() const {
  return (int64_t)(adjStart.size() * sizeof(int64_t) + adjPartner.size() * sizeof(int32_t) +
                   adjDest.size() * sizeof(int64_t) + adjLong.size() * sizeof(int32_t));
}

int64_t NormalEqMap::vectorDeviceBytes() const {
  return (int64_t)((colStart.size() + colEntry.size() + colIdx.size() + rowStart.size() + rowEntry.size() +
                    rowIdx.size()) *
                   sizeof(int32_t));
}

static std::string entryName(int64_t k, int64_t i, int64_t j) {
  return "entry " + std::to_string(k) + " at (" + std::to_string(i) + ", " + std::to_string(j) + ")";
}

// the entries grouped by key (ascending k inside a group): starts [numKeys + 1] and the entry list
static void groupEntries(const std::vector<int32_t>& in, int64_t numKeys, const int64_t* key,
                         std::vector<int32_t>& start, std::vector<int32_t>& list) {
  countingSort(in, list, numKeys, [key](int32_t k) { return key[k]; });
  start.assign(numKeys + 1, 0);
  for (int32_t k : in) start[key[k] + 1]++;
  for (int64_t b = 0; b < numKeys; b++) start[b + 1] += start[b];
}

std::unique_ptr<NormalEqMap> createNormalEqMap(const Solver& solver, int64_t m, int64_t nnz, const int64_t* rows,
                                               const int64_t* cols) {
  const int64_t lim = int64_t(1) << 31;
  if (nnz < 0 || nnz >= lim) {
    throw std::runtime_error("normal equations: nnz = " + std::to_string(nnz) + " is outside [0, 2^31)");
  }
  if (m < 0 || m >= lim) {
    throw std::runtime_error("normal equations: m = " + std::to_string(m) + " is outside [0, 2^31)");
  }
  if (nnz > 0 && (rows == nullptr || cols == nullptr)) {
    throw std::runtime_error("normal equations: the row or column array is NULL");
  }
  std::unique_ptr<NormalEqMap> q(new NormalEqMap);
  const int64_t n = solver.order();
  q->solver = &solver;
  q->m = m;
  q->n = n;
  q->nnz = nnz;
  q->dataSize = solver.dataSize();
  q->numTiles = (q->dataSize + kAssemblyTile - 1) / kAssemblyTile;

  for (int64_t k = 0; k < nnz; k++) {
    const int64_t i = rows[k], j = cols[k];
    if (i < 0 || i >= m || j < 0 || j >= n) {
      throw std::runtime_error("normal equations: " + entryName(k, i, j) + " is out of range [0, " +
                               std::to_string(m) + ") x [0, " + std::to_string(n) + ")");
    }
  }

  // vector lists: entries by column and by row, ascending k inside each
  std::vector<int32_t> all(nnz);
  std::iota(all.begin(), all.end(), 0);
  groupEntries(all, n, cols, q->colStart, q->colEntry);
  groupEntries(all, m, rows, q->rowStart, q->rowEntry);
  std::vector<int32_t>().swap(all);
  q->colIdx.resize(nnz);
  q->rowIdx.resize(nnz);
  for (int64_t x = 0; x < nnz; x++) {
    q->colIdx[x] = (int32_t)rows[q->colEntry[x]];
    q->rowIdx[x] = (int32_t)cols[q->rowEntry[x]];
  }

  // repeated (row, col): the entries by (row, col, k) -- the column lists, stably by row -- hold the
  // repeats of one position side by side; the first repeated entry is the smallest second-of-a-pair
  {
    std::vector<int32_t> byRowCol;
    countingSort(q->colEntry, byRowCol, m, [rows](int32_t k) { return rows[k]; });
    int64_t first = -1, earlier = -1;
    for (int64_t x = 1; x < nnz; x++) {
      const int32_t a = byRowCol[x - 1], b = byRowCol[x];
      if (rows[a] == rows[b] && cols[a] == cols[b] && (first < 0 || b < first)) {
        first = b;
        earlier = a;
      }
    }
    if (first >= 0) {
      // `earlier` is the repeat's predecessor in its group; name the group's first entry
      int64_t k0 = earlier;
      for (int64_t k = 0; k < earlier; k++) {
        if (rows[k] == rows[first] && cols[k] == cols[first]) {
          k0 = k;
          break;
        }
      }
      throw std::runtime_error("normal equations: " + entryName(first, rows[first], cols[first]) +
                               " repeats the position of entry " + std::to_string(k0) +
                               "; duplicate Jacobian entries are not summed");
    }
  }

  // P before anything of its size exists (sum d = nnz < 2^31, so the sum of d (d + 1) / 2 fits int64)
  int64_t P = 0;
  for (int64_t i = 0; i < m; i++) {
    const int64_t d = q->rowStart[i + 1] - q->rowStart[i];
    P += d * (d + 1) / 2;
  }
  if (P >= lim) {
    throw std::runtime_error("normal equations: the Jacobian rows give P = " + std::to_string(P) +
                             " pairs of entries, outside [0, 2^31)");
  }
  q->numPairs = P;

  // pairs in ascending ka (so that the stable sort by offset leaves every run in ascending ka), and
  // the adjoint terms of every entry in ascending partner
  const ScalarLocator loc(solver);
  std::vector<int32_t> pa, pb;
  std::vector<int64_t> pairOff;
  pa.reserve(P);
  pb.reserve(P);
  pairOff.reserve(P);
  q->adjStart.assign(nnz + 1, 0);
  q->adjPartner.reserve(2 * P);
  q->adjDest.reserve(2 * P);
  for (int64_t k = 0; k < nnz; k++) {
    const int64_t i = rows[k], ck = cols[k];
    for (int32_t x = q->rowStart[i]; x < q->rowStart[i + 1]; x++) {
      const int32_t k2 = q->rowEntry[x];
      const int64_t c2 = q->rowIdx[x];
      const int64_t off = loc.offset(std::max(ck, c2), std::min(ck, c2));
      if (off < 0) {
        throw std::runtime_error("normal equations: " + entryName(k, i, ck) + " and entry " + std::to_string(k2) +
                                 " of the same row meet at columns (" + std::to_string(std::max(ck, c2)) + ", " +
                                 std::to_string(std::min(ck, c2)) + ") (params " +
                                 std::to_string(loc.paramOf[std::max(ck, c2)]) + ", " +
                                 std::to_string(loc.paramOf[std::min(ck, c2)]) +
                                 "), which is not in the solver's stored pattern");
      }
      for (int rep = 0; rep < (k2 == k ? 2 : 1); rep++) {
        q->adjPartner.push_back(k2);
        q->adjDest.push_back(off);
      }
      if (k2 == k || c2 < ck) {
        pa.push_back((int32_t)k);
        pb.push_back(k2);
        pairOff.push_back(off);
      }
    }
    q->adjStart[k + 1] = (int64_t)q->adjPartner.size();
    if (q->adjStart[k + 1] - q->adjStart[k] > kAssemblyLongRun) q->adjLong.push_back((int32_t)k);
  }

  // pairs by (offset, ka), then runs, tile index, long runs
  std::vector<int32_t> ids(P), sorted;
  std::iota(ids.begin(), ids.end(), 0);
  const int64_t* off = pairOff.data();
  sortByOffset(ids, sorted, q->numTiles, [off](int32_t p) { return off[p]; });
  q->pairA.resize(P);
  q->pairB.resize(P);
  for (int64_t x = 0; x < P; x++) {
    q->pairA[x] = pa[sorted[x]];
    q->pairB[x] = pb[sorted[x]];
  }
  const int32_t* srt = sorted.data();
  buildTileRuns(P, q->numTiles, [off, srt](int64_t x) { return off[srt[x]]; },
                TileRuns{q->dest, q->runStart, q->tileFirst, q->destLocal, q->longDest, q->tileLongFirst, q->maxRun});
  return q;
}

}  // namespace BaSpaCho
