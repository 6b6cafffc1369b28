// Host map of the coordinate-entry assembly (assembly.h).
#include "assembly.h"

#include <algorithm>
#include <stdexcept>
#include <string>

#include "hip_backend.h"
#include "solver.h"

namespace BaSpaCho {

AssemblyMap::~AssemblyMap() {
  if (dev) hipBackendFreeAssembly(dev);
}

int64_t AssemblyMap::deviceBytes() const {
  return (int64_t)(entryOff.size() * sizeof(int64_t) + runStart.size() * sizeof(int32_t) +
                   runEntry.size() * sizeof(int32_t) + tileFirst.size() * sizeof(int32_t) +
                   destLocal.size() * sizeof(uint16_t) + longDest.size() * sizeof(int32_t) +
                   tileLongFirst.size() * sizeof(int32_t));
}

static std::string entryName(int64_t k, int64_t i, int64_t j) {
  return "entry " + std::to_string(k) + " at (" + std::to_string(i) + ", " + std::to_string(j) + ")";
}

// stable counting sort of idx by key(idx) in [0, numKeys)
template <typename Key>
static void countingSort(const std::vector<int32_t>& in, std::vector<int32_t>& out, int64_t numKeys, Key key) {
  std::vector<int64_t> start(numKeys + 1, 0);
  for (int32_t k : in) start[key(k) + 1]++;
  for (int64_t b = 0; b < numKeys; b++) start[b + 1] += start[b];
  out.resize(in.size());
  for (int32_t k : in) out[start[key(k)]++] = k;
}

std::unique_ptr<AssemblyMap> createAssemblyMap(const Solver& solver, int64_t nnz, const int64_t* rows,
                                               const int64_t* cols, int32_t triangle) {
  if (triangle != AssemblyLower && triangle != AssemblyFull) {
    throw std::runtime_error("assembly: unknown triangle mode " + std::to_string(triangle) +
                             " (0: lower, 1: full)");
  }
  if (nnz < 0 || nnz >= (int64_t(1) << 31)) {
    throw std::runtime_error("assembly: nnz = " + std::to_string(nnz) + " is outside [0, 2^31)");
  }
  if (nnz > 0 && (rows == nullptr || cols == nullptr)) {
    throw std::runtime_error("assembly: the row or column array is NULL");
  }
  std::unique_ptr<AssemblyMap> m(new AssemblyMap);
  m->solver = &solver;
  m->triangle = triangle;
  m->nnz = nnz;
  m->dataSize = solver.dataSize();
  m->numTiles = (m->dataSize + kAssemblyTile - 1) / kAssemblyTile;

  // caller's scalar -> (param, local position), params in param order
  const PermutedCoalescedAccessor acc = solver.accessor();
  const std::vector<int64_t>& perm = solver.paramToSpan();
  const std::vector<int64_t>& spanStart = solver.skel().spanStart;
  const int64_t numParams = (int64_t)perm.size(), n = solver.order();
  std::vector<int64_t> userStart(numParams + 1, 0), paramOf(n);
  for (int64_t p = 0; p < numParams; p++) {
    const int64_t size = spanStart[perm[p] + 1] - spanStart[perm[p]];
    userStart[p + 1] = userStart[p] + size;
    std::fill(paramOf.begin() + userStart[p], paramOf.begin() + userStart[p + 1], p);
  }

  m->entryOff.resize(nnz);
  std::vector<int32_t> kept;
  kept.reserve(nnz);
  for (int64_t k = 0; k < nnz; k++) {
    const int64_t i = rows[k], j = cols[k];
    if (i < 0 || i >= n || j < 0 || j >= n) {
      throw std::runtime_error("assembly: " + entryName(k, i, j) + " is out of range [0, " + std::to_string(n) +
                               ")");
    }
    if (i < j) {
      if (triangle == AssemblyLower) {
        throw std::runtime_error("assembly: " + entryName(k, i, j) +
                                 " has row < col; triangle 'lower' needs row >= col");
      }
      m->entryOff[k] = -1;
      continue;
    }
    const int64_t p = paramOf[i], q = paramOf[j];
    int64_t r = i - userStart[p], c = j - userStart[q];
    const int64_t sp = perm[p], sq = perm[q];
    if (!acc.plainAcc.hasBlock(std::max(sp, sq), std::min(sp, sq))) {
      throw std::runtime_error("assembly: " + entryName(k, i, j) + " (params " + std::to_string(p) + ", " +
                               std::to_string(q) + ") is not in the solver's stored pattern");
    }
    const auto osf = acc.blockOffset(p, q);
    if (sp == sq && r < c) std::swap(r, c);
    const int64_t off = std::get<0>(osf), stride = std::get<1>(osf);
    m->entryOff[k] = std::get<2>(osf) ? off + c * stride + r : off + r * stride + c;
    kept.push_back((int32_t)k);
  }

  // entries by (offset, entry index): LSD counting sort, first on the position inside the tile, then
  // on the tile, both stable on ascending k
  const int64_t* off = m->entryOff.data();
  std::vector<int32_t> byLocal;
  countingSort(kept, byLocal, kAssemblyTile, [off](int32_t k) { return off[k] & (kAssemblyTile - 1); });
  std::vector<int32_t>().swap(kept);
  countingSort(byLocal, m->runEntry, m->numTiles, [off](int32_t k) { return off[k] / kAssemblyTile; });
  std::vector<int32_t>().swap(byLocal);

  // runs, tile index, long runs
  const int64_t numKept = (int64_t)m->runEntry.size();
  m->tileFirst.assign(m->numTiles + 1, 0);
  m->tileLongFirst.assign(m->numTiles + 1, 0);
  for (int64_t x = 0; x < numKept; x++) {
    const int64_t o = off[m->runEntry[x]];
    if (x == 0 || o != m->dest.back()) {
      m->dest.push_back(o);
      m->runStart.push_back((int32_t)x);
      m->destLocal.push_back((uint16_t)(o & (kAssemblyTile - 1)));
      m->tileFirst[o / kAssemblyTile + 1]++;
    }
  }
  m->runStart.push_back((int32_t)numKept);
  const int64_t numDest = (int64_t)m->dest.size();
  for (int64_t u = 0; u < numDest; u++) {
    const int64_t len = m->runStart[u + 1] - m->runStart[u];
    m->maxRun = std::max(m->maxRun, len);
    if (len > kAssemblyLongRun) {
      m->longDest.push_back((int32_t)u);
      m->tileLongFirst[m->dest[u] / kAssemblyTile + 1]++;
    }
  }
  for (int64_t t = 0; t < m->numTiles; t++) {
    m->tileFirst[t + 1] += m->tileFirst[t];
    m->tileLongFirst[t + 1] += m->tileLongFirst[t];
  }
  return m;
}

}  // namespace BaSpaCho
