// Host map of the coordinate-entry assembly (assembly.h).
#include "assembly.h"

#include <algorithm>
#include <stdexcept>
#include <string>

#include "entry_map.h"
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

  const ScalarLocator loc(solver);
  const int64_t n = solver.order();

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
    m->entryOff[k] = loc.offset(i, j);
    if (m->entryOff[k] < 0) {
      throw std::runtime_error("assembly: " + entryName(k, i, j) + " (params " + std::to_string(loc.paramOf[i]) +
                               ", " + std::to_string(loc.paramOf[j]) + ") is not in the solver's stored pattern");
    }
    kept.push_back((int32_t)k);
  }

  // entries by (offset, entry index), then runs, tile index, long runs
  const int64_t* off = m->entryOff.data();
  sortByOffset(kept, m->runEntry, m->numTiles, [off](int32_t k) { return off[k]; });
  const int32_t* runEntry = m->runEntry.data();
  buildTileRuns((int64_t)m->runEntry.size(), m->numTiles, [off, runEntry](int64_t x) { return off[runEntry[x]]; },
                TileRuns{m->dest, m->runStart, m->tileFirst, m->destLocal, m->longDest, m->tileLongFirst, m->maxRun});
  return m;
}

}  // namespace BaSpaCho
