// Host map of the coordinate-entry assembly (assembly.h).
#include "assembly.h"

#include <algorithm>
#include <stdexcept>
#include <string>

#include "solver.h"

namespace BaSpaCho {

std::unique_ptr<AssemblyMap> createAssemblyMap(const Solver& solver, int64_t nnz, const int64_t* rows,
                                               const int64_t* cols, int32_t triangle) {
  if (triangle != AssemblyLower && triangle != AssemblyFull) {
    throw std::runtime_error("assembly: unknown triangle mode " + std::to_string(triangle) +
                             " (0: lower, 1: full)");
  }
  checkBelow2p31("assembly", "nnz", nnz);
  checkEntryArrays("assembly", nnz, rows, cols);
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
  m->tiles.build((int64_t)m->runEntry.size(), m->numTiles, [off, runEntry](int64_t x) { return off[runEntry[x]]; });
  return m;
}

}  // namespace BaSpaCho
