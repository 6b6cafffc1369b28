// Host map of the products with a symmetric matrix given as entries (sym_product.h).
#include "sym_product.h"

#include <algorithm>
#include <numeric>
#include <stdexcept>
#include <string>

#include "entry_map.h"
#include "hip_backend.h"
#include "solver.h"

namespace BaSpaCho {

SymProductMap::~SymProductMap() {
  if (dev) hipBackendFreeSymProduct(dev);
}

int64_t SymProductMap::rowDeviceBytes() const {
  return (int64_t)((rowStart.size() + termEntry.size() + termIdx.size() + longRows.size()) * sizeof(int32_t));
}

int64_t SymProductMap::entryDeviceBytes() const {
  return (int64_t)((entRow.size() + entCol.size()) * sizeof(int32_t));
}

static std::string entryName(int64_t k, int64_t i, int64_t j) {
  return "entry " + std::to_string(k) + " at (" + std::to_string(i) + ", " + std::to_string(j) + ")";
}

std::unique_ptr<SymProductMap> createSymProductMap(int64_t n, int64_t nnz, const int64_t* rows, const int64_t* cols,
                                                   int32_t triangle) {
  const int64_t lim = int64_t(1) << 31;
  if (triangle != AssemblyLower && triangle != AssemblyFull) {
    throw std::runtime_error("symmetric product: unknown triangle mode " + std::to_string(triangle) +
                             " (0: lower, 1: full)");
  }
  if (nnz < 0 || nnz >= lim) {
    throw std::runtime_error("symmetric product: nnz = " + std::to_string(nnz) + " is outside [0, 2^31)");
  }
  if (n < 0 || n >= lim) {
    throw std::runtime_error("symmetric product: order n = " + std::to_string(n) + " is outside [0, 2^31)");
  }
  if (nnz > 0 && (rows == nullptr || cols == nullptr)) {
    throw std::runtime_error("symmetric product: the row or column array is NULL");
  }
  std::unique_ptr<SymProductMap> m(new SymProductMap);
  m->triangle = triangle;
  m->n = n;
  m->nnz = nnz;

  // the entries under the assembly's index rules; T = the term count, before anything of its size exists
  m->entRow.resize(nnz);
  m->entCol.resize(nnz);
  int64_t T = 0;
  for (int64_t k = 0; k < nnz; k++) {
    const int64_t i = rows[k], j = cols[k];
    if (i < 0 || i >= n || j < 0 || j >= n) {
      throw std::runtime_error("symmetric product: " + entryName(k, i, j) + " is out of range [0, " +
                               std::to_string(n) + ")");
    }
    if (i < j) {
      if (triangle == AssemblyLower) {
        throw std::runtime_error("symmetric product: " + entryName(k, i, j) +
                                 " has row < col; triangle 'lower' needs row >= col");
      }
      m->entRow[k] = -1;
      m->entCol[k] = -1;
      continue;
    }
    m->entRow[k] = (int32_t)i;
    m->entCol[k] = (int32_t)j;
    m->kept++;
    T += i == j ? 1 : 2;
  }
  if (T >= lim) {
    throw std::runtime_error("symmetric product: the entries give " + std::to_string(T) +
                             " terms (one per diagonal entry, two per off-diagonal one), outside [0, 2^31)");
  }

  // the terms in ascending k, then stably by row: every row list ascends in k
  std::vector<int32_t> tEntry, tRow, tIdx;
  tEntry.reserve(T);
  tRow.reserve(T);
  tIdx.reserve(T);
  for (int64_t k = 0; k < nnz; k++) {
    const int32_t i = m->entRow[k], j = m->entCol[k];
    if (i < 0) continue;
    tEntry.push_back((int32_t)k);
    tRow.push_back(i);
    tIdx.push_back(j);
    if (i != j) {
      tEntry.push_back((int32_t)k);
      tRow.push_back(j);
      tIdx.push_back(i);
    }
  }
  std::vector<int32_t> ids(T), sorted;
  std::iota(ids.begin(), ids.end(), 0);
  const int32_t* key = tRow.data();
  countingSort(ids, sorted, n, [key](int32_t t) { return key[t]; });
  std::vector<int32_t>().swap(ids);
  m->rowStart.assign(n + 1, 0);
  for (int32_t r : tRow) m->rowStart[r + 1]++;
  for (int64_t i = 0; i < n; i++) m->rowStart[i + 1] += m->rowStart[i];
  m->termEntry.resize(T);
  m->termIdx.resize(T);
  for (int64_t t = 0; t < T; t++) {
    m->termEntry[t] = tEntry[sorted[t]];
    m->termIdx[t] = tIdx[sorted[t]];
  }
  for (int64_t i = 0; i < n; i++) {
    const int64_t len = m->rowStart[i + 1] - m->rowStart[i];
    m->maxRow = std::max(m->maxRow, len);
    if (len > kAssemblyLongRun) m->longRows.push_back((int32_t)i);
  }
  return m;
}

std::unique_ptr<SymProductMap> createSymProductMap(const Solver& solver, int64_t nnz, const int64_t* rows,
                                                   const int64_t* cols, int32_t triangle) {
  std::unique_ptr<SymProductMap> m = createSymProductMap(solver.order(), nnz, rows, cols, triangle);
  m->solver = &solver;
  return m;
}

}  // namespace BaSpaCho
