// Host map of the products with a symmetric matrix given as entries (sym_product.h).
#include "sym_product.h"

#include <algorithm>
#include <numeric>
#include <stdexcept>
#include <string>

#include "solver.h"

namespace BaSpaCho {

std::unique_ptr<SymProductMap> createSymProductMap(int64_t n, int64_t nnz, const int64_t* rows, const int64_t* cols,
                                                   int32_t triangle) {
  const int64_t lim = int64_t(1) << 31;
  if (triangle != AssemblyLower && triangle != AssemblyFull) {
    throw std::runtime_error("symmetric product: unknown triangle mode " + std::to_string(triangle) +
                             " (0: lower, 1: full)");
  }
  checkBelow2p31("symmetric product", "nnz", nnz);
  checkBelow2p31("symmetric product", "order n", n);
  checkEntryArrays("symmetric product", nnz, rows, cols);
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
  m->rows.build(T, n, [&](int32_t t) { return tRow[t]; }, [&](int32_t t) { return tEntry[t]; },
                [&](int32_t t) { return tIdx[t]; }, true);
  return m;
}

std::unique_ptr<SymProductMap> createSymProductMap(const Solver& solver, int64_t nnz, const int64_t* rows,
                                                   const int64_t* cols, int32_t triangle) {
  std::unique_ptr<SymProductMap> m = createSymProductMap(solver.order(), nnz, rows, cols, triangle);
  m->solver = &solver;
  return m;
}

}  // namespace BaSpaCho
