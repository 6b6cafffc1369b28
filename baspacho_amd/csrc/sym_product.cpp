// Host map of the products with a symmetric matrix given as entries (sym_product.h).
#include "sym_product.h"

#include <algorithm>
#include <numeric>
#include <stdexcept>
#include <string>
#include <utility>

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

// ---- the built-in preconditioners of the conjugate gradient --------------------
std::unique_ptr<CgPrecondPlan> createCgPrecondPlan(const SymProductMap& map, int32_t kind,
                                                   const std::vector<int64_t>& blockSizes) {
  if (kind != CgJacobi && kind != CgBlockJacobi) {
    throw std::runtime_error("cg preconditioner: unknown kind " + std::to_string(kind) +
                             " (1: jacobi, 2: block_jacobi)");
  }
  std::unique_ptr<CgPrecondPlan> p(new CgPrecondPlan);
  p->kind = kind;
  p->n = map.n;
  if (kind == CgJacobi) {
    p->blockStart.resize(map.n + 1);
    std::iota(p->blockStart.begin(), p->blockStart.end(), 0);
  } else {
    int64_t at = 0;
    p->blockStart.push_back(0);
    for (size_t b = 0; b < blockSizes.size(); b++) {
      const int64_t w = blockSizes[b];
      if (w < 1) throw std::runtime_error("cg preconditioner: param " + std::to_string(b) + " has size " + std::to_string(w));
      if (w > kCgMaxBlockWidth) {
        throw std::runtime_error("cg preconditioner: param " + std::to_string(b) + " has " + std::to_string(w) +
                                 " scalars; block_jacobi takes blocks of at most " +
                                 std::to_string(kCgMaxBlockWidth));
      }
      at += w;
      p->blockStart.push_back((int32_t)std::min<int64_t>(at, INT32_MAX));
    }
    if (at != map.n) {
      throw std::runtime_error("cg preconditioner: the params hold " + std::to_string(at) + " scalars, the order is " +
                               std::to_string(map.n));
    }
  }
  p->numBlocks = (int64_t)p->blockStart.size() - 1;
  p->scalarBlock.resize(map.n);
  p->blockOff.assign(p->numBlocks + 1, 0);
  for (int64_t b = 0; b < p->numBlocks; b++) {
    const int64_t w = p->blockStart[b + 1] - p->blockStart[b];
    p->maxWidth = std::max(p->maxWidth, w);
    p->blockOff[b + 1] = p->blockOff[b] + w * w;
    std::fill(p->scalarBlock.begin() + p->blockStart[b], p->scalarBlock.begin() + p->blockStart[b + 1], (int32_t)b);
  }
  // the kept entries inside a diagonal block, in ascending entry index, then stably by block
  std::vector<int32_t> items;
  for (int64_t k = 0; k < map.nnz; k++) {
    const int32_t i = map.entRow[k], j = map.entCol[k];
    if (i >= 0 && p->scalarBlock[i] == p->scalarBlock[j]) items.push_back((int32_t)k);
  }
  RunList runs;
  const auto entryOf = [&](int32_t t) { return items[t]; };
  runs.build((int64_t)items.size(), p->numBlocks, [&](int32_t t) { return p->scalarBlock[map.entRow[items[t]]]; },
             entryOf,
             [&](int32_t t) {
               const int32_t k = items[t], b = p->scalarBlock[map.entRow[k]], s = p->blockStart[b];
               return (map.entRow[k] - s) * (p->blockStart[b + 1] - s) + (map.entCol[k] - s);
             },
             false);
  p->itemStart = std::move(runs.start);
  p->itemEntry = std::move(runs.entry);
  p->itemPos = std::move(runs.idx);
  return p;
}

const CgPrecondPlan& cgPrecondPlan(const SymProductMap& map, int32_t kind) {
  if (kind != CgJacobi && kind != CgBlockJacobi) {
    throw std::runtime_error("cg preconditioner: unknown kind " + std::to_string(kind) +
                             " (1: jacobi, 2: block_jacobi)");
  }
  if (!map.cgPlans[kind]) {
    std::vector<int64_t> sizes;
    if (kind == CgBlockJacobi) {
      if (map.solver == nullptr) throw std::runtime_error("cg preconditioner: the map has no solver to take params from");
      const ScalarLocator loc(*map.solver);
      for (size_t b = 0; b + 1 < loc.userStart.size(); b++) sizes.push_back(loc.userStart[b + 1] - loc.userStart[b]);
    }
    map.cgPlans[kind] = createCgPrecondPlan(map, kind, sizes);
  }
  return *map.cgPlans[kind];
}

// ---- the factorised sparse approximate inverse ----------------------------------
void checkCgFsaiSizes(int64_t elems, int64_t items) {
  const int64_t lim = int64_t(1) << 31;
  if (elems < 0 || elems >= lim) {
    throw std::runtime_error("cg preconditioner: fsai has " + std::to_string(elems) +
                             " elements of G, outside [0, 2^31)");
  }
  if (items < 0 || items >= lim) {
    throw std::runtime_error("cg preconditioner: fsai has " + std::to_string(items) +
                             " items (one per kept entry and row of G that holds both its scalars), outside [0, 2^31)");
  }
}

std::unique_ptr<CgFsaiPlan> createCgFsaiPlan(const SymProductMap& map) {
  std::unique_ptr<CgFsaiPlan> p(new CgFsaiPlan);
  const int64_t n = map.n;
  p->n = n;
  // the kept entries by (row, col): two stable counting sorts, the minor key first
  std::vector<int32_t> kept, byCol, sorted;
  for (int64_t k = 0; k < map.nnz; k++) {
    if (map.entRow[k] >= 0) kept.push_back((int32_t)k);
  }
  countingSort(kept, byCol, n, [&](int32_t k) { return map.entCol[k]; });
  countingSort(byCol, sorted, n, [&](int32_t k) { return map.entRow[k]; });
  std::vector<int32_t>().swap(byCol);

  // the pattern: the distinct columns j < i of row i ascending, the last kCgFsaiMaxRow - 1 of them, then i
  p->rowStart.assign(n + 1, 0);
  {
    size_t x = 0;
    std::vector<int32_t> row;
    for (int64_t i = 0; i < n; i++) {
      row.clear();
      for (; x < sorted.size() && map.entRow[sorted[x]] == i; x++) {
        const int32_t j = map.entCol[sorted[x]];
        if (j < i && (row.empty() || row.back() != j)) row.push_back(j);
      }
      const size_t first = row.size() > (size_t)(kCgFsaiMaxRow - 1) ? row.size() - (size_t)(kCgFsaiMaxRow - 1) : 0;
      const int64_t w = (int64_t)(row.size() - first) + 1;
      if ((int64_t)p->cols.size() + w >= (int64_t(1) << 31)) checkCgFsaiSizes((int64_t)p->cols.size() + w, 0);
      p->cols.insert(p->cols.end(), row.begin() + first, row.end());
      p->cols.push_back((int32_t)i);
      p->rowStart[i + 1] = (int32_t)p->cols.size();
      p->maxWidth = std::max(p->maxWidth, w);
    }
  }
  const int64_t elems = p->elems();
  std::vector<int32_t> rowOf(elems);
  for (int64_t i = 0; i < n; i++) std::fill(rowOf.begin() + p->rowStart[i], rowOf.begin() + p->rowStart[i + 1], (int32_t)i);

  // the columns: the elements of G are given row by row, so every column list ascends in the row
  p->colRuns.build(elems, n, [&](int32_t e) { return p->cols[e]; }, [](int32_t e) { return e; },
                   [&](int32_t e) { return rowOf[e]; }, true);
  p->chunkLongFirst.assign((n + 1023) / 1024 + 1, 0);
  for (int32_t u : p->colRuns.longRuns) p->chunkLongFirst[u / 1024 + 1]++;
  for (size_t c = 0; c + 1 < p->chunkLongFirst.size(); c++) p->chunkLongFirst[c + 1] += p->chunkLongFirst[c];

  // the sorted entries of row a are sorted[rowPtr[a] .. rowPtr[a + 1]), ascending in the column: those at (a, b)
  // by bisection
  std::vector<int64_t> rowPtr(n + 1, 0);
  for (int32_t k : sorted) rowPtr[map.entRow[k] + 1]++;
  for (int64_t i = 0; i < n; i++) rowPtr[i + 1] += rowPtr[i];
  const auto entriesAt = [&](int32_t a, int32_t b) {
    const int32_t* first = sorted.data() + rowPtr[a];
    const int32_t* last = sorted.data() + rowPtr[a + 1];
    const int32_t* lo = std::lower_bound(first, last, b, [&](int32_t k, int32_t col) { return map.entCol[k] < col; });
    const int32_t* hi = std::upper_bound(lo, last, b, [&](int32_t col, int32_t k) { return col < map.entCol[k]; });
    return std::make_pair(lo, hi);
  };
  // the positions of row i, at most 528 of them: f(la w + lb, the entries at (S_i[la], S_i[lb]))
  const auto rowPositions = [&](int64_t i, auto f) {
    const int32_t* s = p->cols.data() + p->rowStart[i];
    const int32_t w = p->rowStart[i + 1] - p->rowStart[i];
    for (int32_t la = 0; la < w; la++) {
      for (int32_t lb = 0; lb <= la; lb++) f(la * w + lb, entriesAt(s[la], s[lb]));
    }
  };
  // the item count from the positions and how often each is given, before anything of its size
  int64_t items = 0;
  for (int64_t i = 0; i < n; i++) {
    rowPositions(i, [&](int32_t, std::pair<const int32_t*, const int32_t*> r) { items += r.second - r.first; });
  }
  checkCgFsaiSizes(elems, items);

  // the items row by row, then in ascending entry index, then stably by row again
  std::vector<int32_t> itEntry, itRow, itPos;
  itEntry.reserve(items);
  itRow.reserve(items);
  itPos.reserve(items);
  for (int64_t i = 0; i < n; i++) {
    rowPositions(i, [&](int32_t pos, std::pair<const int32_t*, const int32_t*> r) {
      for (const int32_t* x = r.first; x != r.second; x++) {
        itEntry.push_back(*x);
        itRow.push_back((int32_t)i);
        itPos.push_back(pos);
      }
    });
  }
  std::vector<int32_t>().swap(sorted);
  std::vector<int32_t> ids(items), byEntry;
  std::iota(ids.begin(), ids.end(), 0);
  countingSort(ids, byEntry, map.nnz, [&](int32_t t) { return itEntry[t]; });
  std::vector<int32_t>().swap(ids);
  RunList runs;
  runs.build(items, n, [&](int32_t t) { return itRow[byEntry[t]]; }, [&](int32_t t) { return itEntry[byEntry[t]]; },
             [&](int32_t t) { return itPos[byEntry[t]]; }, false);
  p->itemStart = std::move(runs.start);
  p->itemEntry = std::move(runs.entry);
  p->itemPos = std::move(runs.idx);
  return p;
}

const CgFsaiPlan& cgFsaiPlan(const SymProductMap& map) {
  if (!map.cgFsai) map.cgFsai = createCgFsaiPlan(map);
  return *map.cgFsai;
}

}  // namespace BaSpaCho
