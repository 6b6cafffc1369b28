// Host map of the products with a sparse Jacobian (jac_product.h).
#include "jac_product.h"

#include <algorithm>
#include <numeric>
#include <stdexcept>
#include <string>

#include "solver.h"
#include "sym_product.h"

namespace BaSpaCho {

std::unique_ptr<JacobianProductMap> createJacobianProductMap(const Solver& solver, int64_t m, int64_t nnz,
                                                             const int64_t* rows, const int64_t* cols) {
  checkBelow2p31("jacobian product", "nnz", nnz);
  checkBelow2p31("jacobian product", "m", m);
  checkEntryArrays("jacobian product", nnz, rows, cols);
  std::unique_ptr<JacobianProductMap> q(new JacobianProductMap);
  const int64_t n = solver.order();
  q->solver = &solver;
  q->m = m;
  q->n = n;
  q->nnz = nnz;
  checkJacobianRange("jacobian product", m, n, nnz, rows, cols);
  const auto rowOf = [rows](int32_t k) { return rows[k]; };
  const auto colOf = [cols](int32_t k) { return cols[k]; };
  const auto self = [](int32_t k) { return k; };
  q->cols.build(nnz, n, colOf, self, rowOf, true);
  q->rows.build(nnz, m, rowOf, self, colOf, true);
  checkJacobianRepeats("jacobian product", m, nnz, rows, cols, q->cols.entry);
  q->scalarStart.resize(n + 1);
  std::iota(q->scalarStart.begin(), q->scalarStart.end(), 0);
  return q;
}

void checkJacBlockItems(int64_t items) {
  if (items < 0 || items >= (int64_t(1) << 31)) {
    throw std::runtime_error("jacobian product: the diagonal blocks of J^T J take " + std::to_string(items) +
                             " pairs of entries, outside [0, 2^31)");
  }
}

static void fillJacBlockItems(const JacobianProductMap& map, JacBlockPlan* p);

std::unique_ptr<JacBlockPlan> createJacBlockPlan(const JacobianProductMap& map, const std::vector<int64_t>& blockSizes) {
  std::unique_ptr<JacBlockPlan> p(new JacBlockPlan);
  p->n = map.n;
  int64_t at = 0;
  p->blockStart.push_back(0);
  for (size_t b = 0; b < blockSizes.size(); b++) {
    const int64_t w = blockSizes[b];
    if (w < 1) {
      throw std::runtime_error("jacobian product: param " + std::to_string(b) + " has size " + std::to_string(w));
    }
    if (w > kCgMaxBlockWidth) {
      throw std::runtime_error("jacobian product: param " + std::to_string(b) + " has " + std::to_string(w) +
                               " scalars; block_jacobi takes blocks of at most " + std::to_string(kCgMaxBlockWidth));
    }
    at += w;
    p->blockStart.push_back((int32_t)std::min<int64_t>(at, INT32_MAX));
  }
  if (at != map.n) {
    throw std::runtime_error("jacobian product: the params hold " + std::to_string(at) + " scalars, the order is " +
                             std::to_string(map.n));
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
  fillJacBlockItems(map, p.get());
  return p;
}

// the items of a plan whose block tables (blockStart, blockOff, scalarBlock; -1: a scalar of no block) stand
static void fillJacBlockItems(const JacobianProductMap& map, JacBlockPlan* p) {
  // the positions of the row lists (row by row, ascending entry index inside a row), stably by the block of
  // their column: block by block, ascending row inside a block
  const RunList& rl = map.rows;
  std::vector<int32_t> rowOfPos(map.nnz);
  for (int64_t i = 0; i < map.m; i++) std::fill(rowOfPos.begin() + rl.start[i], rowOfPos.begin() + rl.start[i + 1], (int32_t)i);
  const int32_t* blk = p->scalarBlock.data();
  const int32_t* col = rl.idx.data();
  std::vector<int32_t> ids, byBlock;
  ids.reserve(map.nnz);
  for (int64_t x = 0; x < map.nnz; x++) {
    if (blk[col[x]] >= 0) ids.push_back((int32_t)x);
  }
  const int64_t taken = (int64_t)ids.size();
  countingSort(ids, byBlock, p->numBlocks, [blk, col](int32_t x) { return blk[col[x]]; });
  // a group: the positions of one (block, row); c of them give c (c + 1) / 2 items
  const auto sameGroup = [&](int64_t x, int64_t y) {
    return blk[col[byBlock[x]]] == blk[col[byBlock[y]]] && rowOfPos[byBlock[x]] == rowOfPos[byBlock[y]];
  };
  int64_t items = 0;
  for (int64_t x = 0, g0 = 0; x < taken; x++) {
    if (!sameGroup(g0, x)) g0 = x;
    items += x - g0 + 1;
  }
  checkJacBlockItems(items);
  p->itemStart.assign(p->numBlocks + 1, 0);
  p->itemA.reserve(items);
  p->itemB.reserve(items);
  p->itemPos.reserve(items);
  for (int64_t x = 0, g0 = 0; x < taken; x++) {
    if (!sameGroup(g0, x)) g0 = x;
    const int32_t b = blk[col[byBlock[x]]], s = p->blockStart[b];
    const int32_t w = p->blockWidth.empty() ? p->blockStart[b + 1] - s : p->blockWidth[b];
    p->itemStart[b + 1] += (int32_t)(x - g0 + 1);
    for (int64_t y = g0; y <= x; y++) {
      int32_t px = byBlock[x], py = byBlock[y];
      if (col[px] < col[py]) std::swap(px, py);
      p->itemA.push_back(rl.entry[px]);
      p->itemB.push_back(rl.entry[py]);
      p->itemPos.push_back((col[px] - s) * w + (col[py] - s));
    }
  }
  for (int64_t b = 0; b < p->numBlocks; b++) p->itemStart[b + 1] += p->itemStart[b];
}

std::unique_ptr<JacBlockPlan> createJacBlockPlanOn(const JacobianProductMap& map, const std::vector<int32_t>& first,
                                                   const std::vector<int32_t>& width) {
  std::unique_ptr<JacBlockPlan> p(new JacBlockPlan);
  p->n = map.n;
  p->numBlocks = (int64_t)first.size();
  p->blockStart = first;
  p->blockStart.push_back((int32_t)map.n);
  p->blockWidth = width;
  p->scalarBlock.assign(map.n, -1);
  p->blockOff.assign(p->numBlocks + 1, 0);
  for (int64_t b = 0; b < p->numBlocks; b++) {
    const int64_t w = width[b];
    if (w > kCgMaxBlockWidth) {
      throw std::runtime_error("jacobian product: the block at scalar " + std::to_string(first[b]) + " has " +
                               std::to_string(w) + " scalars; block_jacobi takes blocks of at most " +
                               std::to_string(kCgMaxBlockWidth));
    }
    p->maxWidth = std::max(p->maxWidth, w);
    p->blockOff[b + 1] = p->blockOff[b] + w * w;
    std::fill(p->scalarBlock.begin() + first[b], p->scalarBlock.begin() + first[b] + w, (int32_t)b);
  }
  fillJacBlockItems(map, p.get());
  return p;
}

const JacBlockPlan& jacBlockPlan(const JacobianProductMap& map) {
  if (!map.blocks) {
    const ScalarLocator loc(*map.solver);
    std::vector<int64_t> sizes;
    for (size_t b = 0; b + 1 < loc.userStart.size(); b++) sizes.push_back(loc.userStart[b + 1] - loc.userStart[b]);
    map.blocks = createJacBlockPlan(map, sizes);
  }
  return *map.blocks;
}

}  // namespace BaSpaCho
