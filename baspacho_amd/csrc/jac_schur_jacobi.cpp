// Host plan of the block diagonal of the reduced matrix S (jac_schur.h): the (eliminated
// param, kept param) pairs with their rows and dense records, the pseudo-pairs of the free rows, the chunks.
// Built from the JacSchurMap's lists alone -- two passes over the rows and two stable counting sorts -- so that it
// never needs the kept item plan.  No device work.
#include <algorithm>
#include <stdexcept>
#include <string>

#include "jac_schur.h"
#include "sym_product.h"

namespace BaSpaCho {

std::unique_ptr<JacSchurJacobiPlan> createJacSchurJacobiPlan(const JacSchurMap& map) {
  const int64_t numBlocks = (int64_t)map.keptWidth.size(), m = map.m, numElim = map.numElim;
  for (int64_t b = 0; b < numBlocks; b++) {
    if (map.keptWidth[b] > kCgMaxBlockWidth) {
      throw std::runtime_error("jacobian schur: kept param " + std::to_string(map.keptParam[b]) + " has " +
                               std::to_string(map.keptWidth[b]) + " scalars; schur_jacobi takes params of at most " +
                               std::to_string(kCgMaxBlockWidth));
    }
  }
  const RunList &rk = map.rowsKept, &re = map.rowsElim;
  // the group of row i, from its first eliminated entry (-1: a free row)
  const auto groupOf = [&](int64_t i) -> int32_t {
    const int32_t x = re.start[i];
    if (x == re.start[i + 1]) return -1;
    return (int32_t)(std::upper_bound(map.elimOff.begin(), map.elimOff.end(), re.idx[x]) - map.elimOff.begin()) - 1;
  };
  // f(i, b, e) for every (row, kept param of one of its entries), the params of a row in the order they first occur
  std::vector<int32_t> seen(numBlocks, -1);
  const auto eachTouch = [&](auto f) {
    std::fill(seen.begin(), seen.end(), -1);
    for (int64_t i = 0; i < m; i++) {
      if (rk.start[i] == rk.start[i + 1]) continue;
      const int32_t e = groupOf(i);
      for (int32_t x = rk.start[i]; x < rk.start[i + 1]; x++) {
        const int32_t b = map.keptScalarBlock[rk.idx[x]];
        if (seen[b] == (int32_t)i) continue;
        seen[b] = (int32_t)i;
        f((int32_t)i, b, e);
      }
    }
  };
  const auto recWidth = [&](int32_t b, int32_t e) {
    return (int64_t)map.keptWidth[b] + (e >= 0 ? map.elimOff[e + 1] - map.elimOff[e] : 0);
  };
  // pass 1: the counts, checked before anything of their size is allocated
  int64_t numRows = 0, numRec = 0;
  eachTouch([&](int32_t, int32_t b, int32_t e) {
    numRows++;
    numRec += recWidth(b, e);
  });
  checkBelow2p31("jacobian schur", "the pair-row count of schur_jacobi", numRows);
  checkBelow2p31("jacobian schur", "the record size of schur_jacobi", numRec);

  std::unique_ptr<JacSchurJacobiPlan> p(new JacSchurJacobiPlan);
  p->numBlocks = numBlocks;
  p->blockOff.assign(numBlocks + 1, 0);
  for (int64_t b = 0; b < numBlocks; b++) {
    p->blockOff[b + 1] = p->blockOff[b] + (int64_t)map.keptWidth[b] * map.keptWidth[b];
  }
  // pass 2: the pair-rows in ascending row, then sorted stably by e (the free rows last) and by b
  std::vector<int32_t> tRow, tBlock, tElim, ids(numRows), byElim, sorted;
  tRow.reserve(numRows);
  tBlock.reserve(numRows);
  tElim.reserve(numRows);
  eachTouch([&](int32_t i, int32_t b, int32_t e) {
    tRow.push_back(i);
    tBlock.push_back(b);
    tElim.push_back(e >= 0 ? e : (int32_t)numElim);
  });
  for (int64_t t = 0; t < numRows; t++) ids[t] = (int32_t)t;
  countingSort(ids, byElim, numElim + 1, [&](int32_t t) { return tElim[t]; });
  countingSort(byElim, sorted, numBlocks, [&](int32_t t) { return tBlock[t]; });

  // the pairs, the pair-rows and the records
  p->rowOf.resize(numRows);
  p->rec.assign(numRec, -1);
  p->blockPair.assign(numBlocks + 1, 0);
  int64_t recAt = 0;
  int32_t prevB = -1, prevE = -1, rowsInPair = 0;
  for (int64_t x = 0; x < numRows; x++) {
    const int32_t t = sorted[x], i = tRow[t], b = tBlock[t], e = tElim[t];
    const bool pseudo = e == (int32_t)numElim;
    if (b != prevB || e != prevE || (pseudo && rowsInPair == kSchurJacobiChunk)) {
      p->pairElim.push_back(pseudo ? -1 : e);
      p->pairRow.push_back((int32_t)x);
      p->pairRec.push_back((int32_t)recAt);
      p->blockPair[b + 1]++;
      (pseudo ? p->numPseudo : p->numReal)++;
      prevB = b;
      prevE = e;
      rowsInPair = 0;
    }
    rowsInPair++;
    p->rowOf[x] = i;
    const int32_t wb = map.keptWidth[b], c0 = map.keptBlockStart[b];
    for (int32_t y = rk.start[i]; y < rk.start[i + 1]; y++) {
      const int32_t c = rk.idx[y];
      if (map.keptScalarBlock[c] == b) p->rec[recAt + (c - c0)] = rk.entry[y];
    }
    if (!pseudo) {
      const int32_t l0 = map.elimOff[e];
      for (int32_t y = re.start[i]; y < re.start[i + 1]; y++) p->rec[recAt + wb + (re.idx[y] - l0)] = re.entry[y];
    }
    recAt += recWidth(b, pseudo ? -1 : e);
  }
  p->pairRow.push_back((int32_t)numRows);
  p->pairRec.push_back((int32_t)numRec);
  for (int64_t b = 0; b < numBlocks; b++) p->blockPair[b + 1] += p->blockPair[b];

  // the chunks
  p->blockChunk.assign(numBlocks + 1, 0);
  p->chunkPart.push_back(0);
  for (int64_t b = 0; b < numBlocks; b++) {
    const int64_t tri = (int64_t)map.keptWidth[b] * (map.keptWidth[b] + 1) / 2;
    for (int32_t q0 = p->blockPair[b]; q0 < p->blockPair[b + 1]; q0 += kSchurJacobiChunk) {
      p->chunkPair.push_back(q0);
      p->chunkBlock.push_back((int32_t)b);
      p->chunkPart.push_back(p->chunkPart.back() + tri);
    }
    p->blockChunk[b + 1] = (int32_t)p->chunkBlock.size();
  }
  p->chunkPair.push_back((int32_t)p->numPairs());
  return p;
}

const JacSchurJacobiPlan& jacSchurJacobiPlan(const JacSchurMap& map) {
  if (!map.schurJacobi) map.schurJacobi = createJacSchurJacobiPlan(map);
  return *map.schurJacobi;
}

}  // namespace BaSpaCho
