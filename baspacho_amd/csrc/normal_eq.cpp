// Host maps of the normal equations of a sparse Jacobian (normal_eq.h).
#include "normal_eq.h"

#include <algorithm>
#include <numeric>
#include <stdexcept>
#include <string>

#include "solver.h"

namespace BaSpaCho {

std::unique_ptr<NormalEqMap> createNormalEqMap(const Solver& solver, int64_t m, int64_t nnz, const int64_t* rows,
                                               const int64_t* cols) {
  checkBelow2p31("normal equations", "nnz", nnz);
  checkBelow2p31("normal equations", "m", m);
  checkEntryArrays("normal equations", nnz, rows, cols);
  std::unique_ptr<NormalEqMap> q(new NormalEqMap);
  const int64_t n = solver.order();
  q->solver = &solver;
  q->m = m;
  q->n = n;
  q->nnz = nnz;
  q->dataSize = solver.dataSize();
  q->numTiles = (q->dataSize + kAssemblyTile - 1) / kAssemblyTile;

  checkJacobianRange("normal equations", m, n, nnz, rows, cols);

  // vector lists: entries by column and by row, ascending k inside each
  const auto rowOf = [rows](int32_t k) { return rows[k]; };
  const auto colOf = [cols](int32_t k) { return cols[k]; };
  const auto self = [](int32_t k) { return k; };
  q->cols.build(nnz, n, colOf, self, rowOf, false);
  q->rows.build(nnz, m, rowOf, self, colOf, false);

  checkJacobianRepeats("normal equations", m, nnz, rows, cols, q->cols.entry);

  // P before anything of its size exists (sum d = nnz < 2^31, so the sum of d (d + 1) / 2 fits int64)
  int64_t P = 0;
  for (int64_t i = 0; i < m; i++) {
    const int64_t d = q->rows.start[i + 1] - q->rows.start[i];
    P += d * (d + 1) / 2;
  }
  if (P >= (int64_t(1) << 31)) {
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
    for (int32_t x = q->rows.start[i]; x < q->rows.start[i + 1]; x++) {
      const int32_t k2 = q->rows.entry[x];
      const int64_t c2 = q->rows.idx[x];
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
    if (isLongRun(q->adjStart[k + 1] - q->adjStart[k])) q->adjLong.push_back((int32_t)k);
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
  q->tiles.build(P, q->numTiles, [off, srt](int64_t x) { return off[srt[x]]; });
  return q;
}

}  // namespace BaSpaCho
