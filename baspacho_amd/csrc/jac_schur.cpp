// Host map of the implicit Schur elimination on a Jacobian's entries (jac_schur.h).
#include "jac_schur.h"

#include <algorithm>
#include <stdexcept>
#include <string>

#include "solver.h"
#include "sym_product.h"

namespace BaSpaCho {

std::unique_ptr<JacSchurMap> createJacSchurMap(const JacobianProductMap& product, int64_t numEliminate,
                                               const int64_t* eliminate) {
  const auto fail = [](const std::string& what) { throw std::runtime_error("jacobian schur: " + what); };
  if (numEliminate < 0 || (numEliminate > 0 && eliminate == nullptr)) fail("the list of eliminated params is NULL");
  if (numEliminate == 0) fail("no param is eliminated; use the plain least squares (lstsq_cg without eliminate)");
  const ScalarLocator loc(*product.solver);
  const int64_t numParams = (int64_t)loc.userStart.size() - 1;
  std::vector<uint8_t> isElim(numParams, 0);
  for (int64_t x = 0; x < numEliminate; x++) {
    const int64_t p = eliminate[x];
    if (p < 0 || p >= numParams) {
      fail("eliminate[" + std::to_string(x) + "] = " + std::to_string(p) + " is out of range [0, " +
           std::to_string(numParams) + ")");
    }
    if (isElim[p]) fail("eliminate[" + std::to_string(x) + "] = " + std::to_string(p) + " is given twice");
    isElim[p] = 1;
  }
  for (int64_t p = 0; p < numParams; p++) {
    const int64_t w = loc.userStart[p + 1] - loc.userStart[p];
    if (isElim[p] && w > kSchurMaxElimWidth) {
      fail("eliminated param " + std::to_string(p) + " has " + std::to_string(w) +
           " scalars; an eliminated param has at most " + std::to_string(kSchurMaxElimWidth));
    }
  }
  if (numEliminate == numParams) fail("every param is eliminated; nothing is kept");

  std::unique_ptr<JacSchurMap> s(new JacSchurMap);
  s->product = &product;
  s->m = product.m;
  s->n = product.n;
  s->nnz = product.nnz;
  const int64_t m = s->m, n = s->n, nnz = s->nnz;
  // the two numberings
  std::vector<int32_t> elimOfParam(numParams, -1), first, width;
  s->keptIndex.assign(n, -1);
  std::vector<int32_t> elimIndex(n, -1), elimOfScalar(n, -1);
  s->elimOff.push_back(0);
  for (int64_t p = 0; p < numParams; p++) {
    const int64_t s0 = loc.userStart[p], s1 = loc.userStart[p + 1];
    if (!isElim[p]) {
      if (s->keptBlockStart.empty()) s->keptBlockStart.push_back(0);
      for (int64_t i = s0; i < s1; i++) {
        s->keptIndex[i] = (int32_t)s->keptScalar.size();
        s->keptScalar.push_back((int32_t)i);
        s->keptScalarBlock.push_back((int32_t)s->keptParam.size());
      }
      s->keptParam.push_back((int32_t)p);
      s->keptFirst.push_back((int32_t)s0);
      s->keptWidth.push_back((int32_t)(s1 - s0));
      s->keptBlockStart.push_back((int32_t)s->keptScalar.size());
      continue;
    }
    elimOfParam[p] = (int32_t)s->elimParam.size();
    for (int64_t i = s0; i < s1; i++) {
      elimIndex[i] = (int32_t)s->elimScalar.size();
      elimOfScalar[i] = elimOfParam[p];
      s->elimScalar.push_back((int32_t)i);
    }
    s->elimParam.push_back((int32_t)p);
    s->elimOff.push_back((int32_t)s->elimScalar.size());
    first.push_back((int32_t)s0);
    width.push_back((int32_t)(s1 - s0));
    s->maxElimWidth = std::max(s->maxElimWidth, s1 - s0);
  }
  s->numElim = (int64_t)s->elimParam.size();
  s->nK = (int64_t)s->keptScalar.size();
  s->nE = (int64_t)s->elimScalar.size();

  // the independence condition, row by row over the product's row lists (entry k, column); rowElim[i]: the
  // eliminated param of row i, or -1
  const RunList& rows = product.rows;
  std::vector<int32_t> rowElim(m, -1), rowOf(nnz), colOf(nnz);
  for (int64_t i = 0; i < m; i++) {
    for (int32_t x = rows.start[i]; x < rows.start[i + 1]; x++) {
      rowOf[rows.entry[x]] = (int32_t)i;
      colOf[rows.entry[x]] = rows.idx[x];
      const int32_t e = elimOfScalar[rows.idx[x]];
      if (e < 0) continue;
      if (rowElim[i] >= 0 && rowElim[i] != e) {
        fail("row " + std::to_string(i) + " has entries in the eliminated params " +
             std::to_string(s->elimParam[std::min(rowElim[i], e)]) + " and " +
             std::to_string(s->elimParam[std::max(rowElim[i], e)]) +
             "; a row may touch one eliminated param only");
      }
      rowElim[i] = e;
    }
  }

  // the lists: the entries of each kind in ascending k, grouped stably
  std::vector<int32_t> keptEntries, elimEntries;
  for (int64_t k = 0; k < nnz; k++) (elimIndex[colOf[k]] >= 0 ? elimEntries : keptEntries).push_back((int32_t)k);
  const int32_t *ke = keptEntries.data(), *ee = elimEntries.data();
  const int32_t *ro = rowOf.data(), *co = colOf.data(), *ki = s->keptIndex.data(), *ei = elimIndex.data();
  const int64_t numKept = (int64_t)keptEntries.size(), numElimEntries = (int64_t)elimEntries.size();
  s->rowsKept.build(numKept, m, [=](int32_t t) { return ro[ke[t]]; }, [=](int32_t t) { return ke[t]; },
                    [=](int32_t t) { return ki[co[ke[t]]]; }, true);
  s->colsKept.build(numKept, s->nK, [=](int32_t t) { return ki[co[ke[t]]]; }, [=](int32_t t) { return ke[t]; },
                    [=](int32_t t) { return ro[ke[t]]; }, true);
  s->rowsElim.build(numElimEntries, m, [=](int32_t t) { return ro[ee[t]]; }, [=](int32_t t) { return ee[t]; },
                    [=](int32_t t) { return ei[co[ee[t]]]; }, true);
  s->colsElim.build(numElimEntries, s->nE, [=](int32_t t) { return ei[co[ee[t]]]; }, [=](int32_t t) { return ee[t]; },
                    [=](int32_t t) { return ro[ee[t]]; }, true);

  // the groups (rows ascending inside each) and the rows of no group
  std::vector<int32_t> grouped;
  for (int64_t i = 0; i < m; i++) (rowElim[i] >= 0 ? grouped : s->freeRows).push_back((int32_t)i);
  const int32_t* re = rowElim.data();
  countingSort(grouped, s->groupRow, s->numElim, [re](int32_t i) { return re[i]; });
  s->groupStart.assign(s->numElim + 1, 0);
  for (int32_t i : grouped) s->groupStart[re[i] + 1]++;
  for (int64_t e = 0; e < s->numElim; e++) {
    s->maxGroup = std::max<int64_t>(s->maxGroup, s->groupStart[e + 1]);
    s->groupStart[e + 1] += s->groupStart[e];
  }

  s->elimBlocks = createJacBlockPlanOn(product, first, width);
  return s;
}

const JacBlockPlan& jacSchurKeptPlan(const JacSchurMap& map) {
  if (!map.keptBlocks) {
    for (size_t b = 0; b < map.keptWidth.size(); b++) {
      if (map.keptWidth[b] > kCgMaxBlockWidth) {
        throw std::runtime_error("jacobian schur: kept param " + std::to_string(map.keptParam[b]) + " has " +
                                 std::to_string(map.keptWidth[b]) + " scalars; block_jacobi takes params of at most " +
                                 std::to_string(kCgMaxBlockWidth));
      }
    }
    map.keptBlocks = createJacBlockPlanOn(*map.product, map.keptFirst, map.keptWidth);
  }
  return *map.keptBlocks;
}

}  // namespace BaSpaCho
