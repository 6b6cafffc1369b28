// Reach plans (reach.h): the cut, the reach of a lump, column groups and Gram items.
#include "reach.h"

#include <algorithm>
#include <map>
#include <queue>
#include <stdexcept>
#include <string>

namespace BaSpaCho {

int64_t reachCutLump(const CoalescedBlockMatrixSkel& skel, const std::vector<int64_t>& elimRanges) {
  const int64_t nLumps = skel.numLumps();
  int64_t cut = nLumps;
  for (int64_t l = 0; l < nLumps; l++) {
    if (skel.lumpStart[l + 1] - skel.lumpStart[l] > kReachMaxWidth) {
      cut = l;
      break;
    }
  }
  for (size_t r = 0; r + 1 < elimRanges.size(); r++) {
    if (elimRanges[r] < cut && cut < elimRanges[r + 1]) cut = elimRanges[r];
  }
  return cut;
}

std::vector<int32_t> reachOfLump(const CoalescedBlockMatrixSkel& skel, int64_t lump, int64_t cutLump) {
  std::vector<int32_t> out;
  if (lump >= cutLump) return out;
  // rows lie below their column: every lump found is larger than the one it was found from, so taking
  // the smallest pending lump first visits them in ascending order
  std::priority_queue<int64_t, std::vector<int64_t>, std::greater<int64_t>> pending;
  pending.push(lump);
  while (!pending.empty()) {
    const int64_t l = pending.top();
    pending.pop();
    if (!out.empty() && out.back() == (int32_t)l) continue;
    out.push_back((int32_t)l);
    int64_t last = l;
    for (int64_t c = skel.chainColPtr[l]; c < skel.chainColPtr[l + 1]; c++) {
      const int64_t rl = skel.spanToLump[skel.chainRowSpan[c]];
      if (rl == last || rl >= cutLump) continue;  // (the diagonal block, a repeat, or behind the cut)
      pending.push(rl);
      last = rl;
    }
  }
  return out;
}

ReachPlan buildReachPlan(const CoalescedBlockMatrixSkel& skel, const std::vector<int64_t>& elimRanges,
                         const std::vector<int64_t>& spans, const std::vector<int64_t>& pairRow,
                         const std::vector<int64_t>& pairCol, const std::vector<int64_t>& outOffsets) {
  const int64_t nSpans = skel.numSpans(), nLumps = skel.numLumps(), nQ = (int64_t)spans.size();
  if (pairRow.size() != pairCol.size()) throw std::runtime_error("reach plan: row and column pairs differ in number");
  if (!outOffsets.empty() && outOffsets.size() != pairRow.size() + 1) {
    throw std::runtime_error("reach plan: the output offsets must hold one more entry than there are pairs");
  }
  ReachPlan p;
  p.cutLump = reachCutLump(skel, elimRanges);
  p.cutSpan = skel.lumpToSpan[p.cutLump];
  p.cutScalar = skel.lumpStart[p.cutLump];
  std::map<int64_t, std::pair<int32_t, int32_t>> listOfLump;
  for (int64_t q = 0; q < nQ; q++) {
    const int64_t s = spans[q];
    if (s < 0 || s >= nSpans) {
      throw std::runtime_error("reach plan: span " + std::to_string(s) + " is not in [0, " + std::to_string(nSpans) + ")");
    }
    const int64_t lump = skel.spanToLump[s], width = skel.spanStart[s + 1] - skel.spanStart[s];
    p.querySpan.push_back(s);
    p.queryLump.push_back(lump);
    p.queryCol0.push_back(p.numCols);
    p.queryWidth.push_back(width);
    if (p.numCols + width > (int64_t)INT32_MAX) throw std::runtime_error("reach plan: too many columns");
    if (lump >= p.cutLump) {
      p.queryListBegin.push_back(0);
      p.queryListEnd.push_back(0);
      for (int64_t c = 0; c < width; c++) {
        p.unitCol.push_back(p.numCols + c);
        p.unitRow.push_back(skel.spanStart[s] + c);
      }
    } else {
      auto it = listOfLump.find(lump);
      if (it == listOfLump.end()) {
        const std::vector<int32_t> r = reachOfLump(skel, lump, p.cutLump);
        const int32_t b = (int32_t)p.reachLumps.size();
        p.reachLumps.insert(p.reachLumps.end(), r.begin(), r.end());
        it = listOfLump.emplace(lump, std::make_pair(b, (int32_t)p.reachLumps.size())).first;
      }
      p.queryListBegin.push_back(it->second.first);
      p.queryListEnd.push_back(it->second.second);
      for (int64_t c0 = 0; c0 < width; c0 += kReachCols) {
        ReachGroup g{};
        g.row0 = skel.spanStart[s] + c0;
        g.col0 = (int32_t)(p.numCols + c0);
        g.k = (int32_t)std::min<int64_t>(kReachCols, width - c0);
        g.listBegin = it->second.first;
        g.listEnd = it->second.second;
        g.query = (int32_t)q;
        p.groups.push_back(g);
      }
    }
    p.numCols += width;
  }
  const int64_t order = skel.order();
  for (size_t k = 0; k < pairRow.size(); k++) {
    const int64_t a = pairRow[k], b = pairCol[k];
    if (a < 0 || a >= nQ || b < 0 || b >= nQ) throw std::runtime_error("reach plan: a pair names a query out of range");
    GramItem it{};
    it.colP = (int32_t)p.queryCol0[a];
    it.nP = (int32_t)p.queryWidth[a];
    it.colQ = (int32_t)p.queryCol0[b];
    it.nQ = (int32_t)p.queryWidth[b];
    it.outOff = outOffsets.empty() ? p.outSize : outOffsets[k];
    if (!outOffsets.empty() && outOffsets[k + 1] - outOffsets[k] < (int64_t)it.nP * it.nQ) {
      throw std::runtime_error("reach plan: the output offsets leave block " + std::to_string(k) + " less than its " +
                               std::to_string((int64_t)it.nP * it.nQ) + " elements");
    }
    p.outSize = outOffsets.empty() ? p.outSize + (int64_t)it.nP * it.nQ : std::max(p.outSize, outOffsets[k + 1]);
    it.rangeBegin = (int32_t)p.rangeStart.size();
    int64_t rows = 0, open = -1, openEnd = -1;  // the range being grown
    const auto add = [&](int64_t r0, int64_t r1) {
      if (r0 == openEnd) {
        openEnd = r1;
        return;
      }
      if (open >= 0) {
        p.rangeStart.push_back(open);
        p.rangePrefix.push_back(rows);
        rows += openEnd - open;
      }
      open = r0;
      openEnd = r1;
    };
    int32_t i = p.queryListBegin[a], j = p.queryListBegin[b];
    const int32_t ie = p.queryListEnd[a], je = p.queryListEnd[b];
    while (i < ie && j < je) {
      const int32_t li = p.reachLumps[i], lj = p.reachLumps[j];
      if (li == lj) {
        add(skel.lumpStart[li], skel.lumpStart[li + 1]);
        i++;
        j++;
      } else if (li < lj) {
        i++;
      } else {
        j++;
      }
    }
    if (p.cutLump < nLumps) add(p.cutScalar, order);
    add(-2, -2);  // flush
    it.rangeEnd = (int32_t)p.rangeStart.size();
    it.rows = rows;
    p.items.push_back(it);
  }
  return p;
}

}  // namespace BaSpaCho
