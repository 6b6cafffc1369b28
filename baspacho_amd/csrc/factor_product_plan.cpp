#include "factor_product_plan.h"

#include <algorithm>

namespace BaSpaCho {

FactorProductPlan buildFactorProductPlan(const CoalescedBlockMatrixSkel& sk) {
  FactorProductPlan p;
  const int64_t nSpans = sk.numSpans(), nLumps = sk.numLumps(), order = sk.order();
  const int64_t nChains = (int64_t)sk.chainRowSpan.size();
  BASPACHO_CHECK_LT(order, (int64_t)INT32_MAX);
  BASPACHO_CHECK_LT(nChains, (int64_t)INT32_MAX);

  // ---- y = L x: the chains of every row span (counting sort by chainRowSpan), ascending column lump
  p.spanChainPtr.assign(nSpans + 1, 0);
  for (int64_t c = 0; c < nChains; c++) p.spanChainPtr[sk.chainRowSpan[c] + 1]++;
  for (int64_t s = 0; s < nSpans; s++) p.spanChainPtr[s + 1] += p.spanChainPtr[s];
  p.spanChain.resize(nChains);
  p.spanChainLump.resize(nChains);
  std::vector<int32_t> next(p.spanChainPtr.begin(), p.spanChainPtr.end() - 1);
  for (int64_t l = 0; l < nLumps; l++) {
    for (int64_t c = sk.chainColPtr[l]; c < sk.chainColPtr[l + 1]; c++) {
      const int32_t at = next[sk.chainRowSpan[c]]++;
      p.spanChain[at] = (int32_t)c;
      p.spanChainLump[at] = (int32_t)l;
    }
  }
  p.rowToSpan.resize(order);
  p.spanLong.assign(nSpans, 0);
  for (int64_t s = 0; s < nSpans; s++) {
    const int64_t last = sk.spanStart[s + 1] - 1;  // the row of the span with the most terms
    int64_t terms = 0, narrow = 0;
    for (int32_t q = p.spanChainPtr[s]; q < p.spanChainPtr[s + 1]; q++) {
      const int64_t l = p.spanChainLump[q];
      terms += std::min(sk.lumpStart[l + 1], last + 1) - sk.lumpStart[l];
      if (sk.lumpStart[l + 1] - sk.lumpStart[l] <= kFactorProductLaneChain) narrow++;
    }
    const bool huge = terms > kFactorProductLongTerms && narrow >= kFactorProductHugeChains &&
                      sk.spanStart[s + 1] - sk.spanStart[s] <= 64;
    p.spanLong[s] = huge ? 2 : terms > kFactorProductLongTerms ? 1 : 0;
    for (int64_t i = sk.spanStart[s]; i <= last; i++) {
      p.rowToSpan[i] = (int32_t)s;
      if (p.spanLong[s] == 1) p.longRows.push_back((int32_t)i);
    }
    if (huge) {
      p.hugeSpans.push_back((int32_t)s);
      p.hugeWidePtr.push_back((int32_t)p.hugeWide.size());
      for (int32_t q = p.spanChainPtr[s]; q < p.spanChainPtr[s + 1]; q++) {
        const int64_t l = p.spanChainLump[q];
        if (sk.lumpStart[l + 1] - sk.lumpStart[l] > kFactorProductLaneChain) p.hugeWide.push_back(q);
      }
    }
  }
  p.hugeWidePtr.push_back((int32_t)p.hugeWide.size());

  // ---- y = L^T x: packed columns of the narrow lumps, strips and row chunks of the others
  for (int64_t l = 0; l < nLumps; l++) {
    const int64_t n0 = sk.lumpStart[l], w = sk.lumpStart[l + 1] - n0;
    const int64_t cBeg = sk.chainColPtr[l], cEnd = sk.chainColPtr[l + 1];
    const int64_t R = sk.chainRowsTillEnd[cEnd - 1];
    BASPACHO_CHECK_LT(R, (int64_t)INT32_MAX);
    if (w <= kFactorProductNarrow) {
      for (int64_t j = 0; j < w; j++) {
        p.smallColLump.push_back((int32_t)l);
        p.smallCol.push_back((int32_t)(n0 + j));
      }
      continue;
    }
    for (int64_t c0 = 0; c0 < w; c0 += kFactorProductStrip) {
      const int64_t nc = std::min(kFactorProductStrip, w - c0), rows = R - c0;
      const int64_t nChunks = std::max<int64_t>(1, (rows + kFactorProductChunkRows - 1) / kFactorProductChunkRows);
      const int64_t per = (rows + nChunks - 1) / nChunks;
      if (nChunks > 1) {
        BASPACHO_CHECK_LT(p.partElems + nChunks * kFactorProductStrip, (int64_t)INT32_MAX);
        p.ltFolds.push_back({(int32_t)(n0 + c0), (int32_t)nc, (int32_t)p.partElems, (int32_t)nChunks});
      }
      int64_t chain = cBeg;
      for (int64_t k = 0; k < nChunks; k++) {
        LtTask t{};
        t.dataOff = sk.chainData[cBeg];
        t.lump = (int32_t)l;
        t.w = (int32_t)w;
        t.c0 = (int32_t)c0;
        t.nc = (int32_t)nc;
        // (a chunk may be empty when a lump has more than 65 000 rows: its partial sums are 0)
        t.rBeg = (int32_t)std::min(R, c0 + k * per);
        t.rEnd = (int32_t)std::min(R, c0 + (k + 1) * per);
        while (chain + 1 < cEnd && sk.chainRowsTillEnd[chain] <= t.rBeg) chain++;
        t.chain = (int32_t)chain;
        t.part = nChunks > 1 ? (int32_t)(p.partElems + k * kFactorProductStrip) : -1;
        p.ltTasks.push_back(t);
      }
      if (nChunks > 1) p.partElems += nChunks * kFactorProductStrip;
    }
  }
  return p;
}

std::vector<int64_t> factorProductPlanRecords(const FactorProductPlan& p) {
  std::vector<int64_t> out = {(int64_t)p.spanChainPtr.size() - 1, (int64_t)p.spanChain.size(),
                              (int64_t)p.longRows.size(),         (int64_t)p.ltTasks.size(),
                              (int64_t)p.ltFolds.size(),          (int64_t)p.smallCol.size(),
                              p.partElems,                        (int64_t)p.hugeSpans.size(),
                              (int64_t)p.hugeWide.size()};
  out.insert(out.end(), p.spanChainPtr.begin(), p.spanChainPtr.end());
  out.insert(out.end(), p.spanChain.begin(), p.spanChain.end());
  out.insert(out.end(), p.spanChainLump.begin(), p.spanChainLump.end());
  out.insert(out.end(), p.spanLong.begin(), p.spanLong.end());
  out.insert(out.end(), p.longRows.begin(), p.longRows.end());
  for (const LtTask& t : p.ltTasks) {
    out.insert(out.end(), {t.dataOff, (int64_t)t.lump, (int64_t)t.w, (int64_t)t.c0, (int64_t)t.nc, (int64_t)t.rBeg,
                           (int64_t)t.rEnd, (int64_t)t.chain, (int64_t)t.part});
  }
  for (const LtFold& f : p.ltFolds) {
    out.insert(out.end(), {(int64_t)f.col0, (int64_t)f.nc, (int64_t)f.part0, (int64_t)f.numChunks});
  }
  out.insert(out.end(), p.smallColLump.begin(), p.smallColLump.end());
  out.insert(out.end(), p.smallCol.begin(), p.smallCol.end());
  out.insert(out.end(), p.hugeSpans.begin(), p.hugeSpans.end());
  out.insert(out.end(), p.hugeWidePtr.begin(), p.hugeWidePtr.end());
  out.insert(out.end(), p.hugeWide.begin(), p.hugeWide.end());
  return out;
}

}  // namespace BaSpaCho
