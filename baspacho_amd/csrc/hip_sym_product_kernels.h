// Products with a symmetric matrix given as coordinate entries, on the device.  Map: sym_product.{h,cpp}
// (built on the host, each part uploaded by hip_extensions.hip on first use); conventions and numbers:
// DESIGN.md section 21.
//
//   symProductMv:    out[i, j] = sum of values[k] * x[idx, j] over the terms (k, idx) of row i, in list
//                    order, from +0 (+0 for a row without terms).  Every element of out is written
//                    exactly once; out is never read.
//   symProductOuter: out[k] = sum over j ascending of g[r, j] * x[c, j] (+ g[c, j] * x[r, j] when
//                    r != c), (r, c) the position of entry k; 0 for a skipped entry.
//
// x, g and out of symProductMv are [n, q] row-major.  Every product is rounded before it is added (rmul /
// radd: contraction off), so the results are bitwise the numpy restatements.  No atomics, no memset, no
// LDS, a summation order fixed by the map alone; member b = blockIdx.y of a batch is bitwise the single
// call.  Accesses are one element wide: the operands need the alignment of their element type only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "hip_normal_eq_kernels.h"
#include "sym_product.h"

namespace BaSpaCho {
namespace hipk {

// Workgroups [0, shortWgs): one thread per output (i, j), j fastest (runDotVec's shape: the q vectors of
// a row sit in adjacent lanes), rows with more than kAssemblyLongRun terms left out.  Workgroups from
// shortWgs on: one wave per (long row, j), j fastest; it loads 64 terms at a time, one per lane -- the
// entry and x indices coalesced, the values and x gathered 64 wide instead of one after the other -- and
// every lane folds the 64 products in lane order through readlane: the same sequential sum.
template <typename T>
__global__ void __launch_bounds__(kAsmThreads)
    symProductMv(int64_t n, int32_t q, int32_t shortWgs, int64_t numLongWaves, const int32_t* __restrict__ rowStart,
                 const int32_t* __restrict__ termEntry, const int32_t* __restrict__ termIdx,
                 const int32_t* __restrict__ longRows, DataRef<const T> vref, DataRef<const T> xref,
                 DataRef<T> oref) {
  const GP<const T> vals = pickData(vref);
  const GP<const T> x = pickData(xref);
  const GP<T> out = pickData(oref);
  if ((int32_t)blockIdx.x < shortWgs) {
    const int64_t t = (int64_t)blockIdx.x * kAsmThreads + threadIdx.x;
    if (t >= n * q) return;
    const int64_t i = t / q;
    const int32_t j = (int32_t)(t - i * q);
    const int32_t e0 = rowStart[i], e1 = rowStart[i + 1];
    if (e1 - e0 > kAssemblyLongRun) return;
    T s = T(0);
    for (int32_t e = e0; e < e1; e++) s = radd(s, rmul(vals[termEntry[e]], x[(int64_t)termIdx[e] * q + j]));
    out[t] = s;
    return;
  }
  const int lane = threadIdx.x & 63;
  const int64_t w = ((int64_t)blockIdx.x - shortWgs) * kNeqWavesPerWg + (int)(threadIdx.x >> 6);
  if (w >= numLongWaves) return;
  const int32_t l = __builtin_amdgcn_readfirstlane((int32_t)(w / q));
  const int32_t j = __builtin_amdgcn_readfirstlane((int32_t)(w - (int64_t)l * q));
  const int32_t i = __builtin_amdgcn_readfirstlane(longRows[l]);
  const int32_t e0 = __builtin_amdgcn_readfirstlane(rowStart[i]);
  const int32_t e1 = __builtin_amdgcn_readfirstlane(rowStart[i + 1]);
  T s = T(0);
  for (int32_t c = e0; c < e1; c += 64) {
    const int cnt = e1 - c < 64 ? e1 - c : 64;
    const T p = lane < cnt ? rmul(vals[termEntry[c + lane]], x[(int64_t)termIdx[c + lane] * q + j]) : T(0);
    s = foldLanes(s, p, cnt);
  }
  if (lane == 0) out[(int64_t)i * q + j] = s;
}

// One thread per entry: coalesced reads of the entry lists and writes of out, gathered rows of g and x
template <typename T>
__global__ void __launch_bounds__(kAsmThreads)
    symProductOuter(int64_t nnz, int32_t q, const int32_t* __restrict__ entRow, const int32_t* __restrict__ entCol,
                    DataRef<const T> gref, DataRef<const T> xref, DataRef<T> oref) {
  const GP<const T> g = pickData(gref);
  const GP<const T> x = pickData(xref);
  const GP<T> out = pickData(oref);
  const int64_t k = (int64_t)blockIdx.x * kAsmThreads + threadIdx.x;
  if (k >= nnz) return;
  const int32_t r = entRow[k];
  if (r < 0) {
    out[k] = T(0);
    return;
  }
  const int32_t c = entCol[k];
  const int64_t r0 = (int64_t)r * q, c0 = (int64_t)c * q;
  T s = T(0);
  if (r != c) {
    for (int32_t j = 0; j < q; j++) s = radd(s, radd(rmul(g[r0 + j], x[c0 + j]), rmul(g[c0 + j], x[r0 + j])));
  } else {
    for (int32_t j = 0; j < q; j++) s = radd(s, rmul(g[r0 + j], x[c0 + j]));
  }
  out[k] = s;
}

}  // namespace hipk
}  // namespace BaSpaCho
