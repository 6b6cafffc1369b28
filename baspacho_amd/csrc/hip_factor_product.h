// Products with the Cholesky factor, y = L x and y = L^T x (plan in
// factor_product_plan.h).  Launched by hip_extensions.hip.
//
// L: a buffer in the numeric layout; only the stored elements with i >= j are read (never the
// strictly-upper elements of the diagonal blocks).  x, y: order x nRHS, column-major, leading dimensions
// ldx, ldy, internal order.  x and L are only read; every element of y is written exactly once and never
// read.  No atomics, no memset.  The terms of every sum are added in an order that the plan fixes:
// gridDim.y is the batch member and gridDim.z a group of kFpRhs right-hand sides, and neither enters
// the order, so column k of a call is bitwise the call with that column alone and member q of a batch
// is bitwise the single call.  Products are contracted into fma where the compiler does so.
//
//   factorProductLx:     workgroups [0, shortWgs): one lane per row of the short spans, the row's terms
//                        added chain after chain, column after column.  Workgroups from shortWgs on: one
//                        wave per row of longRows.  The chains of the row are taken 64 at a time, one per
//                        lane; a lane adds the terms of its chain if the chain's lump has at most
//                        kFpLaneChain columns, and the wider chains of the 64 are then taken one after the
//                        other by the whole wave, lane t adding the columns t, t + 64, ...  The 64 lane
//                        sums are folded in lane order.
//   factorProductLxSpans: one workgroup of 16 waves per huge span (many chains of narrow lumps, the
//                        camera rows of BAL): see the kernel.
//   factorProductLt:     workgroups [0, numTasks): one LtTask each (a strip of at most 64 columns, one per
//                        lane, and a chunk of rows): wave v adds the rows rBeg + v, rBeg + v + 4, ... in
//                        ascending order, the four wave sums are folded in wave order through LDS.  The
//                        other workgroups: one lane per packed column of the narrow lumps, rows ascending.
//   factorProductLtFold: the partial sums of the split strips, folded in chunk order.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "factor_product_plan.h"
#include "hip_device_common.h"
#include "hip_ordered_sum.h"

namespace BaSpaCho {
namespace hipk {

constexpr int kFpThreads = 256;
constexpr int kFpWaves = kFpThreads / 64;
constexpr int kFpRhs = 4;         // right-hand sides per workgroup (gridDim.z = groups of them)
constexpr int kFpLaneChain = (int)kFactorProductLaneChain;  // long rows: a chain of a lump this narrow is summed by one lane
constexpr int kFpSpanWaves = 16;  // waves of the workgroup of a huge span
constexpr int kFpSpanThreads = 64 * kFpSpanWaves;

// the tables of the plan on the device
struct FactorProductDev {
  const int32_t *spanChainPtr, *spanChain, *spanChainLump, *rowToSpan, *spanLong, *longRows;
  const int32_t *hugeSpans, *hugeWidePtr, *hugeWide;
  const LtTask* ltTasks;
  const LtFold* ltFolds;
  const int32_t *smallColLump, *smallCol;
};

// the operands of one launch: x and y of the members, their leading dimensions, the right-hand sides
template <typename T>
struct FactorProductArgs {
  DataRef<const T> L, x;
  DataRef<T> y;
  int64_t ldx, ldy;
  int32_t nRHS;
};

template <typename T>
__global__ void __launch_bounds__(kFpThreads)
    factorProductLx(FactorProductDev pl, SkelDev sk, int32_t order, int32_t shortWgs, int32_t numLong,
                    FactorProductArgs<T> a) {
  const GP<const T> L = pickData(a.L);
  const GP<const T> x = pickData(a.x);
  const GP<T> y = pickData(a.y);
  const int32_t k0 = (int32_t)blockIdx.z * kFpRhs;
  const int kb = a.nRHS - k0 < kFpRhs ? a.nRHS - k0 : kFpRhs;
  T acc[kFpRhs];
#pragma unroll
  for (int kk = 0; kk < kFpRhs; kk++) acc[kk] = T(0);

  if ((int32_t)blockIdx.x < shortWgs) {
    const int32_t i = (int32_t)blockIdx.x * kFpThreads + (int32_t)threadIdx.x;
    if (i >= order) return;
    const int32_t s = pl.rowToSpan[i];
    if (pl.spanLong[s]) return;
    const int64_t li = i - sk.spanStart[s];
    for (int32_t p = pl.spanChainPtr[s], p1 = pl.spanChainPtr[s + 1]; p < p1; p++) {
      const int32_t l = pl.spanChainLump[p];
      const int64_t n0 = sk.lumpStart[l], w = sk.lumpStart[l + 1] - n0;
      const int64_t cnt = i - n0 + 1 < w ? i - n0 + 1 : w;
      const int64_t off = sk.chainData[pl.spanChain[p]] + li * w;
      for (int64_t j = 0; j < cnt; j++) {
        const T v = L[off + j];
#pragma unroll
        for (int kk = 0; kk < kFpRhs; kk++) {
          if (kk < kb) acc[kk] += v * x[n0 + j + (k0 + kk) * a.ldx];
        }
      }
    }
#pragma unroll
    for (int kk = 0; kk < kFpRhs; kk++) {
      if (kk < kb) y[i + (k0 + kk) * a.ldy] = acc[kk];
    }
    return;
  }

  const int lane = threadIdx.x & 63;
  const int32_t r = waveUniform(((int32_t)blockIdx.x - shortWgs) * kFpWaves + (int32_t)(threadIdx.x >> 6));
  if (r >= numLong) return;
  const int32_t i = waveUniform(pl.longRows[r]);
  const int32_t s = waveUniform(pl.rowToSpan[i]);
  const int64_t li = i - sk.spanStart[s];
  const int32_t p0 = waveUniform(pl.spanChainPtr[s]), p1 = waveUniform(pl.spanChainPtr[s + 1]);
  for (int32_t pg = p0; pg < p1; pg += 64) {
    const int32_t p = pg + lane;
    const bool have = p < p1;
    int64_t n0 = 0, cnt = 0, off = 0, w = 0;
    if (have) {
      const int32_t l = pl.spanChainLump[p];
      n0 = sk.lumpStart[l];
      w = sk.lumpStart[l + 1] - n0;
      cnt = i - n0 + 1 < w ? i - n0 + 1 : w;
      off = sk.chainData[pl.spanChain[p]] + li * w;
    }
    const bool wide = have && w > kFpLaneChain;
    if (have && !wide) {
      for (int64_t j = 0; j < cnt; j++) {
        const T v = L[off + j];
#pragma unroll
        for (int kk = 0; kk < kFpRhs; kk++) {
          if (kk < kb) acc[kk] += v * x[n0 + j + (k0 + kk) * a.ldx];
        }
      }
    }
    unsigned long long mask = __ballot(wide);
    while (mask != 0ull) {
      const int src = __builtin_ctzll(mask);
      mask &= mask - 1ull;
      const int64_t offU = __shfl(off, src), n0U = __shfl(n0, src);
      const int32_t cntU = __shfl((int32_t)cnt, src);
      for (int32_t j = lane; j < cntU; j += 64) {
        const T v = L[offU + j];
#pragma unroll
        for (int kk = 0; kk < kFpRhs; kk++) {
          if (kk < kb) acc[kk] += v * x[n0U + j + (k0 + kk) * a.ldx];
        }
      }
    }
  }
#pragma unroll
  for (int kk = 0; kk < kFpRhs; kk++) {
    if (kk < kb) {
      const T sum = foldLanes(T(0), acc[kk], 64);
      if (lane == 0) y[i + (k0 + kk) * a.ldy] = sum;
    }
  }
}

// One workgroup of kFpSpanWaves waves per huge span (h <= 64 rows).  Lane t of a wave stands for row
// t % h of the span and slot g = t / h of the G = 64 / h slots of the wave (the lanes from G h on idle).
// The chains of the span are taken G at a time, group after group dealt to the waves in turn; slot g
// of a group holds one chain, and its lanes add the terms of their rows if the chain's lump has at
// most kFpLaneChain columns: a wave reads whole blocks of h x w contiguous elements.  The wider chains
// (hugeWide) are then taken one after the other by all waves: the lane of slot g in wave v adds the
// columns v G + g, v G + g + 16 G, ... of its row.  Every lane sum goes to LDS, and the thread of row r
// folds the sums of its row in wave order, slot order.
template <typename T>
__global__ void __launch_bounds__(kFpSpanThreads)
    factorProductLxSpans(FactorProductDev pl, SkelDev sk, FactorProductArgs<T> a) {
  __shared__ T red[kFpSpanWaves][kFpRhs][64];
  const GP<const T> L = pickData(a.L);
  const GP<const T> x = pickData(a.x);
  const GP<T> y = pickData(a.y);
  const int32_t k0 = (int32_t)blockIdx.z * kFpRhs;
  const int kb = a.nRHS - k0 < kFpRhs ? a.nRHS - k0 : kFpRhs;
  T acc[kFpRhs];
#pragma unroll
  for (int kk = 0; kk < kFpRhs; kk++) acc[kk] = T(0);

  const int lane = threadIdx.x & 63;
  const int wave = waveUniform((int32_t)(threadIdx.x >> 6));
  const int32_t s = pl.hugeSpans[blockIdx.x];
  const int64_t i0 = sk.spanStart[s];
  const int32_t h = (int32_t)(sk.spanStart[s + 1] - i0);
  const int32_t G = 64 / h, g = lane / h, li = lane - g * h;
  const bool on = g < G;
  const int64_t i = i0 + li;
  const int32_t p0 = pl.spanChainPtr[s], p1 = pl.spanChainPtr[s + 1];
  for (int32_t pg = p0 + wave * G; pg < p1; pg += kFpSpanWaves * G) {
    const int32_t p = pg + g;
    if (on && p < p1) {
      const int32_t l = pl.spanChainLump[p];
      const int64_t n0 = sk.lumpStart[l], w = sk.lumpStart[l + 1] - n0;
      if (w <= kFpLaneChain) {
        const int64_t cnt = i - n0 + 1 < w ? i - n0 + 1 : w;
        const int64_t off = sk.chainData[pl.spanChain[p]] + li * w;
        for (int64_t j = 0; j < cnt; j++) {
          const T v = L[off + j];
#pragma unroll
          for (int kk = 0; kk < kFpRhs; kk++) {
            if (kk < kb) acc[kk] += v * x[n0 + j + (k0 + kk) * a.ldx];
          }
        }
      }
    }
  }
  for (int32_t q = pl.hugeWidePtr[blockIdx.x], q1 = pl.hugeWidePtr[blockIdx.x + 1]; q < q1; q++) {
    const int32_t p = pl.hugeWide[q];
    const int32_t l = pl.spanChainLump[p];
    const int64_t n0 = sk.lumpStart[l], w = sk.lumpStart[l + 1] - n0;
    if (on) {
      const int64_t cnt = i - n0 + 1 < w ? i - n0 + 1 : w;
      const int64_t off = sk.chainData[pl.spanChain[p]] + li * w;
      for (int64_t j = wave * G + g; j < cnt; j += kFpSpanWaves * G) {
        const T v = L[off + j];
#pragma unroll
        for (int kk = 0; kk < kFpRhs; kk++) {
          if (kk < kb) acc[kk] += v * x[n0 + j + (k0 + kk) * a.ldx];
        }
      }
    }
  }
#pragma unroll
  for (int kk = 0; kk < kFpRhs; kk++) red[wave][kk][lane] = acc[kk];
  __syncthreads();
  if ((int32_t)threadIdx.x >= h) return;
  const int32_t r = (int32_t)threadIdx.x;
#pragma unroll
  for (int kk = 0; kk < kFpRhs; kk++) {
    if (kk < kb) {
      T sum = T(0);
      for (int v = 0; v < kFpSpanWaves; v++) {
        for (int32_t gg = 0; gg < G; gg++) sum += red[v][kk][gg * h + r];
      }
      y[i0 + r + (k0 + kk) * a.ldy] = sum;
    }
  }
}

// part: the partial sums of the split strips, partElems per (member of the launch, right-hand side)
template <typename T>
__global__ void __launch_bounds__(kFpThreads)
    factorProductLt(FactorProductDev pl, SkelDev sk, int32_t numTasks, int32_t numSmall, FactorProductArgs<T> a,
                    T* __restrict__ part, int64_t partElems) {
  __shared__ T red[kFpWaves][kFpRhs][64];
  const GP<const T> L = pickData(a.L);
  const GP<const T> x = pickData(a.x);
  const GP<T> y = pickData(a.y);
  const int32_t k0 = (int32_t)blockIdx.z * kFpRhs;
  const int kb = a.nRHS - k0 < kFpRhs ? a.nRHS - k0 : kFpRhs;
  T acc[kFpRhs];
#pragma unroll
  for (int kk = 0; kk < kFpRhs; kk++) acc[kk] = T(0);

  if ((int32_t)blockIdx.x >= numTasks) {
    // one lane per column of a narrow lump: the rows from the diagonal down, chain after chain
    const int32_t t = ((int32_t)blockIdx.x - numTasks) * kFpThreads + (int32_t)threadIdx.x;
    if (t >= numSmall) return;
    const int32_t l = pl.smallColLump[t], n = pl.smallCol[t];
    const int64_t w = sk.lumpStart[l + 1] - sk.lumpStart[l], j = n - sk.lumpStart[l];
    const int64_t cBeg = sk.chainColPtr[l], cEnd = sk.chainColPtr[l + 1];
    const int64_t base = sk.chainData[cBeg];
    int64_t rowA = 0;
    for (int64_t c = cBeg; c < cEnd; c++) {
      const int64_t rowB = sk.chainRowsTillEnd[c];
      const int64_t g0 = sk.spanStart[sk.chainRowSpan[c]] - rowA;
      for (int64_t r = rowA > j ? rowA : j; r < rowB; r++) {
        const T v = L[base + r * w + j];
#pragma unroll
        for (int kk = 0; kk < kFpRhs; kk++) {
          if (kk < kb) acc[kk] += v * x[g0 + r + (k0 + kk) * a.ldx];
        }
      }
      rowA = rowB;
    }
#pragma unroll
    for (int kk = 0; kk < kFpRhs; kk++) {
      if (kk < kb) y[n + (k0 + kk) * a.ldy] = acc[kk];
    }
    return;
  }

  const LtTask t = pl.ltTasks[blockIdx.x];
  const int lane = threadIdx.x & 63;
  const int wave = waveUniform((int32_t)(threadIdx.x >> 6));
  const int32_t j = t.c0 + lane;
  const bool active = lane < t.nc;
  const int32_t cFirst = waveUniform((int32_t)sk.chainColPtr[t.lump]);
  if (t.rBeg < t.rEnd) {
    int32_t c = t.chain;
    int32_t rowA = c == cFirst ? 0 : waveUniform((int32_t)sk.chainRowsTillEnd[c - 1]);
    for (;;) {
      const int32_t rowB = waveUniform((int32_t)sk.chainRowsTillEnd[c]);
      const int64_t g0 = waveUniform(sk.spanStart[sk.chainRowSpan[c]]) - rowA;
      const int32_t segEnd = rowB < t.rEnd ? rowB : t.rEnd;
      // the first row of this wave at or after the beginning of the segment
      int32_t r = rowA > t.rBeg ? rowA : t.rBeg;
      r += (wave - (r - t.rBeg)) & (kFpWaves - 1);
      for (; r < segEnd; r += kFpWaves) {
        if (active && r >= j) {
          const T v = L[t.dataOff + (int64_t)r * t.w + j];
#pragma unroll
          for (int kk = 0; kk < kFpRhs; kk++) {
            if (kk < kb) acc[kk] += v * x[g0 + r + (k0 + kk) * a.ldx];
          }
        }
      }
      if (rowB >= t.rEnd) break;
      rowA = rowB;
      c++;
    }
  }
#pragma unroll
  for (int kk = 0; kk < kFpRhs; kk++) red[wave][kk][lane] = acc[kk];
  __syncthreads();
  if (wave != 0 || !active) return;
  const int64_t n = sk.lumpStart[t.lump] + j;
#pragma unroll
  for (int kk = 0; kk < kFpRhs; kk++) {
    if (kk < kb) {
      T sum = red[0][kk][lane];
#pragma unroll
      for (int v = 1; v < kFpWaves; v++) sum += red[v][kk][lane];
      if (t.part < 0) {
        y[n + (k0 + kk) * a.ldy] = sum;
      } else {
        part[((int64_t)blockIdx.y * a.nRHS + (k0 + kk)) * partElems + t.part + lane] = sum;
      }
    }
  }
}

// one lane per (split strip, column); gridDim.z = right-hand sides
template <typename T>
__global__ void __launch_bounds__(kFpThreads)
    factorProductLtFold(const LtFold* __restrict__ folds, int32_t numFolds, DataRef<T> yref, int64_t ldy, int32_t nRHS,
                        const T* __restrict__ part, int64_t partElems) {
  const GP<T> y = pickData(yref);
  const int32_t f = ((int32_t)blockIdx.x * kFpThreads + (int32_t)threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (f >= numFolds) return;
  const LtFold fd = folds[f];
  if (lane >= fd.nc) return;
  const int32_t k = (int32_t)blockIdx.z;
  const T* p = part + ((int64_t)blockIdx.y * nRHS + k) * partElems + fd.part0 + lane;
  T sum = p[0];
  for (int32_t c = 1; c < fd.numChunks; c++) sum += p[(int64_t)c * kFactorProductStrip];
  y[fd.col0 + lane + k * ldy] = sum;
}

}  // namespace hipk
}  // namespace BaSpaCho
