// Normal equations of a sparse Jacobian on the device.  Maps: normal_eq.{h,cpp} (built on the host,
// each part uploaded by hip_backend.hip on first use); conventions and numbers: DESIGN.md section 17.
//
//   normalEqTiles:          out[e] = sum of values[ka] * values[kb] over the pairs that map to element
//                           e, in ascending ka, starting from +0 (0 where none does).  Every element of
//                           the layout is written exactly once; out is never read.
//   normalEqAdjointEntries: gradValues[k] = sum of gradData[dest] * values[partner] over the terms of
//                           entry k, in list order, from +0.
//   runDotVec:              out[u, j] = sum of values[k] * x[idx, j] over the entries of run u, in list
//                           order, from +0: J^T r over the column lists, J v over the row lists.
//
// Every product is rounded before it is added (rmul / radd: contraction off), so the results are
// bitwise the numpy restatements.  No atomics, no memset, a summation order fixed by the map alone;
// member q = blockIdx.y of a batch is bitwise the single call.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "hip_assembly_kernels.h"
#include "normal_eq.h"

namespace BaSpaCho {
namespace hipk {

constexpr int kNeqWavesPerWg = kAsmThreads / 64;

// a * b and a + b as two roundings: the compiler contracts a * b + c into one fma by default, and
// the pragma keeps both operations out of it
template <typename T>
__device__ __forceinline__ T rmul(T a, T b) {
#pragma clang fp contract(off)
  return a * b;
}
template <typename T>
__device__ __forceinline__ T radd(T a, T b) {
#pragma clang fp contract(off)
  return a + b;
}

// s + the first cnt lanes' p, one after the other in lane order (cnt wave-uniform)
template <typename T>
__device__ __forceinline__ T foldLanes(T s, T p, int cnt) {
  if (cnt == 64) {
#pragma unroll
    for (int i = 0; i < 64; i++) s = radd(s, laneValue(p, i));
  } else {
    for (int i = 0; i < cnt; i++) s = radd(s, laneValue(p, i));
  }
  return s;
}

// assembleTiles with a product of two gathered values per item: one workgroup per tile of kAsmTile
// layout elements, an LDS image of the tile zeroed first.  Runs of at most kAssemblyLongRun pairs: one
// lane per destination.  Longer runs (a column that many residuals touch, on its diagonal element):
// one wave per destination loads 64 pairs at a time and every lane folds the 64 products in order
// through readlane.  The image is then stored coalesced.  LDS: kAsmTile values of T.
template <typename T>
__global__ void __launch_bounds__(kAsmThreads)
    normalEqTiles(int64_t dataSize, const int32_t* __restrict__ tileFirst,
                  const int32_t* __restrict__ tileLongFirst, const int32_t* __restrict__ runStart,
                  const int32_t* __restrict__ pairA, const int32_t* __restrict__ pairB,
                  const uint16_t* __restrict__ destLocal, const int32_t* __restrict__ longDest,
                  DataRef<const T> vref, DataRef<T> oref) {
  __shared__ T img[kAsmTile];
  const GP<const T> vals = pickData(vref);
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * kAsmTile;
#pragma unroll
  for (int m = 0; m < kAsmTile / kAsmThreads; m++) img[m * kAsmThreads + tid] = T(0);
  __syncthreads();

  const int32_t d0 = tileFirst[blockIdx.x], d1 = tileFirst[blockIdx.x + 1];
  for (int32_t d = d0 + tid; d < d1; d += kAsmThreads) {
    const int32_t r0 = runStart[d], r1 = runStart[d + 1];
    if (r1 - r0 > kAssemblyLongRun) continue;
    T s = T(0);
    for (int32_t r = r0; r < r1; r++) s = radd(s, rmul(vals[pairA[r]], vals[pairB[r]]));
    img[destLocal[d]] = s;
  }

  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int32_t l0 = tileLongFirst[blockIdx.x], l1 = tileLongFirst[blockIdx.x + 1];
  for (int32_t l = l0 + wave; l < l1; l += kNeqWavesPerWg) {
    const int32_t d = __builtin_amdgcn_readfirstlane(longDest[l]);
    const int32_t r0 = __builtin_amdgcn_readfirstlane(runStart[d]);
    const int32_t r1 = __builtin_amdgcn_readfirstlane(runStart[d + 1]);
    T s = T(0);
    for (int32_t c = r0; c < r1; c += 64) {
      const int cnt = r1 - c < 64 ? r1 - c : 64;
      const T p = lane < cnt ? rmul(vals[pairA[c + lane]], vals[pairB[c + lane]]) : T(0);
      s = foldLanes(s, p, cnt);
    }
    if (lane == 0) img[destLocal[d]] = s;
  }
  __syncthreads();

  const GP<T> out = pickData(oref);
  const int64_t rest = dataSize - base;
  const int len = rest < kAsmTile ? (int)rest : kAsmTile;
  for (int i = tid; i < len; i += kAsmThreads) out[base + i] = img[i];
}

// Workgroups [0, shortWgs): one lane per entry, entries with more than kAssemblyLongRun terms left
// out.  Workgroups from shortWgs on: one wave per entry of adjLong, 64 terms loaded at a time and
// folded in order through readlane.  Every entry is written exactly once.
template <typename T>
__global__ void __launch_bounds__(kAsmThreads)
    normalEqAdjointEntries(int64_t nnz, int32_t shortWgs, int32_t numLong, const int64_t* __restrict__ adjStart,
                           const int32_t* __restrict__ adjPartner, const int64_t* __restrict__ adjDest,
                           const int32_t* __restrict__ adjLong, DataRef<const T> vref, DataRef<const T> gref,
                           DataRef<T> oref) {
  const GP<const T> vals = pickData(vref);
  const GP<const T> g = pickData(gref);
  const GP<T> out = pickData(oref);
  if ((int32_t)blockIdx.x < shortWgs) {
    const int64_t k = (int64_t)blockIdx.x * kAsmThreads + threadIdx.x;
    if (k >= nnz) return;
    const int64_t t0 = adjStart[k], t1 = adjStart[k + 1];
    if (t1 - t0 > kAssemblyLongRun) return;
    T s = T(0);
    for (int64_t t = t0; t < t1; t++) s = radd(s, rmul(g[adjDest[t]], vals[adjPartner[t]]));
    out[k] = s;
    return;
  }
  const int lane = threadIdx.x & 63;
  const int32_t l =
      __builtin_amdgcn_readfirstlane(((int32_t)blockIdx.x - shortWgs) * kNeqWavesPerWg + (int)(threadIdx.x >> 6));
  if (l >= numLong) return;
  const int32_t k = __builtin_amdgcn_readfirstlane(adjLong[l]);
  const int64_t t0 = adjStart[k], t1 = adjStart[k + 1];
  T s = T(0);
  for (int64_t c = t0; c < t1; c += 64) {
    const int cnt = __builtin_amdgcn_readfirstlane(t1 - c < 64 ? (int)(t1 - c) : 64);
    const T p = lane < cnt ? rmul(g[adjDest[c + lane]], vals[adjPartner[c + lane]]) : T(0);
    s = foldLanes(s, p, cnt);
  }
  if (lane == 0) out[k] = s;
}

// One thread per output (u, j), j fastest: the q vectors of a run sit in adjacent lanes, so x and out
// are touched in rows of q values.  x is [*, q] and out [numRuns, q], both row-major.
template <typename T>
__global__ void __launch_bounds__(kAsmThreads)
    runDotVec(int64_t numRuns, int32_t q, const int32_t* __restrict__ runStart,
              const int32_t* __restrict__ runEntry, const int32_t* __restrict__ runIdx, DataRef<const T> vref,
              DataRef<const T> xref, DataRef<T> oref) {
  const GP<const T> vals = pickData(vref);
  const GP<const T> x = pickData(xref);
  const GP<T> out = pickData(oref);
  const int64_t t = (int64_t)blockIdx.x * kAsmThreads + threadIdx.x;
  if (t >= numRuns * q) return;
  const int64_t u = t / q;
  const int32_t j = (int32_t)(t - u * q);
  T s = T(0);
  for (int32_t e = runStart[u]; e < runStart[u + 1]; e++) {
    s = radd(s, rmul(vals[runEntry[e]], x[(int64_t)runIdx[e] * q + j]));
  }
  out[t] = s;
}

}  // namespace hipk
}  // namespace BaSpaCho
