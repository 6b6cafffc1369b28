// Assembly of coordinate entries into the numeric layout, and its adjoint.  Map: assembly.{h,cpp}
// (built on the host, uploaded by hip_backend.hip on first use); conventions and numbers: DESIGN.md
// section 14.
//
//   assembleTiles:          out[e] = sum of values[k] over the entries k that map to element e, in
//                           ascending k, starting from +0 (0 where none does).  Every element of the
//                           layout is written exactly once; out is never read.
//   assembleAdjointEntries: grad_values[k] = grad_data[entryOff[k]], 0 where entryOff[k] = -1.
//
// No atomics, no memset, a summation order fixed by the map alone: results are bitwise reproducible,
// and member q = blockIdx.y of a batch is bitwise the single call.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "assembly.h"
#include "hip_device_common.h"

namespace BaSpaCho {
namespace hipk {

constexpr int kAsmTile = (int)kAssemblyTile;
constexpr int kAsmThreads = 256;
constexpr int kAsmAdjPer = 4;  // entries per thread of the adjoint

// lane i's value, in every lane (i wave-uniform)
__device__ __forceinline__ double laneValue(double v, int i) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)b, i), hi = __builtin_amdgcn_readlane((int)(b >> 32), i);
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ float laneValue(float v, int i) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), i));
}

// One workgroup per tile of kAsmTile layout elements, an LDS image of the tile zeroed first.  Runs of
// at most kAssemblyLongRun entries: one lane per destination adds its entries in order.  Longer runs:
// one wave per destination gathers 64 entries at a time and every lane folds them in entry order
// through readlane, so the order stays sequential while the loads go 64 wide.  The image is then
// stored coalesced.  LDS: kAsmTile values of T.
template <typename T>
__global__ void __launch_bounds__(kAsmThreads)
    assembleTiles(int64_t dataSize, const int32_t* __restrict__ tileFirst,
                  const int32_t* __restrict__ tileLongFirst, const int32_t* __restrict__ runStart,
                  const int32_t* __restrict__ runEntry, const uint16_t* __restrict__ destLocal,
                  const int32_t* __restrict__ longDest, DataRef<const T> vref, DataRef<T> oref) {
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
    for (int32_t r = r0; r < r1; r++) s += vals[runEntry[r]];
    img[destLocal[d]] = s;
  }

  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int32_t l0 = tileLongFirst[blockIdx.x], l1 = tileLongFirst[blockIdx.x + 1];
  for (int32_t l = l0 + wave; l < l1; l += kAsmThreads / 64) {
    const int32_t d = __builtin_amdgcn_readfirstlane(longDest[l]);
    const int32_t r0 = __builtin_amdgcn_readfirstlane(runStart[d]);
    const int32_t r1 = __builtin_amdgcn_readfirstlane(runStart[d + 1]);
    T s = T(0);
    for (int32_t c = r0; c < r1; c += 64) {
      const int cnt = r1 - c < 64 ? r1 - c : 64;
      const T v = lane < cnt ? vals[runEntry[c + lane]] : T(0);
      if (cnt == 64) {
#pragma unroll
        for (int i = 0; i < 64; i++) s += laneValue(v, i);
      } else {
        for (int i = 0; i < cnt; i++) s += laneValue(v, i);
      }
    }
    if (lane == 0) img[destLocal[d]] = s;
  }
  __syncthreads();

  const GP<T> out = pickData(oref);
  const int64_t rest = dataSize - base;
  const int len = rest < kAsmTile ? (int)rest : kAsmTile;
  for (int i = tid; i < len; i += kAsmThreads) out[base + i] = img[i];
}

// One thread per kAsmAdjPer entries (strided by the workgroup): coalesced reads of entryOff and
// writes of grad_values, gathered reads of grad_data.
template <typename T>
__global__ void __launch_bounds__(kAsmThreads)
    assembleAdjointEntries(int64_t nnz, const int64_t* __restrict__ entryOff, DataRef<const T> gref,
                           DataRef<T> oref) {
  const GP<const T> g = pickData(gref);
  const GP<T> out = pickData(oref);
  const int64_t k0 = (int64_t)blockIdx.x * (kAsmThreads * kAsmAdjPer) + threadIdx.x;
  int64_t o[kAsmAdjPer];
#pragma unroll
  for (int m = 0; m < kAsmAdjPer; m++) {
    const int64_t k = k0 + m * kAsmThreads;
    o[m] = k < nnz ? entryOff[k] : -1;
  }
#pragma unroll
  for (int m = 0; m < kAsmAdjPer; m++) {
    const int64_t k = k0 + m * kAsmThreads;
    if (k < nnz) out[k] = o[m] >= 0 ? g[o[m]] : T(0);
  }
}

}  // namespace hipk
}  // namespace BaSpaCho
