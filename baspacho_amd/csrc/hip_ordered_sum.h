// Device side of the entry maps (entry_map.h): sums of a fixed list of terms in a fixed order, for the
// assembly of coordinate entries (assembly.h), the normal equations of a sparse
// Jacobian (normal_eq.h, section 17) and the products with a matrix given as entries (sym_product.h,
// section 21).  Launched by hip_extensions.hip.
//
//   orderedSumTiles:        out[e] = sum of the terms of the run of layout element e, in list order, from
//                           +0 (0 for an element without a run).  Every element of the layout is written
//                           exactly once; out is never read.  Term of the assembly: values[k]; of the
//                           Hessian: values[ka] * values[kb].
//   orderedSumRuns:         out[u, j] = sum of the terms of run u for vector j, in list order, from +0.
//                           The adjoint of the Hessian (gradData[dest] * values[partner], q = 1), J^T r and
//                           J v over the column and row lists, A x over the row lists (values[k] * x[idx, j]).
//   assembleAdjointEntries: grad_values[k] = grad_data[entryOff[k]], 0 where entryOff[k] = -1.
//   symProductOuter:        out[k] = sum over j ascending of g[r, j] * x[c, j] (+ g[c, j] * x[r, j] when
//                           r != c), (r, c) the position of entry k; 0 for a skipped entry.
//   symProductResidual:     r = b - A x and d = |A| |x| + |b| over the row lists of A x, in one pass with
//                           two accumulators (section 23); without b: d = |A| |x|.
//
// A run of at most kAssemblyLongRun terms is summed by one lane (sumRunByLane); a longer one by a wave
// that loads 64 terms at a time and folds them in lane order through readlane (sumRunByWave): the same
// sequential sum.  Every product is rounded before it is added (rmul / radd: contraction off, here and
// nowhere else), so the results are bitwise the numpy restatements.  No atomics, no memset; member
// blockIdx.y of a batch is bitwise the single call.  Vectors are [*, q] row-major.  Accesses are one
// element wide: the operands need the alignment of their element type only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "assembly.h"
#include "hip_device_common.h"

namespace BaSpaCho {
namespace hipk {

constexpr int kAsmTile = (int)kAssemblyTile;
constexpr int kAsmThreads = 256;
constexpr int kAsmWavesPerWg = kAsmThreads / 64;
constexpr int kAsmAdjPer = 4;  // entries per thread of the assembly's adjoint

// lane i's value, in every lane (i wave-uniform)
__device__ __forceinline__ double laneValue(double v, int i) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)b, i), hi = __builtin_amdgcn_readlane((int)(b >> 32), i);
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ float laneValue(float v, int i) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), i));
}

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

// the value of lane 0's v, in a scalar register
__device__ __forceinline__ int32_t waveUniform(int32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t waveUniform(int64_t v) {
  const int lo = __builtin_amdgcn_readfirstlane((int)v), hi = __builtin_amdgcn_readfirstlane((int)(v >> 32));
  return ((int64_t)hi << 32) | (unsigned)lo;
}

// term(begin) + ... + term(end - 1), a left fold from +0: by one lane ...
template <typename I, typename Term>
__device__ __forceinline__ auto sumRunByLane(I begin, I end, Term term) {
  decltype(term(begin)) s = 0;
  for (I x = begin; x < end; x++) s = radd(s, term(x));
  return s;
}
// ... and by a wave (begin and end wave-uniform): 64 positions loaded at a time, one per lane, folded in
// lane order.  The sum is in every lane.
template <typename I, typename Term>
__device__ __forceinline__ auto sumRunByWave(I begin, I end, int lane, Term term) {
  using T = decltype(term(begin));
  T s = 0;
  for (I c = begin; c < end; c += 64) {
    const int cnt = end - c < 64 ? (int)(end - c) : 64;
    s = foldLanes(s, lane < cnt ? term(c + lane) : T(0), cnt);
  }
  return s;
}

// ---- the terms: bind(q, j) picks the batch member's operands and gives term(x), the rounded term at
// list position x for vector j of q
template <typename T>
struct EntryTerm {  // values[entry[x]]
  const int32_t* __restrict__ entry;
  DataRef<const T> vals;
  __device__ __forceinline__ auto bind(int32_t = 1, int32_t = 0) const {
    const GP<const T> v = pickData(vals);
    const int32_t* __restrict__ e = entry;
    return [=](auto x) { return v[e[x]]; };
  }
};
template <typename T>
struct PairTerm {  // values[pairA[x]] * values[pairB[x]]
  const int32_t* __restrict__ pairA;
  const int32_t* __restrict__ pairB;
  DataRef<const T> vals;
  __device__ __forceinline__ auto bind(int32_t = 1, int32_t = 0) const {
    const GP<const T> v = pickData(vals);
    const int32_t* __restrict__ a = pairA;
    const int32_t* __restrict__ b = pairB;
    return [=](auto x) { return rmul(v[a[x]], v[b[x]]); };
  }
};
template <typename T>
struct AdjointTerm {  // gradData[dest[x]] * values[partner[x]]
  const int64_t* __restrict__ dest;
  const int32_t* __restrict__ partner;
  DataRef<const T> grad, vals;
  __device__ __forceinline__ auto bind(int32_t = 1, int32_t = 0) const {
    const GP<const T> g = pickData(grad), v = pickData(vals);
    const int64_t* __restrict__ d = dest;
    const int32_t* __restrict__ p = partner;
    return [=](auto x) { return rmul(g[d[x]], v[p[x]]); };
  }
};
template <typename T>
struct DotTerm {  // values[entry[x]] * vec[idx[x], j]
  const int32_t* __restrict__ entry;
  const int32_t* __restrict__ idx;
  DataRef<const T> vals, vec;
  __device__ __forceinline__ auto bind(int32_t q, int32_t j) const {
    const GP<const T> v = pickData(vals), w = pickData(vec);
    const int32_t* __restrict__ e = entry;
    const int32_t* __restrict__ i = idx;
    return [=](auto x) { return rmul(v[e[x]], w[(int64_t)i[x] * q + j]); };
  }
};

// One workgroup per tile of kAsmTile layout elements, an LDS image of the tile zeroed first.  The runs
// of the tile's destinations [tileFirst[t], tileFirst[t + 1]) go one per lane, those of its long
// destinations longDest[tileLongFirst[t] .. tileLongFirst[t + 1]) one per wave.  The image is then
// stored coalesced.  LDS: kAsmTile values of T.
template <typename T, typename Term>
__global__ void __launch_bounds__(kAsmThreads)
    orderedSumTiles(int64_t dataSize, const int32_t* __restrict__ tileFirst,
                    const int32_t* __restrict__ tileLongFirst, const int32_t* __restrict__ runStart,
                    const uint16_t* __restrict__ destLocal, const int32_t* __restrict__ longDest, Term terms,
                    DataRef<T> oref) {
  __shared__ T img[kAsmTile];
  const auto term = terms.bind();
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * kAsmTile;
#pragma unroll
  for (int m = 0; m < kAsmTile / kAsmThreads; m++) img[m * kAsmThreads + tid] = T(0);
  __syncthreads();

  const int32_t d0 = tileFirst[blockIdx.x], d1 = tileFirst[blockIdx.x + 1];
  for (int32_t d = d0 + tid; d < d1; d += kAsmThreads) {
    const int32_t r0 = runStart[d], r1 = runStart[d + 1];
    if (isLongRun(r1 - r0)) continue;
    img[destLocal[d]] = sumRunByLane(r0, r1, term);
  }

  const int lane = tid & 63;
  const int wave = waveUniform(tid >> 6);
  const int32_t l0 = tileLongFirst[blockIdx.x], l1 = tileLongFirst[blockIdx.x + 1];
  for (int32_t l = l0 + wave; l < l1; l += kAsmWavesPerWg) {
    const int32_t d = waveUniform(longDest[l]);
    const T s = sumRunByWave(waveUniform(runStart[d]), waveUniform(runStart[d + 1]), lane, term);
    if (lane == 0) img[destLocal[d]] = s;
  }
  __syncthreads();

  const GP<T> out = pickData(oref);
  const int64_t rest = dataSize - base;
  const int len = rest < kAsmTile ? (int)rest : kAsmTile;
  for (int i = tid; i < len; i += kAsmThreads) out[base + i] = img[i];
}

// Output (u, j) at out[u * q + j], the terms of run u at positions [start[u], start[u + 1]).  Workgroups
// [0, shortWgs): one thread per output, j fastest (the q vectors of a run sit in adjacent lanes), the
// runs of longRuns left out.  Workgroups from shortWgs on: one wave per (long run, j), j fastest.
// longRuns lists the runs of more than kAssemblyLongRun terms; NULL: there is no such list, and the lane
// path takes every run whatever its length.  Every output is written exactly once.
template <typename T, typename Term, typename Start>
__global__ void __launch_bounds__(kAsmThreads)
    orderedSumRuns(int64_t numRuns, int32_t q, int32_t shortWgs, int64_t numLongWaves,
                   const Start* __restrict__ start, const int32_t* __restrict__ longRuns, Term terms,
                   DataRef<T> oref) {
  const GP<T> out = pickData(oref);
  if ((int32_t)blockIdx.x < shortWgs) {
    const int64_t t = (int64_t)blockIdx.x * kAsmThreads + threadIdx.x;
    if (t >= numRuns * q) return;
    const int64_t u = t / q;
    const int32_t j = (int32_t)(t - u * q);
    const Start r0 = start[u], r1 = start[u + 1];
    if (longRuns != nullptr && isLongRun(r1 - r0)) return;
    out[t] = sumRunByLane(r0, r1, terms.bind(q, j));
    return;
  }
  const int lane = threadIdx.x & 63;
  const int64_t w = ((int64_t)blockIdx.x - shortWgs) * kAsmWavesPerWg + (int)(threadIdx.x >> 6);
  if (w >= numLongWaves) return;
  const int32_t l = waveUniform((int32_t)(w / q));
  const int32_t j = waveUniform((int32_t)(w - (int64_t)l * q));
  const int32_t u = waveUniform(longRuns[l]);
  const T s = sumRunByWave(waveUniform(start[u]), waveUniform(start[u + 1]), lane, terms.bind(q, j));
  if (lane == 0) out[(int64_t)u * q + j] = s;
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

__device__ __forceinline__ double absValue(double v) { return __builtin_fabs(v); }
__device__ __forceinline__ float absValue(float v) { return __builtin_fabsf(v); }

// The residual of A x = b and its scale over the row lists of a SymProductMap, in
// one pass over the lists with two accumulators: with s the terms rmul(values[k], x[idx, j]) of row i
// and t the terms rmul(|values[k]|, |x[idx, j]|), both folded in list order from +0,
//   kHasB:  r[i, j] = radd(b[i, j], -s) and d[i, j] = radd(|b[i, j]|, t);
//   !kHasB: d[i, j] = t (|A| |x|; b and r are not touched).
// The launch shape is orderedSumRuns' (workgroups [0, shortWgs): one thread per output, the rows of
// longRuns left out; from shortWgs on: one wave per (long row, j), two foldLanes per 64 terms).  Every
// element of r and d is written exactly once and neither is read.
template <typename T, bool kHasB>
__global__ void __launch_bounds__(kAsmThreads)
    symProductResidual(int64_t numRuns, int32_t q, int32_t shortWgs, int64_t numLongWaves,
                       const int32_t* __restrict__ start, const int32_t* __restrict__ longRuns,
                       const int32_t* __restrict__ entry, const int32_t* __restrict__ idx, DataRef<const T> vref,
                       DataRef<const T> xref, DataRef<const T> bref, DataRef<T> rref, DataRef<T> dref) {
  const GP<const T> v = pickData(vref), x = pickData(xref);
  const GP<const T> b = kHasB ? pickData(bref) : GP<const T>(nullptr);
  const GP<T> r = kHasB ? pickData(rref) : GP<T>(nullptr);
  const GP<T> d = pickData(dref);
  T s = 0, t = 0;
  int64_t at;
  if ((int32_t)blockIdx.x < shortWgs) {
    at = (int64_t)blockIdx.x * kAsmThreads + threadIdx.x;
    if (at >= numRuns * q) return;
    const int64_t u = at / q;
    const int32_t j = (int32_t)(at - u * q);
    const int32_t r0 = start[u], r1 = start[u + 1];
    if (isLongRun(r1 - r0)) return;
    for (int32_t p = r0; p < r1; p++) {
      const T a = v[entry[p]], w = x[(int64_t)idx[p] * q + j];
      s = radd(s, rmul(a, w));
      t = radd(t, rmul(absValue(a), absValue(w)));
    }
  } else {
    const int lane = threadIdx.x & 63;
    const int64_t w = ((int64_t)blockIdx.x - shortWgs) * kAsmWavesPerWg + (int)(threadIdx.x >> 6);
    if (w >= numLongWaves) return;
    const int32_t l = waveUniform((int32_t)(w / q));
    const int32_t j = waveUniform((int32_t)(w - (int64_t)l * q));
    const int32_t u = waveUniform(longRuns[l]);
    const int32_t r0 = waveUniform(start[u]), r1 = waveUniform(start[u + 1]);
    for (int32_t c = r0; c < r1; c += 64) {
      const int cnt = r1 - c < 64 ? (int)(r1 - c) : 64;
      T ps = 0, pt = 0;
      if (lane < cnt) {
        const T a = v[entry[c + lane]], xv = x[(int64_t)idx[c + lane] * q + j];
        ps = rmul(a, xv);
        pt = rmul(absValue(a), absValue(xv));
      }
      s = foldLanes(s, ps, cnt);
      t = foldLanes(t, pt, cnt);
    }
    if (lane != 0) return;
    at = (int64_t)u * q + j;
  }
  if (kHasB) {
    const T bv = b[at];
    r[at] = radd(bv, -s);
    d[at] = radd(absValue(bv), t);
  } else {
    d[at] = t;
  }
}

}  // namespace hipk
}  // namespace BaSpaCho
