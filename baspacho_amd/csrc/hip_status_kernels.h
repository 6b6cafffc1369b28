// Status of a factor and damping of the diagonal, on the device.  Work list: hip_backend.hip (GradDev's
// firstLump table, shared with logDet); conventions and numbers: DESIGN.md section 18.
//
// CONVENTIONS.  `data` is the solver's numeric layout.  Both kernels walk the stored diagonal elements
// of the internal scalars g in [g0, g1) (g0 = spanStart[spanBegin], g1 = spanStart[spanEnd]: the range
// need not sit on a lump boundary).  Diagonal element i of lump l is at chainData[chainColPtr[l]] +
// i (w_l + 1), as for logDet.
//
//   factorStatus: a diagonal d is GOOD when d > 0 and d is finite in T, BAD otherwise (NaN, +-Inf, 0,
//                 -0, negative).  The test is made on the bit pattern (0 < bits < bits of +Inf as a
//                 signed integer), so a positive denormal is good whatever the denormal mode.  The
//                 record of matrix q is four 8-byte words at out + 4 q:
//                   w[0]  lowest bad internal scalar in the range, -1 when there is none
//                   w[1]  number of bad diagonals in the range
//                   w[2]  bits of the double minimum over the good diagonals, +inf when there is none
//                   w[3]  bits of the double maximum over the good diagonals, 0.0 when there is none
//                 float widens exactly to double.  An empty range gives {-1, 0, +inf, 0.0}.  `data` is
//                 only read; nothing but the record is written.
//   dampDiagonal: d <- (d * (1 + alpha)) + beta, every operation rounded in T (rmul / radd: contraction
//                 off): t = radd(1, alpha); d = radd(rmul(d, t), beta), bitwise the numpy statement with
//                 T scalars.  alpha = ab[2 q], beta = ab[2 q + 1] are DEVICE values.  In place; no other
//                 element of the buffer is read or written.
//
// BATCH: matrix q = blockIdx.y finds its data through pickData.  No atomics; min, max and the integer
// sum do not depend on the order of reduction, so the record is exact and member q of a batch is
// bitwise the single call.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "hip_grad_kernels.h"
#include "hip_ordered_sum.h"

namespace BaSpaCho {
namespace hipk {

// partial record of one workgroup: `first` is kStatusNone where the workgroup saw no bad diagonal
constexpr int64_t kStatusNone = INT64_MAX;
struct StatusPart {
  int64_t first, count;
  double mn, mx;
};
static_assert(sizeof(StatusPart) == 32, "one partial record is four 8-byte words");

__device__ __forceinline__ bool goodDiagonal(double d) {
  const int64_t b = __double_as_longlong(d);
  return b > 0 && b < 0x7FF0000000000000ll;
}
__device__ __forceinline__ bool goodDiagonal(float d) {
  const int32_t b = __float_as_int(d);
  return b > 0 && b < 0x7F800000;
}

__device__ __forceinline__ void statusMerge(StatusPart& a, const StatusPart& b) {
  a.first = b.first < a.first ? b.first : a.first;
  a.count += b.count;
  a.mn = b.mn < a.mn ? b.mn : a.mn;
  a.mx = b.mx > a.mx ? b.mx : a.mx;
}

// the 256 records of a workgroup into red[0]
__device__ __forceinline__ void statusReduce(StatusPart* red, const StatusPart& mine, int tid) {
  red[tid] = mine;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      StatusPart a = red[tid];
      statusMerge(a, red[tid + s]);
      red[tid] = a;
    }
    __syncthreads();
  }
}

// the lump of diagonal element g: bisection on lumpStart in [lo, hi] (lumpStart[lo] <= g)
__device__ __forceinline__ int32_t lumpOfScalar(const SkelDev& sk, int64_t g, int32_t lo, int32_t hi) {
  while (lo < hi) {
    const int32_t mid = (lo + hi + 1) >> 1;
    if (sk.lumpStart[mid] <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Pass 1: workgroup x scans the diagonal elements of chunk b = b0 + x, [b * kLogDetChunk, ...) clipped
// to [g0, g1), of matrix blockIdx.y into part[blockIdx.y * nParts + x].  firstLump as for logDetPartial.
template <typename T>
__global__ void __launch_bounds__(256) factorStatusPartial(SkelDev sk, const int32_t* __restrict__ firstLump,
                                                           int64_t g0, int64_t g1, int64_t b0, int nParts,
                                                           DataRef<const T> dref, StatusPart* __restrict__ part) {
  __shared__ StatusPart red[256];
  const GP<const T> data = pickData(dref);
  const int tid = threadIdx.x;
  const int64_t b = b0 + blockIdx.x;
  const int32_t lo0 = firstLump[b], hi0 = firstLump[b + 1];
  StatusPart acc{kStatusNone, 0, __longlong_as_double(0x7FF0000000000000ll), 0.0};
#pragma unroll
  for (int m = 0; m < kLogDetChunk / 256; m++) {
    const int64_t g = b * kLogDetChunk + m * 256 + tid;
    if (g >= g0 && g < g1) {
      const int32_t l = lumpOfScalar(sk, g, lo0, hi0);
      const int64_t c0 = sk.lumpStart[l], w = sk.lumpStart[l + 1] - c0;
      const T d = data[sk.chainData[sk.chainColPtr[l]] + (g - c0) * (w + 1)];
      if (goodDiagonal(d)) {
        const double v = (double)d;
        acc.mn = v < acc.mn ? v : acc.mn;
        acc.mx = v > acc.mx ? v : acc.mx;
      } else {
        acc.first = g < acc.first ? g : acc.first;  // (g ascends with m: the first one stays)
        acc.count++;
      }
    }
  }
  statusReduce(red, acc, tid);
  if (tid == 0) part[(int64_t)blockIdx.y * nParts + blockIdx.x] = red[0];
}

// Pass 2: one workgroup per matrix merges its nParts partial records; out + 4 * blockIdx.y.
__global__ void __launch_bounds__(256) factorStatusFinal(const StatusPart* __restrict__ part, int nParts,
                                                         int64_t* __restrict__ out) {
  __shared__ StatusPart red[256];
  const int tid = threadIdx.x;
  const StatusPart* p = part + (int64_t)blockIdx.y * nParts;
  StatusPart acc{kStatusNone, 0, __longlong_as_double(0x7FF0000000000000ll), 0.0};
  for (int b = tid; b < nParts; b += 256) statusMerge(acc, p[b]);
  statusReduce(red, acc, tid);
  if (tid == 0) {
    int64_t* w = out + 4 * (int64_t)blockIdx.y;
    w[0] = red[0].first == kStatusNone ? -1 : red[0].first;
    w[1] = red[0].count;
    w[2] = __double_as_longlong(red[0].mn);
    w[3] = __double_as_longlong(red[0].mx);
  }
}

// One thread per scalar: workgroup x owns the elements [base + 256 x, base + 256 x + 256), base a
// multiple of 256 at or below g0, so a workgroup lies in one chunk of firstLump.  ab: the alpha / beta
// pairs of the members of this launch (ab[2 blockIdx.y], ab[2 blockIdx.y + 1]).
template <typename T>
__global__ void __launch_bounds__(256) dampDiagonal(SkelDev sk, const int32_t* __restrict__ firstLump, int64_t g0,
                                                    int64_t g1, int64_t base, DataRef<T> dref,
                                                    const T* __restrict__ ab) {
  const int64_t first = base + (int64_t)blockIdx.x * 256;
  const int64_t g = first + threadIdx.x;
  if (g < g0 || g >= g1) return;
  const GP<T> data = pickData(dref);
  const int64_t b = first / kLogDetChunk;
  const int32_t l = lumpOfScalar(sk, g, firstLump[b], firstLump[b + 1]);
  const int64_t c0 = sk.lumpStart[l], w = sk.lumpStart[l + 1] - c0;
  const int64_t at = sk.chainData[sk.chainColPtr[l]] + (g - c0) * (w + 1);
  const T alpha = ab[2 * blockIdx.y], beta = ab[2 * blockIdx.y + 1];
  const T t = radd(T(1), alpha);
  data[at] = radd(rmul(data[at], t), beta);
}

}  // namespace hipk
}  // namespace BaSpaCho
