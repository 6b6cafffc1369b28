// Error bounds on the device: the column reductions behind the backward error and
// the 1-norm (maxRatio, colMax), and the step kernels of the 1-norm estimate of A^-1 from a factor
// (Solver::invNorm1Estimate; Hager's estimator in Higham's form).  Launched by hip_extensions.hip.
//
// CONVENTIONS.  Arrays of the reductions are [n, q] row-major; vectors of the estimator hold n = order
// values in the solver's internal order (as for solve()).  Matrix blockIdx.y of a batch finds its operands
// through pickData or at a fixed stride.  Every reduction runs in two passes: workgroup x of pass 1 owns
// the kRedChunk rows [x kRedChunk, (x + 1) kRedChunk); thread t takes the rows x kRedChunk + m 256 + t,
// m = 0 .. 3, in this order, and the 256 thread values are folded in LDS (for s = 128 .. 1: entry t < s
// becomes entry t merged with entry t + s); pass 2 is one workgroup per result whose thread t merges the
// partials t, t + 256, ... in this order and folds the same way.  No atomics: sums have one fixed order,
// max and arg-max do not depend on it.  Sums are taken in double for both precisions.
//
// THE STATE RECORD of the estimator: kNormEstWords = 12 8-byte words per matrix,
//   w[0]      bits of est, a double: the estimate so far, the result once the last step has run
//   w[1]      j: the column of the next unit vector (the arg-max of the last z), -1 before the first
//   w[2]      pass: how many vectors x = A^-1 v were measured (1 .. 5; the alt solve is not counted)
//   w[3]      stop reason: 0 running / ran out of schedule, 1 n == 1, 2 repeated sign vector, 3 no
//             increase, 4 pass limit (5), 5 same column again, 6 a non-finite vector
//   w[4]      1 when the value of the alternating vector won, 0 otherwise
//   w[5 .. 9] the j chosen after pass 1 .. 5, -1 where none was chosen
//   w[10]     bits of the alternating vector's value 2 ||x||_1 / (3 n), a double (0.0 for n == 1)
//   w[11]     0
// The step kernels of a stopped matrix (w[3] != 0) leave its record alone and change nothing but its
// work vectors.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "hip_device_common.h"

namespace BaSpaCho {
namespace hipk {

constexpr int kRedThreads = 256;
constexpr int kRedChunk = 1024;  // rows per workgroup of a first pass
constexpr int kNormEstWords = 12;

enum NormEstStop : int64_t {
  NormEstRunning = 0,
  NormEstOrderOne = 1,
  NormEstRepeatedSigns = 2,
  NormEstNoIncrease = 3,
  NormEstPassLimit = 4,
  NormEstSameColumn = 5,
  NormEstNonFinite = 6
};

struct NormEstState {
  double est;
  int64_t j, pass, stop, altWon;
  int64_t jOf[5];
  double alt;
  int64_t zero;
};
static_assert(sizeof(NormEstState) == 8 * kNormEstWords, "the state record is twelve 8-byte words");

// one partial of a reduction: a value and an integer that goes with it (flag or index)
struct RedPart {
  double v;
  int64_t k;
};
static_assert(sizeof(RedPart) == 16, "one partial is two 8-byte words");

__device__ __forceinline__ double redNaN() { return __longlong_as_double(0x7FF8000000000000ll); }
__device__ __forceinline__ double redInf() { return __longlong_as_double(0x7FF0000000000000ll); }
__device__ __forceinline__ bool redFinite(double v) { return __builtin_fabs(v) < redInf(); }

// the merges: a NaN-keeping maximum, a sum with an all-of flag, an arg-max that keeps the lowest index
struct MergeMax {
  __device__ __forceinline__ RedPart operator()(const RedPart& a, const RedPart& b) const {
    if (a.v != a.v || b.v != b.v) return RedPart{redNaN(), 0};
    return RedPart{b.v > a.v ? b.v : a.v, 0};
  }
};
struct MergeSum {
  __device__ __forceinline__ RedPart operator()(const RedPart& a, const RedPart& b) const {
    return RedPart{a.v + b.v, a.k & b.k};
  }
};
struct MergeArgMax {
  // (operands by value: a select between two references keeps both in memory, which cost scratch)
  __device__ __forceinline__ RedPart operator()(RedPart a, RedPart b) const {
    const double av = a.v, bv = b.v;
    const int64_t ak = a.k, bk = b.k;
    const bool takeB = bv > av || (bv == av && bk < ak);
    return RedPart{takeB ? bv : av, takeB ? bk : ak};
  }
};

// the 256 values of a workgroup into red[0]
template <typename Merge>
__device__ __forceinline__ void redFold(RedPart* red, const RedPart& mine, int tid, Merge merge) {
  red[tid] = mine;
  __syncthreads();
  for (int s = kRedThreads / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = merge(red[tid], red[tid + s]);
    __syncthreads();
  }
}

// ---- column reductions -----------------------------------------------------------------------------
// |r| / d of the backward error, in double: NaN when either operand is NaN, 0 when r == 0, +inf when
// d == 0 and r != 0, the quotient otherwise (inf / inf is NaN)
template <typename T>
__device__ __forceinline__ double ratioOf(T r, T d) {
  const double a = __builtin_fabs((double)r), b = (double)d;
  if (a != a || b != b) return redNaN();
  if (a == 0.0) return 0.0;
  if (b == 0.0) return redInf();
  return a / b;
}

// Pass 1 of maxRatio (kRatio: a = r, b = d, start 0) and of colMax (!kRatio: a alone, start -inf):
// workgroup x = p q + j reduces rows of chunk p of column j into part[(blockIdx.y q + j) nParts + p]
template <typename T, bool kRatio>
__global__ void __launch_bounds__(kRedThreads)
    colMaxPartial(int64_t n, int32_t q, int32_t nParts, DataRef<const T> aref, DataRef<const T> bref,
                  RedPart* __restrict__ part) {
  __shared__ RedPart red[kRedThreads];
  const GP<const T> a = pickData(aref);
  const GP<const T> b = kRatio ? pickData(bref) : GP<const T>(nullptr);
  const int tid = threadIdx.x;
  const int64_t p = blockIdx.x / q;
  const int32_t j = (int32_t)(blockIdx.x - p * q);
  RedPart acc{kRatio ? 0.0 : -redInf(), 0};
#pragma unroll
  for (int m = 0; m < kRedChunk / kRedThreads; m++) {
    const int64_t i = p * kRedChunk + m * kRedThreads + tid;
    if (i < n) {
      const int64_t at = i * q + j;
      const double v = kRatio ? ratioOf(a[at], b[at]) : (double)a[at];
      acc = MergeMax()(acc, RedPart{v, 0});
    }
  }
  redFold(red, acc, tid, MergeMax());
  if (tid == 0) part[((int64_t)blockIdx.y * q + j) * nParts + p] = red[0];
}

// Pass 2: workgroup (j, matrix) merges its nParts partials into out[matrix q + j]
__global__ void __launch_bounds__(kRedThreads)
    colMaxFinal(int32_t q, int32_t nParts, double start, const RedPart* __restrict__ part,
                double* __restrict__ out) {
  __shared__ RedPart red[kRedThreads];
  const int tid = threadIdx.x;
  const int64_t slot = (int64_t)blockIdx.y * q + blockIdx.x;
  const RedPart* p = part + slot * nParts;
  RedPart acc{start, 0};
  for (int b = tid; b < nParts; b += kRedThreads) acc = MergeMax()(acc, p[b]);
  redFold(red, acc, tid, MergeMax());
  if (tid == 0) out[slot] = red[0].v;
}

// ---- the estimator's step kernels --------------------------------------------------------------------
// the work of matrix blockIdx.y: x at work + y stride (n values of T), xi behind it, the partials at
// partOff bytes from x (all in bytes from the base)
struct NormEstWork {
  char* base;
  int64_t stride, partOff;
  template <typename T>
  __device__ __forceinline__ GP<T> x() const {
    return (GP<T>)(T*)(base + (int64_t)blockIdx.y * stride);
  }
  __device__ __forceinline__ RedPart* part() const {
    return (RedPart*)(base + (int64_t)blockIdx.y * stride + partOff);
  }
};

__device__ __forceinline__ void normEstReset(NormEstState& s) {
  s.est = 0.0;
  s.j = -1;
  s.pass = 0;
  s.stop = NormEstRunning;
  s.altWon = 0;
  for (int i = 0; i < 5; i++) s.jOf[i] = -1;
  s.alt = 0.0;
  s.zero = 0;
}

// The writers, one thread per element.  kind 0: x = 1 / n everywhere, and the record reset; kind 1: x =
// e_j, j from the record (nothing for a stopped matrix); kind 2: x_i = (-1)^i (1 + i / (n - 1)) (1 for
// n == 1), computed in double and rounded to T
template <typename T>
__global__ void __launch_bounds__(kRedThreads)
    normEstWrite(int64_t n, int kind, NormEstWork work, NormEstState* __restrict__ state) {
  NormEstState& st = state[blockIdx.y];
  const int64_t i = (int64_t)blockIdx.x * kRedThreads + threadIdx.x;
  if (kind == 0 && i == 0) normEstReset(st);
  if (i >= n) return;
  const GP<T> x = work.x<T>();
  if (kind == 0) {
    x[i] = (T)(1.0 / (double)n);
  } else if (kind == 1) {
    if (st.stop != NormEstRunning) return;
    x[i] = i == st.j ? T(1) : T(0);
  } else {
    const double v = n > 1 ? 1.0 + (double)i / (double)(n - 1) : 1.0;
    x[i] = (T)((i & 1) ? -v : v);
  }
}

// x <- D x, one thread per element
template <typename T>
__global__ void __launch_bounds__(kRedThreads) normEstScale(int64_t n, NormEstWork work, DataRef<const T> dref) {
  const int64_t i = (int64_t)blockIdx.x * kRedThreads + threadIdx.x;
  if (i >= n) return;
  const GP<const T> d = pickData(dref);
  const GP<T> x = work.x<T>();
  x[i] = x[i] * d[i];
}

// Pass 1 of ||x||_1: the partial sum of |x_i| in double and whether sgn(x_i) == xi_i on all rows of the
// chunk (sgn(v) = +1 for v >= 0, -1 otherwise).  kSigns: xi_i and x_i are then both set to sgn(x_i): xi
// keeps the sign vector for the comparison of the next pass, x is the right-hand side of z = A^-1 xi.
template <typename T, bool kSigns>
__global__ void __launch_bounds__(kRedThreads) normEstSumPartial(int64_t n, NormEstWork work) {
  __shared__ RedPart red[kRedThreads];
  const int tid = threadIdx.x;
  const GP<T> x = work.x<T>();
  const GP<T> xi = x + n;
  RedPart acc{0.0, 1};
#pragma unroll
  for (int m = 0; m < kRedChunk / kRedThreads; m++) {
    const int64_t i = (int64_t)blockIdx.x * kRedChunk + m * kRedThreads + tid;
    if (i < n) {
      const T v = x[i];
      const T sg = v >= T(0) ? T(1) : T(-1);
      acc.v += __builtin_fabs((double)v);
      if (kSigns) {
        acc.k &= xi[i] == sg ? 1 : 0;
        xi[i] = sg;
        x[i] = sg;
      }
    }
  }
  redFold(red, acc, tid, MergeSum());
  if (tid == 0) work.part()[blockIdx.x] = red[0];
}

// Pass 2 of ||x||_1 and the decision of the pass, one workgroup per matrix.  alt = false: the record
// moves on by one measured vector.  alt = true: the value of the alternating vector is weighed in and
// the estimate written to out[matrix]
__global__ void __launch_bounds__(kRedThreads)
    normEstSumFinal(int64_t n, int32_t nParts, bool alt, NormEstWork work, NormEstState* __restrict__ state,
                    double* __restrict__ out) {
  __shared__ RedPart red[kRedThreads];
  const int tid = threadIdx.x;
  const RedPart* p = work.part();
  RedPart acc{0.0, 1};
  for (int b = tid; b < nParts; b += kRedThreads) acc = MergeSum()(acc, p[b]);
  redFold(red, acc, tid, MergeSum());
  if (tid != 0) return;
  NormEstState& st = state[blockIdx.y];
  const double sum = red[0].v;
  if (alt) {
    if (n > 1) {
      const double v = 2.0 * sum / (3.0 * (double)n);
      st.alt = v;
      if (v != v) {
        st.est = v;
      } else if (v > st.est) {
        st.est = v;
        st.altWon = 1;
      }
    }
    out[blockIdx.y] = st.est;
    return;
  }
  if (st.stop != NormEstRunning) return;
  const int64_t pass = ++st.pass;
  if (!redFinite(sum)) {
    st.est = sum;
    st.stop = NormEstNonFinite;
  } else if (pass == 1) {
    st.est = sum;
    if (n == 1) st.stop = NormEstOrderOne;
  } else if (red[0].k) {
    st.est = sum > st.est ? sum : st.est;
    st.stop = NormEstRepeatedSigns;
  } else if (sum <= st.est) {
    st.stop = NormEstNoIncrease;
  } else {
    st.est = sum;
    if (pass == 5) st.stop = NormEstPassLimit;
  }
}

// Pass 1 of the arg-max of |z_i|, the lowest index on ties
template <typename T>
__global__ void __launch_bounds__(kRedThreads) normEstArgMaxPartial(int64_t n, NormEstWork work) {
  __shared__ RedPart red[kRedThreads];
  const int tid = threadIdx.x;
  const GP<T> z = work.x<T>();
  RedPart acc{-1.0, INT64_MAX};
#pragma unroll
  for (int m = 0; m < kRedChunk / kRedThreads; m++) {
    const int64_t i = (int64_t)blockIdx.x * kRedChunk + m * kRedThreads + tid;
    if (i < n) acc = MergeArgMax()(acc, RedPart{__builtin_fabs((double)z[i]), i});
  }
  redFold(red, acc, tid, MergeArgMax());
  if (tid == 0) work.part()[blockIdx.x] = red[0];
}

// Pass 2 of the arg-max and the decision: j <- the arg-max; from the second pass on, the matrix stops
// when |z[j of the last pass]| already is the maximum
template <typename T>
__global__ void __launch_bounds__(kRedThreads)
    normEstArgMaxFinal(int64_t n, int32_t nParts, NormEstWork work, NormEstState* __restrict__ state) {
  __shared__ RedPart red[kRedThreads];
  const int tid = threadIdx.x;
  const RedPart* p = work.part();
  RedPart acc{-1.0, INT64_MAX};
  for (int b = tid; b < nParts; b += kRedThreads) acc = MergeArgMax()(acc, p[b]);
  redFold(red, acc, tid, MergeArgMax());
  if (tid != 0) return;
  NormEstState& st = state[blockIdx.y];
  if (st.stop != NormEstRunning) return;
  const double bestV = red[0].v;
  const int64_t bestK = red[0].k;
  if (bestK < 0 || bestK >= n || !redFinite(bestV)) {  // (every |z_i| a NaN, or an infinite one)
    st.est = redNaN();
    st.stop = NormEstNonFinite;
    return;
  }
  const int64_t jLast = st.j, pass = st.pass;
  st.j = bestK;
  int64_t* w = reinterpret_cast<int64_t*>(state) + (int64_t)blockIdx.y * kNormEstWords;
  w[4 + pass] = bestK;  // jOf[pass - 1]
  if (pass >= 2 && __builtin_fabs((double)work.x<T>()[jLast]) == bestV) st.stop = NormEstSameColumn;
}

}  // namespace hipk
}  // namespace BaSpaCho
