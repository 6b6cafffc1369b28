// The Lanczos recurrence on the device: the dot products, the fused vector updates
// and the full reorthogonalisation of Solver::lanczos*.  The product w = A v is not here: it is the
// caller's (symProduct's mv, or any operator).  Launched by hip_extensions.hip.  Streaming kernels: no
// matrix cores, no persistent launch, no flags, no atomics.  At the end: kvCombine, the combinations V y of
// the basis vectors behind f(A) v, which reads no state record.
//
// CONVENTIONS are those of hip_cg_kernels.h: vectors are [n, q] row-major arrays of T, matrix blockIdx.y of
// a batch finds its operands through pickData, column c of matrix m is one problem with its own state
// record, state[m q + c].  Every dot product is the two-pass sum stated there (cgChunkRows, redFold; operands
// to double, every product rounded before it is added); the vector updates work in T with every product
// rounded in T before it is added, the scalars being the record's doubles rounded to T.
//
// THE BASIS of a member is one array: slot s is the [n, q] vector at basis + s slotStride elements.
//
// THE STATE RECORD: kLzWords = 12 8-byte words per (matrix, start vector),
//   w[0]  steps done
//   w[1]  stop reason: 0 running, 2 step limit, 3 invariant subspace (ww <= thr2 (alpha^2 + beta_prev^2)),
//         4 a non-finite sum, 5 zero start vector (1 is unused: the shared codes keep cg's numbers)
//   w[2]  bits of vv = v0.v0
//   w[3]  bits of the last alpha = v_j . A v_j
//   w[4]  bits of the last beta = sqrt(ww)
//   w[5]  bits of the last ww = w.w of the orthogonalised w
//   w[6]  bits of thr2 = breakdown^2
//   w[7]  kmax, the step limit
//   w[8] .. w[11]  0
// THE COEFFICIENTS of a problem are 2 kmax doubles, alpha_0 .. alpha_{kmax-1} then beta_0 .. beta_{kmax-1},
// problem (m, c) at coef + (m q + c) 2 kmax; the kernels write entry j at step j and nothing else.
// FROZEN COLUMNS.  Every kernel leaves the basis, the coefficients and the record of a stopped column (w[1]
// != 0) bitwise unchanged; only w, the partials and the projection coefficients, which are scratch, may change.
//
// THE WORK of a member (lanczosWorkBytes): the partials of kmax sums, sum i of column c at part[(i q + c)
// nParts ..] (so that the plain dot products, which are sum 0, use the layout of the conjugate gradient),
// then, CgWork::badOff bytes in, the projection coefficients c_i of column c at proj[c kmax + i].
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "hip_cg_kernels.h"

namespace BaSpaCho {
namespace hipk {

constexpr int kLzWords = 12;
// Basis vectors per LDS fold of the projection.  The bits of a sum do not depend on the grouping; the group
// trades barriers (9 per fold, whatever the group) against LDS (kLzGroup 2 KiB) and live registers (kLzGroup
// accumulators beside the 4 cached rows of w).  8: 16 KiB of LDS, 9 barriers per 8 vectors read.
constexpr int kLzGroup = 8;
constexpr int kLzRows = kRedChunk / kRedThreads;  // rows of w a thread keeps in registers

enum LzStop : int64_t { LzRunning = 0, LzStepLimit = 2, LzInvariant = 3, LzNonFinite = 4, LzZeroStart = 5 };

struct LzState {
  int64_t steps, stop;
  double vv, alpha, beta, ww, thr2;
  int64_t kmax, zero[4];
};
static_assert(sizeof(LzState) == 8 * kLzWords, "the state record is twelve 8-byte words");

// which decision a second pass takes
enum LzFold : int32_t {
  LzFoldVV = 0,     // init: the record reset, vv
  LzFoldAlpha = 1,  // alpha
  LzFoldStep = 2    // ww: alpha_j and beta_j stored, the step counted, the stop tests
};

__device__ __forceinline__ double* lzProj(const CgWork& work) { return (double*)work.bad(); }

// Pass 2 and the decision, workgroup (c, matrix); the partials are those of sum 0
__global__ void __launch_bounds__(kRedThreads)
    lzFold(int32_t q, int32_t nParts, int32_t kind, double thr2, int64_t kmax, CgWork work,
           LzState* __restrict__ state, double* __restrict__ coef) {
  __shared__ RedPart red[kRedThreads];
  const int tid = threadIdx.x;
  const int32_t c = blockIdx.x;
  LzState& st = state[(int64_t)blockIdx.y * q + c];
  if (kind != LzFoldVV && st.stop != LzRunning) return;  // (uniform: the record is not written before the fold)
  const RedPart* p = work.part() + (int64_t)c * nParts;
  RedPart acc{0.0, 1};
  for (int b = tid; b < nParts; b += kRedThreads) acc = MergeSum()(acc, p[b]);
  redFold(red, acc, tid, MergeSum());
  if (tid != 0) return;
  const double sum = red[0].v;
  if (kind == LzFoldVV) {
    st.steps = 0;
    st.vv = sum;
    st.alpha = st.beta = st.ww = 0.0;
    st.thr2 = thr2;
    st.kmax = kmax;
    st.zero[0] = st.zero[1] = st.zero[2] = st.zero[3] = 0;
    st.stop = sum == 0.0 ? LzZeroStart : !redFinite(sum) ? LzNonFinite : LzRunning;
  } else if (kind == LzFoldAlpha) {
    st.alpha = sum;
  } else {
    const double alpha = st.alpha, betaPrev = st.beta, beta = __builtin_sqrt(sum);
    const int64_t j = st.steps;
    st.beta = beta;
    st.ww = sum;
    if (j < kmax) {
      double* co = coef + ((int64_t)blockIdx.y * q + c) * 2 * kmax;
      co[j] = alpha;
      co[kmax + j] = beta;
    }
    st.steps = j + 1;
    if (!redFinite(alpha) || !redFinite(sum)) {
      st.stop = LzNonFinite;
    } else if (sum <= rmul(st.thr2, radd(rmul(alpha, alpha), rmul(betaPrev, betaPrev)))) {
      st.stop = LzInvariant;
    } else if (j + 1 >= st.kmax) {
      st.stop = LzStepLimit;
    }
  }
}

// out = in * T(1 / sqrt(vv)) (start: v_0 from v0) or in * T(1 / beta) (v_{j+1} from w), one thread per element
template <typename T>
__global__ void __launch_bounds__(kRedThreads)
    lzNormalize(int64_t n, int32_t q, bool start, DataRef<const T> inref, DataRef<T> basisref, int64_t outOff,
                const LzState* __restrict__ state) {
  const int64_t e = (int64_t)blockIdx.x * kRedThreads + threadIdx.x;
  if (e >= n * q) return;
  const LzState& st = state[(int64_t)blockIdx.y * q + (int32_t)(e % q)];
  if (st.stop != LzRunning) return;
  const T scale = (T)(1.0 / (start ? __builtin_sqrt(st.vv) : st.beta));
  pickData(basisref)[outOff + e] = rmul(pickData(inref)[e], scale);
}

// Pass 1 of v.w with v a slot of the basis; workgroups as cgDotPartial's
template <typename T>
__global__ void __launch_bounds__(kRedThreads)
    lzDotPartial(int64_t n, int32_t q, int32_t nParts, DataRef<const T> basisref, int64_t vOff, DataRef<const T> wref,
                 CgWork work, const LzState* __restrict__ state) {
  __shared__ RedPart red[kRedThreads];
  const int tid = threadIdx.x;
  const int64_t p = blockIdx.x / q;
  const int32_t c = (int32_t)(blockIdx.x - p * q);
  if (state[(int64_t)blockIdx.y * q + c].stop != LzRunning) return;
  const GP<const T> v = pickData(basisref) + vOff, w = pickData(wref);
  RedPart acc{0.0, 1};
  cgChunkRows(n, p, tid, [&](int64_t i) {
    const int64_t at = i * q + c;
    acc.v = radd(acc.v, cgProd((double)v[at], (double)w[at]));
  });
  redFold(red, acc, tid, MergeSum());
  if (tid == 0) work.part()[(int64_t)c * nParts + p] = red[0];
}

// w = (w - alpha v_j) - beta_prev v_{j-1} (the second term absent at step 0) with the partials of w.w
template <typename T>
__global__ void __launch_bounds__(kRedThreads)
    lzUpdate(int64_t n, int32_t q, int32_t nParts, DataRef<const T> basisref, int64_t vOff, int64_t prevOff,
             DataRef<T> wref, CgWork work, const LzState* __restrict__ state) {
  __shared__ RedPart red[kRedThreads];
  const int tid = threadIdx.x;
  const int64_t p = blockIdx.x / q;
  const int32_t c = (int32_t)(blockIdx.x - p * q);
  const LzState& st = state[(int64_t)blockIdx.y * q + c];
  if (st.stop != LzRunning) return;
  const T alpha = (T)st.alpha, beta = (T)st.beta;
  const bool first = st.steps == 0;
  const GP<const T> basis = pickData(basisref);
  const GP<const T> v = basis + vOff, vp = basis + prevOff;
  const GP<T> w = pickData(wref);
  RedPart acc{0.0, 1};
  cgChunkRows(n, p, tid, [&](int64_t i) {
    const int64_t at = i * q + c;
    T wn = radd(w[at], -rmul(alpha, v[at]));
    if (!first) wn = radd(wn, -rmul(beta, vp[at]));
    w[at] = wn;
    acc.v = radd(acc.v, cgProd((double)wn, (double)wn));
  });
  redFold(red, acc, tid, MergeSum());
  if (tid == 0) work.part()[(int64_t)c * nParts + p] = red[0];
}

// the LDS fold of redFold on kLzGroup sums at once: the same tree, one barrier per level for the group
__device__ __forceinline__ void lzFoldGroup(double (*red)[kRedThreads], const double* mine, int tid) {
#pragma unroll
  for (int g = 0; g < kLzGroup; g++) red[g][tid] = mine[g];
  __syncthreads();
  for (int s = kRedThreads / 2; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int g = 0; g < kLzGroup; g++) red[g][tid] = red[g][tid] + red[g][tid + s];
    }
    __syncthreads();
  }
}

// PROJECT, pass 1: the partials of c_i = v_i . w, i = 0 .. count - 1, of chunk p of column c in one pass over
// w and the slots.  The workgroup keeps its 1024 rows of w in registers (kLzRows doubles per thread) and
// takes the slots kLzGroup at a time: each thread's sums in the order of cgChunkRows, then one LDS fold for
// the group.  Bounded by the bytes of the slots: (count + 1) n q sizeof(T) read per call.
template <typename T>
__global__ void __launch_bounds__(kRedThreads)
    lzProjectPartial(int64_t n, int32_t q, int32_t nParts, int32_t count, DataRef<const T> basisref, int64_t slotStride,
                     DataRef<const T> wref, CgWork work, const LzState* __restrict__ state) {
  __shared__ double red[kLzGroup][kRedThreads];
  const int tid = threadIdx.x;
  const int64_t p = blockIdx.x / q;
  const int32_t c = (int32_t)(blockIdx.x - p * q);
  if (state[(int64_t)blockIdx.y * q + c].stop != LzRunning) return;
  const GP<const T> basis = pickData(basisref), w = pickData(wref);
  double wr[kLzRows];
#pragma unroll
  for (int m = 0; m < kLzRows; m++) {
    const int64_t i = p * kRedChunk + m * kRedThreads + tid;
    wr[m] = i < n ? (double)w[i * q + c] : 0.0;
  }
  RedPart* part = work.part();
  for (int32_t i0 = 0; i0 < count; i0 += kLzGroup) {
    double acc[kLzGroup];
#pragma unroll
    for (int g = 0; g < kLzGroup; g++) {
      acc[g] = 0.0;
      if (i0 + g < count) {  // (uniform)
        const GP<const T> v = basis + (int64_t)(i0 + g) * slotStride;
#pragma unroll
        for (int m = 0; m < kLzRows; m++) {
          const int64_t i = p * kRedChunk + m * kRedThreads + tid;
          if (i < n) acc[g] = radd(acc[g], cgProd((double)v[i * q + c], wr[m]));
        }
      }
    }
    lzFoldGroup(red, acc, tid);
    if (tid < kLzGroup && i0 + tid < count) {
      part[((int64_t)(i0 + tid) * q + c) * nParts + p] = RedPart{red[tid][0], 1};
    }
    __syncthreads();  // red is written again by the next group
  }
}

// PROJECT, pass 2: workgroup (i q + c, matrix) folds the partials of sum i of column c into proj[c kmax + i]
__global__ void __launch_bounds__(kRedThreads)
    lzProjectFold(int32_t q, int32_t nParts, int64_t kmax, CgWork work, const LzState* __restrict__ state) {
  __shared__ RedPart red[kRedThreads];
  const int tid = threadIdx.x;
  const int32_t i = blockIdx.x / q, c = blockIdx.x - i * q;
  if (state[(int64_t)blockIdx.y * q + c].stop != LzRunning) return;
  const RedPart* p = work.part() + (int64_t)blockIdx.x * nParts;
  RedPart acc{0.0, 1};
  for (int b = tid; b < nParts; b += kRedThreads) acc = MergeSum()(acc, p[b]);
  redFold(red, acc, tid, MergeSum());
  if (tid == 0) lzProj(work)[(int64_t)c * kmax + i] = red[0].v;
}

// SUBTRACT: w = w - T(c_i) v_i for i = 0 .. count - 1 in this order, each product rounded before it is
// subtracted, with the partials of w.w of the result (sum 0).  The rows of w stay in registers over the
// slots.  Bounded by the bytes of the slots: (count + 2) n q sizeof(T) moved per call.
template <typename T>
__global__ void __launch_bounds__(kRedThreads)
    lzSubtract(int64_t n, int32_t q, int32_t nParts, int32_t count, int64_t kmax, DataRef<const T> basisref,
               int64_t slotStride, DataRef<T> wref, CgWork work, const LzState* __restrict__ state) {
  __shared__ RedPart red[kRedThreads];
  const int tid = threadIdx.x;
  const int64_t p = blockIdx.x / q;
  const int32_t c = (int32_t)(blockIdx.x - p * q);
  if (state[(int64_t)blockIdx.y * q + c].stop != LzRunning) return;
  const GP<const T> basis = pickData(basisref);
  const GP<T> w = pickData(wref);
  const double* proj = lzProj(work) + (int64_t)c * kmax;
  T wr[kLzRows];
#pragma unroll
  for (int m = 0; m < kLzRows; m++) {
    const int64_t i = p * kRedChunk + m * kRedThreads + tid;
    wr[m] = i < n ? w[i * q + c] : T(0);
  }
  for (int32_t k = 0; k < count; k++) {
    const T ck = (T)proj[k];
    const GP<const T> v = basis + (int64_t)k * slotStride;
#pragma unroll
    for (int m = 0; m < kLzRows; m++) {
      const int64_t i = p * kRedChunk + m * kRedThreads + tid;
      if (i < n) wr[m] = radd(wr[m], -rmul(ck, v[i * q + c]));
    }
  }
  RedPart acc{0.0, 1};
#pragma unroll
  for (int m = 0; m < kLzRows; m++) {
    const int64_t i = p * kRedChunk + m * kRedThreads + tid;
    if (i < n) {
      w[i * q + c] = wr[m];
      acc.v = radd(acc.v, cgProd((double)wr[m], (double)wr[m]));
    }
  }
  redFold(red, acc, tid, MergeSum());
  if (tid == 0) work.part()[(int64_t)c * nParts + p] = red[0];
}

// COMBINE: out_f[:, c] = (accumulate ? out_f[:, c] : +0) + sum_i T(y[c, f, i]) v_i[:, c]
// for the kNf outputs f of column c in one pass over the slots, v_i the slot `i` of the basis handed in (the
// launcher has moved it to the first slot of the call).  Term i has the Lanczos index first + i and is taken
// when first + i < limit[c]: the indices ascend, so the terms taken are the first `take` ones and no slot
// behind them is read.  The sum runs over i ascending in T, every product rounded before it is added; which
// terms one call holds does not change the bits of a chain of calls.  The coefficients of problem (m, c) are
// the doubles y[((m q + c) kNf + f) ldy + i]; their address does not depend on the lane.  The thread's kLzRows
// rows times kNf sums stay in registers; the slots are loaded kKvGroup at a time, all loads of a group ahead of
// its additions, which keep their order.  No LDS, no atomics.  Reads take n sizeof(T) bytes per column, writes
// kNf n sizeof(T).
constexpr int kKvMaxOut = 4;
// Slots per group: 4 keeps 16 loads per thread in flight; 8 costs 152 to 181 registers in double (3 to 2 waves per
// SIMD) and spills scalar registers at 4 outputs
constexpr int kKvGroup = 4;

template <typename T, int kNf>
__global__ void __launch_bounds__(kRedThreads)
    kvCombine(int64_t n, int32_t q, int32_t count, int64_t first, DataRef<const T> basisref, int64_t slotOff,
              int64_t slotStride, const double* __restrict__ y, int64_t ldy, const int64_t* __restrict__ limit,
              DataRef<T> outref, int64_t outStride, bool accumulate) {
  const int tid = threadIdx.x;
  const int64_t p = blockIdx.x / q;
  const int32_t c = (int32_t)(blockIdx.x - p * q);
  const int64_t prob = (int64_t)blockIdx.y * q + c;
  const int64_t room = limit[prob] - first;
  const int32_t take = room <= 0 ? 0 : room < count ? (int32_t)room : count;  // (uniform)
  if (take == 0 && accumulate) return;
  const GP<const T> basis = pickData(basisref) + slotOff;
  const GP<T> out = pickData(outref);
  const double* yc = y + prob * kNf * ldy;
  T acc[kNf][kLzRows];
#pragma unroll
  for (int f = 0; f < kNf; f++) {
#pragma unroll
    for (int m = 0; m < kLzRows; m++) {
      const int64_t i = p * kRedChunk + m * kRedThreads + tid;
      acc[f][m] = accumulate && i < n ? out[f * outStride + i * q + c] : T(0);
    }
  }
  int32_t k = 0;
  for (; k + kKvGroup <= take; k += kKvGroup) {
    T v[kKvGroup][kLzRows];
#pragma unroll
    for (int g = 0; g < kKvGroup; g++) {
      const GP<const T> vg = basis + (int64_t)(k + g) * slotStride;
#pragma unroll
      for (int m = 0; m < kLzRows; m++) {
        const int64_t i = p * kRedChunk + m * kRedThreads + tid;
        v[g][m] = i < n ? vg[i * q + c] : T(0);
      }
    }
#pragma unroll
    for (int g = 0; g < kKvGroup; g++) {
#pragma unroll
      for (int f = 0; f < kNf; f++) {
        const T yk = (T)yc[f * ldy + k + g];
#pragma unroll
        for (int m = 0; m < kLzRows; m++) acc[f][m] = radd(acc[f][m], rmul(yk, v[g][m]));
      }
    }
  }
  for (; k < take; k++) {
    const GP<const T> vk = basis + (int64_t)k * slotStride;
    T v[kLzRows];
#pragma unroll
    for (int m = 0; m < kLzRows; m++) {
      const int64_t i = p * kRedChunk + m * kRedThreads + tid;
      v[m] = i < n ? vk[i * q + c] : T(0);
    }
#pragma unroll
    for (int f = 0; f < kNf; f++) {
      const T yk = (T)yc[f * ldy + k];
#pragma unroll
      for (int m = 0; m < kLzRows; m++) acc[f][m] = radd(acc[f][m], rmul(yk, v[m]));
    }
  }
#pragma unroll
  for (int f = 0; f < kNf; f++) {
#pragma unroll
    for (int m = 0; m < kLzRows; m++) {
      const int64_t i = p * kRedChunk + m * kRedThreads + tid;
      if (i < n) out[f * outStride + i * q + c] = acc[f][m];
    }
  }
}

}  // namespace hipk
}  // namespace BaSpaCho
