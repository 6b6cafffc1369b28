// Preconditioned conjugate gradient on the device: the dot products, the fused
// vector updates and the built-in preconditioners of Solver::cg* (Jacobi, block-Jacobi, and the factorised
// sparse approximate inverse of section 27 at the end of the file).  The product A p is not here: it
// is the caller's (symProduct's mv, or any operator).  Launched by hip_extensions.hip.  Streaming
// kernels: no matrix cores, no persistent launch, no flags, no atomics.
//
// CONVENTIONS.  Vectors are [n, q] row-major arrays of T, one per matrix; matrix blockIdx.y of a batch
// finds its operands through pickData.  Column j of matrix m is one problem with its own state record,
// state[m q + j].  The dot products follow the reductions of hip_norm_est_kernels.h: workgroup (chunk
// x, column j) of pass 1 owns the rows [x kRedChunk, (x + 1) kRedChunk) of column j, thread t adds the
// products of the rows x kRedChunk + m 256 + t, m = 0 .. 3, in this order from +0, the 256 thread values
// are folded by redFold; pass 2 is one workgroup per column whose thread t adds the partials t, t + 256,
// ... in this order from +0 and folds the same way.  Operands are converted to double, every product is
// rounded before it is added (rmul / radd), for both precisions.  The vector updates work in T with
// every product rounded in T before it is added; alpha and beta are the record's doubles rounded to T.
//
// THE STATE RECORD: kCgWords = 12 8-byte words per (matrix, right-hand side),
//   w[0]  iterations done (x updates)
//   w[1]  stop reason: 0 running, 1 converged (rr <= tol^2 bb), 2 step limit, 3 breakdown (pAp not > 0,
//         or r.z not > 0), 4 a non-finite sum, 5 zero right-hand side (x = 0, 0 iterations)
//   w[2]  bits of rz = r.z of the current direction, a double (r.r without a preconditioner)
//   w[3]  bits of pAp, the last p.Ap
//   w[4]  bits of rr, the last r.r
//   w[5]  bits of bb = b.b
//   w[6]  bits of the last alpha = rz / pAp
//   w[7]  bits of the last beta = rz(new) / rz(old); 0 before the first
//   w[8]  bits of tol^2
//   w[9]  the step limit
//   w[10], w[11]  0
// FROZEN COLUMNS.  Every kernel leaves x, r, p, z and the record of a stopped column (w[1] != 0) bitwise
// unchanged; only the partials and Ap, which are scratch, may change.  The records are read by the
// kernels, never by the host.
//
// THE STATUS RECORD of a built-in preconditioner: 2 8-byte words per matrix, {the caller's scalar of the
// first bad pivot (the lowest one) or -1, the number of bad blocks}.  A block whose pivot is not a
// positive finite number gets the zero matrix as its inverse (fsai: a row of G, which becomes zeros).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "hip_device_common.h"
#include "hip_norm_est_kernels.h"
#include "hip_ordered_sum.h"

namespace BaSpaCho {
namespace hipk {

constexpr int kCgWords = 12;
constexpr int kCgMaxBlock = 32;     // widest diagonal block of the block-Jacobi preconditioner
constexpr int kCgBuildThreads = 64;  // one wave per block

enum CgStop : int64_t {
  CgRunning = 0,
  CgConverged = 1,
  CgStepLimit = 2,
  CgBreakdown = 3,
  CgNonFinite = 4,
  CgZeroRhs = 5
};

struct CgState {
  int64_t iter, stop;
  double rz, pAp, rr, bb, alpha, beta, tol2;
  int64_t maxSteps, zero[2];
};
static_assert(sizeof(CgState) == 8 * kCgWords, "the state record is twelve 8-byte words");

// which decision a second pass takes
enum CgFold : int32_t {
  CgFoldBB = 0,     // init: the record reset, bb
  CgFoldRR0 = 1,    // init: rr of the first residual, converged / step limit 0
  CgFoldAlpha = 2,  // pAp, alpha
  CgFoldRR = 3,     // rr after an update, the iteration counted, converged / step limit
  CgFoldBeta = 4    // rz, beta
};

// the work of matrix blockIdx.y: the partials (q columns of nParts each), the bad-pivot words of a
// preconditioner build behind them at badOff bytes
struct CgWork {
  char* base;
  int64_t stride, badOff;
  __device__ __forceinline__ RedPart* part() const { return (RedPart*)(base + (int64_t)blockIdx.y * stride); }
  __device__ __forceinline__ int32_t* bad() const {
    return (int32_t*)(base + (int64_t)blockIdx.y * stride + badOff);
  }
};

// the tables of a preconditioner plan on the device (sym_product.h, CgPrecondPlan)
struct CgPrecondDev {
  const int32_t* blockStart;   // [numBlocks + 1] caller's scalars
  const int64_t* blockOff;     // [numBlocks + 1] elements of the inverse
  const int32_t* scalarBlock;  // [n]
  const int32_t *itemStart, *itemEntry, *itemPos;
};

__device__ __forceinline__ CgState& cgStateOf(CgState* state, int32_t q, int32_t j) {
  return state[(int64_t)blockIdx.y * q + j];
}

// the rows of thread tid in chunk p, in order: f(i) for i = p kRedChunk + m 256 + tid < n
template <typename F>
__device__ __forceinline__ void cgChunkRows(int64_t n, int64_t p, int tid, F f) {
#pragma unroll
  for (int m = 0; m < kRedChunk / kRedThreads; m++) {
    const int64_t i = p * kRedChunk + m * kRedThreads + tid;
    if (i < n) f(i);
  }
}

__device__ __forceinline__ double cgProd(double a, double b) { return rmul(a, b); }

// Pass 1 of a.b per column: workgroup x = p q + j, the partial to part[j nParts + p]
template <typename T>
__global__ void __launch_bounds__(kRedThreads)
    cgDotPartial(int64_t n, int32_t q, int32_t nParts, DataRef<const T> aref, DataRef<const T> bref, CgWork work,
                 const CgState* __restrict__ state, bool always) {
  __shared__ RedPart red[kRedThreads];
  const int tid = threadIdx.x;
  const int64_t p = blockIdx.x / q;
  const int32_t j = (int32_t)(blockIdx.x - p * q);
  if (!always && state[(int64_t)blockIdx.y * q + j].stop != CgRunning) return;
  const GP<const T> a = pickData(aref), b = pickData(bref);
  RedPart acc{0.0, 1};
  cgChunkRows(n, p, tid, [&](int64_t i) {
    const int64_t at = i * q + j;
    acc.v = radd(acc.v, cgProd((double)a[at], (double)b[at]));
  });
  redFold(red, acc, tid, MergeSum());
  if (tid == 0) work.part()[(int64_t)j * nParts + p] = red[0];
}

// Pass 2 and the decision, workgroup (j, matrix)
__global__ void __launch_bounds__(kRedThreads)
    cgFold(int32_t q, int32_t nParts, int32_t kind, bool plain, double tol2, int64_t maxSteps, CgWork work,
           CgState* __restrict__ state) {
  __shared__ RedPart red[kRedThreads];
  const int tid = threadIdx.x;
  const int32_t j = blockIdx.x;
  CgState& st = cgStateOf(state, q, j);
  if (kind != CgFoldBB && st.stop != CgRunning) return;  // (uniform: the record is not written before the fold)
  const RedPart* p = work.part() + (int64_t)j * nParts;
  RedPart acc{0.0, 1};
  for (int b = tid; b < nParts; b += kRedThreads) acc = MergeSum()(acc, p[b]);
  redFold(red, acc, tid, MergeSum());
  if (tid != 0) return;
  const double sum = red[0].v;
  switch (kind) {
    case CgFoldBB:
      st.iter = 0;
      st.rz = st.pAp = st.rr = st.alpha = st.beta = 0.0;
      st.bb = sum;
      st.tol2 = tol2;
      st.maxSteps = maxSteps;
      st.zero[0] = st.zero[1] = 0;
      st.stop = sum == 0.0 ? CgZeroRhs : !redFinite(sum) ? CgNonFinite : CgRunning;
      break;
    case CgFoldRR0:
    case CgFoldRR:
      st.rr = sum;
      if (kind == CgFoldRR) st.iter++;
      if (!redFinite(sum)) {
        st.stop = CgNonFinite;
      } else if (sum <= rmul(st.tol2, st.bb)) {
        st.stop = CgConverged;
      } else if (st.iter >= st.maxSteps) {
        st.stop = CgStepLimit;
      } else if (plain) {  // z = r: r.z is r.r
        st.beta = kind == CgFoldRR ? sum / st.rz : 0.0;
        st.rz = sum;
      }
      break;
    case CgFoldAlpha:
      st.pAp = sum;
      if (!redFinite(sum)) {
        st.stop = CgNonFinite;
      } else if (!(sum > 0.0)) {
        st.stop = CgBreakdown;
      } else {
        st.alpha = st.rz / sum;
      }
      break;
    default:  // CgFoldBeta
      if (!redFinite(sum)) {
        st.rz = sum;
        st.stop = CgNonFinite;
      } else if (!(sum > 0.0)) {
        st.rz = sum;
        st.stop = CgBreakdown;
      } else {
        st.beta = st.iter > 0 ? sum / st.rz : 0.0;
        st.rz = sum;
      }
      break;
  }
}

// init, one thread per element: x = 0 and r = 0 in the columns of a zero right-hand side
template <typename T>
__global__ void __launch_bounds__(kRedThreads)
    cgStart(int64_t n, int32_t q, DataRef<T> xref, DataRef<T> rref, const CgState* __restrict__ state) {
  const int64_t e = (int64_t)blockIdx.x * kRedThreads + threadIdx.x;
  if (e >= n * q) return;
  const int32_t j = (int32_t)(e % q);
  if (state[(int64_t)blockIdx.y * q + j].stop != CgZeroRhs) return;
  pickData(xref)[e] = T(0);
  pickData(rref)[e] = T(0);
}

// x += alpha p and r -= alpha Ap with the partials of the new r.r; workgroups as cgDotPartial's
template <typename T>
__global__ void __launch_bounds__(kRedThreads)
    cgUpdateXR(int64_t n, int32_t q, int32_t nParts, DataRef<const T> pref, DataRef<const T> apref, DataRef<T> xref,
               DataRef<T> rref, CgWork work, const CgState* __restrict__ state) {
  __shared__ RedPart red[kRedThreads];
  const int tid = threadIdx.x;
  const int64_t c = blockIdx.x / q;
  const int32_t j = (int32_t)(blockIdx.x - c * q);
  const CgState& st = state[(int64_t)blockIdx.y * q + j];
  if (st.stop != CgRunning) return;
  const T alpha = (T)st.alpha;
  const GP<const T> p = pickData(pref), ap = pickData(apref);
  const GP<T> x = pickData(xref), r = pickData(rref);
  RedPart acc{0.0, 1};
  cgChunkRows(n, c, tid, [&](int64_t i) {
    const int64_t at = i * q + j;
    x[at] = radd(x[at], rmul(alpha, p[at]));
    const T rn = radd(r[at], -rmul(alpha, ap[at]));
    r[at] = rn;
    acc.v = radd(acc.v, cgProd((double)rn, (double)rn));
  });
  redFold(red, acc, tid, MergeSum());
  if (tid == 0) work.part()[(int64_t)j * nParts + c] = red[0];
}

// z = M^-1 r with the partials of r.z.  kKind 0: z is the caller's and only read; 1: Jacobi, z_i = r_i
// inv_i; 2: block-Jacobi, z_i = T(sum_j double(Minv_ij) double(r_j)) over the block of i, j ascending
template <typename T, int kKind>
__global__ void __launch_bounds__(kRedThreads)
    cgPrecond(int64_t n, int32_t q, int32_t nParts, CgPrecondDev pl, DataRef<const T> mref, DataRef<const T> rref,
              DataRef<T> zref, CgWork work, const CgState* __restrict__ state) {
  __shared__ RedPart red[kRedThreads];
  const int tid = threadIdx.x;
  const int64_t c = blockIdx.x / q;
  const int32_t j = (int32_t)(blockIdx.x - c * q);
  if (state[(int64_t)blockIdx.y * q + j].stop != CgRunning) return;
  const GP<const T> r = pickData(rref);
  const GP<const T> minv = kKind == 0 ? GP<const T>(nullptr) : pickData(mref);
  const GP<T> z = pickData(zref);
  RedPart acc{0.0, 1};
  cgChunkRows(n, c, tid, [&](int64_t i) {
    const int64_t at = i * q + j;
    T zi;
    if (kKind == 0) {
      zi = z[at];
    } else if (kKind == 1) {
      zi = rmul(r[at], minv[i]);
      z[at] = zi;
    } else {
      const int32_t b = pl.scalarBlock[i];
      const int64_t s0 = pl.blockStart[b], w = pl.blockStart[b + 1] - s0;
      const GP<const T> row = minv + pl.blockOff[b] + (i - s0) * w;
      double s = 0.0;
      for (int64_t k = 0; k < w; k++) s = radd(s, cgProd((double)row[k], (double)r[(s0 + k) * q + j]));
      zi = (T)s;
      z[at] = zi;
    }
    acc.v = radd(acc.v, cgProd((double)r[at], (double)zi));
  });
  redFold(red, acc, tid, MergeSum());
  if (tid == 0) work.part()[(int64_t)j * nParts + c] = red[0];
}

// p = z + beta p (p = z before the first iteration), one thread per element
template <typename T>
__global__ void __launch_bounds__(kRedThreads)
    cgDirection(int64_t n, int32_t q, DataRef<const T> zref, DataRef<T> pref, const CgState* __restrict__ state) {
  const int64_t e = (int64_t)blockIdx.x * kRedThreads + threadIdx.x;
  if (e >= n * q) return;
  const CgState& st = state[(int64_t)blockIdx.y * q + (int32_t)(e % q)];
  if (st.stop != CgRunning) return;
  const GP<const T> z = pickData(zref);
  const GP<T> p = pickData(pref);
  p[e] = st.iter == 0 ? z[e] : radd(z[e], rmul((T)st.beta, p[e]));
}

// ---- the built-in preconditioners ---------------------------------------------------------------------
// Jacobi, one thread per scalar: d = the scalar's diagonal entries added in ascending entry index from +0
// in double, inv = T(1 / d); a d that is not positive and finite is a bad pivot
template <typename T>
__global__ void __launch_bounds__(kRedThreads)
    cgJacobiBuild(int64_t n, CgPrecondDev pl, DataRef<const T> vref, DataRef<T> mref, CgWork work) {
  const int64_t i = (int64_t)blockIdx.x * kRedThreads + threadIdx.x;
  if (i >= n) return;
  const GP<const T> v = pickData(vref);
  double d = 0.0;
  for (int32_t t = pl.itemStart[i]; t < pl.itemStart[i + 1]; t++) d = radd(d, (double)v[pl.itemEntry[t]]);
  const bool ok = d > 0.0 && redFinite(d);
  pickData(mref)[i] = ok ? (T)(1.0 / d) : T(0);
  work.bad()[i] = ok ? -1 : 0;
}

// The rest of a block-Jacobi build, shared with hip_cgls_kernels.h, by one wave on the block A (w x w, lower
// triangle, row-major, in LDS) with Li zeroed: Cholesky, L^-1, the inverse stored as T; the zero matrix and
// the pivot's step in *badWord for a bad pivot, -1 there else
template <typename T>
__device__ __forceinline__ void cgBlockInvert(double* A, double* Li, int w, int lane, GP<T> out, int32_t* badWord) {
  int bad = -1;
  for (int k = 0; k < w; k++) {
    const double d = A[k * w + k];  // (the same value in every lane: the loop stays uniform)
    if (!(d > 0.0) || !redFinite(d)) {
      bad = k;
      break;
    }
    const double s = __builtin_sqrt(d);
    __syncthreads();
    if (lane == 0) A[k * w + k] = s;
    for (int i = k + 1 + lane; i < w; i += kCgBuildThreads) A[i * w + k] = A[i * w + k] / s;
    __syncthreads();
    // the trailing lower triangle: element (i, c), k < c <= i
    for (int e = lane; e < w * w; e += kCgBuildThreads) {
      const int i = e / w, c = e - i * w;
      if (c > k && c <= i) A[e] = radd(A[e], -rmul(A[i * w + k], A[c * w + k]));
    }
    __syncthreads();
  }
  if (bad >= 0) {
    for (int e = lane; e < w * w; e += kCgBuildThreads) out[e] = T(0);
    if (lane == 0) *badWord = bad;
    return;
  }
  // column c of L^-1 by lane c
  for (int c = lane; c < w; c += kCgBuildThreads) {
    Li[c * w + c] = 1.0 / A[c * w + c];
    for (int i = c + 1; i < w; i++) {
      double s = 0.0;
      for (int k = c; k < i; k++) s = radd(s, rmul(A[i * w + k], Li[k * w + c]));
      Li[i * w + c] = -s / A[i * w + i];
    }
  }
  __syncthreads();
  for (int e = lane; e < w * w; e += kCgBuildThreads) {
    const int i = e / w, c = e - i * w;
    double s = 0.0;
    for (int k = i > c ? i : c; k < w; k++) s = radd(s, rmul(Li[k * w + i], Li[k * w + c]));
    out[e] = (T)s;
  }
  if (lane == 0) *badWord = -1;
}

// Block-Jacobi, one wave per block of width w <= kCgMaxBlock, all in double in LDS: the block's entries
// added in ascending entry index (duplicates and both triangles of the storage: an entry (i, j), i >= j,
// lands at (i, j)); Cholesky, column by column; L^-1 by forward substitution, column by column; the
// inverse M^-1_ij = sum_{k >= max(i, j)} L^-1_ki L^-1_kj, k ascending, stored as T, row-major, both
// triangles.  Every product is rounded before it is added.
template <typename T>
__global__ void __launch_bounds__(kCgBuildThreads)
    cgBlockBuild(CgPrecondDev pl, DataRef<const T> vref, DataRef<T> mref, CgWork work) {
  __shared__ double A[kCgMaxBlock * kCgMaxBlock];
  __shared__ double Li[kCgMaxBlock * kCgMaxBlock];
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int w = pl.blockStart[b + 1] - pl.blockStart[b];
  const GP<const T> v = pickData(vref);
  const GP<T> out = pickData(mref) + pl.blockOff[b];
  for (int e = lane; e < w * w; e += kCgBuildThreads) {
    A[e] = 0.0;
    Li[e] = 0.0;
  }
  __syncthreads();
  // every element is owned by one lane, which meets its entries in ascending entry index
  for (int32_t t = pl.itemStart[b]; t < pl.itemStart[b + 1]; t++) {
    const int32_t pos = pl.itemPos[t];
    if ((pos & (kCgBuildThreads - 1)) == lane) A[pos] = radd(A[pos], (double)v[pl.itemEntry[t]]);
  }
  __syncthreads();
  cgBlockInvert<T>(A, Li, w, lane, out, work.bad() + b);
}

// the status record of a build, one workgroup per matrix: v counts the bad blocks, k is the lowest bad scalar
struct MergeBadPivot {
  __device__ __forceinline__ RedPart operator()(const RedPart& a, const RedPart& b) const {
    return RedPart{a.v + b.v, a.k < b.k ? a.k : b.k};
  }
};
__global__ void __launch_bounds__(kRedThreads)
    cgPrecondStatus(int64_t numBlocks, CgPrecondDev pl, CgWork work, int64_t* __restrict__ status) {
  __shared__ RedPart red[kRedThreads];
  const int tid = threadIdx.x;
  const int32_t* bad = work.bad();
  RedPart acc{0.0, INT64_MAX};
  for (int64_t b = tid; b < numBlocks; b += kRedThreads) {
    if (bad[b] >= 0) acc = MergeBadPivot()(acc, RedPart{1.0, (int64_t)pl.blockStart[b] + bad[b]});
  }
  redFold(red, acc, tid, MergeBadPivot());
  if (tid != 0) return;
  status[2 * (int64_t)blockIdx.y] = red[0].v > 0.0 ? red[0].k : -1;
  status[2 * (int64_t)blockIdx.y + 1] = (int64_t)red[0].v;
}

// ---- the factorised sparse approximate inverse M^-1 = G^T G ---------------------
constexpr int kCgFsaiMaxRow = 32;    // widest row of G
constexpr int kCgFsaiRowsPerWg = 4;  // one wave per row

// the tables of a CgFsaiPlan on the device (sym_product.h)
struct CgFsaiDev {
  const int32_t *rowStart, *cols;                                  // [n + 1], [elements of G]
  const int32_t *itemStart, *itemEntry, *itemPos;                  // [n + 1], [items] x 2
  const int32_t *colStart, *colPos, *colRow;                       // [n + 1], [elements of G] x 2
  const int32_t *longCols, *chunkLongFirst;                        // the long columns, those of every chunk
};

// Row i of G by one wave, all in double in the wave's part of LDS: the local matrix A[S_i, S_i] (lower
// triangle) from its items in ascending entry index, Cholesky column by column with cgBlockBuild's
// operations, then the last row of L^-1 by back substitution: g_{w-1} = 1 / L_{w-1,w-1}, g_c = -(sum_{k >
// c} L_kc g_k) / L_cc, k ascending from +0, every product rounded.  A bad pivot gives a row of zeros and its
// local step in the bad word of the row.  The waves of a workgroup do not meet: only waveSync.
template <typename T>
__global__ void __launch_bounds__(64 * kCgFsaiRowsPerWg)
    cgFsaiBuild(int64_t n, CgFsaiDev pl, DataRef<const T> vref, DataRef<T> gref, CgWork work) {
  __shared__ double lds[kCgFsaiRowsPerWg][kCgFsaiMaxRow * kCgFsaiMaxRow + kCgFsaiMaxRow];
  const int lane = threadIdx.x & 63;
  const int wave = waveUniform((int32_t)(threadIdx.x >> 6));
  const int64_t i = (int64_t)blockIdx.x * kCgFsaiRowsPerWg + wave;
  if (i >= n) return;
  double* A = lds[wave];
  double* g = A + kCgFsaiMaxRow * kCgFsaiMaxRow;
  const int32_t g0 = waveUniform(pl.rowStart[i]);
  const int w = waveUniform(pl.rowStart[i + 1]) - g0;
  const GP<const T> v = pickData(vref);
  const GP<T> out = pickData(gref) + g0;
  for (int e = lane; e < w * w; e += 64) A[e] = 0.0;
  waveSync();
  // every element is owned by one lane, which meets its entries in ascending entry index
  const int32_t t0 = waveUniform(pl.itemStart[i]), t1 = waveUniform(pl.itemStart[i + 1]);
  for (int32_t t = t0; t < t1; t++) {
    const int32_t pos = pl.itemPos[t];
    if ((pos & 63) == lane) A[pos] = radd(A[pos], (double)v[pl.itemEntry[t]]);
  }
  waveSync();
  int bad = -1;
  for (int k = 0; k < w; k++) {
    const double d = A[k * w + k];  // (the same value in every lane: the loop stays uniform)
    if (!(d > 0.0) || !redFinite(d)) {
      bad = k;
      break;
    }
    const double s = __builtin_sqrt(d);
    waveSync();
    if (lane == 0) A[k * w + k] = s;
    for (int r = k + 1 + lane; r < w; r += 64) A[r * w + k] = A[r * w + k] / s;
    waveSync();
    // the trailing lower triangle: element (r, c), k < c <= r
    for (int e = lane; e < w * w; e += 64) {
      const int r = e / w, c = e - r * w;
      if (c > k && c <= r) A[e] = radd(A[e], -rmul(A[r * w + k], A[c * w + k]));
    }
    waveSync();
  }
  if (bad >= 0) {
    if (lane < w) out[lane] = T(0);
    if (lane == 0) work.bad()[i] = bad;
    return;
  }
  if (lane == 0) {
    g[w - 1] = 1.0 / A[(w - 1) * w + (w - 1)];
    for (int c = w - 2; c >= 0; c--) {
      double s = 0.0;
      for (int k = c + 1; k < w; k++) s = radd(s, rmul(A[k * w + c], g[k]));
      g[c] = -s / A[c * w + c];
    }
    work.bad()[i] = -1;
  }
  waveSync();
  if (lane < w) out[lane] = (T)g[lane];
}

// t = G r, one lane per (row, right-hand side): t_i = T(sum_c double(G_ic) double(r_cols[c])), c ascending
template <typename T>
__global__ void __launch_bounds__(kRedThreads)
    cgFsaiLower(int64_t n, int32_t q, CgFsaiDev pl, DataRef<const T> gref, DataRef<const T> rref, DataRef<T> tref,
                const CgState* __restrict__ state) {
  const int64_t e = (int64_t)blockIdx.x * kRedThreads + threadIdx.x;
  if (e >= n * q) return;
  const int64_t i = e / q;
  const int32_t j = (int32_t)(e - i * q);
  if (state[(int64_t)blockIdx.y * q + j].stop != CgRunning) return;
  const GP<const T> g = pickData(gref), r = pickData(rref);
  const int32_t* __restrict__ cols = pl.cols;
  const double s = sumRunByLane(pl.rowStart[i], pl.rowStart[i + 1],
                                [=](int32_t x) { return cgProd((double)g[x], (double)r[(int64_t)cols[x] * q + j]); });
  pickData(tref)[e] = (T)s;
}

// z = G^T t with the partials of r.z, in cgPrecond's workgroups: z_i = T(sum double(G_ki) double(t_k)) over
// column i of G, k ascending.  The long columns of the chunk go first, one wave each (the same sequential
// sum); then every thread takes its rows in cgPrecond's order, the short columns summed by the lane.
template <typename T>
__global__ void __launch_bounds__(kRedThreads)
    cgFsaiUpper(int64_t n, int32_t q, int32_t nParts, CgFsaiDev pl, DataRef<const T> gref, DataRef<const T> tref,
                DataRef<const T> rref, DataRef<T> zref, CgWork work, const CgState* __restrict__ state) {
  __shared__ RedPart red[kRedThreads];
  const int tid = threadIdx.x;
  const int64_t c = blockIdx.x / q;
  const int32_t j = (int32_t)(blockIdx.x - c * q);
  if (state[(int64_t)blockIdx.y * q + j].stop != CgRunning) return;
  const GP<const T> g = pickData(gref), t = pickData(tref), r = pickData(rref);
  const GP<T> z = pickData(zref);
  const int32_t* __restrict__ colPos = pl.colPos;
  const int32_t* __restrict__ colRow = pl.colRow;
  const auto term = [=](int32_t x) { return cgProd((double)g[colPos[x]], (double)t[(int64_t)colRow[x] * q + j]); };
  const int lane = tid & 63;
  const int wave = waveUniform((int32_t)(tid >> 6));
  const int32_t l0 = pl.chunkLongFirst[c], l1 = pl.chunkLongFirst[c + 1];
  for (int32_t l = l0 + wave; l < l1; l += kRedThreads / 64) {
    const int32_t u = waveUniform(pl.longCols[l]);
    const double s = sumRunByWave(waveUniform(pl.colStart[u]), waveUniform(pl.colStart[u + 1]), lane, term);
    if (lane == 0) z[(int64_t)u * q + j] = (T)s;
  }
  if (l1 > l0) __syncthreads();  // (uniform) the long columns' z, read back below
  // the thread's rows side by side, so that their loads overlap: every sum still takes its own terms in
  // list order from +0 (sumRunByLane's sum)
  constexpr int kRows = kRedChunk / kRedThreads;
  int32_t r0[kRows], len[kRows], most = 0;
  double s[kRows];
  bool isLong[kRows];
#pragma unroll
  for (int m = 0; m < kRows; m++) {
    const int64_t i = c * kRedChunk + m * kRedThreads + tid;
    r0[m] = i < n ? pl.colStart[i] : 0;
    len[m] = i < n ? pl.colStart[i + 1] - r0[m] : 0;
    isLong[m] = isLongRun(len[m]);
    if (isLong[m]) len[m] = 0;
    most = len[m] > most ? len[m] : most;
    s[m] = 0.0;
  }
  for (int32_t k = 0; k < most; k++) {
#pragma unroll
    for (int m = 0; m < kRows; m++) {
      // (the load is not under the condition, so that the rows' loads are in flight together: a row that
      // has ended reads its first term again, a valid position, and drops it)
      const double v = term(r0[m] + (k < len[m] ? k : 0));
      if (k < len[m]) s[m] = radd(s[m], v);
    }
  }
  RedPart acc{0.0, 1};
#pragma unroll
  for (int m = 0; m < kRows; m++) {  // (cgChunkRows' rows, in its order)
    const int64_t i = c * kRedChunk + m * kRedThreads + tid;
    if (i >= n) continue;
    const int64_t at = i * q + j;
    T zi;
    if (isLong[m]) {
      zi = z[at];
    } else {
      zi = (T)s[m];
      z[at] = zi;
    }
    acc.v = radd(acc.v, cgProd((double)r[at], (double)zi));
  }
  redFold(red, acc, tid, MergeSum());
  if (tid == 0) work.part()[(int64_t)j * nParts + c] = red[0];
}

// the status record of an fsai build: the bad word of row i is the local step of its bad pivot
__global__ void __launch_bounds__(kRedThreads)
    cgFsaiStatus(int64_t n, CgFsaiDev pl, CgWork work, int64_t* __restrict__ status) {
  __shared__ RedPart red[kRedThreads];
  const int tid = threadIdx.x;
  const int32_t* bad = work.bad();
  RedPart acc{0.0, INT64_MAX};
  for (int64_t i = tid; i < n; i += kRedThreads) {
    if (bad[i] >= 0) acc = MergeBadPivot()(acc, RedPart{1.0, (int64_t)pl.cols[pl.rowStart[i] + bad[i]]});
  }
  redFold(red, acc, tid, MergeBadPivot());
  if (tid != 0) return;
  status[2 * (int64_t)blockIdx.y] = red[0].v > 0.0 ? red[0].k : -1;
  status[2 * (int64_t)blockIdx.y + 1] = (int64_t)red[0].v;
}

}  // namespace hipk
}  // namespace BaSpaCho
