// Matrix-free least squares on the device: CGLS for (J^T J + D) x = J^T r + c from
// the entries of J alone, over the lists of a JacobianProductMap (jac_product.h).  The products with their
// epilogues, the squared column norms, the damping vector, the fused updates, the curvature, the
// preconditioner application with its two reductions, and the Jacobi and block-Jacobi builds for J^T J + D.
// bb, the direction and the status of a build are hip_cg_kernels.h's.  Launched by hip_extensions.hip.
// Streaming kernels: no matrix cores, no persistent launch, no flags, no atomics.
//
// CONVENTIONS.  Those of hip_cg_kernels.h: vectors [rows, q] row-major, matrix blockIdx.y of a batch through
// pickData, one state record (CgState, the same twelve words and stop codes) per (matrix, column), with
// rz = s.z, pAp = delta = |J p|^2 + p^T D p, rr = s.s and bb = |J^T r + c|^2; reductions in two passes in
// double in cgDotPartial's order; every product rounded before it is added.  x, p, s, z live in n-space,
// res = r - J x and t = J p in m-space.  d is the damping vector, d_i = T(alpha colsq_i + beta), colsq_i the
// squared norm of column i of J in double.  An absent operand (r, c, d, x) is a NULL DataRef and its step
// is omitted, not added as a zero.
// FROZEN COLUMNS.  Every kernel that is given the records leaves x, res, s, z, p and the record of a stopped
// column bitwise unchanged; t and the partials are scratch.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "hip_cg_kernels.h"

namespace BaSpaCho {
namespace hipk {

template <typename T>
__device__ __forceinline__ bool cglsGiven(const DataRef<T>& d) {
  return d.single != nullptr || d.many != nullptr;
}

// what the thread or lane that holds the sum of a run does with it
enum CglsEpilogue : int32_t {
  CglsPlain = 0,     // out = sum
  CglsResidual = 1,  // out = radd(a, -sum): res = r - J x (a = r; absent: -sum)
  CglsNormal = 2     // out = radd(radd(sum, -rmul(d, x)), a): s = J^T res - D x + c (a = c)
};

// The run lists of one product on the device, in orderedSumRuns' launch shape
struct CglsRuns {
  int64_t numRuns, numLongWaves;
  int32_t shortWgs;
  const int32_t *start, *longRuns, *entry, *idx;
};

// out[u, j] = epilogue(sum over run u of rmul(values[entry], vec[idx, j])), the sum in list order from +0:
// orderedSumRuns over a DotTerm with its lane path and its wave path (the same sequential sum), then the
// epilogue by the thread or lane that stores.  state NULL: every column; else the stopped ones are skipped.
template <typename T, int kEpi>
__global__ void __launch_bounds__(kAsmThreads)
    cglsProduct(CglsRuns runs, int32_t q, DataRef<const T> vref, DataRef<const T> wref, DataRef<const T> aref,
                DataRef<const T> dref, DataRef<const T> xref, DataRef<T> oref, const CgState* __restrict__ state) {
  const DotTerm<T> terms{runs.entry, runs.idx, vref, wref};
  T s;
  int64_t u;
  int32_t j;
  if ((int32_t)blockIdx.x < runs.shortWgs) {
    const int64_t t = (int64_t)blockIdx.x * kAsmThreads + threadIdx.x;
    if (t >= runs.numRuns * q) return;
    u = t / q;
    j = (int32_t)(t - u * q);
    if (state != nullptr && state[(int64_t)blockIdx.y * q + j].stop != CgRunning) return;
    const int32_t r0 = runs.start[u], r1 = runs.start[u + 1];
    if (isLongRun(r1 - r0)) return;
    s = sumRunByLane(r0, r1, terms.bind(q, j));
  } else {
    const int lane = threadIdx.x & 63;
    const int64_t w = ((int64_t)blockIdx.x - runs.shortWgs) * kAsmWavesPerWg + (int)(threadIdx.x >> 6);
    if (w >= runs.numLongWaves) return;
    const int32_t l = waveUniform((int32_t)(w / q));
    j = waveUniform((int32_t)(w - (int64_t)l * q));
    if (state != nullptr && state[(int64_t)blockIdx.y * q + j].stop != CgRunning) return;
    u = waveUniform(runs.longRuns[l]);
    s = sumRunByWave(waveUniform(runs.start[u]), waveUniform(runs.start[u + 1]), lane, terms.bind(q, j));
    if (lane != 0) return;
  }
  const int64_t at = u * q + j;
  if (kEpi == CglsResidual) {
    s = cglsGiven(aref) ? radd(pickData(aref)[at], -s) : -s;
  } else if (kEpi == CglsNormal) {
    if (cglsGiven(dref)) s = radd(s, -rmul(pickData(dref)[u], pickData(xref)[at]));
    if (cglsGiven(aref)) s = radd(s, pickData(aref)[at]);
  }
  pickData(oref)[at] = s;
}

// colsq[c] = the fold over column c's entries, in ascending entry index from +0, of rmul(double v, double v):
// one thread per short column, one wave per long one
template <typename T>
__global__ void __launch_bounds__(kAsmThreads)
    cglsColSq(CglsRuns runs, DataRef<const T> vref, DataRef<double> oref) {
  const GP<const T> v = pickData(vref);
  const int32_t* __restrict__ e = runs.entry;
  const auto term = [=](int32_t x) { return rmul((double)v[e[x]], (double)v[e[x]]); };
  const GP<double> out = pickData(oref);
  if ((int32_t)blockIdx.x < runs.shortWgs) {
    const int64_t u = (int64_t)blockIdx.x * kAsmThreads + threadIdx.x;
    if (u >= runs.numRuns) return;
    const int32_t r0 = runs.start[u], r1 = runs.start[u + 1];
    if (isLongRun(r1 - r0)) return;
    out[u] = sumRunByLane(r0, r1, term);
    return;
  }
  const int lane = threadIdx.x & 63;
  const int64_t l = ((int64_t)blockIdx.x - runs.shortWgs) * kAsmWavesPerWg + (int)(threadIdx.x >> 6);
  if (l >= runs.numLongWaves) return;
  const int32_t u = waveUniform(runs.longRuns[l]);
  const double s = sumRunByWave(waveUniform(runs.start[u]), waveUniform(runs.start[u + 1]), lane, term);
  if (lane == 0) out[u] = s;
}

// d_i = T(radd(rmul(alpha, colsq_i), beta)), one thread per scalar
template <typename T>
__global__ void __launch_bounds__(kRedThreads)
    cglsDamp(int64_t n, double alpha, double beta, DataRef<const double> cref, DataRef<T> dref) {
  const int64_t i = (int64_t)blockIdx.x * kRedThreads + threadIdx.x;
  if (i >= n) return;
  pickData(dref)[i] = (T)radd(rmul(alpha, pickData(cref)[i]), beta);
}

// Pass 1 of delta = |t|^2 + p^T D p in one launch, the list of column j holding nTotal = mParts + nParts
// partials: workgroups [0, mParts q) take the m-chunks of t.t exactly as cgDotPartial does, the rest the
// n-chunks of rmul(rmul(double p, double p), double d) behind them, in the same order.  Each x = c q + j.
template <typename T>
__global__ void __launch_bounds__(kRedThreads)
    cglsDeltaPartial(int64_t m, int64_t n, int32_t q, int32_t mParts, int32_t nTotal, DataRef<const T> tref,
                     DataRef<const T> pref, DataRef<const T> dref, CgWork work, const CgState* __restrict__ state) {
  __shared__ RedPart red[kRedThreads];
  const int tid = threadIdx.x;
  const bool inM = (int64_t)blockIdx.x < (int64_t)mParts * q;
  const int64_t w = inM ? blockIdx.x : blockIdx.x - (int64_t)mParts * q;
  const int64_t c = w / q;
  const int32_t j = (int32_t)(w - c * q);
  if (state[(int64_t)blockIdx.y * q + j].stop != CgRunning) return;
  RedPart acc{0.0, 1};
  if (inM) {
    const GP<const T> t = pickData(tref);
    cgChunkRows(m, c, tid, [&](int64_t i) {
      const double tv = (double)t[i * q + j];
      acc.v = radd(acc.v, cgProd(tv, tv));
    });
  } else {
    const GP<const T> p = pickData(pref), d = pickData(dref);
    cgChunkRows(n, c, tid, [&](int64_t i) {
      const double pv = (double)p[i * q + j];
      acc.v = radd(acc.v, rmul(rmul(pv, pv), (double)d[i]));
    });
  }
  redFold(red, acc, tid, MergeSum());
  if (tid == 0) work.part()[(int64_t)j * nTotal + (inM ? 0 : mParts) + c] = red[0];
}

// x += alpha p over the n rows and res -= alpha t over the m rows, in one launch: workgroups [0, nParts q)
// take the n-chunks, the rest the m-chunks, each x = c q + j
template <typename T>
__global__ void __launch_bounds__(kRedThreads)
    cglsUpdate(int64_t n, int64_t m, int32_t q, int32_t nParts, DataRef<const T> pref, DataRef<const T> tref,
               DataRef<T> xref, DataRef<T> rref, const CgState* __restrict__ state) {
  const int tid = threadIdx.x;
  const bool inN = (int64_t)blockIdx.x < (int64_t)nParts * q;
  const int64_t w = inN ? blockIdx.x : blockIdx.x - (int64_t)nParts * q;
  const int64_t c = w / q;
  const int32_t j = (int32_t)(w - c * q);
  const CgState& st = state[(int64_t)blockIdx.y * q + j];
  if (st.stop != CgRunning) return;
  const T alpha = (T)st.alpha;
  if (inN) {
    const GP<const T> p = pickData(pref);
    const GP<T> x = pickData(xref);
    cgChunkRows(n, c, tid, [&](int64_t i) {
      const int64_t at = i * q + j;
      x[at] = radd(x[at], rmul(alpha, p[at]));
    });
  } else {
    const GP<const T> t = pickData(tref);
    const GP<T> r = pickData(rref);
    cgChunkRows(m, c, tid, [&](int64_t i) {
      const int64_t at = i * q + j;
      r[at] = radd(r[at], -rmul(alpha, t[at]));
    });
  }
}

// The fold of delta and the two updates in one launch, for bsp_cgls_iterate_*: cglsUpdate's workgroups, each of
// which first folds the nTotal partials of its column exactly as cgFold does (the same sum in every workgroup)
// and takes cgFold's CgFoldAlpha decision from it; the workgroup of the column's first chunk writes pAp, alpha
// and the stop code to the record.  Nobody reads what that workgroup writes but the stop code, and a workgroup
// that sees the new stop code leaves as its own decision would make it leave.
template <typename T>
__global__ void __launch_bounds__(kRedThreads)
    cglsAlphaUpdate(int64_t n, int64_t m, int32_t q, int32_t nParts, int32_t nTotal, DataRef<const T> pref,
                    DataRef<const T> tref, DataRef<T> xref, DataRef<T> rref, CgWork work, CgState* __restrict__ state) {
  __shared__ RedPart red[kRedThreads];
  const int tid = threadIdx.x;
  const bool inN = (int64_t)blockIdx.x < (int64_t)nParts * q;
  const int64_t w = inN ? blockIdx.x : blockIdx.x - (int64_t)nParts * q;
  const int64_t c = w / q;
  const int32_t j = (int32_t)(w - c * q);
  CgState& st = state[(int64_t)blockIdx.y * q + j];
  // (one read per workgroup: another workgroup may write the stop code while this one starts)
  __shared__ int64_t stop;
  if (tid == 0) stop = st.stop;
  __syncthreads();
  if (stop != CgRunning) return;
  const double rz = st.rz;
  const RedPart* part = work.part() + (int64_t)j * nTotal;
  RedPart acc{0.0, 1};
  for (int b = tid; b < nTotal; b += kRedThreads) acc = MergeSum()(acc, part[b]);
  redFold(red, acc, tid, MergeSum());
  const double sum = red[0].v;
  const bool finite = redFinite(sum), go = finite && sum > 0.0;
  if (tid == 0 && c == 0 && (inN || nParts == 0)) {
    st.pAp = sum;
    if (!finite) {
      st.stop = CgNonFinite;
    } else if (!go) {
      st.stop = CgBreakdown;
    } else {
      st.alpha = rz / sum;
    }
  }
  if (!go) return;
  const T alpha = (T)(rz / sum);
  if (inN) {
    const GP<const T> p = pickData(pref);
    const GP<T> x = pickData(xref);
    cgChunkRows(n, c, tid, [&](int64_t i) {
      const int64_t at = i * q + j;
      x[at] = radd(x[at], rmul(alpha, p[at]));
    });
  } else {
    const GP<const T> t = pickData(tref);
    const GP<T> r = pickData(rref);
    cgChunkRows(m, c, tid, [&](int64_t i) {
      const int64_t at = i * q + j;
      r[at] = radd(r[at], -rmul(alpha, t[at]));
    });
  }
}

// z = M^-1 s as cgPrecond does (kKind 0: z is the caller's and only read -- s itself without a
// preconditioner; 1: Jacobi; 2: block-Jacobi), with the partials of s.s in the first list of the column
// (part[j nParts + c]) and those of s.z in the second (part[(q + j) nParts + c])
template <typename T, int kKind>
__global__ void __launch_bounds__(kRedThreads)
    cglsApply(int64_t n, int32_t q, int32_t nParts, CgPrecondDev pl, DataRef<const T> mref, DataRef<const T> sref,
              DataRef<T> zref, CgWork work, const CgState* __restrict__ state) {
  __shared__ RedPart red[kRedThreads];
  const int tid = threadIdx.x;
  const int64_t c = blockIdx.x / q;
  const int32_t j = (int32_t)(blockIdx.x - c * q);
  if (state[(int64_t)blockIdx.y * q + j].stop != CgRunning) return;
  const GP<const T> s = pickData(sref);
  const GP<const T> minv = kKind == 0 ? GP<const T>(nullptr) : pickData(mref);
  const GP<T> z = pickData(zref);
  const bool same = kKind == 0 && (GP<const T>)z == s;  // no preconditioner: z is s itself
  RedPart ss{0.0, 1}, sz{0.0, 1};
  cgChunkRows(n, c, tid, [&](int64_t i) {
    const int64_t at = i * q + j;
    const T si = s[at];
    T zi;
    if (kKind == 0) {
      zi = z[at];
    } else if (kKind == 1) {
      zi = rmul(si, minv[i]);
      z[at] = zi;
    } else {
      const int32_t b = pl.scalarBlock[i];
      const int64_t s0 = pl.blockStart[b], w = pl.blockStart[b + 1] - s0;
      const GP<const T> row = minv + pl.blockOff[b] + (i - s0) * w;
      double a = 0.0;
      for (int64_t k = 0; k < w; k++) a = radd(a, cgProd((double)row[k], (double)s[(s0 + k) * q + j]));
      zi = (T)a;
      z[at] = zi;
    }
    ss.v = radd(ss.v, cgProd((double)si, (double)si));
    if (!same) sz.v = radd(sz.v, cgProd((double)si, (double)zi));
  });
  redFold(red, ss, tid, MergeSum());
  if (tid == 0) work.part()[(int64_t)j * nParts + c] = red[0];
  if (same) {  // s.z is s.s term by term: the same partial
    if (tid == 0) work.part()[((int64_t)q + j) * nParts + c] = red[0];
    return;
  }
  __syncthreads();
  redFold(red, sz, tid, MergeSum());
  if (tid == 0) work.part()[((int64_t)q + j) * nParts + c] = red[0];
}

// Pass 2 of cglsApply and the decision, workgroup (j, matrix): counts the iteration (not at the start);
// ss: non-finite stops with 4, ss <= tol^2 bb with 1, then the step limit with 2; else gamma = s.z:
// non-finite stops with 4, not > 0 with 3; else beta = gamma / gamma(old) (0 before the first iteration)
__global__ void __launch_bounds__(kRedThreads)
    cglsFold(int32_t q, int32_t nParts, bool start, CgWork work, CgState* __restrict__ state) {
  __shared__ RedPart red[kRedThreads];
  const int tid = threadIdx.x;
  const int32_t j = blockIdx.x;
  CgState& st = cgStateOf(state, q, j);
  if (st.stop != CgRunning) return;  // (uniform: the record is not written before the folds)
  const RedPart* p0 = work.part() + (int64_t)j * nParts;
  const RedPart* p1 = work.part() + ((int64_t)q + j) * nParts;
  RedPart acc{0.0, 1};
  for (int b = tid; b < nParts; b += kRedThreads) acc = MergeSum()(acc, p0[b]);
  redFold(red, acc, tid, MergeSum());
  const double ss = red[0].v;
  __syncthreads();
  acc = RedPart{0.0, 1};
  for (int b = tid; b < nParts; b += kRedThreads) acc = MergeSum()(acc, p1[b]);
  redFold(red, acc, tid, MergeSum());
  if (tid != 0) return;
  const double sz = red[0].v;
  if (!start) st.iter++;
  st.rr = ss;
  if (!redFinite(ss)) {
    st.stop = CgNonFinite;
  } else if (ss <= rmul(st.tol2, st.bb)) {
    st.stop = CgConverged;
  } else if (st.iter >= st.maxSteps) {
    st.stop = CgStepLimit;
  } else if (!redFinite(sz)) {
    st.rz = sz;
    st.stop = CgNonFinite;
  } else if (!(sz > 0.0)) {
    st.rz = sz;
    st.stop = CgBreakdown;
  } else {
    st.beta = st.iter > 0 ? sz / st.rz : 0.0;
    st.rz = sz;
  }
}

// ---- the preconditioners of N = J^T J + D ---------------------------------------------------------------
// Jacobi, one thread per scalar: inv_i = T(1 / radd(colsq_i, double(d_i))) (d absent: 1 / colsq_i); a
// denominator that is not positive and finite is a bad pivot with inv = 0
template <typename T>
__global__ void __launch_bounds__(kRedThreads)
    cglsJacobiBuild(int64_t n, DataRef<const double> cref, DataRef<const T> dref, DataRef<T> mref, CgWork work) {
  const int64_t i = (int64_t)blockIdx.x * kRedThreads + threadIdx.x;
  if (i >= n) return;
  double d = pickData(cref)[i];
  if (cglsGiven(dref)) d = radd(d, (double)pickData(dref)[i]);
  const bool ok = d > 0.0 && redFinite(d);
  pickData(mref)[i] = ok ? (T)(1.0 / d) : T(0);
  work.bad()[i] = ok ? -1 : 0;
}

// the item tables of a JacBlockPlan on the device; the block tables are a CgPrecondDev's.  blockWidth: the
// widths of a plan over a subset of the params (block b starts at blockStart[b]), NULL for one over all of them
struct CglsBlockItems {
  const int32_t *itemStart, *itemA, *itemB, *itemPos;
  const int32_t* blockWidth = nullptr;
};

// Block-Jacobi, one wave per block, all in double in LDS: G_ab = the block's items (a >= b) added in list
// order (ascending Jacobian row) from +0, each rmul(double v_ka, double v_kb): 64 items loaded at a time, one
// per lane, and added in rounds, the r-th item of every element in round r, so that an element meets its
// items in list order; double(d) added to the diagonal last; the rest is cgBlockInvert (it reads the lower
// triangle only, so G is not mirrored)
template <typename T>
__global__ void __launch_bounds__(kCgBuildThreads)
    cglsBlockBuild(CgPrecondDev pl, CglsBlockItems it, DataRef<const T> vref, DataRef<const T> dref, DataRef<T> mref,
                   CgWork work) {
  __shared__ double A[kCgMaxBlock * kCgMaxBlock];
  __shared__ double Li[kCgMaxBlock * kCgMaxBlock];
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int32_t s0 = pl.blockStart[b];
  const int w = it.blockWidth != nullptr ? it.blockWidth[b] : pl.blockStart[b + 1] - s0;
  const GP<const T> v = pickData(vref);
  const GP<T> out = pickData(mref) + pl.blockOff[b];
  for (int e = lane; e < w * w; e += kCgBuildThreads) {
    A[e] = 0.0;
    Li[e] = 0.0;
  }
  __syncthreads();
  const int32_t t0 = waveUniform(it.itemStart[b]), t1 = waveUniform(it.itemStart[b + 1]);
  for (int32_t c = t0; c < t1; c += 64) {
    const int cnt = t1 - c < 64 ? (int)(t1 - c) : 64;
    const bool mine = lane < cnt;
    int32_t pos = -1;
    double pr = 0.0;
    if (mine) {
      pos = it.itemPos[c + lane];
      pr = rmul((double)v[it.itemA[c + lane]], (double)v[it.itemB[c + lane]]);
    }
    // rank: how many earlier items of the chunk land on this lane's element (the items of one Jacobian row
    // land on different elements, so the ranks stay small)
    int rank = 0;
    for (int i = 0; i + 1 < cnt; i++) {
      const int32_t pi = __builtin_amdgcn_readlane(pos, i);
      rank += (i < lane && pi == pos) ? 1 : 0;
    }
    // round r adds the r-th item of every element: each element still meets its items in list order
    for (int r = 0; __builtin_amdgcn_ballot_w64(mine && rank >= r) != 0; r++) {
      if (mine && rank == r) A[pos] = radd(A[pos], pr);
      waveSync();
    }
  }
  __syncthreads();
  if (cglsGiven(dref)) {
    const GP<const T> d = pickData(dref);
    if (lane < w) A[lane * w + lane] = radd(A[lane * w + lane], (double)d[s0 + lane]);
  }
  __syncthreads();
  cgBlockInvert<T>(A, Li, w, lane, out, work.bad() + b);
}

}  // namespace hipk
}  // namespace BaSpaCho
