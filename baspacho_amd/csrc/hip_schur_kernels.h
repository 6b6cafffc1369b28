// Implicit Schur elimination for the matrix-free least squares: products with the reduced
// matrix S = C - F^T B^-1 F of N = J^T J + D, the reduction of the right-hand side and the back-substitution,
// over the lists of a JacSchurMap (jac_schur.h).  S and F are never formed.  The inverses of the diagonal blocks
// of B are built by cglsBlockBuild on the map's plan.  Launched by hip_extensions.hip.
// Streaming kernels: no matrix cores, no persistent launch, no flags, no atomics, no scratch, no barrier.
// At the end of the file: the block diagonal of S as preconditioner (section 30), two kernels of one wave per
// workgroup that do stage through LDS behind barriers.
//
// CONVENTIONS.  Those of hip_cgls_kernels.h: vectors [rows, q] row-major, matrix blockIdx.y of a batch through
// pickData, every product rounded before it is added, all in T.  Kept vectors are [nK, q], full ones [n, q], t is
// [m, q].  Binv holds the inverse of block e row-major at blockOff[e].
// ORDERS (part of the interface; tests/schur_ref.py restates them).  With v the values:
//   a_i   = the fold from +0 over row i's kept entries, ascending k, of rmul(v_k, p[kept index of col_k])
//   u_l   = the fold from +0 over eliminated scalar l's entries, ascending k, of rmul(v_k, a[row_k])
//   y_l   = the fold from +0 over l' ascending, inside the param, of rmul(Binv[l, l'], u_l')
//   f_i   = the fold from +0 over row i's eliminated entries, ascending k, of rmul(v_k, y[col_k])
//   product:  t_i = radd(a_i, -f_i) (a row of no group: t_i = a_i); out_c = radd(fold over kept column c of
//             rmul(v_k, t[row_k]), rmul(d_c, p_c)), the last step omitted without d
//   reduce:   u_l = g_l of the full g; t_i = f_i (+0 for a row of no group); b_c = radd(g_c, -fold over kept
//             column c of rmul(v_k, t[row_k]))
//   back:     a, u from x_k as in the product; y = Binv (radd(g_l, -u_l)); x_l = y_l, x_c = x_k[c]
// FROZEN COLUMNS.  Given the records, the columns of a stopped record are skipped: nothing of theirs is written.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "hip_cgls_kernels.h"

namespace BaSpaCho {
namespace hipk {

constexpr int kSchurMaxW = 8;  // widest eliminated param (kSchurMaxElimWidth)

enum SchurMode : int32_t { SchurProduct = 0, SchurReduce = 1, SchurBack = 2 };

// the tables of a JacSchurMap on the device
struct SchurDev {
  int64_t numGroups, numFree, nK;
  const int32_t *groupStart, *groupRow, *freeRows, *elimOff, *elimScalar, *keptScalar;
  const int64_t* blockOff;
  const int32_t *rkStart, *rkEntry, *rkIdx;  // rowsKept
  const int32_t *reStart, *reEntry, *reIdx;  // rowsElim
  const int32_t *ceStart, *ceEntry, *ceIdx;  // colsElim
};

// Eight values of one thread in named registers: at<L>() is element L, schurEach8(f) calls
// f(integral_constant<int, L>) for L = 0 .. 7
template <typename T>
struct SchurRegs {
  T r0, r1, r2, r3, r4, r5, r6, r7;
  template <int L>
  __device__ __forceinline__ T& at() {
    if constexpr (L == 0) return r0;
    else if constexpr (L == 1) return r1;
    else if constexpr (L == 2) return r2;
    else if constexpr (L == 3) return r3;
    else if constexpr (L == 4) return r4;
    else if constexpr (L == 5) return r5;
    else if constexpr (L == 6) return r6;
    else return r7;
  }
};
template <typename F>
__device__ __forceinline__ void schurEach8(F f) {
  f(std::integral_constant<int, 0>());
  f(std::integral_constant<int, 1>());
  f(std::integral_constant<int, 2>());
  f(std::integral_constant<int, 3>());
  f(std::integral_constant<int, 4>());
  f(std::integral_constant<int, 5>());
  f(std::integral_constant<int, 6>());
  f(std::integral_constant<int, 7>());
}
static_assert(kSchurMaxW == 8, "SchurRegs and schurEach8 hold eight values");

// The group kernel: one thread per (group, column j) walks the rows of its eliminated param twice, so that the
// entries of a group are read by one thread and t is the only traffic in m-space; behind them one thread per
// (row of no group, j), and in SchurBack one per (kept scalar, j) for the scatter.  The runs are summed by the
// lane in list order whatever their length (sumRunByLane: sumRunByWave's order).  u stays in registers; y, which
// the second walk indexes by the column of each entry, lies in LDS (element l of thread tid at l 256 + tid, read and
// written by that thread alone: no barrier), as an array of the thread's own would lie in private memory.
// vec: p or x_k [nK, q]
// (SchurProduct, SchurBack); g [n, q] (SchurReduce, SchurBack); out: the full x (SchurBack).
template <typename T, int kMode>
__global__ void __launch_bounds__(kAsmThreads)
    schurGroups(SchurDev sd, int32_t q, DataRef<const T> vref, DataRef<const T> bref, DataRef<const T> wref,
                DataRef<const T> gref, DataRef<T> tref, DataRef<T> oref, const CgState* __restrict__ state) {
  const int64_t id = (int64_t)blockIdx.x * kAsmThreads + threadIdx.x;
  const int64_t nGroup = sd.numGroups * q, nFree = sd.numFree * q;
  const int64_t nScatter = kMode == SchurBack ? sd.nK * q : 0;
  if (id >= nGroup + nFree + nScatter) return;
  const int64_t local = id < nGroup ? id : id < nGroup + nFree ? id - nGroup : id - nGroup - nFree;
  const int64_t unit = local / q;
  const int32_t j = (int32_t)(local - unit * q);
  if (state != nullptr && state[(int64_t)blockIdx.y * q + j].stop != CgRunning) return;
  const GP<T> t = pickData(tref);
  const DotTerm<T> keptTerms{sd.rkEntry, sd.rkIdx, vref, wref};
  if (id >= nGroup + nFree) {  // (SchurBack alone) the kept scalars into the caller's order
    pickData(oref)[(int64_t)sd.keptScalar[unit] * q + j] = pickData(wref)[unit * q + j];
    return;
  }
  if (id >= nGroup) {  // a row of no group
    if (kMode == SchurBack) return;
    const int32_t i = sd.freeRows[unit];
    t[(int64_t)i * q + j] =
        kMode == SchurProduct ? sumRunByLane(sd.rkStart[i], sd.rkStart[i + 1], keptTerms.bind(q, j)) : T(0);
    return;
  }
  const int32_t g0 = sd.groupStart[unit], g1 = sd.groupStart[unit + 1];
  const int32_t l0 = sd.elimOff[unit], w = sd.elimOff[unit + 1] - l0;
  const GP<const T> v = pickData(vref);
  __shared__ T ys[kMode == SchurBack ? 1 : kSchurMaxW * kAsmThreads];
  SchurRegs<T> u{};
  if (kMode != SchurReduce) {
    for (int32_t x = g0; x < g1; x++) {
      const int32_t i = sd.groupRow[x];
      t[(int64_t)i * q + j] = sumRunByLane(sd.rkStart[i], sd.rkStart[i + 1], keptTerms.bind(q, j));
    }
    const int32_t* __restrict__ ce = sd.ceEntry;
    const int32_t* __restrict__ ci = sd.ceIdx;
    schurEach8([&](auto L) {
      constexpr int l = decltype(L)::value;
      if (l < w) {
        // (t's elements of this group were written by this thread)
        u.template at<l>() = sumRunByLane(sd.ceStart[l0 + l], sd.ceStart[l0 + l + 1],
                                          [=](int32_t z) { return rmul(v[ce[z]], t[(int64_t)ci[z] * q + j]); });
      }
    });
  }
  if (kMode != SchurProduct) {
    const GP<const T> g = pickData(gref);
    schurEach8([&](auto L) {
      constexpr int l = decltype(L)::value;
      const T gl = l < w ? g[(int64_t)sd.elimScalar[l0 + l] * q + j] : T(0);
      u.template at<l>() = kMode == SchurReduce ? gl : radd(gl, -u.template at<l>());
    });
  }
  const GP<const T> binv = pickData(bref) + sd.blockOff[unit];
  const int tid = threadIdx.x;
  schurEach8([&](auto L) {
    constexpr int l = decltype(L)::value;
    if (l < w) {
      T s = T(0);
      schurEach8([&](auto K) {
        constexpr int k = decltype(K)::value;
        if (k < w) s = radd(s, rmul(binv[l * w + k], u.template at<k>()));
      });
      if (kMode == SchurBack) {
        pickData(oref)[(int64_t)sd.elimScalar[l0 + l] * q + j] = s;
      } else {
        ys[l * kAsmThreads + tid] = s;
      }
    }
  });
  if (kMode == SchurBack) return;
  const int32_t* __restrict__ re = sd.reEntry;
  const int32_t* __restrict__ ri = sd.reIdx;
  for (int32_t x = g0; x < g1; x++) {
    const int32_t i = sd.groupRow[x];
    const T f = sumRunByLane(sd.reStart[i], sd.reStart[i + 1],
                             [&](int32_t z) { return rmul(v[re[z]], ys[(ri[z] - l0) * kAsmThreads + tid]); });
    const int64_t at = (int64_t)i * q + j;
    t[at] = kMode == SchurProduct ? radd(t[at], -f) : f;
  }
}

// The product over the kept columns with its epilogue: cglsProduct's two paths over colsKept (vec = t), then
// SchurProduct: out_c = radd(sum, rmul(d[keptScalar c], p_c)) (d absent: the sum); SchurReduce: out_c =
// radd(g[keptScalar c], -sum)
template <typename T, int kMode>
__global__ void __launch_bounds__(kAsmThreads)
    schurKeptColumns(CglsRuns runs, const int32_t* __restrict__ keptScalar, int32_t q, DataRef<const T> vref,
                     DataRef<const T> tref, DataRef<const T> dref, DataRef<const T> xref, DataRef<T> oref,
                     const CgState* __restrict__ state) {
  const DotTerm<T> terms{runs.entry, runs.idx, vref, tref};
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
  if (kMode == SchurProduct) {
    if (cglsGiven(dref)) s = radd(s, rmul(pickData(dref)[keptScalar[u]], pickData(xref)[at]));
  } else {
    s = radd(pickData(xref)[(int64_t)keptScalar[u] * q + j], -s);
  }
  pickData(oref)[at] = s;
}

// The Jacobi preconditioner of S on the kept scalars, one thread per kept scalar c at the caller's scalar s:
// cglsJacobiBuild's rule, inv_c = T(1 / radd(colsq_s, double(d_s))) (d absent: 1 / colsq_s), the diagonal of C; a
// denominator that is not positive and finite is a bad pivot with inv = 0
template <typename T>
__global__ void __launch_bounds__(kRedThreads)
    schurJacobiBuild(int64_t nK, const int32_t* __restrict__ keptScalar, DataRef<const double> cref,
                     DataRef<const T> dref, DataRef<T> mref, CgWork work) {
  const int64_t c = (int64_t)blockIdx.x * kRedThreads + threadIdx.x;
  if (c >= nK) return;
  const int32_t s = keptScalar[c];
  double d = pickData(cref)[s];
  if (cglsGiven(dref)) d = radd(d, (double)pickData(dref)[s]);
  const bool ok = d > 0.0 && redFinite(d);
  pickData(mref)[c] = ok ? (T)(1.0 / d) : T(0);
  work.bad()[c] = ok ? -1 : 0;
}

// ---- the block diagonal of S: "schur_jacobi"  ---------------------------------------
// S_bb = D_bb + sum over the pairs (e, b) of W_eb + sum over the pseudo-pairs of G, W_eb = G_eb - F_eb^T Binv_e
// F_eb, over the tables of a JacSchurJacobiPlan (jac_schur.h).  Two launches, no atomics, all in double for both T.
// ORDERS (part of the interface; tests/schur_jacobi_ref.py restates them).  v(i, s): the value of the pair-row's
// record at scalar s, a term existing only where both of its entries do.  Every sum is a left fold from +0:
//   G[a, c] = over the pair's rows, ascending, of rmul(v(i, a), v(i, c))         (a >= c in b)
//   F[l, c] = over the pair's rows, ascending, of rmul(v(i, l), v(i, c))         (l in e, c in b)
//   Y[l, c] = over l' ascending of rmul(Binv[l, l'], F[l', c])
//   E[a, c] = over l ascending of rmul(F[l, a], Y[l, c]);  W[a, c] = radd(G[a, c], -E[a, c]) (a pseudo-pair: G)
//   P[a, c] = over the chunk's pairs in list order of W[a, c];  A[a, c] = over b's chunks, ascending, of P[a, c]
//   A[a, a] = radd(A[a, a], double(d[s0 + a])) where d is given; then cgBlockInvert
constexpr int kSjThreads = 64;                                         // one wave per chunk
constexpr int kSjMaxTri = kCgMaxBlock * (kCgMaxBlock + 1) / 2;         // lower-triangle elements of the widest block
constexpr int kSjPerLane = (kSjMaxTri + kSjThreads - 1) / kSjThreads;  // ... of one lane: 9
constexpr int kSjMaxF = kSchurMaxW * kCgMaxBlock;                      // elements of the widest F
constexpr int kSjFPerLane = kSjMaxF / kSjThreads;                      // ... of one lane: 4
constexpr int kSjMaxRec = kCgMaxBlock + kSchurMaxW;                    // widest record
constexpr int kSjRowBatch = 8;                                         // pair-rows staged in LDS at a time

struct SchurJacobiDev {
  const int32_t *chunkPair, *chunkBlock;
  const int64_t* chunkPart;
  const int32_t *pairElim, *pairRow, *pairRec, *rec;
  const int32_t *keptWidth, *keptFirst, *elimOff, *blockChunk;
  const int64_t *elimBlockOff, *blockOff;
};

// (a, c), a >= c, of lower-triangle element el = a (a + 1) / 2 + c, packed as a | c << 8
__device__ __forceinline__ int sjElement(int el) {
  int a = 0;
  while ((a + 1) * (a + 2) / 2 <= el) a++;
  return a | ((el - a * (a + 1) / 2) << 8);
}

// The chunk kernel, one wave per (chunk, matrix): the pairs of the chunk in list order; a lane keeps the running
// sums P of its elements lane + 64 r in registers.  The rows of a pair are walked serially, kSjRowBatch of them
// staged in LDS at a time (entry index and value of every record slot); F and Y go through LDS.
template <typename T>
__global__ void __launch_bounds__(kSjThreads)
    schurJacobiChunks(SchurJacobiDev sj, DataRef<const T> vref, DataRef<const T> bref, DataRef<double> pref) {
  __shared__ double rowv[kSjRowBatch * kSjMaxRec];
  __shared__ int32_t rowk[kSjRowBatch * kSjMaxRec];
  __shared__ double Fs[kSjMaxF], Ys[kSjMaxF], Bs[kSchurMaxW * kSchurMaxW];
  const int lane = threadIdx.x;
  const int64_t h = blockIdx.x;
  const int32_t b = sj.chunkBlock[h];
  const int w = sj.keptWidth[b], tri = w * (w + 1) / 2;
  const GP<const T> v = pickData(vref);
  int ac[kSjPerLane], lc[kSjFPerLane];
  double P[kSjPerLane];
#pragma unroll
  for (int r = 0; r < kSjPerLane; r++) {
    const int el = lane + kSjThreads * r;
    ac[r] = el < tri ? sjElement(el) : 0;
    P[r] = 0.0;
  }
#pragma unroll
  for (int r = 0; r < kSjFPerLane; r++) {
    const int el = lane + kSjThreads * r, l = el / w;
    lc[r] = l | ((el - l * w) << 8);
  }
  const int32_t p0 = sj.chunkPair[h], p1 = sj.chunkPair[h + 1];
  for (int32_t p = p0; p < p1; p++) {
    const int32_t e = sj.pairElim[p];
    int we = 0;
    if (e >= 0) {
      const int32_t l0 = sj.elimOff[e];
      we = sj.elimOff[e + 1] - l0;
      // (the Bs of the pair before were last read ahead of a barrier of that pair)
      if (lane < we * we) Bs[lane] = (double)pickData(bref)[sj.elimBlockOff[e] + lane];
    }
    const int wt = w + we, nf = we * w;
    const int32_t r0 = sj.pairRow[p], r1 = sj.pairRow[p + 1];
    const int32_t* __restrict__ rec = sj.rec + sj.pairRec[p];
    double G[kSjPerLane], F[kSjFPerLane];
#pragma unroll
    for (int r = 0; r < kSjPerLane; r++) G[r] = 0.0;
#pragma unroll
    for (int r = 0; r < kSjFPerLane; r++) F[r] = 0.0;
    for (int32_t rb = r0; rb < r1; rb += kSjRowBatch) {
      const int nr = r1 - rb < kSjRowBatch ? (int)(r1 - rb) : kSjRowBatch;
      __syncthreads();  // the batch before is consumed
      for (int x = lane; x < nr * wt; x += kSjThreads) {
        const int32_t k = rec[(int64_t)(rb - r0) * wt + x];
        rowk[x] = k;
        rowv[x] = k >= 0 ? (double)v[k] : 0.0;
      }
      __syncthreads();
      for (int i = 0; i < nr; i++) {
        const double* rv = rowv + i * wt;
        const int32_t* rk = rowk + i * wt;
#pragma unroll
        for (int r = 0; r < kSjPerLane; r++) {
          const int a = ac[r] & 255, c = ac[r] >> 8;
          if (lane + kSjThreads * r < tri && rk[a] >= 0 && rk[c] >= 0) G[r] = radd(G[r], rmul(rv[a], rv[c]));
        }
#pragma unroll
        for (int r = 0; r < kSjFPerLane; r++) {
          const int l = lc[r] & 255, c = lc[r] >> 8;
          if (lane + kSjThreads * r < nf && rk[w + l] >= 0 && rk[c] >= 0) F[r] = radd(F[r], rmul(rv[w + l], rv[c]));
        }
      }
    }
    if (e < 0) {  // a pseudo-pair: W = G  (uniform)
#pragma unroll
      for (int r = 0; r < kSjPerLane; r++) P[r] = radd(P[r], G[r]);
      continue;
    }
    __syncthreads();  // the F and Y of the pair before are consumed
#pragma unroll
    for (int r = 0; r < kSjFPerLane; r++) {
      if (lane + kSjThreads * r < nf) Fs[lane + kSjThreads * r] = F[r];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kSjFPerLane; r++) {
      if (lane + kSjThreads * r < nf) {
        const int l = lc[r] & 255, c = lc[r] >> 8;
        double s = 0.0;
        for (int k = 0; k < we; k++) s = radd(s, rmul(Bs[l * we + k], Fs[k * w + c]));
        Ys[lane + kSjThreads * r] = s;
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kSjPerLane; r++) {
      if (lane + kSjThreads * r < tri) {
        const int a = ac[r] & 255, c = ac[r] >> 8;
        double s = 0.0;
        for (int l = 0; l < we; l++) s = radd(s, rmul(Fs[l * w + a], Ys[l * w + c]));
        P[r] = radd(P[r], radd(G[r], -s));
      }
    }
  }
  const GP<double> out = pickData(pref) + sj.chunkPart[h];
#pragma unroll
  for (int r = 0; r < kSjPerLane; r++) {
    if (lane + kSjThreads * r < tri) out[lane + kSjThreads * r] = P[r];
  }
}

// The block kernel, one wave per (kept block, matrix): the chunk partials folded in ascending chunk, d added to the
// diagonal, cgBlockInvert (it reads the lower triangle only)
template <typename T>
__global__ void __launch_bounds__(kCgBuildThreads)
    schurJacobiBlocks(SchurJacobiDev sj, DataRef<const double> pref, DataRef<const T> dref, DataRef<T> mref,
                      CgWork work) {
  __shared__ double A[kCgMaxBlock * kCgMaxBlock];
  __shared__ double Li[kCgMaxBlock * kCgMaxBlock];
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int w = sj.keptWidth[b], tri = w * (w + 1) / 2;
  for (int x = lane; x < w * w; x += kCgBuildThreads) {
    A[x] = 0.0;
    Li[x] = 0.0;
  }
  __syncthreads();
  const GP<const double> part = pickData(pref);
  const int32_t h0 = sj.blockChunk[b], h1 = sj.blockChunk[b + 1];
  for (int el = lane; el < tri; el += kCgBuildThreads) {
    const int at = sjElement(el);
    double s = 0.0;
    for (int32_t h = h0; h < h1; h++) s = radd(s, part[sj.chunkPart[h] + el]);
    A[(at & 255) * w + (at >> 8)] = s;
  }
  __syncthreads();
  if (cglsGiven(dref)) {
    const GP<const T> d = pickData(dref);
    if (lane < w) A[lane * w + lane] = radd(A[lane * w + lane], (double)d[sj.keptFirst[b] + lane]);
  }
  __syncthreads();
  cgBlockInvert<T>(A, Li, w, lane, pickData(mref) + sj.blockOff[b], work.bad() + b);
}

}  // namespace hipk
}  // namespace BaSpaCho
