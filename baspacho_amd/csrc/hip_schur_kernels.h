// Implicit Schur elimination for the matrix-free least squares: products with the reduced
// matrix S = C - F^T B^-1 F of N = J^T J + D, the reduction of the right-hand side and the back-substitution,
// over the lists of a JacSchurMap (jac_schur.h).  S and F are never formed.  The inverses of the diagonal blocks
// of B are built by cglsBlockBuild on the map's plan.  Launched by hip_extensions.hip.
// Streaming kernels: no matrix cores, no persistent launch, no flags, no atomics, no scratch, no barrier.
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

}  // namespace hipk
}  // namespace BaSpaCho
