// Kernels of the reach solves (reach.h): W = L^-1 E restricted to the reach of
// every column below the cut, and the Gram blocks W_P^T W_Q.  No atomics, no flags between workgroups:
// a workgroup of reachSolveL only ever touches its own columns of W, a workgroup of gramBlocks only
// its own block of the output.
#pragma once

#include "hip_device_common.h"
#include "reach.h"

namespace BaSpaCho {
namespace hipk {

static_assert(kReachMaxWidth == kPanelWidth, "the cut of the reach plan is the panel width");
static_assert(kReachCols == 16, "reachSolveL gives every wave four columns");

// unit entries of the queries at or beyond the cut, which have no workgroup in reachSolveL
template <typename T>
__global__ __launch_bounds__(256) void reachUnits(const int64_t* unitCol, const int64_t* unitRow, int64_t n, T* Wp,
                                                  int64_t order) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) ((GP<T>)Wp)[unitCol[i] * order + unitRow[i]] = T(1);
}

// One workgroup per column group: x = its k <= 16 unit columns, then for every lump I of the reach, in
// ascending order: x_I <- L_II^-1 x_I (L_II and x_I staged in LDS; a wave substitutes four columns, a
// lane per row, the finished x_j handed round with readlane), and x_row -= L[row, I] x_I for every row
// of the lump column below its diagonal block (a thread per row, sixteen accumulators).  The first
// lump starts at the query's own offset: x is zero above it.  W: column-major, leading dimension
// `order`, zeroed by the caller.
template <typename T>
__global__ __launch_bounds__(256) void reachSolveL(const ReachGroup* groups, const int32_t* reachLumps, SkelDev sk,
                                                   DataRef<const T> lref, T* Wp, int64_t order) {
  constexpr int NB = kPanelWidth, LD = NB + 1, NC = kReachCols;
  __shared__ T Ls[NB * LD];
  __shared__ T xs[NB * NC];
  const ReachGroup g = groups[blockIdx.x];
  GP<const T> data = pickData(lref);
  GP<T> W = (GP<T>)Wp + (int64_t)g.col0 * order;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, k = g.k;
  if (tid < k) W[(int64_t)tid * order + g.row0 + tid] = T(1);
  __syncthreads();
  for (int li = g.listBegin; li < g.listEnd; li++) {
    const int64_t l = reachLumps[li];
    const int64_t ls = sk.lumpStart[l];
    const int n = (int)(sk.lumpStart[l + 1] - ls);
    const int s = li == g.listBegin ? (int)(g.row0 - ls) : 0;
    const int nn = n - s;  // 1 .. 64
    const int64_t cBeg = sk.chainColPtr[l], cEnd = sk.chainColPtr[l + 1];
    GP<const T> Lb = data + sk.chainData[cBeg];  // the lump column: row-major, n columns
    const int64_t x0 = ls + s;
    for (int e = tid; e < nn * nn; e += 256) {
      const int i = e / nn, j = e - i * nn;
      Ls[i * LD + j] = Lb[(int64_t)(s + i) * n + s + j];
    }
    for (int e = tid; e < NB * NC; e += 256) {
      const int i = e & (NB - 1), c = e / NB;
      xs[i * NC + c] = (i < nn && c < k) ? W[(int64_t)c * order + x0 + i] : T(0);
    }
    __syncthreads();
    if (wave * 4 < k) {
      T b[4];
#pragma unroll
      for (int q = 0; q < 4; q++) b[q] = xs[lane * NC + wave * 4 + q];
      const bool mine = lane < nn;
      const T rinv = mine ? T(1) / Ls[lane * LD + lane] : T(0);
      for (int j = 0; j < nn; j++) {
        const T lij = Ls[lane * LD + j];
        const T rj = readLaneT(rinv, j);
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const T xj = readLaneT(b[q], j) * rj;
          if (lane == j) {
            b[q] = xj;
          } else if (mine && lane > j) {
            b[q] = fma(-lij, xj, b[q]);
          }
        }
      }
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int c = wave * 4 + q;
        xs[lane * NC + c] = b[q];
        if (mine && c < k) W[(int64_t)c * order + x0 + lane] = b[q];
      }
    }
    __syncthreads();
    const int64_t rowsTot = sk.chainRowsTillEnd[cEnd - 1];
    for (int64_t r = n + tid; r < rowsTot; r += 256) {
      int64_t lo = cBeg, hi = cEnd - 1;  // the first chain that ends behind row r
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (sk.chainRowsTillEnd[mid] > r) {
          hi = mid;
        } else {
          lo = mid + 1;
        }
      }
      const int64_t grow = sk.spanStart[sk.chainRowSpan[lo]] + (r - sk.chainRowsTillEnd[lo - 1]);
      GP<const T> Lr = Lb + r * n + s;
      T acc[NC];
#pragma unroll
      for (int c = 0; c < NC; c++) acc[c] = T(0);
      for (int j = 0; j < nn; j++) {
        const T v = Lr[j];
#pragma unroll
        for (int c = 0; c < NC; c++) acc[c] = fma(v, xs[j * NC + c], acc[c]);
      }
#pragma unroll
      for (int c = 0; c < NC; c++) {
        if (c < k) W[(int64_t)c * order + grow] -= acc[c];
      }
    }
    // the writes of this lump step before the reads of the next
    __syncthreads();
  }
}

// One workgroup per pair: the nP x nQ block W_P^T W_Q over the item's rows, in 16 x 16 pieces.  The rows
// are taken 64 at a time in the order of the ranges, both operands staged in LDS; wave w sums rows
// 16 w .. 16 w + 15 of every chunk, a lane four elements of the piece; the four partial sums of an
// element are added as (0 + 1) + (2 + 3) and the element is written once: bitwise reproducible.
template <typename T>
__global__ __launch_bounds__(256) void gramBlocks(const GramItem* items, const int64_t* rangeStart,
                                                  const int64_t* rangePrefix, const T* Wp, int64_t order, T* outp) {
  constexpr int LP = 17, LQ = 16;
  __shared__ T tP[64 * LP];
  __shared__ T tQ[64 * LQ];
  __shared__ T red[4 * 256];
  const GramItem it = items[blockIdx.x];
  GP<const T> W = (GP<const T>)Wp;
  GP<T> out = (GP<T>)outp + it.outOff;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, a = lane & 15, bq = lane >> 4;
  for (int p0 = 0; p0 < it.nP; p0 += 16) {
    for (int q0 = 0; q0 < it.nQ; q0 += 16) {
      const int np = min(16, it.nP - p0), nq = min(16, it.nQ - q0);
      T acc[4] = {T(0), T(0), T(0), T(0)};
      for (int64_t v0 = 0; v0 < it.rows; v0 += 64) {
        __syncthreads();
        const int64_t v = v0 + lane;
        int64_t grow = -1;
        if (v < it.rows) {
          int lo = it.rangeBegin, hi = it.rangeEnd - 1;  // the last range that begins at or before row v
          while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (rangePrefix[mid] <= v) {
              lo = mid;
            } else {
              hi = mid - 1;
            }
          }
          grow = rangeStart[lo] + (v - rangePrefix[lo]);
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int c = wave * 4 + i;
          tP[lane * LP + c] = (grow >= 0 && c < np) ? W[(int64_t)(it.colP + p0 + c) * order + grow] : T(0);
          tQ[lane * LQ + c] = (grow >= 0 && c < nq) ? W[(int64_t)(it.colQ + q0 + c) * order + grow] : T(0);
        }
        __syncthreads();
        for (int r = wave * 16; r < wave * 16 + 16; r++) {
          const T pa = tP[r * LP + a];
#pragma unroll
          for (int i = 0; i < 4; i++) acc[i] = fma(pa, tQ[r * LQ + bq * 4 + i], acc[i]);
        }
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 4; i++) red[wave * 256 + a * 16 + bq * 4 + i] = acc[i];
      __syncthreads();
      const int oa = tid >> 4, ob = tid & 15;
      if (oa < np && ob < nq) {
        out[(int64_t)(p0 + oa) * it.nQ + q0 + ob] = (red[tid] + red[256 + tid]) + (red[512 + tid] + red[768 + tid]);
      }
    }
  }
}

}  // namespace hipk
}  // namespace BaSpaCho
