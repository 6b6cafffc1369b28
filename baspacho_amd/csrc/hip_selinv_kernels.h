// Selected inversion (Takahashi recurrence) on the factor's own storage: Z = A^-1 restricted to the
// block pattern of L overwrites L in place.  Plan: hip_plan.h (SelInvPlanHost); schedule and launch:
// hip_backend.hip (HipSymbolicCtx::selectedInverse); algorithm: DESIGN.md, "Selected inversion".
//
// A NODE is a column block [c0, c0 + w) of one lump (w <= kSelInvW).  R = every row of the lump column
// below the block: first the rest of the lump's own diagonal block (nRest rows), then its chain rows.
// Row a of R is row c1 + a of the lump column (c1 = c0 + w), so the node's L_RI is simply
// data[lumpOff + (c1 + a) * lda + c0 + j].  For a node, with Linv = L_II^-1:
//   U    = L_RI Linv                        (r x w)
//   Z_RI = -Z_RR U                          (Z_RR gathered: own trailing block / own chain rows /
//                                             blocks of the lumps that own the chain rows)
//   Z_II = Linv^T Linv - U^T Z_RI           (written full and symmetric)
// Every element of Z has exactly one writer and every sum runs in a fixed order: the result is
// bitwise reproducible.
//
// BATCH: every kernel runs the same launch for `gridDim.y` matrices of one structure.  Matrix
// q = blockIdx.y finds its data through pickData (hip_kernels.h: the GP<T> pointer keeps the global
// address space down to the access) and uses slice q of every scratch buffer (SelInvStrides).  The
// arithmetic of a matrix does not depend on q: member q of a batch is bitwise a single call (a single
// call is DataRef{data, nullptr} with gridDim.y = 1).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "hip_device_common.h"
#include "hip_plan.h"

namespace BaSpaCho {
namespace hipk {

// elements per matrix of each selected-inversion scratch buffer (the plan's linvElems (Linv and DD),
// uElems, pElems, wElems): matrix blockIdx.y of a batch works in slice blockIdx.y
struct SelInvStrides {
  int64_t linv, u, p, w;
};

// Z(a, b) of a node's R x R block, a and b row indices of R (any order).  Own-lump columns (b < nRest)
// are read from the lump column itself: the trailing diagonal block is stored full and symmetric, the
// chain rows below it hold Z_RI of the blocks to the right.  Chain x chain entries go through the
// node's pair table (block of span sa in the column of span sb's lump, (0,0) offset and stride).
__device__ __forceinline__ int64_t selinvZAddr(const SelInvNode& nd, const int32_t* __restrict__ rowChain,
                                               const int32_t* __restrict__ rowLocal,
                                               const int64_t* __restrict__ pairOff,
                                               const int32_t* __restrict__ pairStr, int a, int b) {
  const int64_t c1 = nd.c0 + nd.w;
  if (b < nd.nRest) return nd.lumpOff + (c1 + a) * nd.lda + c1 + b;
  if (a < nd.nRest) return nd.lumpOff + (c1 + b) * nd.lda + c1 + a;
  const int ia = nd.rowBase + a - nd.nRest, ib = nd.rowBase + b - nd.nRest;
  const int ka = rowChain[ia], kb = rowChain[ib];
  const int la = rowLocal[ia], lb = rowLocal[ib];
  if (ka >= kb) {
    const int64_t p = nd.pairBase + (int64_t)ka * (ka + 1) / 2 + kb;
    return pairOff[p] + (int64_t)la * pairStr[p] + lb;
  }
  const int64_t p = nd.pairBase + (int64_t)kb * (kb + 1) / 2 + ka;
  return pairOff[p] + (int64_t)lb * pairStr[p] + la;
}

// S1: per node, Linv = L_II^-1 (lower) and DD = Linv^T Linv, both kSelInvW x kSelInvW in scratch
// (zero outside w x w).  One workgroup of 256 per node.
template <typename T>
__global__ void __launch_bounds__(256) selinvDiagInverse(const SelInvNode* __restrict__ nodes,
                                                         DataRef<T> dref, T* __restrict__ linv,
                                                         T* __restrict__ dd, SelInvStrides st) {
  constexpr int W = kSelInvW;
  __shared__ T Ls[W][W + 1];
  __shared__ T Xs[W][W + 1];
  const GP<T> data = pickData(dref);
  linv += (int64_t)blockIdx.y * st.linv;
  dd += (int64_t)blockIdx.y * st.linv;
  const SelInvNode nd = nodes[blockIdx.x];
  const int w = nd.w, tid = threadIdx.x;
  for (int e = tid; e < W * W; e += 256) {
    const int i = e / W, j = e % W;
    Ls[i][j] = (i < w && j <= i) ? data[nd.lumpOff + (int64_t)(nd.c0 + i) * nd.lda + nd.c0 + j] : T(0);
    Xs[i][j] = T(0);
  }
  __syncthreads();
  if (tid < w) {  // column tid of the inverse: forward substitution
    const int j = tid;
    for (int i = j; i < w; i++) {
      T s = (i == j) ? T(1) : T(0);
      for (int k = j; k < i; k++) s -= Ls[i][k] * Xs[k][j];
      Xs[i][j] = s / Ls[i][i];
    }
  }
  __syncthreads();
  T* lo = linv + (int64_t)blockIdx.x * W * W;
  T* ddo = dd + (int64_t)blockIdx.x * W * W;
  for (int e = tid; e < W * W; e += 256) {
    const int i = e / W, j = e % W;
    lo[e] = Xs[i][j];
    T s = T(0);
    for (int k = (i > j ? i : j); k < w; k++) s += Xs[k][i] * Xs[k][j];
    ddo[e] = s;
  }
}

// S2: U[a, :] = L_RI[a, :] Linv for a 64-row tile of a node (task = node, first row)
template <typename T>
__global__ void __launch_bounds__(256) selinvFormU(const SelInvNode* __restrict__ nodes,
                                                   const int2* __restrict__ tasks,
                                                   DataRef<T> dref, const T* __restrict__ linv,
                                                   T* __restrict__ U, SelInvStrides st) {
  constexpr int W = kSelInvW;
  __shared__ T Xs[W][W + 1];
  __shared__ T Rs[64][W + 1];
  const GP<T> data = pickData(dref);
  linv += (int64_t)blockIdx.y * st.linv;
  U += (int64_t)blockIdx.y * st.u;
  const int2 tk = tasks[blockIdx.x];
  const SelInvNode nd = nodes[tk.x];
  const int a0 = tk.y, w = nd.w, tid = threadIdx.x;
  const int rows = min(64, nd.r - a0);
  const T* lo = linv + (int64_t)tk.x * W * W;
  for (int e = tid; e < W * W; e += 256) Xs[e / W][e % W] = lo[e];
  for (int e = tid; e < 64 * W; e += 256) {
    const int i = e / W, j = e % W;
    Rs[i][j] = (i < rows && j < w)
                   ? data[nd.lumpOff + (int64_t)(nd.c0 + w + a0 + i) * nd.lda + nd.c0 + j]
                   : T(0);
  }
  __syncthreads();
  for (int e = tid; e < 64 * W; e += 256) {
    const int i = e / W, j = e % W;
    if (i >= rows) continue;
    T s = T(0);
    for (int k = j; k < w; k++) s += Rs[i][k] * Xs[k][j];
    U[nd.uOff + (int64_t)(a0 + i) * W + j] = s;
  }
}

// S3: partial products P[kc][a, :] = sum_{b in chunk kc} Z(a, b) U[b, :] of a 64-row tile
// (task = node, first row, chunk).  16 x 16 threads, 4 x 4 outputs each, 16 source rows per step.
template <typename T>
__global__ void __launch_bounds__(256) selinvZrrTimesU(
    const SelInvNode* __restrict__ nodes, const int4* __restrict__ tasks,
    const int32_t* __restrict__ rowChain, const int32_t* __restrict__ rowLocal,
    const int64_t* __restrict__ pairOff, const int32_t* __restrict__ pairStr,
    DataRef<T> dref, const T* __restrict__ U, T* __restrict__ P, SelInvStrides st) {
  constexpr int W = kSelInvW, KB = 16;
  __shared__ T Zs[KB][64 + 1];  // Zs[kb][row]
  __shared__ T Us[KB][W + 1];
  const GP<T> data = pickData(dref);
  U += (int64_t)blockIdx.y * st.u;
  P += (int64_t)blockIdx.y * st.p;
  const int4 tk = tasks[blockIdx.x];
  const SelInvNode nd = nodes[tk.x];
  const int a0 = tk.y, tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  const int rows = min(64, nd.r - a0);
  const int b0 = tk.z * nd.kChunk, b1 = min(nd.r, b0 + nd.kChunk);
  T acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = T(0);
  for (int bb = b0; bb < b1; bb += KB) {
    // Z tile: 64 rows x 16 columns; lanes run along the columns (contiguous for own-lump columns)
    for (int e = tid; e < 64 * KB; e += 256) {
      const int i = e / KB, k = e % KB, b = bb + k;
      Zs[k][i] = (i < rows && b < b1)
                     ? data[selinvZAddr(nd, rowChain, rowLocal, pairOff, pairStr, a0 + i, b)]
                     : T(0);
    }
    for (int e = tid; e < KB * W; e += 256) {
      const int k = e / W, j = e % W, b = bb + k;
      Us[k][j] = b < b1 ? U[nd.uOff + (int64_t)b * W + j] : T(0);
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < KB; k++) {
      T zr[4], ur[4];
#pragma unroll
      for (int i = 0; i < 4; i++) zr[i] = Zs[k][ty + 16 * i];
#pragma unroll
      for (int j = 0; j < 4; j++) ur[j] = Us[k][tx + 16 * j];
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] += zr[i] * ur[j];
    }
    __syncthreads();
  }
  T* po = P + nd.pOff + (int64_t)tk.z * nd.r * W;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int a = ty + 16 * i;
    if (a >= rows) continue;
#pragma unroll
    for (int j = 0; j < 4; j++) po[(int64_t)(a0 + a) * W + tx + 16 * j] = acc[i][j];
  }
}

// S4: Z_RI = -sum_kc P[kc] of a 64-row tile, written over L_RI (and, for rows inside the lump's own
// diagonal block, also transposed into its upper triangle), plus the tile's share of U^T Z_RI
// (W x W, to scratch slot `tile`).  Task = node, first row; task index = slot.
template <typename T>
__global__ void __launch_bounds__(256) selinvReduceZ(const SelInvNode* __restrict__ nodes,
                                                     const int2* __restrict__ tasks,
                                                     DataRef<T> dref, const T* __restrict__ U,
                                                     const T* __restrict__ P, T* __restrict__ Wp,
                                                     SelInvStrides st) {
  constexpr int W = kSelInvW;
  __shared__ T Zt[64][W + 1];
  __shared__ T Ut[64][W + 1];
  const GP<T> data = pickData(dref);
  U += (int64_t)blockIdx.y * st.u;
  P += (int64_t)blockIdx.y * st.p;
  Wp += (int64_t)blockIdx.y * st.w;
  const int2 tk = tasks[blockIdx.x];
  const SelInvNode nd = nodes[tk.x];
  const int a0 = tk.y, w = nd.w, tid = threadIdx.x;
  const int rows = min(64, nd.r - a0);
  const int64_t c1 = nd.c0 + w;
  for (int e = tid; e < 64 * W; e += 256) {
    const int i = e / W, j = e % W;
    T z = T(0), u = T(0);
    if (i < rows) {
      const int64_t a = a0 + i;
      for (int kc = 0; kc < nd.nk; kc++) z -= P[nd.pOff + ((int64_t)kc * nd.r + a) * W + j];
      u = U[nd.uOff + a * W + j];
      if (j < w) {
        data[nd.lumpOff + (c1 + a) * nd.lda + nd.c0 + j] = z;
        if (a < nd.nRest) data[nd.lumpOff + (int64_t)(nd.c0 + j) * nd.lda + c1 + a] = z;
      }
    }
    Zt[i][j] = z;
    Ut[i][j] = u;
  }
  __syncthreads();
  T* wo = Wp + (int64_t)blockIdx.x * W * W;
  for (int e = tid; e < W * W; e += 256) {
    const int i = e / W, j = e % W;
    T s = T(0);
    for (int k = 0; k < rows; k++) s += Ut[k][i] * Zt[k][j];
    wo[e] = s;
  }
}

// S5: Z_II = DD - sum over the node's tiles of U^T Z_RI, written full and symmetric (the lower
// triangle is computed, the upper one mirrored: symmetric to the last bit)
template <typename T>
__global__ void __launch_bounds__(256) selinvDiagBlock(const SelInvNode* __restrict__ nodes,
                                                       DataRef<T> dref, const T* __restrict__ dd,
                                                       const T* __restrict__ Wp, SelInvStrides st) {
  constexpr int W = kSelInvW;
  const GP<T> data = pickData(dref);
  dd += (int64_t)blockIdx.y * st.linv;
  Wp += (int64_t)blockIdx.y * st.w;
  const SelInvNode nd = nodes[blockIdx.x];
  const int w = nd.w;
  for (int e = threadIdx.x; e < W * W; e += 256) {
    const int i = e / W, j = e % W;
    if (i >= w || j > i) continue;
    T s = dd[(int64_t)blockIdx.x * W * W + e];
    for (int t = 0; t < nd.nTiles; t++) s -= Wp[(int64_t)(nd.tileBase + t) * W * W + i * W + j];
    data[nd.lumpOff + (int64_t)(nd.c0 + i) * nd.lda + nd.c0 + j] = s;
    data[nd.lumpOff + (int64_t)(nd.c0 + j) * nd.lda + nd.c0 + i] = s;
  }
}

// ------------------------------------------------------------------------------------------
// Small lumps (width <= kSelInvSmallW, <= kSelInvSmallChains chains below, r * n <= kSelInvSmallElems):
// the whole recurrence of one lump in one wave, operands in LDS.  The chain-pair table of the lump is
// found on the device (binary search of span sa in the chain list of span sb's lump), so the plan
// holds one 16-byte descriptor per lump.
template <typename T>
__global__ void __launch_bounds__(64) selinvSmallLumps(const SelInvSmall* __restrict__ lumps,
                                                       SkelDev sk, DataRef<T> dref) {
  constexpr int NW = kSelInvSmallW, NC = kSelInvSmallChains, NE = kSelInvSmallElems;
  static_assert(NC < 256, "chain ordinals are stored in bytes");
  __shared__ T Xs[NW][NW + 1];
  __shared__ T Us[NE];
  __shared__ T Zr[NE];
  __shared__ int64_t pOff[NC * (NC + 1) / 2];
  __shared__ int32_t pStr[NC * (NC + 1) / 2];
  __shared__ int32_t cRow0[NC + 1];
  __shared__ uint8_t rowK[NE];
  __shared__ int16_t rowL[NE];
  const GP<T> data = pickData(dref);
  const SelInvSmall ls = lumps[blockIdx.x];
  const int n = ls.n, r = ls.r, k = ls.k, lane = threadIdx.x;
  const int64_t cBeg = ls.chainBegin;
  // chains below the diagonal: first row in R
  if (lane < k) {
    const int64_t c = cBeg + lane;
    const int64_t s = sk.chainRowSpan[c];
    cRow0[lane] = (int)(sk.chainRowsTillEnd[c] - (sk.spanStart[s + 1] - sk.spanStart[s]) - n);
  }
  if (lane == 0) cRow0[k] = r;
  // pair table: for ka >= kb, the block of span sa in the column of span sb's lump
  for (int p = lane; p < k * (k + 1) / 2; p += 64) {
    int ka = 0;
    while ((ka + 1) * (ka + 2) / 2 <= p) ka++;
    const int kb = p - ka * (ka + 1) / 2;
    const int64_t sa = sk.chainRowSpan[cBeg + ka], sb = sk.chainRowSpan[cBeg + kb];
    const int64_t J = sk.spanToLump[sb];
    int64_t lo = sk.chainColPtr[J], hi = sk.chainColPtr[J + 1] - 1;
    while (lo < hi) {  // the block exists: the rows of a lump form a clique in the factor's pattern
      const int64_t mid = (lo + hi) / 2;
      if (sk.chainRowSpan[mid] < sa) lo = mid + 1; else hi = mid;
    }
    pOff[p] = sk.chainData[lo] + sk.spanStart[sb] - sk.lumpStart[J];
    pStr[p] = (int32_t)(sk.lumpStart[J + 1] - sk.lumpStart[J]);
  }
  // diagonal block and the rows below it
  for (int e = lane; e < NW * NW; e += 64) {
    const int i = e / NW, j = e % NW;
    Xs[i][j] = T(0);
  }
  for (int e = lane; e < r * n; e += 64) Zr[e] = data[ls.diagOff + (int64_t)n * n + e];
  __syncthreads();
  for (int a = lane; a < r; a += 64) {
    int kk = 0;
    while (cRow0[kk + 1] <= a) kk++;
    rowK[a] = (uint8_t)kk;
    rowL[a] = (int16_t)(a - cRow0[kk]);
  }
  if (lane < n) {  // column `lane` of L_II^-1
    const int j = lane;
    for (int i = j; i < n; i++) {
      T s = (i == j) ? T(1) : T(0);
      for (int q = j; q < i; q++) s -= data[ls.diagOff + i * n + q] * Xs[q][j];
      Xs[i][j] = s / data[ls.diagOff + i * n + i];
    }
  }
  __syncthreads();
  for (int e = lane; e < r * n; e += 64) {
    const int a = e / n, j = e % n;
    T s = T(0);
    for (int q = j; q < n; q++) s += Zr[a * n + q] * Xs[q][j];
    Us[e] = s;
  }
  __syncthreads();
  for (int a = lane; a < r; a += 64) {
    T acc[NW];
#pragma unroll
    for (int j = 0; j < NW; j++) acc[j] = T(0);
    const int ka = rowK[a], la = rowL[a];
    for (int b = 0; b < r; b++) {
      const int kb = rowK[b], lb = rowL[b];
      int64_t addr;
      if (ka >= kb) {
        const int p = ka * (ka + 1) / 2 + kb;
        addr = pOff[p] + (int64_t)la * pStr[p] + lb;
      } else {
        const int p = kb * (kb + 1) / 2 + ka;
        addr = pOff[p] + (int64_t)lb * pStr[p] + la;
      }
      const T z = data[addr];
#pragma unroll
      for (int j = 0; j < NW; j++)
        if (j < n) acc[j] += z * Us[b * n + j];
    }
#pragma unroll
    for (int j = 0; j < NW; j++)
      if (j < n) Zr[a * n + j] = -acc[j];
  }
  __syncthreads();
  for (int e = lane; e < r * n; e += 64) data[ls.diagOff + (int64_t)n * n + e] = Zr[e];
  for (int e = lane; e < n * n; e += 64) {
    const int i = e / n, j = e % n;
    if (j > i) continue;
    T s = T(0);
    for (int q = i; q < n; q++) s += Xs[q][i] * Xs[q][j];
    for (int a = 0; a < r; a++) s -= Us[a * n + i] * Zr[a * n + j];
    data[ls.diagOff + i * n + j] = s;
    data[ls.diagOff + j * n + i] = s;
  }
}

}  // namespace hipk
}  // namespace BaSpaCho
