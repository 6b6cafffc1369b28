// Reverse mode of selected inversion: the gradient of every slot of Z (as selectedInverse writes it,
// mirrors included) becomes Lbar = df/dL on the pattern of L, in place.  Plan: the selected-inversion
// plan (hip_plan.h, SelInvPlanHost) and its scratch; schedule and launch: hip_backend.hip
// (HipSymbolicCtx::selectedInverseAdjoint); math: DESIGN.md section 19.
//
// A NODE is a column block I = [c0, c0 + w) of one lump with the rows R below it (hip_selinv_kernels.h).
// The forward step of a node is  W = L_II^-1,  U = L_RI W,  Z_RI = -Z_RR U,  Z_II = W^T W - U^T Z_RI.
// Nodes run in DESCENDING level, the reverse of selectedInverse, so that every slot of a node holds its
// complete gradient when the node runs.  With g the gradient buffer:
//   S_II = (g_II + g_II^T) / 2;   S_RI = (g_RI + mirror^T) / 2       (the mirror: own-lump rows of R
//                                                                     in the columns right of I)
//   T    = 2 S_RI - U S_II
//   g(a, b) += D(a, b) for every ordered (a, b) of R x R, D = -(T U^T + U T^T) / 2     (the scatter:
//                                                  slots by selinvZAddr, all of them right of I)
//   Ubar = -2 (Z_RI S_II + Z_RR S_RI)
//   Wbar = 2 W S_II + L_RI^T Ubar
//   g_RI = Ubar W^T;   mirror = 0;   g_II = -tril(W^T Wbar W^T), 0 above the diagonal
// L and Z are only read.  Scratch of a level (slices as selected inversion): linv holds W; the U buffer
// holds S_RI, so that selinvZrrTimesU (data = Z) forms the partial products of Z_RR S_RI in P; slot 0 of
// a node's P holds T until the scatter has run; the Wp slot of a 64-row tile holds its rows of U until
// the scatter has run, then the tile's share of L_RI^T Ubar.
//
// DETERMINISM.  D is symmetric and every pair of rows is formed once, from a >= b: (a, b) and (b, a) meet
// in one slot unless both rows lie in one diagonal block, and that slot takes 2 D(a, b); else each of
// the two slots takes D(a, b).  Slots are still shared between the nodes of a level (their rows meet in
// common ancestors), so the adds are native float atomics (unsafeAtomicAdd) and their order is not
// fixed: results are close, not bitwise, from run to run and between a batch member and the single
// call.  A level that holds one node has one writer per slot and uses plain read-modify-write
// (ATOMIC = false).  Everything else sums in a fixed order.
//
// BATCH: as the selected-inversion kernels, matrix blockIdx.y reads and writes through pickData and
// works in scratch slice blockIdx.y.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "hip_device_common.h"
#include "hip_plan.h"
#include "hip_selinv_kernels.h"

namespace BaSpaCho {
namespace hipk {

// S_II[i][j] of a node from the gradient buffer (0 outside w x w)
template <typename T>
__device__ __forceinline__ T selinvAdjSII(const GP<T> G, const SelInvNode& nd, int i, int j) {
  if (i >= nd.w || j >= nd.w) return T(0);
  const int64_t d = nd.lumpOff + (int64_t)nd.c0 * nd.lda + nd.c0;
  return T(0.5) * (G[d + (int64_t)i * nd.lda + j] + G[d + (int64_t)j * nd.lda + i]);
}

// A1: of a 64-row tile of a node (task = node, first row; task index = Wp slot):  U = L_RI W to the
// tile's Wp slot, S_RI (mirror folded) to the U buffer, T = 2 S_RI - U S_II to slot 0 of the node's P.
// Columns past w are written as zeros.
template <typename T>
__global__ void __launch_bounds__(256) selinvAdjStage(const SelInvNode* __restrict__ nodes,
                                                      const int2* __restrict__ tasks, DataRef<const T> lref,
                                                      DataRef<T> gref, const T* __restrict__ linv,
                                                      T* __restrict__ U, T* __restrict__ P, T* __restrict__ Wp,
                                                      SelInvStrides st) {
  constexpr int W = kSelInvW, PER = 64 * W / 256;
  __shared__ T Xs[W][W + 1];   // W, then S_II
  __shared__ T Rs[64][W + 1];  // L_RI, then U
  const GP<const T> L = pickData(lref);
  const GP<T> G = pickData(gref);
  linv += (int64_t)blockIdx.y * st.linv;
  U += (int64_t)blockIdx.y * st.u;
  P += (int64_t)blockIdx.y * st.p;
  Wp += (int64_t)blockIdx.y * st.w;
  const int2 tk = tasks[blockIdx.x];
  const SelInvNode nd = nodes[tk.x];
  const int a0 = tk.y, w = nd.w, tid = threadIdx.x;
  const int rows = min(64, nd.r - a0);
  const int64_t c1 = nd.c0 + w;
  const T* lo = linv + (int64_t)tk.x * W * W;
  for (int e = tid; e < W * W; e += 256) Xs[e / W][e % W] = lo[e];
  for (int e = tid; e < 64 * W; e += 256) {
    const int i = e / W, j = e % W;
    Rs[i][j] = (i < rows && j < w) ? L[nd.lumpOff + (c1 + a0 + i) * nd.lda + nd.c0 + j] : T(0);
  }
  __syncthreads();
  T u[PER];
#pragma unroll
  for (int m = 0; m < PER; m++) {
    const int e = m * 256 + tid, i = e / W, j = e % W;
    T s = T(0);
    for (int k = j; k < w; k++) s += Rs[i][k] * Xs[k][j];
    u[m] = s;
  }
  __syncthreads();
  T* uo = Wp + (int64_t)blockIdx.x * W * W;
#pragma unroll
  for (int m = 0; m < PER; m++) {
    const int e = m * 256 + tid, i = e / W, j = e % W;
    Rs[i][j] = u[m];
    uo[e] = u[m];
    Xs[i][j] = selinvAdjSII<T>(G, nd, i, j);
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < PER; m++) {
    const int e = m * 256 + tid, i = e / W, j = e % W;
    if (i >= rows) continue;
    const int64_t a = a0 + i;
    T s = T(0), t = T(0);
    if (j < w) {
      T g = G[nd.lumpOff + (c1 + a) * nd.lda + nd.c0 + j];
      if (a < nd.nRest) g += G[nd.lumpOff + (int64_t)(nd.c0 + j) * nd.lda + c1 + a];
      s = T(0.5) * g;
      T us = T(0);
      for (int k = 0; k < w; k++) us += Rs[i][k] * Xs[k][j];
      t = T(2) * s - us;
    }
    U[nd.uOff + a * W + j] = s;
    P[nd.pOff + a * W + j] = t;
  }
}

// A2: the scatter of one task of the Z_RR product's list (node, first row a0, chunk of source rows).
// D is symmetric, so only the pairs a >= b are formed: D(a, b) = -(T_a . U_b + U_a . T_b) / 2 for the 64
// rows a from a0 and the b of the chunk, 64 at a time (sub-tiles with every b past every a are skipped).
// A pair whose two orders meet in one slot adds 2 D there; a pair with a slot per order (both rows in
// one diagonal block) adds D to both, the second through a transposed LDS image so that consecutive
// lanes again hold consecutive addresses.  The sub-tiles of a task are dealt to the gridDim.z workgroups
// that share it (the loop of one workgroup over a whole chunk is a chain of barriers, and a level has
// too few tasks to hide it).  16 x 16 threads, 4 x 4 outputs each, 16 columns of T and U per step.
template <typename T, bool ATOMIC>
__global__ void __launch_bounds__(256) selinvAdjScatter(
    const SelInvNode* __restrict__ nodes, const int4* __restrict__ tasks,
    const int32_t* __restrict__ rowChain, const int32_t* __restrict__ rowLocal,
    const int64_t* __restrict__ pairOff, const int32_t* __restrict__ pairStr, DataRef<T> gref,
    const T* __restrict__ P, const T* __restrict__ Wp, SelInvStrides st) {
  constexpr int W = kSelInvW, KB = 16;
  static_assert(4 * KB == 64, "the four operand tiles double as the 64 x 64 image of D");
  __shared__ T Sh[4 * KB][64 + 1];
  T(*Ta)[64 + 1] = Sh, (*Ua)[64 + 1] = Sh + KB, (*Tb)[64 + 1] = Sh + 2 * KB, (*Ub)[64 + 1] = Sh + 3 * KB;
  const GP<T> G = pickData(gref);
  P += (int64_t)blockIdx.y * st.p;
  Wp += (int64_t)blockIdx.y * st.w;
  const int4 tk = tasks[blockIdx.x];
  const SelInvNode nd = nodes[tk.x];
  const int a0 = tk.y, w = nd.w, tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  const int rows = min(64, nd.r - a0);
  const int b0 = tk.z * nd.kChunk, b1 = min(nd.r, b0 + nd.kChunk);
  const T* Tn = P + nd.pOff;                          // T, r x W
  const T* Un = Wp + (int64_t)nd.tileBase * W * W;    // U: 64-row tiles of W columns, one after the other
  const auto add = [&](int64_t addr, T v) {
    if (ATOMIC) {
      unsafeAtomicAdd((T*)(G + addr), v);
    } else {
      G[addr] += v;
    }
  };
  for (int bb = b0 + 64 * blockIdx.z; bb < b1 && bb < a0 + rows; bb += 64 * gridDim.z) {
    T acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) acc[i][j] = T(0);
    for (int k0 = 0; k0 < w; k0 += KB) {
      for (int e = tid; e < 64 * KB; e += 256) {
        const int i = e / KB, k = e % KB;
        const bool kin = k0 + k < w, ain = kin && i < rows, bin = kin && bb + i < b1;
        const int64_t ao = (int64_t)(a0 + i) * W + k0 + k, bo = (int64_t)(bb + i) * W + k0 + k;
        Ta[k][i] = ain ? Tn[ao] : T(0);
        Ua[k][i] = ain ? Un[ao] : T(0);
        Tb[k][i] = bin ? Tn[bo] : T(0);
        Ub[k][i] = bin ? Un[bo] : T(0);
      }
      __syncthreads();
#pragma unroll 4
      for (int k = 0; k < KB; k++) {
        T ta[4], ua[4], tb[4], ub[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
          ta[i] = Ta[k][ty + 16 * i];
          ua[i] = Ua[k][ty + 16 * i];
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
          tb[j] = Tb[k][tx + 16 * j];
          ub[j] = Ub[k][tx + 16 * j];
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
          for (int j = 0; j < 4; j++) acc[i][j] += ta[i] * ub[j] + ua[i] * tb[j];
      }
      __syncthreads();
    }
    int mirror = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int al = ty + 16 * i, a = a0 + al;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int bl = tx + 16 * j, b = bb + bl;
        T v = T(-0.5) * acc[i][j];
        Sh[al][bl] = v;  // D(a, b), for the pairs with a slot per order
        if (al >= rows || b >= b1 || a < b) continue;
        const int64_t addr = selinvZAddr(nd, rowChain, rowLocal, pairOff, pairStr, a, b);
        if (a != b) {
          if (addr == selinvZAddr(nd, rowChain, rowLocal, pairOff, pairStr, b, a)) {
            v = -acc[i][j];
          } else {
            mirror = 1;
          }
        }
        add(addr, v);
      }
    }
    if (__syncthreads_or(mirror)) {
      // the slots (b, a) of the pairs a > b that have one: row b along ty, column a along the lanes
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int bl = ty + 16 * i, b = bb + bl;
        if (b >= b1) continue;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int al = tx + 16 * j, a = a0 + al;
          if (al >= rows || a <= b) continue;
          const int64_t addr = selinvZAddr(nd, rowChain, rowLocal, pairOff, pairStr, b, a);
          if (addr != selinvZAddr(nd, rowChain, rowLocal, pairOff, pairStr, a, b)) add(addr, Sh[al][bl]);
        }
      }
      __syncthreads();
    }
  }
}

// A3: of a 64-row tile (task = node, first row; task index = Wp slot): Ubar = -2 (Z_RI S_II + sum_kc
// P[kc]) (the partial products of Z_RR S_RI, in that order), g_RI = Ubar W^T written over the tile's
// gradient, the mirror of its own-lump rows zeroed, and the tile's share of L_RI^T Ubar (W x W) to its
// Wp slot.
template <typename T>
__global__ void __launch_bounds__(256) selinvAdjReduce(const SelInvNode* __restrict__ nodes,
                                                       const int2* __restrict__ tasks, DataRef<const T> lref,
                                                       DataRef<const T> zref, DataRef<T> gref,
                                                       const T* __restrict__ linv, const T* __restrict__ P,
                                                       T* __restrict__ Wp, SelInvStrides st) {
  constexpr int W = kSelInvW, PER = 64 * W / 256;
  __shared__ T As[W][W + 1];   // S_II, then W, then L_RI
  __shared__ T Bs[64][W + 1];  // Z_RI, then Ubar
  const GP<const T> L = pickData(lref);
  const GP<const T> Z = pickData(zref);
  const GP<T> G = pickData(gref);
  linv += (int64_t)blockIdx.y * st.linv;
  P += (int64_t)blockIdx.y * st.p;
  Wp += (int64_t)blockIdx.y * st.w;
  const int2 tk = tasks[blockIdx.x];
  const SelInvNode nd = nodes[tk.x];
  const int a0 = tk.y, w = nd.w, tid = threadIdx.x;
  const int rows = min(64, nd.r - a0);
  const int64_t c1 = nd.c0 + w;
  const T* lo = linv + (int64_t)tk.x * W * W;
#pragma unroll
  for (int m = 0; m < PER; m++) {
    const int e = m * 256 + tid, i = e / W, j = e % W;
    As[i][j] = selinvAdjSII<T>(G, nd, i, j);
    Bs[i][j] = (i < rows && j < w) ? Z[nd.lumpOff + (c1 + a0 + i) * nd.lda + nd.c0 + j] : T(0);
  }
  __syncthreads();
  T v[PER];
#pragma unroll
  for (int m = 0; m < PER; m++) {
    const int e = m * 256 + tid, i = e / W, j = e % W;
    T s = T(0);
    if (i < rows && j < w) {
      for (int k = 0; k < w; k++) s += Bs[i][k] * As[k][j];
      for (int kc = 0; kc < nd.nk; kc++) s += P[nd.pOff + ((int64_t)kc * nd.r + a0 + i) * W + j];
      s *= T(-2);
    }
    v[m] = s;
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < PER; m++) {
    const int e = m * 256 + tid, i = e / W, j = e % W;
    Bs[i][j] = v[m];
    As[i][j] = lo[e];
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < PER; m++) {
    const int e = m * 256 + tid, i = e / W, j = e % W;
    if (i < rows && j < w) {
      const int64_t a = a0 + i;
      T s = T(0);
      for (int q = 0; q <= j; q++) s += Bs[i][q] * As[j][q];
      G[nd.lumpOff + (c1 + a) * nd.lda + nd.c0 + j] = s;
      if (a < nd.nRest) G[nd.lumpOff + (int64_t)(nd.c0 + j) * nd.lda + c1 + a] = T(0);
    }
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < PER; m++) {
    const int e = m * 256 + tid, i = e / W, j = e % W;
    As[i][j] = (i < rows && j < w) ? L[nd.lumpOff + (c1 + a0 + i) * nd.lda + nd.c0 + j] : T(0);
  }
  __syncthreads();
  T* wo = Wp + (int64_t)blockIdx.x * W * W;
  for (int e = tid; e < W * W; e += 256) {
    const int i = e / W, j = e % W;
    T s = T(0);
    for (int k = 0; k < rows; k++) s += As[k][i] * Bs[k][j];
    wo[e] = s;
  }
}

// A4: of a node: Wbar = 2 W S_II + sum over the node's tiles of L_RI^T Ubar, then g_II = -tril(W^T Wbar
// W^T) with zeros above the diagonal.  One workgroup of 256 per node.
template <typename T>
__global__ void __launch_bounds__(256) selinvAdjDiag(const SelInvNode* __restrict__ nodes, DataRef<T> gref,
                                                     const T* __restrict__ linv, const T* __restrict__ Wp,
                                                     SelInvStrides st) {
  constexpr int W = kSelInvW, PER = W * W / 256;
  __shared__ T Xs[W][W + 1];  // W
  __shared__ T Bs[W][W + 1];  // S_II, then Wbar W^T
  __shared__ T Cs[W][W + 1];  // Wbar
  const GP<T> G = pickData(gref);
  linv += (int64_t)blockIdx.y * st.linv;
  Wp += (int64_t)blockIdx.y * st.w;
  const SelInvNode nd = nodes[blockIdx.x];
  const int w = nd.w, tid = threadIdx.x;
  const T* lo = linv + (int64_t)blockIdx.x * W * W;
#pragma unroll
  for (int m = 0; m < PER; m++) {
    const int e = m * 256 + tid, i = e / W, j = e % W;
    Xs[i][j] = lo[e];
    Bs[i][j] = selinvAdjSII<T>(G, nd, i, j);
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < PER; m++) {
    const int e = m * 256 + tid, i = e / W, j = e % W;
    T s = T(0);
    if (i < w && j < w) {
      for (int k = 0; k <= i; k++) s += Xs[i][k] * Bs[k][j];
      s *= T(2);
      for (int t = 0; t < nd.nTiles; t++) s += Wp[(int64_t)(nd.tileBase + t) * W * W + e];
    }
    Cs[i][j] = s;
  }
  __syncthreads();
  T v[PER];
#pragma unroll
  for (int m = 0; m < PER; m++) {
    const int e = m * 256 + tid, i = e / W, j = e % W;
    T s = T(0);
    for (int q = 0; q <= j; q++) s += Cs[i][q] * Xs[j][q];
    v[m] = s;
  }
#pragma unroll
  for (int m = 0; m < PER; m++) {
    const int e = m * 256 + tid;
    Bs[e / W][e % W] = v[m];
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < PER; m++) {
    const int e = m * 256 + tid, i = e / W, j = e % W;
    if (i >= w || j >= w) continue;
    T s = T(0);
    if (j <= i) {
      for (int p = i; p < w; p++) s += Xs[p][i] * Bs[p][j];
      s = -s;
    }
    G[nd.lumpOff + (int64_t)(nd.c0 + i) * nd.lda + nd.c0 + j] = s;
  }
}

// ------------------------------------------------------------------------------------------
// Small lumps (the eligibility of selinvSmallLumps): the whole reverse step of one lump (one node,
// c0 = 0, w = n, nRest = 0) in one wave, operands in LDS.  The pair table is found on the device, as
// there.  The scatter runs over the flat (a, b) pairs, consecutive lanes on consecutive b; rows of
// different chains meet in one slot (2 D from a > b), rows of one chain have a slot per order.
template <typename T>
__global__ void __launch_bounds__(64) selinvAdjSmallLumps(const SelInvSmall* __restrict__ lumps, SkelDev sk,
                                                          DataRef<const T> lref, DataRef<const T> zref,
                                                          DataRef<T> gref) {
  constexpr int NW = kSelInvSmallW, NC = kSelInvSmallChains, NE = kSelInvSmallElems;
  static_assert(NC < 256, "chain ordinals are stored in bytes");
  __shared__ T Xs[NW][NW + 1];  // W
  __shared__ T Ss[NW][NW + 1];  // S_II, then Wbar W^T
  __shared__ T Bs[NW][NW + 1];  // Wbar
  __shared__ T Lr[NE];          // L_RI
  __shared__ T Us[NE];          // U
  __shared__ T Sr[NE];          // S_RI
  __shared__ T Ts[NE];          // T, then Ubar
  __shared__ int64_t pOff[NC * (NC + 1) / 2];
  __shared__ int32_t pStr[NC * (NC + 1) / 2];
  __shared__ int32_t cRow0[NC + 1];
  __shared__ uint8_t rowK[NE];
  __shared__ int16_t rowL[NE];
  const GP<const T> L = pickData(lref);
  const GP<const T> Z = pickData(zref);
  const GP<T> G = pickData(gref);
  const SelInvSmall ls = lumps[blockIdx.x];
  const int n = ls.n, r = ls.r, k = ls.k, lane = threadIdx.x;
  const int64_t cBeg = ls.chainBegin, below = ls.diagOff + (int64_t)n * n;
  if (lane < k) {
    const int64_t c = cBeg + lane;
    const int64_t s = sk.chainRowSpan[c];
    cRow0[lane] = (int)(sk.chainRowsTillEnd[c] - (sk.spanStart[s + 1] - sk.spanStart[s]) - n);
  }
  if (lane == 0) cRow0[k] = r;
  for (int p = lane; p < k * (k + 1) / 2; p += 64) {
    int ka = 0;
    while ((ka + 1) * (ka + 2) / 2 <= p) ka++;
    const int kb = p - ka * (ka + 1) / 2;
    const int64_t sa = sk.chainRowSpan[cBeg + ka], sb = sk.chainRowSpan[cBeg + kb];
    const int64_t J = sk.spanToLump[sb];
    int64_t lo = sk.chainColPtr[J], hi = sk.chainColPtr[J + 1] - 1;
    while (lo < hi) {
      const int64_t mid = (lo + hi) / 2;
      if (sk.chainRowSpan[mid] < sa) lo = mid + 1; else hi = mid;
    }
    pOff[p] = sk.chainData[lo] + sk.spanStart[sb] - sk.lumpStart[J];
    pStr[p] = (int32_t)(sk.lumpStart[J + 1] - sk.lumpStart[J]);
  }
  for (int e = lane; e < NW * NW; e += 64) {
    const int i = e / NW, j = e % NW;
    Xs[i][j] = T(0);
    Ss[i][j] = (i < n && j < n) ? T(0.5) * (G[ls.diagOff + i * n + j] + G[ls.diagOff + j * n + i]) : T(0);
  }
  for (int e = lane; e < r * n; e += 64) {
    Lr[e] = L[below + e];
    Sr[e] = T(0.5) * G[below + e];
  }
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
      for (int q = j; q < i; q++) s -= L[ls.diagOff + i * n + q] * Xs[q][j];
      Xs[i][j] = s / L[ls.diagOff + i * n + i];
    }
  }
  __syncthreads();
  for (int e = lane; e < r * n; e += 64) {
    const int a = e / n, j = e % n;
    T s = T(0);
    for (int q = j; q < n; q++) s += Lr[a * n + q] * Xs[q][j];
    Us[e] = s;
  }
  __syncthreads();
  for (int e = lane; e < r * n; e += 64) {
    const int a = e / n, j = e % n;
    T s = T(0);
    for (int q = 0; q < n; q++) s += Us[a * n + q] * Ss[q][j];
    Ts[e] = T(2) * Sr[e] - s;
  }
  __syncthreads();
  // the scatter
  for (int e = lane; e < r * r; e += 64) {
    const int a = e / r, b = e - a * r;
    const int ka = rowK[a], kb = rowK[b];
    if (ka < kb) continue;  // (b, a) adds both shares
    T s = T(0);
    for (int q = 0; q < n; q++) s += Ts[a * n + q] * Us[b * n + q] + Us[a * n + q] * Ts[b * n + q];
    const int p = ka * (ka + 1) / 2 + kb;
    const int64_t addr = pOff[p] + (int64_t)rowL[a] * pStr[p] + rowL[b];
    unsafeAtomicAdd((T*)(G + addr), ka == kb ? T(-0.5) * s : -s);
  }
  // Ubar, one row of R per lane (every lane keeps its rows in registers until T is dead)
  __syncthreads();
  for (int a0 = 0; a0 < r; a0 += 64) {
    const int a = a0 + lane;
    T acc[NW];
#pragma unroll
    for (int j = 0; j < NW; j++) acc[j] = T(0);
    if (a < r) {
      for (int q = 0; q < n; q++) {
        const T z = Z[below + a * n + q];
#pragma unroll
        for (int j = 0; j < NW; j++)
          if (j < n) acc[j] += z * Ss[q][j];
      }
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
        const T z = Z[addr];
#pragma unroll
        for (int j = 0; j < NW; j++)
          if (j < n) acc[j] += z * Sr[b * n + j];
      }
#pragma unroll
      for (int j = 0; j < NW; j++)
        if (j < n) Ts[a * n + j] = T(-2) * acc[j];  // row a of T is read by nobody else from here on
    }
  }
  __syncthreads();
  for (int e = lane; e < n * n; e += 64) {
    const int i = e / n, j = e % n;
    T s = T(0);
    for (int q = 0; q <= i; q++) s += Xs[i][q] * Ss[q][j];
    s *= T(2);
    for (int a = 0; a < r; a++) s += Lr[a * n + i] * Ts[a * n + j];
    Bs[i][j] = s;
  }
  for (int e = lane; e < r * n; e += 64) {
    const int a = e / n, j = e % n;
    T s = T(0);
    for (int q = 0; q <= j; q++) s += Ts[a * n + q] * Xs[j][q];
    G[below + e] = s;
  }
  __syncthreads();
  for (int e = lane; e < n * n; e += 64) {
    const int i = e / n, j = e % n;
    T s = T(0);
    for (int q = 0; q <= j; q++) s += Bs[i][q] * Xs[j][q];
    Ss[i][j] = s;
  }
  __syncthreads();
  for (int e = lane; e < n * n; e += 64) {
    const int i = e / n, j = e % n;
    T s = T(0);
    if (j <= i) {
      for (int p = i; p < n; p++) s += Xs[p][i] * Ss[p][j];
      s = -s;
    }
    G[ls.diagOff + i * n + j] = s;
  }
}

}  // namespace hipk
}  // namespace BaSpaCho
