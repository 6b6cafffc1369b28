// Reverse-mode sweep of the supernodal Cholesky factor: Lbar = df/dL on the pattern of L becomes the
// gradient of the input data, in place.  Plan: the selected-inversion plan (hip_plan.h, SelInvPlanHost)
// and its scratch; schedule and launch: hip_backend.hip (HipSymbolicCtx::factorAdjoint); math:
// DESIGN.md section 15.
//
// A NODE is a column block [c0, c0 + w) of one lump with the rows R below it (hip_selinv_kernels.h).
// G is the dense symmetric gradient df/dA.  Nodes run right to left, as in selected inversion, so G_RR
// is final when a node runs.  With Linv = L_II^-1:
//   1. Lbar_RI -= 2 G_RR L_RI                    (adjoint of the Schur update A_RR -= L_RI L_RI^T)
//   2. Abar_RI  = Lbar_RI Linv;  G_RI = Abar_RI / 2
//   3. Lbar_II -= tril(Abar_RI^T L_RI)
//   4. K = Linv^T Phi(L_II^T Lbar_II) Linv  (Phi: lower triangle, diagonal halved);  G_II = (K + K^T) / 2
// G is stored as selected inversion stores Z (diagonal blocks full and symmetric, a node's rows inside
// its own lump mirrored into the upper triangle of the lump's diagonal block), so selinvZAddr reads
// G_RR unchanged.  The mirror slots are the strictly-upper elements, which the input does not use:
// the sweep runs in place in the gradient buffer.  L is only read.  A final element-wise pass turns
// the G storage into the data gradient: 2 G_e below the diagonal, G_e on it, 0 above it.
//
// The G_RR L_RI product is selinvZrrTimesU itself, run on a copy of L_RI in the U scratch
// (cholAdjGatherL): its partial products P[kc] = sum_{b in chunk kc} G(a, b) L_RI[b, :].
//
// BATCH: as the selected-inversion kernels, matrix blockIdx.y reads and writes through pickData and
// works in scratch slice blockIdx.y.  No atomics, every sum in a fixed order: bitwise reproducible,
// and member q of a batch is bitwise the single call.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "hip_grad_kernels.h"
#include "hip_device_common.h"
#include "hip_plan.h"
#include "hip_selinv_kernels.h"

namespace BaSpaCho {
namespace hipk {

// U[a, :] = L_RI[a, :] (zero past w) for a 64-row tile of a node (task = node, first row)
template <typename T>
__global__ void __launch_bounds__(256) cholAdjGatherL(const SelInvNode* __restrict__ nodes,
                                                      const int2* __restrict__ tasks, DataRef<const T> lref,
                                                      T* __restrict__ U, SelInvStrides st) {
  constexpr int W = kSelInvW;
  const GP<const T> L = pickData(lref);
  U += (int64_t)blockIdx.y * st.u;
  const int2 tk = tasks[blockIdx.x];
  const SelInvNode nd = nodes[tk.x];
  const int a0 = tk.y, w = nd.w;
  const int rows = min(64, nd.r - a0);
  for (int e = threadIdx.x; e < rows * W; e += 256) {
    const int i = e / W, j = e % W;
    U[nd.uOff + (int64_t)(a0 + i) * W + j] =
        j < w ? L[nd.lumpOff + (int64_t)(nd.c0 + w + a0 + i) * nd.lda + nd.c0 + j] : T(0);
  }
}

// Steps 1-2 of a 64-row tile, plus its share of step 3: Lbar_RI - 2 sum_kc P[kc] (in that order),
// Abar = that times Linv, G_RI = Abar / 2 written over Lbar_RI (and, for rows inside the lump's own
// diagonal block, transposed into its upper triangle), and Abar^T L_RI of the tile's rows (W x W, to
// scratch slot `tile`).  Task = node, first row; task index = slot.
template <typename T>
__global__ void __launch_bounds__(256) cholAdjReduce(const SelInvNode* __restrict__ nodes,
                                                     const int2* __restrict__ tasks, DataRef<T> gref,
                                                     const T* __restrict__ linv, const T* __restrict__ U,
                                                     const T* __restrict__ P, T* __restrict__ Wp,
                                                     SelInvStrides st) {
  constexpr int W = kSelInvW, PER = 64 * W / 256;
  __shared__ T Bt[64][W + 1];  // Lbar_RI, then Abar_RI
  __shared__ T Lt[64][W + 1];  // L_RI
  __shared__ T Xs[W][W + 1];   // Linv
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
    T b = T(0), l = T(0);
    if (i < rows) {
      const int64_t a = a0 + i;
      l = U[nd.uOff + a * W + j];
      if (j < w) {
        T s = T(0);
        for (int kc = 0; kc < nd.nk; kc++) s += P[nd.pOff + ((int64_t)kc * nd.r + a) * W + j];
        b = G[nd.lumpOff + (c1 + a) * nd.lda + nd.c0 + j] - T(2) * s;
      }
    }
    Bt[i][j] = b;
    Lt[i][j] = l;
  }
  __syncthreads();
  T ab[PER];
#pragma unroll
  for (int m = 0; m < PER; m++) {
    const int e = m * 256 + tid, i = e / W, j = e % W;
    T s = T(0);
    for (int k = j; k < w; k++) s += Bt[i][k] * Xs[k][j];
    ab[m] = s;
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < PER; m++) {
    const int e = m * 256 + tid, i = e / W, j = e % W;
    Bt[i][j] = ab[m];
    if (i < rows && j < w) {
      const int64_t a = a0 + i;
      const T g = T(0.5) * ab[m];
      G[nd.lumpOff + (c1 + a) * nd.lda + nd.c0 + j] = g;
      if (a < nd.nRest) G[nd.lumpOff + (int64_t)(nd.c0 + j) * nd.lda + c1 + a] = g;
    }
  }
  __syncthreads();
  T* wo = Wp + (int64_t)blockIdx.x * W * W;
  for (int e = tid; e < W * W; e += 256) {
    const int i = e / W, j = e % W;
    T s = T(0);
    for (int k = 0; k < rows; k++) s += Bt[k][i] * Lt[k][j];
    wo[e] = s;
  }
}

// Steps 3-4 of a node: Lbar_II = tril(Lbar_II) - sum over the node's tiles of tril(Abar^T L_RI), then
// G_II = (K + K^T) / 2, written full and symmetric.  One workgroup of 256 per node.
template <typename T>
__global__ void __launch_bounds__(256) cholAdjDiag(const SelInvNode* __restrict__ nodes, DataRef<const T> lref,
                                                   DataRef<T> gref, const T* __restrict__ linv,
                                                   const T* __restrict__ Wp, SelInvStrides st) {
  constexpr int W = kSelInvW, PER = W * W / 256;
  __shared__ T Ls[W][W + 1];  // L_II, then Phi Linv
  __shared__ T Xs[W][W + 1];  // Linv
  __shared__ T Bs[W][W + 1];  // Lbar_II, then Phi, then K
  const GP<const T> L = pickData(lref);
  const GP<T> G = pickData(gref);
  linv += (int64_t)blockIdx.y * st.linv;
  Wp += (int64_t)blockIdx.y * st.w;
  const SelInvNode nd = nodes[blockIdx.x];
  const int w = nd.w, tid = threadIdx.x;
  const T* lo = linv + (int64_t)blockIdx.x * W * W;
  for (int e = tid; e < W * W; e += 256) {
    const int i = e / W, j = e % W;
    Xs[i][j] = lo[e];
    T l = T(0), b = T(0);
    if (i < w && j <= i) {
      const int64_t a = nd.lumpOff + (int64_t)(nd.c0 + i) * nd.lda + nd.c0 + j;
      l = L[a];
      b = G[a];
      for (int t = 0; t < nd.nTiles; t++) b -= Wp[(int64_t)(nd.tileBase + t) * W * W + e];
    }
    Ls[i][j] = l;
    Bs[i][j] = b;
  }
  __syncthreads();
  T v[PER];
  // Phi(L_II^T Lbar_II): lower triangle, diagonal halved
#pragma unroll
  for (int m = 0; m < PER; m++) {
    const int e = m * 256 + tid, i = e / W, j = e % W;
    T s = T(0);
    if (j <= i) {
      for (int k = i; k < w; k++) s += Ls[k][i] * Bs[k][j];
      if (i == j) s *= T(0.5);
    }
    v[m] = s;
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < PER; m++) {
    const int e = m * 256 + tid;
    Bs[e / W][e % W] = v[m];
  }
  __syncthreads();
  // Phi Linv (lower)
#pragma unroll
  for (int m = 0; m < PER; m++) {
    const int e = m * 256 + tid, p = e / W, j = e % W;
    T s = T(0);
    for (int q = j; q <= p; q++) s += Bs[p][q] * Xs[q][j];
    v[m] = s;
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < PER; m++) {
    const int e = m * 256 + tid;
    Ls[e / W][e % W] = v[m];
  }
  __syncthreads();
  // K = Linv^T (Phi Linv)
#pragma unroll
  for (int m = 0; m < PER; m++) {
    const int e = m * 256 + tid, i = e / W, j = e % W;
    T s = T(0);
    for (int p = (i > j ? i : j); p < w; p++) s += Xs[p][i] * Ls[p][j];
    v[m] = s;
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < PER; m++) {
    const int e = m * 256 + tid;
    Bs[e / W][e % W] = v[m];
  }
  __syncthreads();
  for (int e = tid; e < W * W; e += 256) {
    const int i = e / W, j = e % W;
    if (i >= w || j > i) continue;
    const T s = T(0.5) * (Bs[i][j] + Bs[j][i]);
    G[nd.lumpOff + (int64_t)(nd.c0 + i) * nd.lda + nd.c0 + j] = s;
    G[nd.lumpOff + (int64_t)(nd.c0 + j) * nd.lda + nd.c0 + i] = s;
  }
}

// ------------------------------------------------------------------------------------------
// Small lumps (the eligibility of selinvSmallLumps): steps 1-4 of one whole lump (one node, w = n,
// nRest = 0) in one wave, operands in LDS.  The pair table is found on the device, as there.
template <typename T>
__global__ void __launch_bounds__(64) cholAdjSmallLumps(const SelInvSmall* __restrict__ lumps, SkelDev sk,
                                                        DataRef<const T> lref, DataRef<T> gref) {
  constexpr int NW = kSelInvSmallW, NC = kSelInvSmallChains, NE = kSelInvSmallElems;
  static_assert(NC < 256, "chain ordinals are stored in bytes");
  __shared__ T Ls[NW][NW + 1];  // L_II, then Phi Linv
  __shared__ T Xs[NW][NW + 1];  // Linv
  __shared__ T Bs[NW][NW + 1];  // Lbar_II
  __shared__ T Ps[NW][NW + 1];  // Phi, then K
  __shared__ T Lr[NE];          // L_RI
  __shared__ T Br[NE];          // Lbar_RI, then Abar_RI
  __shared__ int64_t pOff[NC * (NC + 1) / 2];
  __shared__ int32_t pStr[NC * (NC + 1) / 2];
  __shared__ int32_t cRow0[NC + 1];
  __shared__ uint8_t rowK[NE];
  __shared__ int16_t rowL[NE];
  const GP<const T> L = pickData(lref);
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
    const bool in = i < n && j <= i;
    Ls[i][j] = in ? L[ls.diagOff + i * n + j] : T(0);
    Bs[i][j] = in ? G[ls.diagOff + i * n + j] : T(0);
    Xs[i][j] = T(0);
  }
  for (int e = lane; e < r * n; e += 64) {
    Lr[e] = L[below + e];
    Br[e] = G[below + e];
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
      for (int q = j; q < i; q++) s -= Ls[i][q] * Xs[q][j];
      Xs[i][j] = s / Ls[i][i];
    }
  }
  __syncthreads();
  // steps 1-2, one row of R per lane
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
      const T g = G[addr];
#pragma unroll
      for (int j = 0; j < NW; j++)
        if (j < n) acc[j] += g * Lr[b * n + j];
    }
#pragma unroll
    for (int j = 0; j < NW; j++)
      if (j < n) Br[a * n + j] -= T(2) * acc[j];
    // Abar[a, j] needs Lbar[a, q] for q >= j only: ascending j overwrites the row in place
    for (int j = 0; j < n; j++) {
      T s = T(0);
      for (int q = j; q < n; q++) s += Br[a * n + q] * Xs[q][j];
      Br[a * n + j] = s;
    }
  }
  __syncthreads();
  for (int e = lane; e < r * n; e += 64) G[below + e] = T(0.5) * Br[e];
  // step 3
  for (int e = lane; e < n * n; e += 64) {
    const int i = e / n, j = e % n;
    if (j > i) continue;
    T s = Bs[i][j];
    for (int a = 0; a < r; a++) s -= Br[a * n + i] * Lr[a * n + j];
    Bs[i][j] = s;
  }
  __syncthreads();
  // step 4
  for (int e = lane; e < n * n; e += 64) {
    const int i = e / n, j = e % n;
    T s = T(0);
    if (j <= i) {
      for (int q = i; q < n; q++) s += Ls[q][i] * Bs[q][j];
      if (i == j) s *= T(0.5);
    }
    Ps[i][j] = s;
  }
  __syncthreads();
  for (int e = lane; e < n * n; e += 64) {
    const int p = e / n, j = e % n;
    T s = T(0);
    for (int q = j; q <= p; q++) s += Ps[p][q] * Xs[q][j];
    Ls[p][j] = s;
  }
  __syncthreads();
  for (int e = lane; e < n * n; e += 64) {
    const int i = e / n, j = e % n;
    T s = T(0);
    for (int p = (i > j ? i : j); p < n; p++) s += Xs[p][i] * Ls[p][j];
    Ps[i][j] = s;
  }
  __syncthreads();
  for (int e = lane; e < n * n; e += 64) {
    const int i = e / n, j = e % n;
    if (j > i) continue;
    const T s = T(0.5) * (Ps[i][j] + Ps[j][i]);
    G[ls.diagOff + i * n + j] = s;
    G[ls.diagOff + j * n + i] = s;
  }
}

// ------------------------------------------------------------------------------------------
// Final pass over the patternGrad tiles (GradTile): the G storage becomes the data gradient, 2 G_e
// below the diagonal, G_e on it, 0 on the strictly-upper elements of the diagonal blocks.  A tile's
// rows and columns are counted from the top-left of its lump column, so an element is below the
// diagonal when its row is past the diagonal block or greater than its column.
template <typename T>
__global__ void __launch_bounds__(256) cholAdjFinal(const GradTile* __restrict__ tiles, SkelDev sk,
                                                    DataRef<T> gref) {
  constexpr int PER = kGradElems / 256;
  const GP<T> G = pickData(gref);
  const GradTile t = tiles[blockIdx.x];
  const int64_t w = sk.lumpStart[t.lump + 1] - sk.lumpStart[t.lump];
  const int nEl = t.nr * t.nc;
#pragma unroll
  for (int m = 0; m < PER; m++) {
    const int e = m * 256 + threadIdx.x;
    if (e < nEl) {
      const int r = e / t.nc, c = e - r * t.nc;
      const int64_t lr = t.r0 + r, lc = t.c0 + c;
      const int64_t a = t.off + r * w + c;
      const T g = G[a];
      G[a] = (lr >= w || lr > lc) ? T(2) * g : (lr == lc ? g : T(0));
    }
  }
}

// ------------------------------------------------------------------------------------------
// PARTIAL FACTOR.  For P = [L11 0; L21 S] of factorUpTo the trailing block starts
// final: dS/dA22 = I, so the incoming Sbar on the lumps >= the cut, put into G storage, is G_22, and
// only the plan of the lumps before the cut runs (buildSelInvPlan(skel, upToLump)).
//
// Seed, over the patternGrad tiles of the trailing lumps (a suffix of the tile list), in place: elements
// below the diagonal are halved (G_e = Sbar_e / 2), the diagonal is kept, and every halved element of a
// diagonal block is also written to its mirror slot above the diagonal.  A strictly-upper slot is
// written by the tile that owns its lower partner and by nobody else, and it is never read here, so
// tiles do not race.  The mirror goes through LDS (odd row stride: the transposed read is free of
// bank conflicts) so that loads and both stores run along the lanes.
template <typename T>
__global__ void __launch_bounds__(256) cholAdjSeedTrailing(const GradTile* __restrict__ tiles, SkelDev sk,
                                                           DataRef<T> gref) {
  constexpr int PER = kGradElems / 256;
  __shared__ T Ts[kGradElems + kGradRows];
  const GP<T> G = pickData(gref);
  const GradTile t = tiles[blockIdx.x];
  const int64_t w = sk.lumpStart[t.lump + 1] - sk.lumpStart[t.lump];
  const int nEl = t.nr * t.nc, S = t.nc | 1;
  // some element of the tile lies in the diagonal block, strictly below the diagonal
  const bool mirror = t.r0 < w && t.r0 + t.nr - 1 > t.c0;
#pragma unroll
  for (int m = 0; m < PER; m++) {
    const int e = m * 256 + threadIdx.x;
    if (e < nEl) {
      const int r = e / t.nc, c = e - r * t.nc;
      const int64_t lr = t.r0 + r, lc = t.c0 + c;
      if (lr >= w || lr > lc) {
        const int64_t a = t.off + r * w + c;
        const T g = T(0.5) * G[a];
        G[a] = g;
        if (mirror) Ts[r * S + c] = g;
      }
    }
  }
  if (!mirror) return;
  __syncthreads();
  const int64_t lumpOff = t.off - t.r0 * w - t.c0;
#pragma unroll
  for (int m = 0; m < PER; m++) {
    const int e = m * 256 + threadIdx.x;
    if (e < nEl) {
      const int c = e / t.nr, r = e - c * t.nr;  // consecutive lanes: consecutive columns of the mirror
      const int64_t lr = t.r0 + r, lc = t.c0 + c;
      if (lr < w && lr > lc) G[lumpOff + lc * w + lr] = Ts[r * S + c];
    }
  }
}

// ---- the trailing block as a dense matrix ---------------------------------------------------------
// m = order - bar scalars from internal scalar `bar` on (the start of a lump); dense row / column of
// internal scalar i: dest[i - bar] (a permutation of 0 .. m-1), or i - bar without dest.
constexpr int kSchurTile = 64;

// span of internal scalar i, by bisection on spanStart over [s0, numSpans)
__device__ __forceinline__ int64_t schurSpanOf(const SkelDev& sk, int64_t s0, int64_t numSpans, int64_t i) {
  int64_t lo = s0, hi = numSpans - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (sk.spanStart[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// out (m x m, row-major, symmetric) = the trailing block of the layout buffer P, zero where the pattern
// has no block.  One workgroup per pair of 64 x 64 output tiles (I, J), I >= J (blockIdx.x = I (I + 1) / 2
// + J): it finds, for each of its rows and each lump under its columns, the chain that holds the row
// (none: zeros), gathers the lower tile along the columns, and writes tile (I, J) as it is and tile
// (J, I) transposed through LDS.  Every output element is written exactly once; `out` is never read.
template <typename T>
__global__ void __launch_bounds__(256) schurToDense(SkelDev sk, int64_t span0, int64_t numSpans, int64_t bar,
                                                    int64_t m, const int32_t* __restrict__ dest,
                                                    DataRef<const T> pref, DataRef<T> oref) {
  constexpr int TS = kSchurTile, PER = TS * TS / 256;
  constexpr size_t kTable = sizeof(int64_t) * TS * TS, kImage = sizeof(T) * TS * (TS + 1);
  // the chain table (while gathering), then the tile image
  __shared__ __align__(16) unsigned char raw[kTable > kImage ? kTable : kImage];
  __shared__ int32_t rowSpan[TS], rowLoc[TS], colLump[TS], ordLump[TS], dR[TS], dC[TS];
  __shared__ uint8_t colOrd[TS];
  __shared__ int nOrdS;
  int64_t* base = reinterpret_cast<int64_t*>(raw);
  T(*Ts)[TS + 1] = reinterpret_cast<T(*)[TS + 1]>(raw);
  const GP<const T> P = pickData(pref);
  const GP<T> out = pickData(oref);
  const GP<const int32_t> dst = (GP<const int32_t>)dest;
  const int tid = threadIdx.x;
  const int64_t p = blockIdx.x;
  int I = (int)((sqrtf(8.f * (float)p + 1.f) - 1.f) * 0.5f);
  while ((int64_t)(I + 1) * (I + 2) / 2 <= p) I++;
  while ((int64_t)I * (I + 1) / 2 > p) I--;
  const int J = (int)(p - (int64_t)I * (I + 1) / 2);
  const int64_t i0 = (int64_t)I * TS, j0 = (int64_t)J * TS;  // counted from bar
  const int nr = (int)min((int64_t)TS, m - i0), nc = (int)min((int64_t)TS, m - j0);
  if (tid < TS) {
    const int r = tid;
    int32_t sp = 0, loc = 0, d = 0;
    if (r < nr) {
      const int64_t i = bar + i0 + r;
      const int64_t s = schurSpanOf(sk, span0, numSpans, i);
      sp = (int32_t)s;
      loc = (int32_t)(i - sk.spanStart[s]);
      d = dest ? dst[i0 + r] : (int32_t)(i0 + r);
    }
    rowSpan[r] = sp;
    rowLoc[r] = loc;
    dR[r] = d;
  } else if (tid < 2 * TS) {
    const int c = tid - TS;
    int32_t l = -1, d = 0;
    if (c < nc) {
      const int64_t j = bar + j0 + c;
      l = (int32_t)sk.spanToLump[schurSpanOf(sk, span0, numSpans, j)];
      d = dest ? dst[j0 + c] : (int32_t)(j0 + c);
    }
    colLump[c] = l;
    dC[c] = d;
  }
  __syncthreads();
  if (tid < TS) {  // wave 0: ordinal of every column's lump among the lumps under the tile's columns
    const int c = tid;
    const bool first = c < nc && (c == 0 || colLump[c] != colLump[c - 1]);
    const unsigned long long firsts = __ballot(first);
    const int o = __popcll(firsts & (~0ull >> (63 - c))) - 1;
    if (first) ordLump[o] = colLump[c];
    if (c < nc) colOrd[c] = (uint8_t)o;
    if (c == 0) nOrdS = __popcll(firsts);
  }
  __syncthreads();
  const int nOrd = nOrdS;
  // base[r][o]: data offset of (row r, scalar 0) in lump o's column, so that element (r, j) is at
  // base + j (j an internal scalar); -1 where lump o has no block on the span of row r
  for (int x = tid; x < nr * nOrd; x += 256) {
    const int r = x / nOrd, o = x - r * nOrd;
    const int64_t L = ordLump[o], sa = rowSpan[r];
    int64_t lo = sk.chainColPtr[L], hi = sk.chainColPtr[L + 1] - 1;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (sk.chainRowSpan[mid] < sa) lo = mid + 1; else hi = mid;
    }
    int64_t b = -1;
    if (sk.chainRowSpan[lo] == sa) {
      const int64_t l0 = sk.lumpStart[L];
      b = sk.chainData[lo] + (int64_t)rowLoc[r] * (sk.lumpStart[L + 1] - l0) - l0;
    }
    base[r * TS + o] = b;
  }
  __syncthreads();
  T v[PER];
#pragma unroll
  for (int q = 0; q < PER; q++) {
    const int e = q * 256 + tid, r = e / TS, c = e % TS;
    T x = T(0);
    if (r < nr && c < nc && i0 + r >= j0 + c) {
      const int64_t b = base[r * TS + colOrd[c]];
      if (b >= 0) x = P[b + bar + j0 + c];
    }
    v[q] = x;
  }
  __syncthreads();  // the table is dead: its bytes take the image
#pragma unroll
  for (int q = 0; q < PER; q++) {
    const int e = q * 256 + tid;
    Ts[e / TS][e % TS] = v[q];
  }
  __syncthreads();
  if (I == J) {
#pragma unroll
    for (int q = 0; q < PER; q++) {
      const int e = q * 256 + tid, r = e / TS, c = e % TS;
      if (r < nr && c < nc) out[(int64_t)dR[r] * m + dC[c]] = r >= c ? Ts[r][c] : Ts[c][r];
    }
    return;
  }
#pragma unroll
  for (int q = 0; q < PER; q++) {
    const int e = q * 256 + tid, r = e / TS, c = e % TS;
    if (r < nr && c < nc) out[(int64_t)dR[r] * m + dC[c]] = v[q];
  }
#pragma unroll
  for (int q = 0; q < PER; q++) {
    const int e = q * 256 + tid, c = e / TS, r = e % TS;  // consecutive lanes: consecutive columns of (J, I)
    if (r < nr && c < nc) out[(int64_t)dC[c] * m + dR[r]] = Ts[r][c];
  }
}

// The adjoint of schurToDense in the data-gradient convention, over ALL patternGrad tiles (the whole
// buffer is written, never read): for a stored element e = (i, j) of a lump behind the cut
// Gd[i, j] + Gd[j, i] below the diagonal, Gd[i, i] on it, 0 above it; 0 for every element of a lump
// before the cut (tiles < firstTrailing).  Gd is any dense m x m matrix (it need not be symmetric).
// The Gd[j, i] of a tile are read along its rows into LDS, so both reads run along the lanes.
template <typename T>
__global__ void __launch_bounds__(256) schurFromDense(const GradTile* __restrict__ tiles, SkelDev sk,
                                                      int firstTrailing, int64_t bar, int64_t m,
                                                      const int32_t* __restrict__ dest, DataRef<const T> gdref,
                                                      DataRef<T> oref) {
  constexpr int PER = kGradElems / 256;
  __shared__ T Ts[kGradElems + kGradRows];
  __shared__ int32_t rowI[kGradRows], dI[kGradRows], dJ[kGradCols];
  const GP<const T> Gd = pickData(gdref);
  const GP<T> out = pickData(oref);
  const GP<const int32_t> dst = (GP<const int32_t>)dest;
  const GradTile t = tiles[blockIdx.x];
  const int tid = threadIdx.x;
  const int64_t l0 = sk.lumpStart[t.lump];
  const int64_t w = sk.lumpStart[t.lump + 1] - l0;
  const int nEl = t.nr * t.nc, S = t.nc | 1;
  if ((int)blockIdx.x < firstTrailing) {
#pragma unroll
    for (int q = 0; q < PER; q++) {
      const int e = q * 256 + tid;
      if (e < nEl) {
        const int r = e / t.nc, c = e - r * t.nc;
        out[t.off + r * w + c] = T(0);
      }
    }
    return;
  }
  const int64_t jb = l0 + t.c0 - bar;  // tile column 0, counted from bar
  if (tid < t.nr) {  // as patternGradTiles: the scalar of every tile row
    const int64_t r = t.r0 + tid;
    int32_t lo = t.chain, hi = t.chainEnd - 1;
    while (lo < hi) {
      const int32_t mid = (lo + hi) >> 1;
      if (sk.chainRowsTillEnd[mid] > r) hi = mid; else lo = mid + 1;
    }
    const int64_t sp = sk.chainRowSpan[lo];
    const int64_t s0 = sk.spanStart[sp], rows = sk.spanStart[sp + 1] - s0;
    const int64_t i = s0 + r - (sk.chainRowsTillEnd[lo] - rows) - bar;
    rowI[tid] = (int32_t)i;
    dI[tid] = dest ? dst[i] : (int32_t)i;
  } else if (tid >= kGradRows && tid < kGradRows + t.nc) {
    const int c = tid - kGradRows;
    dJ[c] = dest ? dst[jb + c] : (int32_t)(jb + c);
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < PER; q++) {
    const int e = q * 256 + tid;
    if (e < nEl) {
      const int c = e / t.nr, r = e - c * t.nr;
      if (rowI[r] > jb + c) Ts[r * S + c] = Gd[(int64_t)dJ[c] * m + dI[r]];
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < PER; q++) {
    const int e = q * 256 + tid;
    if (e < nEl) {
      const int r = e / t.nc, c = e - r * t.nc;
      const int64_t i = rowI[r], j = jb + c;
      T x = T(0);
      if (i >= j) {
        x = Gd[(int64_t)dI[r] * m + dJ[c]];
        if (i > j) x += Ts[r * S + c];
      }
      out[t.off + r * w + c] = x;
    }
  }
}

}  // namespace hipk
}  // namespace BaSpaCho
