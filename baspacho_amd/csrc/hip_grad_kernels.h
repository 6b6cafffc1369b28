// Gradients on the block pattern of L: the log-determinant of a factor and the write-only projection
// that turns dense gradients into gradients of the stored elements.  Work lists: hip_backend.hip
// (GradDev, built once per structure); conventions and numbers: DESIGN.md section 13.
//
// CONVENTIONS.  `data` is the solver's numeric layout and vectors are in its internal order.  The
// matrix is A(d), symmetric, with A_ij = A_ji = d_e for every stored element e = (i, j): every element
// of the off-diagonal chain blocks and i >= j inside the diagonal blocks (the strictly-upper elements
// of the diagonal blocks are not read by factor()).  For a dense gradient G = df/dA, df/dd_e is
// G_ij + G_ji for i > j, G_ii on the diagonal and 0 on the strictly-upper elements.
//
//   logDet:      out[q] = 2 sum_i log L_ii, accumulated in fp64 for both data types.  Diagonal element
//                i of lump l is at chainData[chainColPtr[l]] + i (w_l + 1).  A non-positive or NaN
//                pivot gives -inf or NaN.
//   patternGrad: for every stored element e = (i, j) of matrix q
//                  i > j:  out_e = s[q] 2 Z_e + alpha sum_k (U_ik V_jk + V_ik U_jk)
//                  i = j:  out_e = s[q] Z_e   + alpha sum_k U_ik V_ik
//                  i < j:  out_e = 0          (strictly-upper elements of the diagonal blocks)
//                U, V column-major n x k (U_ik at U[i + k * ld]); without Z the first term is 0, without
//                U / V the second.  `out` is only written.
//   patternOuter (patternGradTiles<T, true>): the non-symmetric rank-k projection, no Z term
//                  i >= j: out_e = alpha sum_k U_ik V_jk
//                  i < j:  out_e = 0
//
// BATCH: matrix q = blockIdx.y finds its arrays through pickData, as the selinv kernels do.  There are
// no atomics and every sum runs in a fixed order that does not depend on q: results are bitwise
// reproducible and member q of a batch is bitwise the single call.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "hip_device_common.h"

namespace BaSpaCho {
namespace hipk {

// ---- logDet ---------------------------------------------------------------------------------------
// diagonal elements per workgroup of the first pass (256 threads x 8)
constexpr int kLogDetChunk = 2048;

// Pass 1: workgroup b sums log L_ii over the diagonal elements [b * kLogDetChunk, ...) of matrix
// blockIdx.y into part[blockIdx.y * nParts + b].  firstLump[b] is the lump of element b * kLogDetChunk
// (firstLump[nParts] = the last lump): a thread finds the lump of its element by bisection on lumpStart
// between the two.
template <typename T>
__global__ void __launch_bounds__(256) logDetPartial(SkelDev sk, const int32_t* __restrict__ firstLump,
                                                     int64_t n, int nParts, DataRef<const T> dref,
                                                     double* __restrict__ part) {
  __shared__ double red[256];
  const GP<const T> data = pickData(dref);
  const int b = blockIdx.x, tid = threadIdx.x;
  const int32_t lo0 = firstLump[b], hi0 = firstLump[b + 1];
  double acc = 0.0;
#pragma unroll
  for (int m = 0; m < kLogDetChunk / 256; m++) {
    const int64_t g = (int64_t)b * kLogDetChunk + m * 256 + tid;
    if (g < n) {
      int32_t lo = lo0, hi = hi0;  // lumpStart[lo] <= g; the answer is in [lo, hi]
      while (lo < hi) {
        const int32_t mid = (lo + hi + 1) >> 1;
        if (sk.lumpStart[mid] <= g) lo = mid; else hi = mid - 1;
      }
      const int64_t c0 = sk.lumpStart[lo], w = sk.lumpStart[lo + 1] - c0;
      const T d = data[sk.chainData[sk.chainColPtr[lo]] + (g - c0) * (w + 1)];
      acc += log((double)d);
    }
  }
  red[tid] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) part[(int64_t)blockIdx.y * nParts + b] = red[0];
}

// Pass 2: one workgroup per matrix adds its nParts partial sums in a fixed order; out[blockIdx.y].
template <typename T>
__global__ void __launch_bounds__(256) logDetFinal(const double* __restrict__ part, int nParts,
                                                   T* __restrict__ out) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const double* p = part + (int64_t)blockIdx.y * nParts;
  double acc = 0.0;
  for (int b = tid; b < nParts; b += 256) acc += p[b];
  red[tid] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) out[blockIdx.y] = (T)(2.0 * red[0]);
}

// ---- patternGrad ----------------------------------------------------------------------------------
// A tile is rows [r0, r0 + nr) x columns [c0, c0 + nc) of one lump column (rows counted from the top
// of the lump's diagonal block, so the tile's data is data[off + r * w + c], r < nr, c < nc).  Chains
// [chain, chainEnd) hold its rows.  Tiles never cross lumps.
constexpr int kGradRows = 128, kGradCols = 64, kGradElems = 2048, kGradK = 16;

struct GradTile {
  int64_t off;
  int32_t lump, r0, c0, nr, nc, chain, chainEnd, pad;
};
static_assert(sizeof(GradTile) == 40, "GradTile is uploaded as raw bytes");

// One workgroup of 256 per tile; the elements of the tile are walked flat across the lanes
// (e -> (e / nc, e % nc)), so the stores stay coalesced for 3- and 9-wide lumps.  The U / V rows of the
// tile's rows and of its columns go through LDS in chunks of kGradK right-hand sides; each thread keeps
// the sums of its (at most 8) elements in registers.  Dynamic LDS: (kGradRows + kGradCols) x
// (kc + 1) x 4 values of T, kc = min(k, kGradK) (0 without U / V).  Outer = true: patternOuter (only
// the U rows and V columns of the tile are loaded; zref / zScale unused).
template <typename T, bool Outer = false>
__global__ void __launch_bounds__(256) patternGradTiles(const GradTile* __restrict__ tiles, SkelDev sk,
                                                        DataRef<const T> zref, const T* __restrict__ zScale,
                                                        DataRef<const T> uref, DataRef<const T> vref,
                                                        int64_t ld, int k, T alpha, DataRef<T> oref) {
  extern __shared__ __align__(16) unsigned char gradSmem[];
  __shared__ int64_t rowG[kGradRows];
  constexpr int PER = kGradElems / 256;
  const GradTile t = tiles[blockIdx.x];
  const int tid = threadIdx.x;
  const int64_t l0 = sk.lumpStart[t.lump];
  const int64_t w = sk.lumpStart[t.lump + 1] - l0;
  const int64_t j0 = l0 + t.c0;  // global column of tile column 0
  const int nEl = t.nr * t.nc;

  // global row of every tile row: bisection over the tile's chains on chainRowsTillEnd
  if (tid < t.nr) {
    const int64_t r = t.r0 + tid;
    int32_t lo = t.chain, hi = t.chainEnd - 1;  // first chain whose rowsTillEnd > r
    while (lo < hi) {
      const int32_t mid = (lo + hi) >> 1;
      if (sk.chainRowsTillEnd[mid] > r) hi = mid; else lo = mid + 1;
    }
    const int64_t sp = sk.chainRowSpan[lo];
    const int64_t s0 = sk.spanStart[sp], rows = sk.spanStart[sp + 1] - s0;
    rowG[tid] = s0 + r - (sk.chainRowsTillEnd[lo] - rows);
  }
  __syncthreads();

  T acc[PER];
#pragma unroll
  for (int m = 0; m < PER; m++) acc[m] = T(0);

  if (k > 0) {
    const GP<const T> U = pickData(uref);
    const GP<const T> V = pickData(vref);
    const int kcMax = k < kGradK ? k : kGradK, S = kcMax + 1;
    T* Ur = reinterpret_cast<T*>(gradSmem);  // [kGradRows][S]
    T* Vr = Ur + kGradRows * S;
    T* Uc = Vr + kGradRows * S;  // [kGradCols][S]
    T* Vc = Uc + kGradCols * S;
    for (int k0 = 0; k0 < k; k0 += kGradK) {
      const int kc = (k - k0) < kGradK ? (k - k0) : kGradK;
      __syncthreads();  // the previous chunk has been consumed
      for (int x = tid; x < t.nr * kc; x += 256) {
        const int r = x % t.nr, kk = x / t.nr;  // consecutive lanes: consecutive rows of one column
        const int64_t a = rowG[r] + (int64_t)(k0 + kk) * ld;
        Ur[r * S + kk] = U[a];
        if (!Outer) Vr[r * S + kk] = V[a];
      }
      for (int x = tid; x < t.nc * kc; x += 256) {
        const int c = x % t.nc, kk = x / t.nc;
        const int64_t a = j0 + c + (int64_t)(k0 + kk) * ld;
        if (!Outer) Uc[c * S + kk] = U[a];
        Vc[c * S + kk] = V[a];
      }
      __syncthreads();
#pragma unroll
      for (int m = 0; m < PER; m++) {
        const int e = m * 256 + tid;
        if (e < nEl) {
          const int r = e / t.nc, c = e - r * t.nc;
          const int64_t i = rowG[r], j = j0 + c;
          const T* ui = Ur + r * S;
          const T* vi = Vr + r * S;
          const T* uj = Uc + c * S;
          const T* vj = Vc + c * S;
          T s = acc[m];
          if (Outer) {
            if (i >= j)
              for (int kk = 0; kk < kc; kk++) s = fma(ui[kk], vj[kk], s);
          } else if (i > j) {
            for (int kk = 0; kk < kc; kk++) s = fma(ui[kk], vj[kk], fma(vi[kk], uj[kk], s));
          } else {
            for (int kk = 0; kk < kc; kk++) s = fma(ui[kk], vi[kk], s);
          }
          acc[m] = s;
        }
      }
    }
  }

  const bool hasZ = zScale != nullptr;
  const GP<const T> Z = hasZ ? pickData(zref) : GP<const T>(nullptr);
  const T sc = hasZ ? zScale[blockIdx.y] : T(0);
  const GP<T> out = pickData(oref);
#pragma unroll
  for (int m = 0; m < PER; m++) {
    const int e = m * 256 + tid;
    if (e < nEl) {
      const int r = e / t.nc, c = e - r * t.nc;
      const int64_t i = rowG[r], j = j0 + c;
      const int64_t a = t.off + r * w + c;
      T v = T(0);
      if (i >= j) {
        v = alpha * acc[m];
        if (hasZ) {
          const T zs = sc * Z[a];
          v += (i > j) ? T(2) * zs : zs;
        }
      }
      out[a] = v;
    }
  }
}

}  // namespace hipk
}  // namespace BaSpaCho
