// Kernels of the ordered Hessian fill of the BAL pipeline (balFillOrdered, bal_pipeline.h): the same
// H += J^T J, g += J^T r as balFillKernel without atomics, every sum in the order the host plan
// (bal_fill_plan.h) fixes.  The order is stated in bal_pipeline.h and DESIGN.md section 9; the numpy
// model of tests/bal_fill_ref.py restates it.  Included by bal_pipeline.hip only.
//
// Four launches: pairs (camera-point blocks), points (point diagonal blocks and gradient slices),
// camera chunks (partial sums of the camera diagonal block and gradient over one chunk of a camera's
// list, into the plan's scratch) and the fold of the chunk partials.  No workgroup waits for another;
// an element that no observation maps to is not written at all.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "bal_fill_plan.h"
#include "hip_ordered_sum.h"

namespace BaSpaCho {
namespace balfill {

// the plan's tables on the device
struct Tables {
  const int32_t *ptPtr, *ptObs, *pairPtr, *pairStride, *pairFlip;
  const int64_t* pairOff;
  const int32_t *camObs, *camChunkPtr, *chunkCam, *chunkBegin, *chunkEnd;
  const int64_t *ptDiagOff, *camDiagOff, *ptStart, *camStart;
  const int32_t *ptDiagStride, *camDiagStride;
  double* part;  // scratch: partialWords() doubles per chunk
};

// fl(fl(a0 * b0) + fl(a1 * b1)) and fl(s + v), every operation rounded on its own (rmul / radd: an fma
// would round once where the documented order rounds three times)
__device__ __forceinline__ double term(double a0, double b0, double a1, double b1) {
  return hipk::radd(hipk::rmul(a0, b0), hipk::rmul(a1, b1));
}
__device__ __forceinline__ double add(double s, double v) { return hipk::radd(s, v); }

constexpr int kThreads = 256;

// One thread per element of a pair's CS x 3 block: a left fold from +0.0 over the pair's run of ptObs.
template <typename T, int CS>
__global__ __launch_bounds__(kThreads) void balFillPairs(int64_t numPairs, Tables t, const double* Jc,
                                                         const double* Jp, T* data) {
  constexpr int E = 3 * CS;
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t q = g / E;
  if (q >= numPairs) return;
  const int e = (int)(g - q * E), i = e / 3, j = e % 3;  // (camera row, point column)
  double s = 0.0;
  for (int32_t x = t.pairPtr[q]; x < t.pairPtr[q + 1]; x++) {
    const int64_t o = t.ptObs[x];
    const double* jc = Jc + 2 * CS * o;
    const double* jp = Jp + 6 * o;
    s = add(s, term(jc[i], jp[j], jc[CS + i], jp[3 + j]));
  }
  const int64_t bs = t.pairStride[q];
  T* p = data + t.pairOff[q] + (t.pairFlip[q] ? j * bs + i : i * bs + j);
  *p = *p + (T)s;
}

// Twelve threads per point: the nine elements of its diagonal block and the three of its gradient
// slice, each a left fold from +0.0 over the point's list.  A point without observations is left alone.
template <typename T>
__global__ __launch_bounds__(kThreads) void balFillPoints(int64_t numPts, Tables t, const double* Jp,
                                                          const double* res, T* data, T* grad) {
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t p = g / 12;
  if (p >= numPts) return;
  const int e = (int)(g - p * 12);
  const int32_t x0 = t.ptPtr[p], x1 = t.ptPtr[p + 1];
  if (x0 == x1 || (e >= 9 && grad == nullptr)) return;
  const int i = e < 9 ? e / 3 : e - 9, j = e % 3;
  double s = 0.0;
  for (int32_t x = x0; x < x1; x++) {
    const int64_t o = t.ptObs[x];
    const double* jp = Jp + 6 * o;
    const double b0 = e < 9 ? jp[j] : res[2 * o], b1 = e < 9 ? jp[3 + j] : res[2 * o + 1];
    s = add(s, term(jp[i], b0, jp[3 + i], b1));
  }
  T* d = e < 9 ? data + t.ptDiagOff[p] + (int64_t)i * t.ptDiagStride[p] + j : grad + t.ptStart[p] + i;
  *d = *d + (T)s;
}

// element e of a chunk partial: the lower triangle of the camera block row by row, (0,0), (1,0), (1,1),
// (2,0), .., then the gradient entries
template <int CS>
struct Partial {
  static constexpr int kTri = CS * (CS + 1) / 2, kWords = kTri + CS;
  // (a, b) of e < kTri; a gradient entry e >= kTri is (e - kTri, -1)
  __device__ static void decode(int e, int& a, int& b) {
    if (e >= kTri) {
      a = e - kTri;
      b = -1;
      return;
    }
    a = 0;
    while ((a + 1) * (a + 2) / 2 <= e) a++;
    b = e - a * (a + 1) / 2;
  }
};

// One workgroup per chunk.  The chunk's rows -- Jc[o][2][CS] and res[o][2] of the observations
// camObs[begin .. end) -- are staged in LDS, consecutive lanes walking the consecutive words of a row.
// Thread (e, l), l < kBalFillLanes, then folds the terms of element e at the chunk positions l,
// l + kBalFillLanes, .. from +0.0; the lane sums are folded by halving, and lane 0 writes word e of the
// chunk's partial.
template <int CS>
__global__ __launch_bounds__(kThreads) void balFillCamChunks(Tables t, const double* Jc, const double* res) {
  constexpr int W = kBalFillLanes, C = kBalFillChunk, RL = 2 * CS + 2;  // row: J0[CS], J1[CS], r0, r1
  static_assert(Partial<CS>::kWords * W <= kThreads && (W & (W - 1)) == 0 && W <= 64, "lanes per element");
  __shared__ double rows[C * RL];
  __shared__ int32_t obs[C];
  const int tid = threadIdx.x;
  const int64_t k = blockIdx.x;
  const int32_t begin = t.chunkBegin[k];
  const int n = t.chunkEnd[k] - begin;  // 1 .. C
  for (int r = tid; r < n; r += kThreads) obs[r] = t.camObs[begin + r];
  __syncthreads();
  for (int w = tid; w < n * 2 * CS; w += kThreads) {
    const int r = w / (2 * CS), c = w - r * (2 * CS);
    rows[r * RL + c] = Jc[(int64_t)2 * CS * obs[r] + c];
  }
  for (int w = tid; w < 2 * n; w += kThreads) {
    const int r = w >> 1, c = w & 1;
    rows[r * RL + 2 * CS + c] = res[(int64_t)2 * obs[r] + c];
  }
  __syncthreads();
  const int e = tid / W, l = tid % W;
  const bool active = e < Partial<CS>::kWords;
  int a = 0, b = 0;
  if (active) Partial<CS>::decode(e, a, b);
  const int b0 = b < 0 ? 2 * CS : b, b1 = b < 0 ? 2 * CS + 1 : CS + b;
  double s = 0.0;
  if (active) {
    for (int r = l; r < n; r += W) {
      const double* row = rows + r * RL;
      s = add(s, term(row[a], row[b0], row[CS + a], row[b1]));
    }
  }
  // T[l] += T[l + h] for l < h, h = W / 2 .. 1 (every lane of the wave takes part in the shuffles; the
  // W lanes of an element are consecutive lanes of one wave)
#pragma unroll
  for (int h = W / 2; h > 0; h >>= 1) {
    const double o = __shfl_down(s, h, W);
    if (l < h) s = add(s, o);
  }
  if (active && l == 0) t.part[k * Partial<CS>::kWords + e] = s;
}

// One thread per (camera, partial word): a left fold from +0.0 over the camera's chunk partials in chunk
// order, applied once to the diagonal block (both triangles: fl(a * b) == fl(b * a), so the mirrored
// element has the same sum) or to the gradient slice.  A camera without observations is left alone.
template <typename T, int CS>
__global__ __launch_bounds__(kThreads) void balFillCamFold(int64_t numCams, Tables t, T* data, T* grad) {
  constexpr int NW = Partial<CS>::kWords;
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t c = g / NW;
  if (c >= numCams) return;
  const int e = (int)(g - c * NW);
  const int32_t k0 = t.camChunkPtr[c], k1 = t.camChunkPtr[c + 1];
  if (k0 == k1) return;
  int a, b;
  Partial<CS>::decode(e, a, b);
  if (b < 0 && grad == nullptr) return;
  double s = 0.0;
  for (int64_t k = k0; k < k1; k++) s = add(s, t.part[k * NW + e]);
  if (b < 0) {
    T* d = grad + t.camStart[c] + a;
    *d = *d + (T)s;
    return;
  }
  const int64_t ds = t.camDiagStride[c];
  T* d = data + t.camDiagOff[c];
  d[a * ds + b] = d[a * ds + b] + (T)s;
  if (a != b) d[b * ds + a] = d[b * ds + a] + (T)s;
}

}  // namespace balfill
}  // namespace BaSpaCho
