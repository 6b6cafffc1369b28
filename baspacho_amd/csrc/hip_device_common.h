// Device-side types and helpers shared by every kernel header of the MI355X backend: how a kernel
// finds its matrix (DataRef, GP, pickData), the skeleton on the device, wave-level synchronisation,
// the matrix-core wrappers, and the self-validating words and watchdog of the persistent kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include <cstdint>

#include "hip_plan.h"

namespace BaSpaCho {
namespace hipk {

// One matrix (single) or a batch of identical-structure matrices (many, indexed by blockIdx.y);
// replaces the Plain/Batched policy structs of MatOpsCuda.cu:345-368.
template <typename T>
struct DataRef {
  T* single;
  T* const* many;
};

// Pointers that come out of memory (the batch's pointer array) or out of a select are "generic" to
// the compiler, and every access through them becomes a FLAT instruction, which counts against the
// LDS counter as well: each wait for an LDS read then also waits for the global loads in flight
// (the prefetch of the next K chunk, the operands of the next pairs ...).  The round trip through
// the global address space tells the compiler where the data lives; accesses become global_*.
// (a cast to the global address space and back is folded away: the pointers have to KEEP the
// address-space type down to the access, hence GP<T> throughout the kernels)
template <typename T>
using GP = __attribute__((address_space(1))) T*;

template <typename T>
__device__ __forceinline__ GP<T> pickData(const DataRef<T>& d) {
  return (GP<T>)(d.many ? d.many[blockIdx.y] : d.single);
}
__device__ __forceinline__ void atomicSub(GP<double> p, double v) { unsafeAtomicAdd((double*)p, -v); }
__device__ __forceinline__ void atomicSub(GP<float> p, float v) { unsafeAtomicAdd((float*)p, -v); }

__device__ __forceinline__ void waveSync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// workgroup barrier that orders LDS traffic only: __syncthreads() also drains the vector-memory
// counter, i.e. it waits for every global store in flight (hundreds of cycles when a kernel
// stores to memory between barriers, as the panel Cholesky does with its finished columns)
__device__ __forceinline__ void ldsBarrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// 1/sqrt(x): hardware estimate (v_rsq_f64 / v_rsq_f32) refined by Newton steps to full precision.
// The library rsqrt() expands to a full-precision sqrt plus a division (hundreds of dependent
// cycles), which sits on the serial critical path of the panel Cholesky.
__device__ __forceinline__ double fastRsqrt(double x) {
  double y = __builtin_amdgcn_rsq(x);
#pragma unroll
  for (int it = 0; it < 2; it++) {
    const double r = fma(-0.5 * x * y, y, 0.5);  // 0.5 - 0.5 x y^2
    y = fma(y, r, y);
  }
  return y;
}
__device__ __forceinline__ float fastRsqrt(float x) {
  float y = __builtin_amdgcn_rsqf(x);
  const float r = fmaf(-0.5f * x * y, y, 0.5f);
  return fmaf(y, r, y);
}

__device__ __forceinline__ void atomicSub(double* p, double v) { unsafeAtomicAdd(p, -v); }
__device__ __forceinline__ void atomicSub(float* p, float v) { unsafeAtomicAdd(p, -v); }

// device view of the int64 skeleton arrays (also what deviceAccessor() hands out)
struct SkelDev {
  const int64_t* spanStart;
  const int64_t* spanToLump;
  const int64_t* lumpStart;
  const int64_t* spanOffsetInLump;
  const int64_t* chainColPtr;
  const int64_t* chainRowSpan;
  const int64_t* chainData;
  const int64_t* chainRowsTillEnd;
  const int64_t* boardColPtr;
  const int64_t* boardChainColOrd;
};

typedef double double4_t __attribute__((ext_vector_type(4)));
typedef float float4_t __attribute__((ext_vector_type(4)));

template <typename T>
struct Mfma;
template <>
struct Mfma<double> {
  using Acc = double4_t;
  static __device__ __forceinline__ Acc run(double a, double b, Acc c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int row(int lane, int reg) { return (lane >> 4) + 4 * reg; }
  // inverse of (q, reg) -> row: the m with row(16 q + *, reg) == m has 4 q + reg == colOfRow(m)
  static __device__ __forceinline__ int colOfRow(int m) { return 4 * (m & 3) + (m >> 2); }
};
template <>
struct Mfma<float> {
  using Acc = float4_t;
  static __device__ __forceinline__ Acc run(float a, float b, Acc c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int row(int lane, int reg) { return 4 * (lane >> 4) + reg; }
  static __device__ __forceinline__ int colOfRow(int m) { return m; }
};

template <typename T>
__device__ __forceinline__ T readLaneT(T v, int srcLane);
template <>
__device__ __forceinline__ double readLaneT<double>(double v, int srcLane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), srcLane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), srcLane);
  return __hiloint2double(hi, lo);
}
template <>
__device__ __forceinline__ float readLaneT<float>(float v, int srcLane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), srcLane));
}

// ---- words that validate themselves, and the watchdog of every spin (persistent solve sweeps,
// hip_sweep_kernels.h; persistent factor tail, hip_tail_kernel.h)
template <typename T>
struct SweepBits;
template <>
struct SweepBits<double> {
  using U = unsigned long long;
  static constexpr U kArmed = ~0ull, kNan = 0x7ff8000000000000ull;
};
template <>
struct SweepBits<float> {
  using U = unsigned;
  static constexpr U kArmed = ~0u, kNan = 0x7fc00000u;
};

template <typename T>
__device__ __forceinline__ T sweepPeek(GP<const T> p) {
  using U = typename SweepBits<T>::U;
  const U u = __hip_atomic_load((GP<const U>)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return __builtin_bit_cast(T, u);
}
template <typename T>
__device__ __forceinline__ bool sweepValid(T v) {
  using U = typename SweepBits<T>::U;
  return __builtin_bit_cast(U, v) != SweepBits<T>::kArmed;
}
template <typename T>
__device__ __forceinline__ void sweepPublish(GP<T> p, T v) {
  using U = typename SweepBits<T>::U;
  U u = __builtin_bit_cast(U, v);
  if (u == SweepBits<T>::kArmed) u = SweepBits<T>::kNan;
  __hip_atomic_store((GP<U>)p, u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct SweepWatch {
  GP<unsigned> abortWord;
  unsigned* hostErr;
  long long limit;
  long long t0;
  unsigned it;
  __device__ __forceinline__ void reset() {
    t0 = 0;
    it = 0;
  }
  // after an unsuccessful poll: true = give up (wave-uniform)
  __device__ __forceinline__ bool expired() {
    if ((++it & 15u) != 0u) return false;
    if (__hip_atomic_load(abortWord, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) return true;
    const long long now = (long long)wall_clock64();
    if (t0 == 0) {
      t0 = now;
      return false;
    }
    if (now - t0 <= limit) return false;
    __hip_atomic_store(abortWord, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(hostErr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return true;
  }
};

// every lane polls its own N words until all of them (in every lane) have been published
template <typename T, int N>
__device__ __forceinline__ bool sweepWait(GP<const T> (&p)[N], const bool (&need)[N], T (&out)[N],
                                          SweepWatch& watch) {
  watch.reset();
  for (;;) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < N; i++) {
      if (need[i]) {
        out[i] = sweepPeek<T>(p[i]);
        ok = ok && sweepValid(out[i]);
      }
    }
    if (__all(ok)) return true;
    if (watch.expired()) return false;
    __builtin_amdgcn_s_sleep(1);
  }
}

}  // namespace hipk
}  // namespace BaSpaCho
