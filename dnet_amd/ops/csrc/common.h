// Common helpers for dnet_amd HIP kernels (gfx950 / CDNA4 only).
//
// All kernels in this extension are written directly for MI355X: wave64,
// vectorized bf16 loads (short4/short8 reinterpret), f32 accumulation,
// grid sized for 256 CUs in 8 XCDs. No CUDA compatibility paths.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <torch/extension.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#define DNET_CHECK(cond, msg) TORCH_CHECK(cond, msg)
#define DNET_CHECK_HIP(call)                                              \
  do {                                                                    \
    hipError_t _e = (call);                                               \
    TORCH_CHECK(_e == hipSuccess, "HIP error: ", hipGetErrorString(_e));  \
  } while (0)

namespace dnet {

constexpr int kWave = 64;  // CDNA wavefront

using bf16 = __hip_bfloat16;

// Vector types for wide loads (16 B = 8 bf16 per lane).
struct alignas(16) short8 { short x[8]; };
struct alignas(8) short4v { short x[4]; };

__device__ __forceinline__ float b2f(const bf16 v) { return __bfloat162float(v); }
__device__ __forceinline__ bf16 f2b(const float v) { return __float2bfloat16(v); }

// bf16 bits -> float without library calls
__device__ __forceinline__ float bits2f(const short s) {
  union { unsigned u; float f; } cvt;
  cvt.u = (unsigned)(unsigned short)s << 16;
  return cvt.f;
}
__device__ __forceinline__ short f2bits(const float f) {
  // round-to-nearest-even bf16
  union { float f; unsigned u; } cvt;
  cvt.f = f;
  unsigned u = cvt.u;
  unsigned rounding = 0x7FFF + ((u >> 16) & 1);
  return (short)((u + rounding) >> 16);
}

// Wave-wide f32 sum reduction (64 lanes).
__device__ __forceinline__ float wave_reduce_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;  // valid in lane 0
}

__device__ __forceinline__ float wave_reduce_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_down(v, off, 64));
  return v;  // valid in lane 0
}

// Block-wide sum using LDS scratch (scratch must hold >= blockDim.x/64 floats).
__device__ __forceinline__ float block_reduce_sum(float v, float* scratch) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wid = threadIdx.x / kWave;
  v = wave_reduce_sum(v);
  if (lane == 0) scratch[wid] = v;
  __syncthreads();
  const int nw = blockDim.x / kWave;
  float r = 0.f;
  if (threadIdx.x < nw) r = scratch[threadIdx.x];
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) r += __shfl_down(r, off, 64);
  r = __shfl(r, 0, 64);
  if (threadIdx.x == 0) scratch[0] = r;
  __syncthreads();
  r = scratch[0];
  __syncthreads();
  return r;
}

// Split-k partials of the decode GEMM: `splits` slices of `stride` f32 each
// (layout [sk][M][N], gemm_m16.hip.cpp). The consumers sum slices
// 0..splits-1 in that fixed order, in f32, so the result does not depend
// on which split finished first.
__device__ __forceinline__ float sum_slices(const float* p,
                                            const int64_t stride,
                                            const int splits) {
  float v = p[0];
  for (int s = 1; s < splits; ++s) v += p[s * stride];
  return v;
}

__device__ __forceinline__ void slice_add(float& a, const float b) { a += b; }
__device__ __forceinline__ void slice_add(float4& a, const float4 b) {
  a.x += b.x;
  a.y += b.y;
  a.z += b.z;
  a.w += b.w;
}

// out[k] = sum over the slices, in order, of the T (float or float4) at
// p[k], for NP places at once. All SK * NP loads are issued before the
// first add: with a run-time trip count each load waits for the add
// before it, and a consumer that reads 8 slices pays 8 memory latencies
// in a row (measured: rmsnorm 13.1 us against 5.8 us for one slice).
template <typename T, int NP, int SK>
__device__ __forceinline__ void sum_slices_fixed(const float* const (&p)[NP],
                                                 const int64_t stride,
                                                 T (&out)[NP]) {
  T t[SK][NP];
#pragma unroll
  for (int s = 0; s < SK; ++s)
#pragma unroll
    for (int k = 0; k < NP; ++k)
      t[s][k] = *reinterpret_cast<const T*>(p[k] + s * stride);
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    out[k] = t[0][k];
#pragma unroll
    for (int s = 1; s < SK; ++s) slice_add(out[k], t[s][k]);
  }
}

// The split counts pick_splitk produces are powers of two; anything else
// (a forced count) takes the loop.
template <typename T, int NP>
__device__ __forceinline__ void sum_slices_multi(const float* const (&p)[NP],
                                                 const int64_t stride,
                                                 const int splits,
                                                 T (&out)[NP]) {
  switch (splits) {  // uniform over the grid
    case 1: sum_slices_fixed<T, NP, 1>(p, stride, out); break;
    case 2: sum_slices_fixed<T, NP, 2>(p, stride, out); break;
    case 4: sum_slices_fixed<T, NP, 4>(p, stride, out); break;
    case 8: sum_slices_fixed<T, NP, 8>(p, stride, out); break;
    case 16: sum_slices_fixed<T, NP, 16>(p, stride, out); break;
    default:
#pragma unroll
      for (int k = 0; k < NP; ++k) {
        out[k] = *reinterpret_cast<const T*>(p[k]);
        for (int s = 1; s < splits; ++s)
          slice_add(out[k], *reinterpret_cast<const T*>(p[k] + s * stride));
      }
  }
}

inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// The torch-ROCm stream for the current device (what torch kernels launch on).
inline hipStream_t current_stream() {
  return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
}

}  // namespace dnet
