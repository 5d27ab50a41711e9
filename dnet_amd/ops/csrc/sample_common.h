// Row sweeps, the order-preserving key and the fixed-point helpers shared by
// the fused sampler (sample.hip.cpp) and the logprob kernel
// (logprobs.hip.cpp). One 1024-thread workgroup per row; wave w owns a
// contiguous range of 16-byte slots, so wave totals are in vocabulary order.
#pragma once

#include "common.h"

#include <climits>
#include <cmath>

namespace dnet {
namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / kWave;
constexpr int kBins = 2048;          // 11-bit radix digit
constexpr float kFxScale = 0x1p40f;  // fixed-point step 2^-40
constexpr int kCountMask = 0x3FFFFFFF;
constexpr int kPromptBit = 0x40000000;

using u64 = unsigned long long;

template <typename T> struct VecOf;
template <> struct VecOf<short> { static constexpr int n = 8; };  // bf16 bits
template <> struct VecOf<float> { static constexpr int n = 4; };

struct Row {
  const void* l;      // first element of the row
  const int* seen;    // row of the seen table, or nullptr when no penalty acts
  const float* bias;  // row of the logit-bias table, or nullptr when off
  int V;
  int off;            // elements between the previous 16-B boundary and l
  bool seen_vec;      // seen row shares the 16-B phase of the logits row
  bool bias_vec;      // bias row shares it
  float rep, pres, freq;
};

__device__ __forceinline__ float penalise(float l, const int w, const Row& r) {
  const int c = w & kCountMask;
  if ((c > 0 || (w & kPromptBit)) && r.rep != 1.f)
    l = l > 0.f ? __fdiv_rn(l, r.rep) : __fmul_rn(l, r.rep);
  l = __fsub_rn(l, __fmul_rn(r.freq, (float)c));
  if (c > 0) l = __fsub_rn(l, r.pres);
  return l;
}

// Slot s holds elements [s*N - off, s*N - off + N). Elements outside
// [0, V) come back as NaN, which every pass ignores. The bias is added to
// the raw logit first; the penalties act on the sum. kBias = false compiles
// the bias out, so a launch without a table runs the sweeps it always ran.
template <typename T, bool kBias = false>
__device__ __forceinline__ void load_slot(const Row& r, const int s,
                                          float (&v)[VecOf<T>::n]) {
  constexpr int N = VecOf<T>::n;
  const int e0 = s * N - r.off;
  int w[N];
  if (e0 >= 0 && e0 + N <= r.V) {
    const T* p = reinterpret_cast<const T*>(r.l) + e0;
    if constexpr (N == 8) {
      const short8 raw = *reinterpret_cast<const short8*>(p);
#pragma unroll
      for (int j = 0; j < N; ++j) v[j] = bits2f(raw.x[j]);
    } else {
      const float4 raw = *reinterpret_cast<const float4*>(p);
      v[0] = raw.x; v[1] = raw.y; v[2] = raw.z; v[3] = raw.w;
    }
    if (kBias && r.bias) {
      const float* bp = r.bias + e0;
      if (r.bias_vec) {
#pragma unroll
        for (int j = 0; j < N; j += 4) {
          const float4 q = *reinterpret_cast<const float4*>(bp + j);
          v[j] = __fadd_rn(v[j], q.x);
          v[j + 1] = __fadd_rn(v[j + 1], q.y);
          v[j + 2] = __fadd_rn(v[j + 2], q.z);
          v[j + 3] = __fadd_rn(v[j + 3], q.w);
        }
      } else {
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] = __fadd_rn(v[j], bp[j]);
      }
    }
    if (r.seen) {
      const int* sp = r.seen + e0;
      if (r.seen_vec) {
#pragma unroll
        for (int j = 0; j < N; j += 4) {
          const int4 q = *reinterpret_cast<const int4*>(sp + j);
          w[j] = q.x; w[j + 1] = q.y; w[j + 2] = q.z; w[j + 3] = q.w;
        }
      } else {
#pragma unroll
        for (int j = 0; j < N; ++j) w[j] = sp[j];
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const int idx = e0 + j;
      const bool ok = idx >= 0 && idx < r.V;
      float f = NAN;
      if (ok) {
        if constexpr (N == 8)
          f = bits2f(reinterpret_cast<const short*>(r.l)[idx]);
        else
          f = reinterpret_cast<const float*>(r.l)[idx];
        if (kBias && r.bias) f = __fadd_rn(f, r.bias[idx]);
      }
      v[j] = f;
      w[j] = (ok && r.seen) ? r.seen[idx] : 0;
    }
  }
  if (r.seen) {
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = penalise(v[j], w[j], r);
  }
}

// f(idx, penalised logit) over this lane's share of slots [s0, s1).
template <typename T, bool kBias = false, typename F>
__device__ __forceinline__ void sweep(const Row& r, const int s0, const int s1,
                                      const int lane, F&& f) {
  constexpr int N = VecOf<T>::n;
  for (int s = s0 + lane; s < s1; s += kWave) {
    float v[N];
    load_slot<T, kBias>(r, s, v);
    const int e0 = s * N - r.off;
#pragma unroll
    for (int j = 0; j < N; ++j) f(e0 + j, v[j]);
  }
}

// Order-preserving key: a > b  <=>  fkey(a) > fkey(b) for non-NaN floats,
// and a == b <=> equal keys (-0 is folded onto +0 first).
__device__ __forceinline__ unsigned fkey(const float a) {
  const unsigned u = __float_as_uint(a + 0.f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// distance to the max (<= 0), the exponent before scaling
__device__ __forceinline__ float dist(const float l, const float lmax) {
  return __fsub_rn(l, lmax) + 0.f;
}
// e = exp(d / temp) as 2^(d * c), c = log2(e) / temp held as hi + lo so
// that the product rounds once, then the 1-ulp v_exp_f32
struct Scale { float hi, lo; };
// Below 2^-160 (a -inf logit included) the weight is exactly 0: it is 0 in
// fixed point anyway, and d * c.lo must not meet an overflowed d * c.hi.
__device__ __forceinline__ float weight(const float d, const Scale c) {
  if (!(__fmul_rn(d, c.hi) >= -160.f)) return 0.f;
  return __builtin_amdgcn_exp2f(__fmaf_rn(d, c.hi, __fmul_rn(d, c.lo)));
}
__device__ __forceinline__ u64 to_fx(const float e) {
  return (u64)__fmul_rn(e, kFxScale);
}

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return __shfl(v, 0, 64);
}

__device__ __forceinline__ u64 wave_incl_scan_u64(u64 v, const int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const u64 o = __shfl_up(v, off, 64);
    if (lane >= off) v += o;
  }
  return v;
}

// Exclusive prefix sum of v over threadIdx.x. lds holds kWaves values.
__device__ __forceinline__ u64 block_excl_scan_u64(const u64 v, u64* lds) {
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  const u64 incl = wave_incl_scan_u64(v, lane);
  __syncthreads();
  if (lane == kWave - 1) lds[wid] = incl;
  __syncthreads();
  u64 base = 0;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) base += (i < wid) ? lds[i] : 0;
  return base + incl - v;
}

// Wave w owns slots [s0, s1): contiguous, a multiple of 64 long.
template <typename T>
__device__ __forceinline__ void wave_range(const Row& r, const int wid,
                                           int& s0, int& s1) {
  constexpr int N = VecOf<T>::n;
  const int nslots = (r.V + r.off + N - 1) / N;
  const int spw = ((nslots + kWaves - 1) / kWaves + kWave - 1) / kWave * kWave;
  s0 = min(wid * spw, nslots);
  s1 = min(s0 + spw, nslots);
}

}  // namespace
}  // namespace dnet
