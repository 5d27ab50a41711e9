// Chosen-token and ordered top-K logprobs of raw logits, one launch, no sort.
//
// One 1024-thread workgroup per row, built from the sampler's parts
// (sample_common.h): 16-byte sweeps of the bf16 / f32 row out of L2, the
// order-preserving key with an 11/11/10-bit radix select, and 2^-40
// fixed-point sums. A row with n_top < 0 ends at once and writes nothing.
//
//   1. m = max over the non-NaN logits
//   2. T = sum exp(l_i - m) in fixed point, and level 0 of the select
//   3./4. radix levels 1 and 2 -> the exact key of the n_top-th largest
//      logit and how many keys lie strictly above it (rows with n_top = 0
//      stop after pass 2)
//   5. gather the tokens above that key (fewer than n_top, any order) and
//      count the tokens equal to it per wave
//   6. the first waves, in vocabulary order, take the lowest-indexed tied
//      tokens until n_top entries are gathered
//   7. <= 20 entries are ranked by (key descending, index ascending) and
//      written with logp = (l - m) - ln T
//
// The order is decided on the keys of the input values alone, so it is
// fully determined, ties included; T is an integer sum, exact in any order,
// so every value is bit-reproducible.
#include "sample_common.h"

namespace dnet {
namespace {

constexpr int kMaxTop = 20;
constexpr int kList = 32;  // gathered entries, >= kMaxTop

template <typename T>
__global__ __launch_bounds__(kThreads) void logprobs_rows_kernel(
    const T* __restrict__ logits, const int64_t stride, const int V,
    const int64_t* __restrict__ tok, const int* __restrict__ n_top,
    float* __restrict__ logp, float* __restrict__ topv,
    int64_t* __restrict__ topi, const int K) {
  constexpr int N = VecOf<T>::n;
  __shared__ unsigned s_cnt[kBins];
  __shared__ u64 s_red[kWaves];
  __shared__ u64 s_wtot[kWaves];
  __shared__ float s_bv[kWaves];
  __shared__ unsigned s_wties[kWaves];
  __shared__ int s_sel;
  __shared__ u64 s_above;
  __shared__ unsigned s_n;
  __shared__ unsigned s_key[kList];
  __shared__ int s_idx[kList];
  __shared__ float s_val[kList];

  const int b = blockIdx.x;
  const int nt = n_top[b];
  if (nt < 0) return;  // skipped row: outputs untouched
  const int k = min(min(nt, K), kMaxTop);

  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wid = tid / kWave;

  Row r;
  r.l = logits + (int64_t)b * stride;
  r.V = V;
  r.off = (int)(((uintptr_t)r.l & 15) / sizeof(T));
  r.seen = nullptr;
  r.bias = nullptr;
  r.seen_vec = r.bias_vec = false;
  r.rep = 1.f;
  r.pres = r.freq = 0.f;
  int s0, s1;
  wave_range<T>(r, wid, s0, s1);

  // ---- pass 1: max of the non-NaN logits --------------------------------
  float bv = -INFINITY;
  sweep<T>(r, s0, s1, lane, [&](const int, const float x) {
    if (x > bv) bv = x;
  });
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    bv = fmaxf(bv, __shfl_down(bv, off, 64));
  if (lane == 0) s_bv[wid] = bv;
  if (tid == 0) s_n = 0;
  __syncthreads();
  bv = s_bv[0];
#pragma unroll
  for (int i = 1; i < kWaves; ++i) bv = fmaxf(bv, s_bv[i]);
  const float m = bv;
  // m = +inf, or nothing above -inf: every value is NaN, the order stands
  const bool degenerate = !(m > -INFINITY) || m == INFINITY;

  // ---- pass 2: T, radix level 0 ------------------------------------------
  if (k > 0) {
    for (int i = tid; i < kBins; i += kThreads) s_cnt[i] = 0;
    __syncthreads();
  }
  Scale c;  // log2(e) as an f32 pair
  c.hi = (float)1.4426950408889634;
  c.lo = (float)(1.4426950408889634 - (double)c.hi);
  u64 tsum = 0;
  if (!degenerate || k > 0) {
    sweep<T>(r, s0, s1, lane, [&](const int, const float x) {
      if (x != x) return;
      if (!degenerate) tsum += to_fx(weight(dist(x, m), c));
      if (k > 0) atomicAdd(&s_cnt[fkey(x) >> 21], 1u);
    });
  }
  tsum = wave_sum_u64(tsum);
  if (lane == 0) s_wtot[wid] = tsum;
  __syncthreads();  // histogram complete
  u64 T_fx = 0;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) T_fx += s_wtot[i];

  // ---- radix select: the key of the k-th largest logit -------------------
  // fewer than k keys lie above pre_k; on_k drops when k exceeds the
  // non-NaN count, and every non-NaN token is listed
  bool on_k = k > 0;
  unsigned pre_k = 0;
  u64 above_k = 0;
  if (k > 0) {
    const u64 kk = (u64)k;
#pragma unroll 1
    for (int level = 0; level < 3; ++level) {
      const int shift = level == 0 ? 21 : (level == 1 ? 10 : 0);
      const int bits = level == 2 ? 10 : 11;
      const int nb = 1 << bits;
      if (level > 0) {
        for (int i = tid; i < kBins; i += kThreads) s_cnt[i] = 0;
        __syncthreads();
        const int up = shift + bits;  // bits already fixed sit above `up`
        sweep<T>(r, s0, s1, lane, [&](const int, const float x) {
          if (x != x) return;
          const unsigned key = fkey(x);
          if ((key >> up) == pre_k)
            atomicAdd(&s_cnt[(key >> shift) & (nb - 1)], 1u);
        });
      }
      if (tid == 0) s_sel = -1;
      __syncthreads();
      // thread t scans bins from the top: nb-1-2t and nb-2-2t
      const int b0 = nb - 1 - 2 * tid, b1 = b0 - 1;
      const u64 c0 = b0 >= 0 ? s_cnt[b0] : 0, c1 = b1 >= 0 ? s_cnt[b1] : 0;
      const u64 ek = above_k + block_excl_scan_u64(c0 + c1, s_red);
      if (b0 >= 0) {
        if (ek < kk && ek + c0 >= kk) { s_sel = b0; s_above = ek; }
        else if (ek + c0 < kk && ek + c0 + c1 >= kk) {
          s_sel = b1; s_above = ek + c0;
        }
      }
      __syncthreads();
      if (s_sel < 0) on_k = false;
      else { pre_k = (pre_k << bits) | (unsigned)s_sel; above_k = s_above; }
      __syncthreads();
      if (!on_k) break;  // uniform: s_sel is shared
    }
  }

  // ---- pass 5: gather above the key, count ties per wave -----------------
  // every non-NaN key is > 0, so thr = 0 lists all of them
  const unsigned thr = on_k ? pre_k : 0u;
  const unsigned need = on_k ? (unsigned)(k - (int)above_k) : 0u;
  if (k > 0) {
    unsigned ties = 0;
    sweep<T>(r, s0, s1, lane, [&](const int idx, const float x) {
      if (x != x) return;
      const unsigned key = fkey(x);
      if (key > thr) {
        const unsigned pos = atomicAdd(&s_n, 1u);
        if (pos < (unsigned)kList) {
          s_key[pos] = key; s_idx[pos] = idx; s_val[pos] = x;
        }
      } else if (key == thr) {
        ++ties;
      }
    });
    ties = (unsigned)wave_sum_u64(ties);
    if (lane == 0) s_wties[wid] = ties;
    __syncthreads();
  }
  const unsigned n_above = k > 0 ? min(s_n, (unsigned)kMaxTop) : 0u;

  // ---- pass 6: the lowest-indexed ties, in vocabulary order --------------
  if (need > 0) {
    unsigned base = 0;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) base += (i < wid) ? s_wties[i] : 0u;
    for (int it = s0; it < s1 && base < need; it += kWave) {
      const int s = it + lane;
      float v[N];
      unsigned cnt = 0;
      if (s < s1) {
        load_slot<T>(r, s, v);
#pragma unroll
        for (int j = 0; j < N; ++j) cnt += (v[j] == v[j] && fkey(v[j]) == thr);
      }
      const u64 incl = wave_incl_scan_u64(cnt, lane);
      const unsigned total = (unsigned)__shfl(incl, kWave - 1, 64);
      unsigned rank = base + (unsigned)incl - cnt;
      if (cnt > 0 && rank < need) {
#pragma unroll
        for (int j = 0; j < N; ++j) {
          if (v[j] == v[j] && fkey(v[j]) == thr) {
            const unsigned pos = n_above + rank;
            if (rank < need && pos < (unsigned)kList) {
              s_key[pos] = thr; s_idx[pos] = s * N - r.off + j;
              s_val[pos] = v[j];
            }
            ++rank;
          }
        }
      }
      base += total;
    }
  }
  __syncthreads();

  // ---- pass 7: rank the list, write ---------------------------------------
  const int n = (int)min(n_above + need, (unsigned)kMaxTop);
  // only the threads that write a value take the double-precision log
  auto lp = [&](const float x) -> float {
    if (degenerate || x != x) return NAN;
    return (float)((double)dist(x, m) - log((double)T_fx * 0x1p-40));
  };
  if (tid < K) {
    if (tid < n) {
      const unsigned key = s_key[tid];
      const int idx = s_idx[tid];
      int rank = 0;
      for (int j = 0; j < n; ++j)
        rank += (s_key[j] > key || (s_key[j] == key && s_idx[j] < idx));
      topi[(int64_t)b * K + rank] = idx;
      topv[(int64_t)b * K + rank] = lp(s_val[tid]);
    } else {
      topi[(int64_t)b * K + tid] = -1;
      topv[(int64_t)b * K + tid] = NAN;
    }
  }
  if (tid == kWave) {  // the chosen token, on a wave of its own
    const int64_t j = tok[b];
    float x = NAN;
    if (j >= 0 && j < (int64_t)V) {
      if constexpr (N == 8)
        x = bits2f(reinterpret_cast<const short*>(r.l)[j]);
      else
        x = reinterpret_cast<const float*>(r.l)[j];
    }
    logp[b] = lp(x);
  }
}

}  // namespace

void logprobs_rows(torch::Tensor logits, torch::Tensor tok,
                   torch::Tensor n_top, torch::Tensor logp, torch::Tensor topv,
                   torch::Tensor topi) {
  DNET_CHECK(logits.is_cuda() && logits.dim() == 2, "logits: [B, V] on GPU");
  const int64_t B = logits.size(0), V = logits.size(1);
  DNET_CHECK(B >= 1 && V >= 1 && V < (1 << 30), "B >= 1, 1 <= V < 2^30");
  DNET_CHECK(logits.stride(1) == 1 && logits.stride(0) >= V,
             "logits rows must be dense");
  DNET_CHECK(tok.is_cuda() && tok.dtype() == torch::kInt64 &&
                 tok.is_contiguous() && tok.numel() >= B,
             "tok: contiguous int64 with >= B elements on GPU");
  DNET_CHECK(n_top.is_cuda() && n_top.dtype() == torch::kInt32 &&
                 n_top.is_contiguous() && n_top.numel() >= B,
             "n_top: contiguous int32 with >= B elements on GPU");
  DNET_CHECK(logp.is_cuda() && logp.dtype() == torch::kFloat32 &&
                 logp.is_contiguous() && logp.numel() >= B,
             "logp: contiguous f32 with >= B elements on GPU");
  DNET_CHECK(topv.is_cuda() && topv.dtype() == torch::kFloat32 &&
                 topv.dim() == 2 && topv.is_contiguous() && topv.size(0) >= B,
             "topv: contiguous f32 [>= B, K] on GPU");
  const int64_t K = topv.size(1);
  DNET_CHECK(K >= 0 && K <= kMaxTop, "0 <= K <= 20");
  DNET_CHECK(topi.is_cuda() && topi.dtype() == torch::kInt64 &&
                 topi.dim() == 2 && topi.is_contiguous() &&
                 topi.size(0) >= B && topi.size(1) == K,
             "topi: contiguous int64 [>= B, K] on GPU");
  auto stream = current_stream();
  if (logits.dtype() == torch::kBFloat16) {
    hipLaunchKernelGGL(logprobs_rows_kernel<short>, dim3((unsigned)B),
                       dim3(kThreads), 0, stream,
                       (const short*)logits.data_ptr(), logits.stride(0),
                       (int)V, (const int64_t*)tok.data_ptr(),
                       (const int*)n_top.data_ptr(), (float*)logp.data_ptr(),
                       (float*)topv.data_ptr(), (int64_t*)topi.data_ptr(),
                       (int)K);
  } else {
    DNET_CHECK(logits.dtype() == torch::kFloat32, "logits: bf16 or f32");
    hipLaunchKernelGGL(logprobs_rows_kernel<float>, dim3((unsigned)B),
                       dim3(kThreads), 0, stream,
                       (const float*)logits.data_ptr(), logits.stride(0),
                       (int)V, (const int64_t*)tok.data_ptr(),
                       (const int*)n_top.data_ptr(), (float*)logp.data_ptr(),
                       (float*)topv.data_ptr(), (int64_t*)topi.data_ptr(),
                       (int)K);
  }
  DNET_CHECK_HIP(hipGetLastError());
}

}  // namespace dnet
