// Fused per-row token sampler: repetition / presence / frequency penalties,
// temperature, top-k / top-p / min-p and the inverse-CDF draw in one launch,
// without sorting the vocabulary.
//
// One 1024-thread workgroup per row. The row (bf16 or f32 logits, and the
// int32 `seen` table when a penalty is on) is re-read from L2 in up to six
// passes with 16-byte loads; nothing is staged. Wave w owns a contiguous
// range of 16-byte slots, so wave totals are in vocabulary order.
//
//   1. max / argmax (lowest index on ties), first NaN index
//      -> greedy rows, +inf rows and rows with no finite value end here
//   2. e_i = exp((l_i - l_max) / temp), total mass T, and level 0 of the
//      radix select (11 bits of the order-preserving key of the penalised
//      logit l_i itself: temp > 0, so l orders tokens exactly as x = l / temp
//      does and equal keys are exactly the contract's tie classes)
//   3./4. radix levels 1 and 2 (11 + 10 bits): top-k descends a count
//      histogram, top-p a mass histogram, each under its own prefix
//   5. kept mass per wave -> S, the target u*S and the wave that holds it
//      (rows without a filter reuse the wave totals of pass 2)
//   6. that wave alone scans its range for the token
//
// A row is one CU's work, so the passes are bound by instruction issue, not
// by L2: only pass 2 evaluates the exponential for every token (one
// v_exp_f32 on (l - l_max) * (log2(e) / temp)); the select passes compare
// keys and weigh only tokens under the current prefix.
//
// A row whose logit-bias flag is on adds its row of the dense f32 bias table
// to the raw logit (one f32 add) before the penalties, in every pass; a row
// whose flag is off never reads the table. The kernel is compiled twice: a
// call without a table launches the instance that has no bias code at all.
//
// Every mass is carried as an unsigned 64-bit fixed-point number with step
// 2^-40 (e_i <= 1, so a row of 2^18 tokens sums below 2^58). Integer sums
// are exact in any order: LDS histogram atomics, block reductions and the
// draw are bit-reproducible, and the top-p decision `mass_above < p*T` is
// made on the same integers the draw uses.
#include "sample_common.h"

namespace dnet {
namespace {

template <typename T, bool kBias>
__global__ __launch_bounds__(kThreads) void sample_rows_kernel(
    const T* __restrict__ logits, const int64_t stride, const int V,
    const float* __restrict__ temp, const int64_t* __restrict__ top_k,
    const float* __restrict__ top_p, const float* __restrict__ min_p,
    const float* __restrict__ rep, const float* __restrict__ pres,
    const float* __restrict__ freq, int* __restrict__ seen,
    const int64_t seen_stride, const float* __restrict__ bias,
    const int64_t bias_stride, const unsigned char* __restrict__ bias_on,
    const float* __restrict__ u, int64_t* __restrict__ out) {
  constexpr int N = VecOf<T>::n;
  __shared__ u64 s_mass[kBins];
  __shared__ unsigned s_cnt[kBins];
  __shared__ u64 s_red[kWaves];
  __shared__ u64 s_wtot[kWaves];
  __shared__ float s_bv[kWaves];
  __shared__ int s_bi[kWaves];
  __shared__ int s_nan[kWaves];
  __shared__ int s_sel[2];
  __shared__ u64 s_above[2];

  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wid = tid / kWave;

  int* const seen_row = seen ? seen + (int64_t)b * seen_stride : nullptr;
  Row r;
  r.l = logits + (int64_t)b * stride;
  r.V = V;
  r.off = (int)(((uintptr_t)r.l & 15) / sizeof(T));
  r.rep = rep ? rep[b] : 1.f;
  r.pres = pres ? pres[b] : 0.f;
  r.freq = freq ? freq[b] : 0.f;
  const bool pen = seen_row && (r.rep != 1.f || r.pres != 0.f || r.freq != 0.f);
  r.seen = pen ? seen_row : nullptr;
  r.seen_vec = (((uintptr_t)seen_row - 4 * (uintptr_t)r.off) & 15) == 0;
  // a row whose flag is off never touches the bias table
  r.bias = (kBias && bias && (!bias_on || bias_on[b]))
               ? bias + (int64_t)b * bias_stride
               : nullptr;
  r.bias_vec = (((uintptr_t)r.bias - 4 * (uintptr_t)r.off) & 15) == 0;

  int s0, s1;
  wave_range<T>(r, wid, s0, s1);

  // thread 0 publishes the token and counts it
  auto finish = [&](const int tok) {
    out[b] = tok;
    // every row of a batch that carries a table is counted, neutral rows
    // too: their row is zeroed when a request is set on it
    if (seen_row) {
      const int w = seen_row[tok];
      if ((w & kCountMask) != kCountMask) seen_row[tok] = w + 1;
    }
  };

  // ---- pass 1: max, argmax, first NaN ---------------------------------
  float bv = -INFINITY;
  int bi = INT_MAX, nan_i = INT_MAX;
  sweep<T, kBias>(r, s0, s1, lane, [&](const int idx, const float x) {
    if (x > bv) { bv = x; bi = idx; }  // indices rise: ties keep the lowest
    if (x != x && idx >= 0 && idx < V) nan_i = min(nan_i, idx);
  });
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_down(bv, off, 64);
    const int oi = __shfl_down(bi, off, 64);
    const int on = __shfl_down(nan_i, off, 64);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    nan_i = min(nan_i, on);
  }
  if (lane == 0) { s_bv[wid] = bv; s_bi[wid] = bi; s_nan[wid] = nan_i; }
  __syncthreads();
  bv = s_bv[0]; bi = s_bi[0]; nan_i = s_nan[0];
#pragma unroll
  for (int i = 1; i < kWaves; ++i) {
    const float ov = s_bv[i];
    const int oi = s_bi[i];
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    nan_i = min(nan_i, s_nan[i]);
  }
  const float lmax = bv;
  const float t = temp[b];
  if (bi == INT_MAX) {  // nothing above -inf: argmax(nan_to_num(l, 0))
    if (tid == 0) finish(nan_i != INT_MAX ? nan_i : 0);
    return;
  }
  if (!(t > 0.f) || lmax == INFINITY) {
    if (tid == 0) finish(bi);
    return;
  }

  const int64_t k_raw = top_k[b];
  const float p = top_p[b];
  const float mp = fminf(min_p[b], 1.f);
  bool on_k = k_raw > 0 && k_raw < (int64_t)V;
  bool on_p = p < 1.f;
  const bool on_mp = mp > 0.f;

  // ---- pass 2: total mass, radix level 0 ------------------------------
  if (on_k || on_p) {
    for (int i = tid; i < kBins; i += kThreads) { s_cnt[i] = 0; s_mass[i] = 0; }
    __syncthreads();
  }
  // finite also for a denormal temp, so that 0 * c stays 0 at the max
  const double cd = fmin(1.4426950408889634 / (double)t, 3e38);
  Scale c;
  c.hi = (float)cd;
  c.lo = (float)(cd - (double)c.hi);
  u64 tsum = 0;
  sweep<T, kBias>(r, s0, s1, lane, [&](const int, const float x) {
    if (x != x) return;
    const u64 q = to_fx(weight(dist(x, lmax), c));
    tsum += q;
    const unsigned d = fkey(x) >> 21;
    if (on_k) atomicAdd(&s_cnt[d], 1u);
    if (on_p) atomicAdd(&s_mass[d], q);
  });
  tsum = wave_sum_u64(tsum);
  if (lane == 0) s_wtot[wid] = tsum;
  __syncthreads();  // histograms complete
  u64 T_fx = 0;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) T_fx += s_wtot[i];

  // ---- radix select: thresholds as keys --------------------------------
  // top-k keeps key >= pre_k, where fewer than k keys lie above pre_k;
  // top-p keeps key >= pre_p, where the mass above pre_p is < p*T.
  unsigned pre_k = 0, pre_p = 0;
  if (on_k || on_p) {
    const u64 kk = (u64)k_raw;
    u64 pT = p > 0.f ? (u64)ceil((double)p * (double)T_fx) : 0;
    if (pT < 1) pT = 1;  // the max token is always kept
    u64 above_k = 0, above_p = 0;
#pragma unroll 1
    for (int level = 0; level < 3; ++level) {
      const int shift = level == 0 ? 21 : (level == 1 ? 10 : 0);
      const int bits = level == 2 ? 10 : 11;
      const int nb = 1 << bits;
      if (level > 0) {
        for (int i = tid; i < kBins; i += kThreads) { s_cnt[i] = 0; s_mass[i] = 0; }
        __syncthreads();
        const int up = shift + bits;  // bits already fixed sit above `up`
        sweep<T, kBias>(r, s0, s1, lane, [&](const int, const float x) {
          if (x != x) return;
          const unsigned key = fkey(x);
          const unsigned d = (key >> shift) & (nb - 1);
          if (on_k && (key >> up) == pre_k) atomicAdd(&s_cnt[d], 1u);
          if (on_p && (key >> up) == pre_p)
            atomicAdd(&s_mass[d], to_fx(weight(dist(x, lmax), c)));
        });
      }
      if (tid == 0) { s_sel[0] = -1; s_sel[1] = -1; }
      __syncthreads();
      // thread t scans bins from the top: nb-1-2t and nb-2-2t
      const int b0 = nb - 1 - 2 * tid, b1 = b0 - 1;
      const u64 c0 = b0 >= 0 ? s_cnt[b0] : 0, c1 = b1 >= 0 ? s_cnt[b1] : 0;
      const u64 m0 = b0 >= 0 ? s_mass[b0] : 0, m1 = b1 >= 0 ? s_mass[b1] : 0;
      const u64 ek = above_k + block_excl_scan_u64(c0 + c1, s_red);
      const u64 ep = above_p + block_excl_scan_u64(m0 + m1, s_red);
      if (on_k && b0 >= 0) {
        if (ek < kk && ek + c0 >= kk) { s_sel[0] = b0; s_above[0] = ek; }
        else if (ek + c0 < kk && ek + c0 + c1 >= kk) {
          s_sel[0] = b1; s_above[0] = ek + c0;
        }
      }
      if (on_p && b0 >= 0) {
        if (ep < pT && ep + m0 >= pT) { s_sel[1] = b0; s_above[1] = ep; }
        else if (ep + m0 < pT && ep + m0 + m1 >= pT) {
          s_sel[1] = b1; s_above[1] = ep + m0;
        }
      }
      __syncthreads();
      if (on_k) {
        if (s_sel[0] < 0) on_k = false;  // k exceeds the non-NaN count
        else { pre_k = (pre_k << bits) | (unsigned)s_sel[0]; above_k = s_above[0]; }
      }
      if (on_p) {
        if (s_sel[1] < 0) on_p = false;
        else { pre_p = (pre_p << bits) | (unsigned)s_sel[1]; above_p = s_above[1]; }
      }
      __syncthreads();
    }
  }
  const unsigned key_thr = max(on_k ? pre_k : 0u, on_p ? pre_p : 0u);
  auto kept_fx = [&](const float x) -> u64 {
    if (x != x) return 0;
    if (fkey(x) < key_thr) return 0;
    const float e = weight(dist(x, lmax), c);
    return (on_mp && e < mp) ? 0 : to_fx(e);
  };

  // ---- pass 5: kept mass per wave, locate the wave ---------------------
  if (key_thr != 0u || on_mp) {  // else every token is kept: pass 2's totals
    u64 ksum = 0;
    sweep<T, kBias>(r, s0, s1, lane,
             [&](const int, const float x) { ksum += kept_fx(x); });
    ksum = wave_sum_u64(ksum);
    __syncthreads();  // pass 2's totals have been read
    if (lane == 0) s_wtot[wid] = ksum;
    __syncthreads();
  }
  u64 S = 0;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) S += s_wtot[i];
  u64 target = (u64)((double)fmaxf(u[b], 0.f) * (double)S);
  if (target >= S) target = S - 1;  // S >= 2^40: the max token is kept
  int wsel = 0;
  u64 base = 0;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) {
    const u64 w = s_wtot[i];
    if (i == wsel && base + w <= target) { base += w; wsel = i + 1; }
  }
  if (wid != wsel) return;

  // ---- pass 6: the chosen wave scans its range -------------------------
  for (int it = s0; it < s1; it += kWave) {
    const int s = it + lane;
    u64 q[N];
    u64 sum = 0;
    if (s < s1) {
      float v[N];
      load_slot<T, kBias>(r, s, v);
#pragma unroll
      for (int j = 0; j < N; ++j) { q[j] = kept_fx(v[j]); sum += q[j]; }
    } else {
#pragma unroll
      for (int j = 0; j < N; ++j) q[j] = 0;
    }
    const u64 incl = wave_incl_scan_u64(sum, lane);
    const u64 total = __shfl(incl, kWave - 1, 64);
    if (base + total > target) {
      const u64 hit = __ballot(base + incl > target);
      if (lane == __ffsll((long long)hit) - 1) {
        u64 run = base + incl - sum;
        int tok = -1;
#pragma unroll
        for (int j = 0; j < N; ++j) {
          run += q[j];
          if (tok < 0 && run > target) tok = s * N - r.off + j;
        }
        finish(tok);
      }
      return;
    }
    base += total;
  }
  if (lane == 0) finish(bi);  // unreachable: S > target
}

}  // namespace

void sample_rows(torch::Tensor logits, torch::Tensor temp, torch::Tensor top_k,
                 torch::Tensor top_p, torch::Tensor min_p,
                 c10::optional<torch::Tensor> rep,
                 c10::optional<torch::Tensor> pres,
                 c10::optional<torch::Tensor> freq,
                 c10::optional<torch::Tensor> seen, torch::Tensor u,
                 torch::Tensor out_tok, c10::optional<torch::Tensor> bias,
                 c10::optional<torch::Tensor> bias_on) {
  DNET_CHECK(logits.is_cuda() && logits.dim() == 2, "logits: [B, V] on GPU");
  const int64_t B = logits.size(0), V = logits.size(1);
  DNET_CHECK(B >= 1 && V >= 1 && V < (1 << 30), "B >= 1, 1 <= V < 2^30");
  DNET_CHECK(logits.stride(1) == 1 && logits.stride(0) >= V,
             "logits rows must be dense");
  auto f32vec = [&](const torch::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.dtype() == torch::kFloat32 &&
                    t.is_contiguous() && t.numel() >= B,
                name, ": contiguous f32 with >= B elements on GPU");
    return (const float*)t.data_ptr();
  };
  const float* tp = f32vec(temp, "temp");
  const float* pp = f32vec(top_p, "top_p");
  const float* mp = f32vec(min_p, "min_p");
  const float* up = f32vec(u, "u");
  const float* rp = rep.has_value() ? f32vec(*rep, "rep") : nullptr;
  const float* prp = pres.has_value() ? f32vec(*pres, "pres") : nullptr;
  const float* fp = freq.has_value() ? f32vec(*freq, "freq") : nullptr;
  DNET_CHECK(top_k.is_cuda() && top_k.dtype() == torch::kInt64 &&
                 top_k.is_contiguous() && top_k.numel() >= B,
             "top_k: contiguous int64 with >= B elements on GPU");
  DNET_CHECK(out_tok.is_cuda() && out_tok.dtype() == torch::kInt64 &&
                 out_tok.is_contiguous() && out_tok.numel() >= B,
             "out_tok: contiguous int64 with >= B elements on GPU");
  int* sp = nullptr;
  int64_t sstride = 0;
  if (seen.has_value()) {
    DNET_CHECK(seen->is_cuda() && seen->dtype() == torch::kInt32 &&
                   seen->dim() == 2 && seen->size(0) >= B &&
                   seen->size(1) == V && seen->stride(1) == 1 &&
                   seen->stride(0) >= V,
               "seen: int32 [>= B, V] with dense rows on GPU");
    sp = (int*)seen->data_ptr();
    sstride = seen->stride(0);
  }
  const float* bp = nullptr;
  const unsigned char* bop = nullptr;
  int64_t bstride = 0;
  if (bias.has_value()) {
    DNET_CHECK(bias->is_cuda() && bias->dtype() == torch::kFloat32 &&
                   bias->dim() == 2 && bias->size(0) >= B &&
                   bias->size(1) == V && bias->stride(1) == 1 &&
                   bias->stride(0) >= V,
               "bias: f32 [>= B, V] with dense rows on GPU");
    bp = (const float*)bias->data_ptr();
    bstride = bias->stride(0);
    if (bias_on.has_value()) {
      DNET_CHECK(bias_on->is_cuda() &&
                     (bias_on->dtype() == torch::kBool ||
                      bias_on->dtype() == torch::kUInt8) &&
                     bias_on->is_contiguous() && bias_on->numel() >= B,
                 "bias_on: contiguous bool with >= B elements on GPU");
      bop = (const unsigned char*)bias_on->data_ptr();
    }
  }
  auto stream = current_stream();
  // a call without a table launches the kernel compiled without the bias
  auto launch = [&](auto kernel, auto* lp) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(kThreads), 0, stream,
                       lp, logits.stride(0), (int)V, tp,
                       (const int64_t*)top_k.data_ptr(), pp, mp, rp, prp, fp,
                       sp, sstride, bp, bstride, bop, up,
                       (int64_t*)out_tok.data_ptr());
  };
  if (logits.dtype() == torch::kBFloat16) {
    const short* lp = (const short*)logits.data_ptr();
    if (bp) launch(sample_rows_kernel<short, true>, lp);
    else launch(sample_rows_kernel<short, false>, lp);
  } else {
    DNET_CHECK(logits.dtype() == torch::kFloat32, "logits: bf16 or f32");
    const float* lp = (const float*)logits.data_ptr();
    if (bp) launch(sample_rows_kernel<float, true>, lp);
    else launch(sample_rows_kernel<float, false>, lp);
  }
  DNET_CHECK_HIP(hipGetLastError());
}

}  // namespace dnet
