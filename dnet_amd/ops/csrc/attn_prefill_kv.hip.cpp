// MFMA flash prefill attention reading the KV cache in place (gfx950):
// bf16 or int8 group-64 cache, causal + sliding window + sinks.
//
// attn_prefill.hip.cpp needs K/V as freshly materialized contiguous bf16
// [B, Hkv, S, D]; for an int8 cache that meant dequantizing the whole
// slot to HBM per layer and chunk. This kernel takes the cache tensors as
// they are (every stride from the tensor, rows >= kv_len never enter the
// computation) and dequantizes int8 codes on the way into LDS.
//
// Geometry: block = 4 waves, each wave owns 16 q rows of a 64-row q tile
// (grid = ceil(T/64) x Hq x B). K/V are staged 64 positions at a time,
// anchored at absolute multiples of 64, and consumed as two 32-position
// online-softmax steps: attn_prefill's operation order, so the output
// bits equal attn_prefill's on the same K/V values, and a query row sees
// the same steps in the same order however the prompt was chunked (a
// step that is fully masked for a row is an exact no-op: -inf scores
// against the finite m init).
//
// Per s tile:
//   - staging: every thread owns NL 16-byte pieces of the K tile and of
//     the V tile (bf16: 8 elements; int8: 16 codes + their group scale,
//     staged as bf16(code * scale), the value the decode kernels stage).
//     The pieces of tile i+1 are loaded into registers right after tile
//     i went to LDS, i.e. before the MFMA/softmax work of tile i, so the
//     global latency hides behind it.
//   - K goes to k_lds [64][D+8]; V goes transposed to vt_lds [D][64+8].
//     The 8 lanes that hold different d-pieces of 8 rows would all hit
//     one bank on the transposed 2-byte writes; each lane therefore
//     rotates its 8 elements by its piece index (3 select stages) and
//     writes element (j + rot) & 7 at step j: 32 distinct banks.
//   - per 32-position step: QK^T 2 x (D/32) v_mfma_f32_16x16x32_bf16 ->
//     two [16q x 16s] C fragments; mask; fp32 online softmax (16-lane
//     shuffles); P (bf16) through a per-wave LDS slab -> A fragment;
//     PV: D/16 MFMAs.
// Epilogue: sink logit into the denominator, O / rowsum, stored token-
// major [B, T, Hq*D] (what the o-projection consumes).
#include "common.h"

namespace dnet {

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;

struct KvGeom {
  int64_t k_sb, k_sh, k_ss;      // k cache strides (elements)
  int64_t v_sb, v_sh, v_ss;
  int64_t ks_sb, ks_sh, ks_ss;   // k scale strides
  int64_t vs_sb, vs_sh, vs_ss;
};

// out[j] = in[(j + r) & 7] over 8 packed 16-bit elements (w[0] low half =
// element 0)
__device__ __forceinline__ void rot8(unsigned (&w)[4], const int r) {
  if (r & 4) {
    unsigned t = w[0]; w[0] = w[2]; w[2] = t;
    t = w[1]; w[1] = w[3]; w[3] = t;
  }
  if (r & 2) {
    const unsigned t = w[0];
    w[0] = w[1]; w[1] = w[2]; w[2] = w[3]; w[3] = t;
  }
  if (r & 1) {
    const unsigned t = w[0];
    w[0] = (w[0] >> 16) | (w[1] << 16);
    w[1] = (w[1] >> 16) | (w[2] << 16);
    w[2] = (w[2] >> 16) | (w[3] << 16);
    w[3] = (w[3] >> 16) | (t << 16);
  }
}

// 8 int8 codes (two dwords) * scale -> 8 bf16 packed in w[4]
__device__ __forceinline__ void deq8(const unsigned lo, const unsigned hi,
                                     const float s, unsigned (&w)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned src = j < 2 ? lo : hi;
    const int c0 = (int)(int8_t)(src >> (16 * (j & 1)));
    const int c1 = (int)(int8_t)(src >> (16 * (j & 1) + 8));
    w[j] = (unsigned)(unsigned short)f2bits((float)c0 * s) |
           ((unsigned)(unsigned short)f2bits((float)c1 * s) << 16);
  }
}

template <int D, bool Q8, bool WINDOW, bool SINKS>
__global__ __launch_bounds__(256) void attn_prefill_kv_kernel(
    const short* __restrict__ q,       // [B, Hq, T, D]
    const void* __restrict__ kc,       // [B, Hkv, Smax, D] bf16 / int8
    const void* __restrict__ vc,
    const short* __restrict__ kscale,  // [B, Hkv, Smax, D/64] or null
    const short* __restrict__ vscale,
    const short* __restrict__ sinks,   // [Hq] or null
    short* __restrict__ out,           // [B, T, Hq*D]
    const KvGeom g, const int Hq, const int Hkv, const int T,
    const int kv_len, const int q_off, const int window,
    const float scale) {
  constexpr int ST = 64;              // s positions per tile
  constexpr int DC = D / 32;          // QK k-chunks
  constexpr int NV = D / 16;          // PV n-tiles
  constexpr int KP = D + 8;           // k_lds row stride
  constexpr int SP = ST + 8;          // vt_lds / p_lds row stride
  constexpr int EPT = Q8 ? 16 : 8;    // elements per 16-byte piece
  constexpr int CPR = D / EPT;        // pieces per row
  constexpr int NL = ST * CPR / 256;  // pieces per thread per tile
  static_assert(ST * CPR % 256 == 0, "tile must split evenly over 256");
  __shared__ __attribute__((aligned(16))) short k_lds[ST * KP];
  __shared__ __attribute__((aligned(16))) short vt_lds[D * SP];
  __shared__ __attribute__((aligned(16))) short p_lds[4][16 * SP];

  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int h = blockIdx.y;
  const int b = blockIdx.z;
  const int hk = h / (Hq / Hkv);
  const int qt = blockIdx.x * 64 + wave * 16;   // this wave's first q row
  const int row = lane & 15;
  const int hi = lane >> 4;
  const int qrow = min(qt + row, T - 1);

  const short* qp = q + (((int64_t)b * Hq + h) * T + qrow) * D;
  bf16x8 qf[DC];
#pragma unroll
  for (int c = 0; c < DC; ++c)
    qf[c] = *reinterpret_cast<const bf16x8*>(&qp[c * 32 + hi * 8]);

  f32x4 acc[NV];
#pragma unroll
  for (int n = 0; n < NV; ++n) acc[n] = {0.f, 0.f, 0.f, 0.f};
  float m_run[4], l_run[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m_run[r] = -1e30f;
    l_run[r] = 0.f;
  }

  // block-uniform s range; tiles start at absolute multiples of ST
  const int q_hi = min((int)blockIdx.x * 64 + 63, T - 1);
  const int s_end = min(kv_len, q_off + q_hi + 1);
  int s_begin = 0;
  if (WINDOW)
    s_begin = max(0, q_off + (int)blockIdx.x * 64 - window + 1) & ~(ST - 1);

  // this thread's pieces: 8 consecutive lanes take 8 rows of one piece
  // column (see the bank note in the header)
  int p_sr[NL], p_c[NL];
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    const int idx = threadIdx.x + i * 256;
    p_c[i] = (idx >> 3) % CPR;
    p_sr[i] = (idx >> 3) / CPR * 8 + (idx & 7);
  }
  const char* kbase = (const char*)kc +
                      ((int64_t)b * g.k_sb + hk * g.k_sh) * (Q8 ? 1 : 2);
  const char* vbase = (const char*)vc +
                      ((int64_t)b * g.v_sb + hk * g.v_sh) * (Q8 ? 1 : 2);
  const short* ksb = Q8 ? kscale + (int64_t)b * g.ks_sb + hk * g.ks_sh
                        : nullptr;
  const short* vsb = Q8 ? vscale + (int64_t)b * g.vs_sb + hk * g.vs_sh
                        : nullptr;

  uint4 kreg[NL], vreg[NL];
  short kscl[NL], vscl[NL];
  auto load_tile = [&](const int s0) {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      // rows >= kv_len may hold NaN (or NaN scales): never load them. A
      // clamped row is a valid finite one and its P is exactly 0.
      const int64_t sg = min(s0 + p_sr[i], kv_len - 1);
      kreg[i] = *reinterpret_cast<const uint4*>(
          kbase + sg * g.k_ss * (Q8 ? 1 : 2) + p_c[i] * 16);
      vreg[i] = *reinterpret_cast<const uint4*>(
          vbase + sg * g.v_ss * (Q8 ? 1 : 2) + p_c[i] * 16);
      if (Q8) {
        kscl[i] = ksb[sg * g.ks_ss + p_c[i] / 4];
        vscl[i] = vsb[sg * g.vs_ss + p_c[i] / 4];
      }
    }
  };
  // one 8-element unit: K row-major, V transposed with the bank rotation
  auto put_k = [&](const int sr, const int d0, const unsigned (&w)[4]) {
    *reinterpret_cast<uint4*>(&k_lds[sr * KP + d0]) =
        make_uint4(w[0], w[1], w[2], w[3]);
  };
  auto put_vt = [&](const int sr, const int d0, unsigned (&w)[4],
                    const int rot) {
    rot8(w, rot);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int e = (j + rot) & 7;
      vt_lds[(d0 + e) * SP + sr] = (short)(w[j >> 1] >> (16 * (j & 1)));
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int sr = p_sr[i], c = p_c[i], rot = c & 7;
      if (Q8) {
        const float ks = bits2f(kscl[i]), vs = bits2f(vscl[i]);
        unsigned w[4];
        deq8(kreg[i].x, kreg[i].y, ks, w);
        put_k(sr, c * 16, w);
        deq8(kreg[i].z, kreg[i].w, ks, w);
        put_k(sr, c * 16 + 8, w);
        deq8(vreg[i].x, vreg[i].y, vs, w);
        put_vt(sr, c * 16, w, rot);
        deq8(vreg[i].z, vreg[i].w, vs, w);
        put_vt(sr, c * 16 + 8, w, rot);
      } else {
        unsigned w[4] = {kreg[i].x, kreg[i].y, kreg[i].z, kreg[i].w};
        put_k(sr, c * 8, w);
        unsigned u[4] = {vreg[i].x, vreg[i].y, vreg[i].z, vreg[i].w};
        put_vt(sr, c * 8, u, rot);
      }
    }
  };

  if (s_begin < s_end) load_tile(s_begin);
  for (int s0 = s_begin; s0 < s_end; s0 += ST) {
    __syncthreads();   // previous tile's consumers done
    store_tile();
    __syncthreads();
    // next tile's global loads fly during this tile's MFMA/softmax
    if (s0 + ST < s_end) load_tile(s0 + ST);

    // The staged 64 positions are consumed as two 32-position steps, each
    // a complete online-softmax update (own row max, own P rounding, one
    // PV MFMA per n-tile): the operation order of attn_prefill's 32-wide
    // tiles, so both kernels give the same bits on the same K/V values.
#pragma unroll
    for (int half = 0; half < ST / 32; ++half) {
      if (s0 + half * 32 >= s_end) break;   // block-uniform
      // ---- QK^T for two 16-s subtiles ----
      float p_val[2][4];
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        f32x4 sc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < DC; ++c) {
          const bf16x8 kf = *reinterpret_cast<const bf16x8*>(
              &k_lds[(half * 32 + sub * 16 + row) * KP + c * 32 + hi * 8]);
          sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[c], kf, sc, 0, 0,
                                                       0);
        }
        // C layout: lane holds scores[q = hi*4 + r][s = row] of the subtile
        const int spos = s0 + half * 32 + sub * 16 + row;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int qq = qt + hi * 4 + r;
          const float val = sc[r] * scale;
          const int qpos = q_off + qq;
          bool dead = (spos > qpos) || (spos >= kv_len) || (qq >= T);
          if (WINDOW) dead |= (spos <= qpos - window);
          // -inf, not a finite floor: against the finite m init a fully
          // masked step gives exp(-inf) = 0 and corr = 1, an exact no-op
          p_val[sub][r] = dead ? -INFINITY : val;
        }
      }
      // ---- online softmax: row hi*4+r lives in the 16 lanes of one hi ----
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float mx = fmaxf(p_val[0][r], p_val[1][r]);
#pragma unroll
        for (int off = 8; off > 0; off >>= 1)
          mx = fmaxf(mx, __shfl_xor(mx, off, 16));
        const float m_new = fmaxf(m_run[r], mx);
        const float corr = __expf(m_run[r] - m_new);
        float ls = 0.f;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
          p_val[sub][r] = __expf(p_val[sub][r] - m_new);
          ls += p_val[sub][r];
        }
#pragma unroll
        for (int off = 8; off > 0; off >>= 1)
          ls += __shfl_xor(ls, off, 16);
        l_run[r] = l_run[r] * corr + ls;
        m_run[r] = m_new;
#pragma unroll
        for (int n = 0; n < NV; ++n) acc[n][r] *= corr;
      }
      // ---- P -> per-wave LDS slab (bf16), then PV ----
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          p_lds[wave][(hi * 4 + r) * SP + half * 32 + sub * 16 + row] =
              f2bits(p_val[sub][r]);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // wave-local slab
      // A fragment: P[q = lane&15][hi*8 + j] over this step's 32 positions
      const bf16x8 pf = *reinterpret_cast<const bf16x8*>(
          &p_lds[wave][row * SP + half * 32 + hi * 8]);
#pragma unroll
      for (int n = 0; n < NV; ++n) {
        // B fragment: Vt[d = n*16 + lane&15][half*32 + hi*8 + j]
        const bf16x8 vf = *reinterpret_cast<const bf16x8*>(
            &vt_lds[(n * 16 + row) * SP + half * 32 + hi * 8]);
        acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, vf, acc[n], 0, 0,
                                                         0);
      }
    }
  }

  // ---- epilogue: sinks + normalize + token-major store ----
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (SINKS) {
      const float sk = bits2f(sinks[h]);
      const float m2 = fmaxf(m_run[r], sk);
      l_run[r] = l_run[r] * __expf(m_run[r] - m2) + __expf(sk - m2);
      const float corr = __expf(m_run[r] - m2);
#pragma unroll
      for (int n = 0; n < NV; ++n) acc[n][r] *= corr;
    }
    const int qq = qt + hi * 4 + r;
    if (qq >= T) continue;
    const float inv = 1.0f / fmaxf(l_run[r], 1e-30f);
    short* op = out + (((int64_t)b * T + qq) * Hq + h) * D;
#pragma unroll
    for (int n = 0; n < NV; ++n) op[n * 16 + row] = f2bits(acc[n][r] * inv);
  }
}

void attn_prefill_kv(torch::Tensor q, torch::Tensor kcache,
                     torch::Tensor vcache, c10::optional<torch::Tensor> sinks,
                     torch::Tensor out, int64_t kv_len, int64_t q_off,
                     int64_t window, double scale,
                     c10::optional<torch::Tensor> kscale,
                     c10::optional<torch::Tensor> vscale) {
  DNET_CHECK(q.dim() == 4 && kcache.dim() == 4 && vcache.dim() == 4,
             "q [B,Hq,T,D], cache [B,Hkv,Smax,D]");
  const int64_t B = q.size(0), Hq = q.size(1), T = q.size(2), D = q.size(3);
  const int64_t Hkv = kcache.size(1), Smax = kcache.size(2);
  const bool q8 = kcache.scalar_type() == torch::kInt8;
  DNET_CHECK(q.scalar_type() == torch::kBFloat16 &&
                 out.scalar_type() == torch::kBFloat16,
             "q/out bf16");
  DNET_CHECK(q8 || kcache.scalar_type() == torch::kBFloat16,
             "cache bf16 or int8");
  DNET_CHECK(vcache.scalar_type() == kcache.scalar_type(), "k/v cache dtype");
  DNET_CHECK(vcache.size(3) == D && kcache.size(3) == D &&
                 (q8 ? (D == 64 || D == 128)
                     : (D == 64 || D == 96 || D == 128)),
             "attn_prefill_kv: unsupported head dims");
  DNET_CHECK(Hkv > 0 && Hq % Hkv == 0, "GQA heads");
  DNET_CHECK(q.is_contiguous() && out.is_contiguous(), "q/out contiguous");
  DNET_CHECK(out.numel() == B * T * Hq * D, "out [B,T,Hq*D]");
  DNET_CHECK(T >= 1 && kv_len >= 1 && kv_len <= Smax && q_off >= 0,
             "1 <= kv_len <= Smax");
  // 16-byte pieces: bf16 8 elements, int8 16 codes
  const int64_t unit = q8 ? 16 : 8;
  auto cache_ok = [&](const torch::Tensor& t, int64_t last, int64_t u) {
    return t.dim() == 4 && t.size(0) == B && t.size(1) == Hkv &&
           t.size(2) == Smax && t.size(3) == last && t.stride(3) == 1 &&
           t.stride(0) % u == 0 && t.stride(1) % u == 0 &&
           t.stride(2) % u == 0;
  };
  DNET_CHECK(cache_ok(kcache, D, unit) && cache_ok(vcache, D, unit) &&
                 ((uintptr_t)kcache.data_ptr()) % 16 == 0 &&
                 ((uintptr_t)vcache.data_ptr()) % 16 == 0 &&
                 ((uintptr_t)q.data_ptr()) % 16 == 0,
             "cache [B,Hkv,Smax,D], last dim contiguous, 16-byte rows");
  KvGeom g{};
  g.k_sb = kcache.stride(0); g.k_sh = kcache.stride(1);
  g.k_ss = kcache.stride(2);
  g.v_sb = vcache.stride(0); g.v_sh = vcache.stride(1);
  g.v_ss = vcache.stride(2);
  const short *ksp = nullptr, *vsp = nullptr;
  if (q8) {
    DNET_CHECK(kscale.has_value() && vscale.has_value(),
               "int8 cache needs scales");
    DNET_CHECK(kscale->scalar_type() == torch::kBFloat16 &&
                   vscale->scalar_type() == torch::kBFloat16 &&
                   cache_ok(*kscale, D / 64, 1) && cache_ok(*vscale, D / 64, 1),
               "scales bf16 [B,Hkv,Smax,D/64]");
    g.ks_sb = kscale->stride(0); g.ks_sh = kscale->stride(1);
    g.ks_ss = kscale->stride(2);
    g.vs_sb = vscale->stride(0); g.vs_sh = vscale->stride(1);
    g.vs_ss = vscale->stride(2);
    ksp = (const short*)kscale->data_ptr();
    vsp = (const short*)vscale->data_ptr();
  }
  const short* sp = nullptr;
  if (sinks.has_value()) {
    DNET_CHECK(sinks->scalar_type() == torch::kBFloat16 &&
                   sinks->numel() == Hq && sinks->is_contiguous(),
               "sinks bf16 [Hq]");
    sp = (const short*)sinks->data_ptr();
  }
  auto stream = current_stream();
  const dim3 grid((unsigned)((T + 63) / 64), (unsigned)Hq, (unsigned)B);
  const bool win = window > 0;
#define LAUNCH_APK(DD, QQ, WW, SS)                                           \
  hipLaunchKernelGGL((attn_prefill_kv_kernel<DD, QQ, WW, SS>), grid,         \
                     dim3(256), 0, stream, (const short*)q.data_ptr(),       \
                     (const void*)kcache.data_ptr(),                         \
                     (const void*)vcache.data_ptr(), ksp, vsp, sp,           \
                     (short*)out.data_ptr(), g, (int)Hq, (int)Hkv, (int)T,   \
                     (int)kv_len, (int)q_off, (int)window, (float)scale)
#define LAUNCH_APK_WS(DD, QQ)                                  \
  do {                                                         \
    if (win && sp) LAUNCH_APK(DD, QQ, true, true);             \
    else if (win) LAUNCH_APK(DD, QQ, true, false);             \
    else if (sp) LAUNCH_APK(DD, QQ, false, true);              \
    else LAUNCH_APK(DD, QQ, false, false);                     \
  } while (0)
  if (D == 128 && q8) LAUNCH_APK_WS(128, true);
  else if (D == 128) LAUNCH_APK_WS(128, false);
  else if (D == 64 && q8) LAUNCH_APK_WS(64, true);
  else if (D == 64) LAUNCH_APK_WS(64, false);
  else LAUNCH_APK_WS(96, false);
#undef LAUNCH_APK
#undef LAUNCH_APK_WS
}

}  // namespace dnet
