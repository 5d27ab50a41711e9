// Fused prefill RoPE + KV-cache append over a block of T tokens.
//
// The decode kernel (rope_append.hip.cpp) is one block per (batch, head)
// with 2-byte accesses: right for B rows per step, far too many tiny blocks
// for the B*T*(Hq+Hkv) rows of a prefill chunk. This is the throughput
// form: a row of D elements is owned by a small lane group (8 lanes for
// D = 96/128, 4 for D = 64), each lane holding 8 contiguous elements of
// the first half and the 8 matching ones of the second half, so every
// global access is 16 bytes (8 for int8 codes) and a wave carries 8 or 16
// rows. No LDS: the group-64 amax of the int8 cache is a shuffle reduction
// inside the row's lane group.
//
//   q rows: rotated, written bf16 to q_rot [B, Hq, T, D] (the layout the
//           prefill attention kernel reads; no transpose copy afterwards)
//   k rows: rotated, written to cache row p0 + t (bf16, or int8 + scale)
//   v rows: written raw to cache row p0 + t
//
// The rotation rounds each product and the sum to f32 on its own, like
// ops.rope_apply (torch mul, mul, add): q and the bf16 cache rows carry
// the bits of the unfused prefill path.
//
// int8 contract = the decode kernel's: codes quantize the f32 rotation
// (not its bf16 rounding), scale = bf16(max(amax, 1e-8) / 127) per 64
// dims, code = rn(x / scale) clamped to +-127.
#include "common.h"

namespace dnet {

struct RowsGeom {
  int64_t q_sb, q_st, k_sb, k_st, v_sb, v_st;  // input strides (elements)
  int64_t kc_sb, kc_sh, kc_ss;                 // k cache strides
  int64_t vc_sb, vc_sh, vc_ss;                 // v cache strides
  int64_t ks_sb, ks_sh, ks_ss;                 // k scale strides
  int64_t vs_sb, vs_sh, vs_ss;                 // v scale strides
  int64_t rows;                                // B * T * (Hq + Hkv)
  int T, Hq, Hkv, p0;
};

__device__ __forceinline__ void load8(const short* p, float (&x)[8]) {
  const short8 r = *reinterpret_cast<const short8*>(p);
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = bits2f(r.x[j]);
}

__device__ __forceinline__ void load8f(const float* p, float (&x)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  const float4 b = *reinterpret_cast<const float4*>(p + 4);
  x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
  x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
}

__device__ __forceinline__ void store8(short* p, const float (&x)[8]) {
  short8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r.x[j] = f2bits(x[j]);
  *reinterpret_cast<short8*>(p) = r;
}

// 8 codes rn(x / s) clamped to +-127, one 8-byte store
__device__ __forceinline__ void store8q(int8_t* p, const float (&x)[8],
                                        const float s) {
  unsigned w[2] = {0u, 0u};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = min(max(__float2int_rn(x[j] / s), -127), 127);
    w[j >> 2] |= (unsigned)(c & 0xff) << (8 * (j & 3));
  }
  *reinterpret_cast<uint2*>(p) = make_uint2(w[0], w[1]);
}

__device__ __forceinline__ float amax8(const float (&x)[8]) {
  float m = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(x[j]));
  return m;
}

__device__ __forceinline__ float q8scale(const float amax) {
  return bits2f(f2bits(fmaxf(amax, 1e-8f) / 127.f));  // bf16-rounded
}

// grid.x = ceil(rows / (256 / LPR)); block 256.
template <int D, bool Q8>
__global__ __launch_bounds__(256) void rope_append_rows_kernel(
    const short* __restrict__ q, const short* __restrict__ k,
    const short* __restrict__ v, short* __restrict__ qout,
    void* __restrict__ kcache, void* __restrict__ vcache,
    short* __restrict__ kscale, short* __restrict__ vscale,
    const float* __restrict__ cost, const float* __restrict__ sint,
    const RowsGeom g) {
  constexpr int HALF = D / 2;
  constexpr int LPR = D == 64 ? 4 : 8;   // lanes per row (D = 96: 6 active)
  constexpr int NG = D / 64;             // int8 scale groups per row
  const int li = threadIdx.x % LPR;
  const int64_t r = (int64_t)blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
  const int e0 = li * 8;
  // a row's lanes are live or idle together (uniform over the lane group),
  // so the group shuffles below never mix the two
  if (r >= g.rows || e0 >= HALF) return;
  const int nh = g.Hq + g.Hkv;
  const int head = (int)(r % nh);
  const int64_t bt = r / nh;
  const int t = (int)(bt % g.T);
  const int64_t b = bt / g.T;
  const int p = g.p0 + t;

  float c[8], s[8], x1[8], x2[8], r1[8], r2[8];
  load8f(cost + (int64_t)p * HALF + e0, c);
  load8f(sint + (int64_t)p * HALF + e0, s);
  const bool isq = head < g.Hq;
  const int hk = head - g.Hq;
  const short* src = isq ? q + b * g.q_sb + t * g.q_st + (int64_t)head * D
                         : k + b * g.k_sb + t * g.k_st + (int64_t)hk * D;
  load8(src + e0, x1);
  load8(src + HALF + e0, x2);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    // each product and the sum rounded to f32 on its own (no fma
    // contraction): the bits of ops.rope_apply's mul, mul, add
#pragma clang fp contract(off)
    r1[j] = x1[j] * c[j] - x2[j] * s[j];
    r2[j] = x2[j] * c[j] + x1[j] * s[j];
  }
  if (isq) {
    short* dst = qout + ((b * g.Hq + head) * g.T + t) * D;
    store8(dst + e0, r1);
    store8(dst + HALF + e0, r2);
    return;
  }
  const short* vsrc = v + b * g.v_sb + t * g.v_st + (int64_t)hk * D;
  const int64_t koff = b * g.kc_sb + hk * g.kc_sh + p * g.kc_ss;
  const int64_t voff = b * g.vc_sb + hk * g.vc_sh + p * g.vc_ss;
  if (!Q8) {
    short* kd = (short*)kcache + koff;
    store8(kd + e0, r1);
    store8(kd + HALF + e0, r2);
    short* vd = (short*)vcache + voff;
    *reinterpret_cast<short8*>(vd + e0) =
        *reinterpret_cast<const short8*>(vsrc + e0);
    *reinterpret_cast<short8*>(vd + HALF + e0) =
        *reinterpret_cast<const short8*>(vsrc + HALF + e0);
    return;
  }
  // int8 group-64: D = 128 -> first half is group 0, second half group 1;
  // D = 64 -> both halves are the one group
  auto group_max = [](float m) {
#pragma unroll
    for (int off = LPR / 2; off > 0; off >>= 1)
      m = fmaxf(m, __shfl_xor(m, off, LPR));
    return m;
  };
  float v1[8], v2[8];
  load8(vsrc + e0, v1);
  load8(vsrc + HALF + e0, v2);
  auto put = [&](int8_t* dst, short* sc, const float (&a)[8],
                 const float (&bb)[8]) {
    float m0 = amax8(a), m1 = amax8(bb);
    if (NG == 1) m0 = m1 = fmaxf(m0, m1);
    const float s0 = q8scale(group_max(m0));
    const float s1 = NG == 1 ? s0 : q8scale(group_max(m1));
    store8q(dst + e0, a, s0);
    store8q(dst + HALF + e0, bb, s1);
    if (li == 0) {
      sc[0] = f2bits(s0);
      if (NG == 2) sc[1] = f2bits(s1);
    }
  };
  put((int8_t*)kcache + koff,
      kscale + b * g.ks_sb + hk * g.ks_sh + p * g.ks_ss, r1, r2);
  put((int8_t*)vcache + voff,
      vscale + b * g.vs_sb + hk * g.vs_sh + p * g.vs_ss, v1, v2);
}

static bool aligned16(const torch::Tensor& t) {
  return ((uintptr_t)t.data_ptr()) % 16 == 0;
}

// q [B,T,Hq,D], k/v [B,T,Hkv,D] bf16 (head stride D, last dim contiguous,
// token/batch strides free); caches [B,Hkv,Smax,D] bf16 or int8 with
// scales [B,Hkv,Smax,D/64] bf16 (strides free, last dim contiguous);
// qout [B,Hq,T,D] contiguous. Tokens sit at positions p0 .. p0+T-1.
void rope_append_rows(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                      torch::Tensor qout, torch::Tensor kcache,
                      torch::Tensor vcache, int64_t p0,
                      torch::Tensor cos_table, torch::Tensor sin_table,
                      c10::optional<torch::Tensor> kscale,
                      c10::optional<torch::Tensor> vscale) {
  DNET_CHECK(q.dim() == 4 && k.dim() == 4 && v.dim() == 4, "q/k/v [B,T,H,D]");
  const int64_t B = q.size(0), T = q.size(1), Hq = q.size(2), D = q.size(3);
  const int64_t Hkv = k.size(2);
  const bool q8 = kcache.scalar_type() == torch::kInt8;
  DNET_CHECK(q.scalar_type() == torch::kBFloat16 &&
                 k.scalar_type() == torch::kBFloat16 &&
                 v.scalar_type() == torch::kBFloat16 &&
                 qout.scalar_type() == torch::kBFloat16,
             "q/k/v/qout bf16");
  DNET_CHECK(q8 || kcache.scalar_type() == torch::kBFloat16,
             "cache bf16 or int8");
  DNET_CHECK(vcache.scalar_type() == kcache.scalar_type(), "k/v cache dtype");
  DNET_CHECK(q8 ? (D == 64 || D == 128) : (D == 64 || D == 96 || D == 128),
             "rope_append_rows: unsupported head dim");
  DNET_CHECK(k.size(0) == B && k.size(1) == T && k.size(3) == D &&
                 v.sizes() == k.sizes(),
             "k/v shape");
  auto inner = [&](const torch::Tensor& t) {
    return t.stride(3) == 1 && t.stride(2) == D && t.stride(1) % 8 == 0 &&
           t.stride(0) % 8 == 0 && aligned16(t);
  };
  DNET_CHECK(inner(q) && inner(k) && inner(v),
             "q/k/v: last dim contiguous, head stride D, 16-byte rows");
  DNET_CHECK(qout.is_contiguous() && qout.size(0) == B && qout.size(1) == Hq &&
                 qout.size(2) == T && qout.size(3) == D && aligned16(qout),
             "qout [B,Hq,T,D] contiguous");
  auto cache_ok = [&](const torch::Tensor& t, int64_t last, int64_t unit) {
    return t.dim() == 4 && t.size(0) == B && t.size(1) == Hkv &&
           t.size(2) == kcache.size(2) && t.size(3) == last &&
           t.stride(3) == 1 && t.stride(0) % unit == 0 &&
           t.stride(1) % unit == 0 && t.stride(2) % unit == 0;
  };
  DNET_CHECK(cache_ok(kcache, D, 8) && cache_ok(vcache, D, 8) &&
                 aligned16(kcache) && aligned16(vcache),
             "cache [B,Hkv,Smax,D], last dim contiguous, 8-element rows");
  const int64_t Smax = kcache.size(2);
  DNET_CHECK(p0 >= 0 && p0 + T <= Smax, "p0 + T exceeds the cache");
  DNET_CHECK(cos_table.scalar_type() == torch::kFloat32 &&
                 sin_table.scalar_type() == torch::kFloat32 &&
                 cos_table.is_contiguous() && sin_table.is_contiguous() &&
                 cos_table.dim() == 2 && cos_table.size(1) == D / 2 &&
                 sin_table.sizes() == cos_table.sizes() &&
                 cos_table.size(0) >= p0 + T && aligned16(cos_table) &&
                 aligned16(sin_table),
             "cos/sin f32 [>= p0+T, D/2] contiguous");
  RowsGeom g{};
  g.q_sb = q.stride(0); g.q_st = q.stride(1);
  g.k_sb = k.stride(0); g.k_st = k.stride(1);
  g.v_sb = v.stride(0); g.v_st = v.stride(1);
  g.kc_sb = kcache.stride(0); g.kc_sh = kcache.stride(1);
  g.kc_ss = kcache.stride(2);
  g.vc_sb = vcache.stride(0); g.vc_sh = vcache.stride(1);
  g.vc_ss = vcache.stride(2);
  short *ksp = nullptr, *vsp = nullptr;
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
    ksp = (short*)kscale->data_ptr();
    vsp = (short*)vscale->data_ptr();
  }
  g.rows = B * T * (Hq + Hkv);
  g.T = (int)T; g.Hq = (int)Hq; g.Hkv = (int)Hkv; g.p0 = (int)p0;
  if (g.rows == 0) return;
  auto stream = current_stream();
  const int rpb = 256 / (D == 64 ? 4 : 8);
  const dim3 grid((unsigned)cdiv(g.rows, rpb));
#define LAUNCH_RAR(DD, QQ)                                                   \
  hipLaunchKernelGGL((rope_append_rows_kernel<DD, QQ>), grid, dim3(256), 0,  \
                     stream, (const short*)q.data_ptr(),                     \
                     (const short*)k.data_ptr(), (const short*)v.data_ptr(), \
                     (short*)qout.data_ptr(), kcache.data_ptr(),             \
                     vcache.data_ptr(), ksp, vsp,                            \
                     (const float*)cos_table.data_ptr(),                     \
                     (const float*)sin_table.data_ptr(), g)
  if (D == 128 && q8) LAUNCH_RAR(128, true);
  else if (D == 128) LAUNCH_RAR(128, false);
  else if (D == 64 && q8) LAUNCH_RAR(64, true);
  else if (D == 64) LAUNCH_RAR(64, false);
  else LAUNCH_RAR(96, false);
#undef LAUNCH_RAR
}

}  // namespace dnet
