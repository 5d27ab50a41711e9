// Token-routed MFMA expert GEMMs for int4 (W4A16) MoE banks, T > 64 rows:
// the moe_gateup_rows / moe_down_rows pair of moe_rows.hip.cpp for uint8
// nibble banks in the pack_int4_mfma layout with bf16 group scales. The
// plan of moe_route (slots sorted by expert, 64-row tiles) and the combine
// launch are used as they are; only the GEMM is new.
//
// The 64-row body of moe_rows.hip.cpp dequantises its weight strip once
// per tile (4 MFMAs per converted fragment) and consumes every group of
// weight loads before it issues the next. int4 pays more VALU per weight
// than int8, so this body is built around the unpack instead:
//
//  - 128-row work items. The plan emits an expert's 64-row tiles one after
//    the other. The block at grid index y takes tile y only when it is an
//    even tile of its expert ((first - offsets[e]) / 64 even) and covers
//    tile y + 1 as well when that one belongs to the same expert; blocks on
//    odd tiles leave at once. Rows of a pair are contiguous slots. The
//    number of stacked 16-row A tiles is block-uniform, MT = 8 for a pair
//    with more than 64 rows and MT = 4 otherwise, so an expert with one
//    tile does not pay for a second half. Every dequantised B fragment
//    feeds MT MFMAs (v_mfma_f32_16x16x32_bf16), 8 where the rows exist.
//  - Two B sets per wave. A wave holds 16 gate columns and the matching 16
//    up columns (the GLU runs on the accumulators), or down columns h and
//    h + 16, so one A fragment read from LDS feeds two MFMAs. A block's
//    four waves cover 64 act columns or 128 down columns.
//  - A in LDS. The rows (x gathered through slot_token for gate/up,
//    contiguous act slots for down) are staged 256 k at a time with 16 B
//    loads into rows of 256 + 8 elements (the pad spreads the 16 rows of a
//    fragment read over the banks). Rows past the end read the last live
//    row and are never stored. 128 rows * 528 B + the row sources = 66.5
//    KB in one (dynamic) __shared__ object: two blocks per CU.
//  - Pipelined weight stream. A lane's 16 B nibble load is the four B
//    fragments of one 128-k quad (pack_int4_mfma: [quad][slice][chunk]).
//    The loads of quad q + 1 (two rows and their group scales) are issued
//    before quad q is unpacked and multiplied and stay in flight across
//    the LDS stage boundary: the barriers are the raw s_barrier with
//    lgkmcnt-only waits of gemm_m16, which leave vmcnt alone.
//  - Unpack. bf16(q * s), q = nibble - 8, is built per 32-bit word from
//    two masks (low nibbles, high nibbles in place), one v_cvt_f32_ubyteN
//    per value and one fma per value: low nibbles n * s - 8s, high nibbles
//    (16n) * (s / 16) - 8s. Both products are exact in f32 and the fma
//    rounds once, to a value that f32 holds exactly, so the single
//    round-to-nearest-even to bf16 gives the bits of deq4 (common.h). With
//    one packed convert per pair that is 22 VALU instructions per 8 weights.
//
// K is never split: a slot's dot product runs over k in one fixed order in
// one wave, so its bits depend on its token and expert only, not on the
// pair or tile it landed in (each C row of an MFMA depends on its own A
// row alone). No atomics, no zeroed outputs, no host sync.
//
// gate/up epilogue: bias + GLU on the accumulators -> act[slot, I] bf16.
// down epilogue: y[slot, H] = we[t, e] * (acc + bias) f32, plain stores;
// moe_rows_combine then sums each token's slots in ascending-expert order.
#include "moe_common.h"

namespace dnet {

using i32x4 = __attribute__((ext_vector_type(4))) int;
using f32x2 = __attribute__((ext_vector_type(2))) float;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;

constexpr int kI4XT = 256;             // k per LDS stage
constexpr int kI4SE = kI4XT + 8;       // row stride in bf16 elems (16 B pad)
constexpr int kI4Rows = 128;           // rows of a tile pair

struct RowsInt4Lds {
  short a[kI4Rows * kI4SE];
  int rowsrc[kI4Rows];
};

// 8 offset-8 nibbles of one word (k ascending from the low nibble) ->
// bf16(q * s); s16 = s / 16, m8 = -8 * s
__device__ __forceinline__ bf16x8 deq4_word(const int w, const float s,
                                            const float s16, const float m8) {
  unsigned lo = (unsigned)w & 0x0F0F0F0Fu;
  unsigned hi = (unsigned)w & 0xF0F0F0F0u;
  // opaque: keeps the byte extracts as v_cvt_f32_ubyteN of the two masks
  asm("" : "+v"(lo));
  asm("" : "+v"(hi));
  bf16x8 b;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    // byte j of both masks: one packed f32 -> bf16 convert per pair
    const f32x2 v = {
        __builtin_fmaf((float)((lo >> (8 * j)) & 0xFFu), s, m8),
        __builtin_fmaf((float)((hi >> (8 * j)) & 0xFFu), s16, m8)};
    const bf16x2 p = __builtin_convertvector(v, bf16x2);
    b[2 * j] = p[0];
    b[2 * j + 1] = p[1];
  }
  return b;
}

// One work item of 16 * MT rows starting at slot `first` of expert e.
// DOWN = 0: a = x [T, K], bank [E, 2*NC, K/2] (gate rows then up rows),
//           act[slot, NC] = glu(gate, up); a wave owns 16 columns.
// DOWN = 1: a = act [slots_cap, K], bank [E, NC, K/2],
//           y[slot, NC] = we[t, e] * (a . w + bias); a wave owns 32 columns.
template <int MT, int DOWN, int GLU>
__device__ __forceinline__ void rows_int4_body(
    RowsInt4Lds& lds, const short* __restrict__ a,
    const uint8_t* __restrict__ w, const short* __restrict__ scales,
    const short* __restrict__ bias, const int* __restrict__ slot_token,
    const float* __restrict__ we, short* __restrict__ act,
    float* __restrict__ y, const int e, const int first, const int rows,
    const int K, const int NC, const int E, const int G, const float alpha,
    const float limit) {
  const int wave = threadIdx.x / kWave;
  const int lane = threadIdx.x & (kWave - 1);
  const int col = lane & 15;
  const int sl = lane >> 4;            // k-slice of this lane
  if (threadIdx.x < 16 * MT) {
    // rows past the end read the last live row; never stored
    const int slot = first + min((int)threadIdx.x, rows - 1);
    lds.rowsrc[threadIdx.x] = DOWN ? slot : slot_token[slot];
  }
  // this lane's two weight rows (a down wave past NC keeps the barriers,
  // reads clamped rows and stores nothing)
  const int c0 = (blockIdx.x * 4 + wave) * (DOWN ? 32 : 16);
  const bool valid = c0 < NC;
  int64_t wr[2];
  if (DOWN) {
    wr[0] = (int64_t)e * NC + min(c0 + col, NC - 1);
    wr[1] = (int64_t)e * NC + min(c0 + 16 + col, NC - 1);
  } else {
    wr[0] = (int64_t)e * 2 * NC + min(c0 + col, NC - 1);
    wr[1] = wr[0] + NC;
  }
  const uint8_t* wp[2];
  const short* sp[2];
#pragma unroll
  for (int z = 0; z < 2; ++z) {
    wp[z] = w + wr[z] * (K / 2) + sl * 16;
    sp[z] = scales + wr[z] * (K / G);
  }

  f32x4 acc[MT][2];
#pragma unroll
  for (int t = 0; t < MT; ++t)
    acc[t][0] = acc[t][1] = {0.f, 0.f, 0.f, 0.f};

  const int nq = K / 128;
  // the stream's registers: quad q + 1 while quad q is consumed
  i32x4 wn[2];
  short sn[2];
#pragma unroll
  for (int z = 0; z < 2; ++z) {
    wn[z] = *reinterpret_cast<const i32x4*>(wp[z]);
    sn[z] = sp[z][0];
  }
  // byte offset and scale index of the quad in wn / sn; a group holds
  // gquads quads
  const int gquads = G / 128;
  int wofs = 0, sidx = 0, gfill = 0;
  // staging: thread -> 16 B vector (tid & 31) of rows (tid >> 5) + 8 * i
  const int svec = (threadIdx.x & 31) * 8;
  const int srow = threadIdx.x >> 5;
  const short* arow = &lds.a[col * kI4SE + sl * 8];

  for (int k0 = 0; k0 < K; k0 += kI4XT) {
    const int tk = min(kI4XT, K - k0);   // 256, or a 128-k tail
    // raw barriers (lgkmcnt only): the weight loads in flight survive them
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    asm volatile("s_barrier" ::: "memory");
    if (svec < tk) {
#pragma unroll
      for (int h = 0; h < MT / 4; ++h) {     // 8 row loads in flight
        short8 v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
          v[i] = *reinterpret_cast<const short8*>(
              &a[(int64_t)lds.rowsrc[srow + 8 * (h * 8 + i)] * K + k0 + svec]);
#pragma unroll
        for (int i = 0; i < 8; ++i)
          *reinterpret_cast<short8*>(
              &lds.a[(srow + 8 * (h * 8 + i)) * kI4SE + svec]) = v[i];
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    asm volatile("s_barrier" ::: "memory");
#pragma unroll
    for (int u = 0; u < kI4XT / 128; ++u) {
      if (u * 128 >= tk) break;          // block-uniform
      const int q = k0 / 128 + u;
      i32x4 wq[2];
      float s[2], s16[2], m8[2];
#pragma unroll
      for (int z = 0; z < 2; ++z) {
        wq[z] = wn[z];
        s[z] = bits2f(sn[z]);
        s16[z] = s[z] * 0.0625f;
        m8[z] = s[z] * -8.f;
      }
      // next quad's loads, issued before this quad's unpack (the last
      // quad re-reads itself: stays in the row)
      if (q + 1 < nq) {
        wofs += 64;
        if (++gfill == gquads) {
          gfill = 0;
          ++sidx;
        }
      }
#pragma unroll
      for (int z = 0; z < 2; ++z) {
        wn[z] = *reinterpret_cast<const i32x4*>(wp[z] + wofs);
        sn[z] = sp[z][sidx];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bf16x8 b0 = deq4_word(wq[0][c], s[0], s16[0], m8[0]);
        const bf16x8 b1 = deq4_word(wq[1][c], s[1], s16[1], m8[1]);
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          const bf16x8 af = *reinterpret_cast<const bf16x8*>(
              &arow[t * 16 * kI4SE + u * 128 + c * 32]);
          acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, b0,
                                                              acc[t][0], 0, 0, 0);
          acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, b1,
                                                              acc[t][1], 0, 0, 0);
        }
      }
    }
  }

  // C: lane covers column (lane & 15), rows (lane >> 4) * 4 + 0..3 per tile
  if (!valid) return;
  const int n = c0 + col;
  float bz[2] = {0.f, 0.f};
  if (bias != nullptr) {
    bz[0] = bits2f(bias[wr[0]]);
    bz[1] = bits2f(bias[wr[1]]);
  }
#pragma unroll
  for (int t = 0; t < MT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = t * 16 + sl * 4 + r;
      if (m >= rows) continue;
      const int64_t slot = first + m;
      if (DOWN) {
        const float wt = we[(int64_t)slot_token[slot] * E + e];
        y[slot * NC + n] = wt * (acc[t][0][r] + bz[0]);
        y[slot * NC + n + 16] = wt * (acc[t][1][r] + bz[1]);
      } else {
        act[slot * NC + n] = f2bits(apply_glu<GLU>(
            acc[t][0][r] + bz[0], acc[t][1][r] + bz[1], alpha, limit));
      }
    }
  }
}

// grid: (column strips, tiles_cap)
template <int DOWN, int GLU>
__global__ __launch_bounds__(256, 2) void moe_rows_int4_kernel(
    const short* __restrict__ a, const uint8_t* __restrict__ w,
    const short* __restrict__ scales, const short* __restrict__ bias,
    const int* __restrict__ slot_token, const int* __restrict__ offsets,
    const int* __restrict__ tiles, const int* __restrict__ ntiles,
    const float* __restrict__ we, short* __restrict__ act,
    float* __restrict__ y, const int K, const int NC, const int E, const int G,
    const float alpha, const float limit) {
  extern __shared__ __attribute__((aligned(16))) char rows_int4_smem[];
  RowsInt4Lds& lds = *reinterpret_cast<RowsInt4Lds*>(rows_int4_smem);
  const int tile = blockIdx.y;
  const int nt = ntiles[0];
  if (tile >= nt) return;              // block-uniform, as all exits here
  const int e = tiles[tile * 3 + 0];
  const int first = tiles[tile * 3 + 1];
  int rows = tiles[tile * 3 + 2];
  // an expert's odd tiles belong to the block of the tile before them
  if (((first - offsets[e]) / 64) & 1) return;
  if (tile + 1 < nt && tiles[(tile + 1) * 3 + 0] == e)
    rows += tiles[(tile + 1) * 3 + 2];
  if (rows > 64)
    rows_int4_body<8, DOWN, GLU>(lds, a, w, scales, bias, slot_token, we, act,
                                 y, e, first, rows, K, NC, E, G, alpha, limit);
  else
    rows_int4_body<4, DOWN, GLU>(lds, a, w, scales, bias, slot_token, we, act,
                                 y, e, first, rows, K, NC, E, G, alpha, limit);
}

// 66.5 KB of dynamic LDS: above the 64 KB default, below the CU's 160 KB
template <int DOWN, int GLU, typename... Args>
static void rows_int4_launch(dim3 grid, hipStream_t stream, Args... args) {
  static const bool raised = []() {
    DNET_CHECK_HIP(hipFuncSetAttribute(
        reinterpret_cast<const void*>(&moe_rows_int4_kernel<DOWN, GLU>),
        hipFuncAttributeMaxDynamicSharedMemorySize, sizeof(RowsInt4Lds)));
    return true;
  }();
  (void)raised;
  hipLaunchKernelGGL((moe_rows_int4_kernel<DOWN, GLU>), grid, dim3(256),
                     sizeof(RowsInt4Lds), stream, args...);
}

static bool is_i32(const torch::Tensor& t) {
  return t.scalar_type() == torch::kInt && t.is_contiguous();
}

// One bank [E, rows, K/2] + scales [E, rows, K/group] (+ bias [E, rows]).
static void rows_int4_check_bank(const torch::Tensor& w,
                                 const c10::optional<torch::Tensor>& scales,
                                 const c10::optional<torch::Tensor>& bias,
                                 int64_t rows, int64_t K, int64_t group,
                                 bool packed) {
  DNET_CHECK(packed, "moe rows int4: pack_int4_mfma layout only");
  DNET_CHECK(K > 0 && K % 128 == 0 && group > 0 && group % 128 == 0 &&
                 K % group == 0,
             "moe rows int4: inner dim and group must be multiples of 128");
  DNET_CHECK(w.dim() == 3 && w.scalar_type() == torch::kByte &&
                 w.is_contiguous() && w.size(0) <= 1024 &&
                 w.size(1) == rows && w.size(2) == K / 2,
             "moe rows int4: bank shape");
  DNET_CHECK(scales.has_value() && scales->dim() == 3 &&
                 scales->scalar_type() == torch::kBFloat16 &&
                 scales->is_contiguous() && scales->size(0) == w.size(0) &&
                 scales->size(1) == rows && scales->size(2) == K / group,
             "moe rows int4: scales shape");
  if (bias.has_value())
    DNET_CHECK(bias->is_contiguous() && bias->numel() == w.size(0) * rows &&
                   bias->scalar_type() == torch::kBFloat16,
               "moe rows int4: bias");
}

void moe_rows_int4_gateup(torch::Tensor x, torch::Tensor w,
                          c10::optional<torch::Tensor> scales,
                          c10::optional<torch::Tensor> bias,
                          torch::Tensor slot_token, torch::Tensor offsets,
                          torch::Tensor tiles, torch::Tensor ntiles,
                          torch::Tensor act, int64_t group, bool packed,
                          int64_t glu, double alpha, double limit) {
  DNET_CHECK(x.dim() == 2 && x.scalar_type() == torch::kBFloat16 &&
                 x.is_contiguous() && w.dim() == 3, "x");
  const int64_t K = x.size(1), E = w.size(0), I = w.size(1) / 2;
  DNET_CHECK(I > 0 && I % 128 == 0 && I % std::max<int64_t>(group, 1) == 0,
             "moe rows int4: I must be a multiple of 128 and of the group");
  rows_int4_check_bank(w, scales, bias, 2 * I, K, group, packed);
  DNET_CHECK(is_i32(slot_token) && is_i32(offsets) && is_i32(tiles) &&
                 is_i32(ntiles) && offsets.numel() == E + 1 &&
                 tiles.dim() == 2 && tiles.size(1) == 3 &&
                 tiles.size(0) <= 65535 && ntiles.numel() == 1, "plan");
  DNET_CHECK(act.scalar_type() == torch::kBFloat16 && act.is_contiguous() &&
                 act.dim() == 2 && act.size(0) == slot_token.numel() &&
                 act.size(1) == I, "act");
  if (tiles.size(0) == 0) return;
  const dim3 grid((unsigned)(I / 64), (unsigned)tiles.size(0));
  auto launch = [&](auto gluc) {
    rows_int4_launch<0, decltype(gluc)::value>(
        grid, current_stream(), (const short*)x.data_ptr(),
        (const uint8_t*)w.data_ptr(), (const short*)scales->data_ptr(),
        bias.has_value() ? (const short*)bias->data_ptr() : nullptr,
        (const int*)slot_token.data_ptr(), (const int*)offsets.data_ptr(),
        (const int*)tiles.data_ptr(), (const int*)ntiles.data_ptr(),
        (const float*)nullptr, (short*)act.data_ptr(), (float*)nullptr,
        (int)K, (int)I, (int)E, (int)group, (float)alpha, (float)limit);
  };
  if (glu == 1) launch(std::integral_constant<int, 1>{});
  else launch(std::integral_constant<int, 0>{});
}

void moe_rows_int4_down(torch::Tensor act, torch::Tensor w,
                        c10::optional<torch::Tensor> scales,
                        c10::optional<torch::Tensor> bias, torch::Tensor we,
                        torch::Tensor slot_token, torch::Tensor token_slots,
                        torch::Tensor offsets, torch::Tensor tiles,
                        torch::Tensor ntiles, torch::Tensor y,
                        torch::Tensor out, int64_t group, bool packed) {
  DNET_CHECK(act.dim() == 2 && act.scalar_type() == torch::kBFloat16 &&
                 act.is_contiguous() && act.size(0) == slot_token.numel() &&
                 w.dim() == 3 && we.dim() == 2, "act");
  const int64_t I = act.size(1), E = w.size(0), H = w.size(1);
  const int64_t T = we.size(0);
  DNET_CHECK(H > 0 && H % 64 == 0, "moe rows int4: H % 64");
  rows_int4_check_bank(w, scales, bias, H, I, group, packed);
  DNET_CHECK(we.scalar_type() == torch::kFloat && we.is_contiguous() &&
                 we.size(1) == E, "we");
  DNET_CHECK(is_i32(slot_token) && is_i32(token_slots) && is_i32(offsets) &&
                 is_i32(tiles) && is_i32(ntiles) &&
                 offsets.numel() == E + 1 && tiles.dim() == 2 &&
                 tiles.size(1) == 3 && tiles.size(0) <= 65535 &&
                 ntiles.numel() == 1 && token_slots.dim() == 2 &&
                 token_slots.size(0) == T, "plan");
  DNET_CHECK(y.scalar_type() == torch::kFloat && y.is_contiguous() &&
                 y.dim() == 2 && y.size(0) == slot_token.numel() &&
                 y.size(1) == H, "y");
  DNET_CHECK(out.scalar_type() == torch::kFloat && out.is_contiguous() &&
                 out.dim() == 2 && out.size(0) == T && out.size(1) == H,
             "out");
  if (T == 0) return;
  auto stream = current_stream();
  if (tiles.size(0) > 0) {
    const dim3 grid((unsigned)cdiv(H, 128), (unsigned)tiles.size(0));
    rows_int4_launch<1, 0>(
        grid, stream, (const short*)act.data_ptr(),
        (const uint8_t*)w.data_ptr(), (const short*)scales->data_ptr(),
        bias.has_value() ? (const short*)bias->data_ptr() : nullptr,
        (const int*)slot_token.data_ptr(), (const int*)offsets.data_ptr(),
        (const int*)tiles.data_ptr(), (const int*)ntiles.data_ptr(),
        (const float*)we.data_ptr(), (short*)nullptr, (float*)y.data_ptr(),
        (int)I, (int)H, (int)E, (int)group, 0.f, 0.f);
  }
  moe_rows_combine(y, token_slots, out, stream);
}

}  // namespace dnet
