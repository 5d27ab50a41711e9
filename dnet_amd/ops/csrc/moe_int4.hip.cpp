// MFMA grouped-expert decode kernels for int4 (W4A16, group 128k) MoE
// banks: the moe_gateup / moe_down pair of moe.hip.cpp for uint8 nibble
// banks with bf16 group scales, 1 <= M <= 64 rows in one pass.
//
// The FMA kernels of moe.hip.cpp give one wave one output row and 2*M
// accumulators per lane; with int4 every weight also costs an unpack per
// row tile. Here a wave owns a 16-column strip of one expert and feeds
// v_mfma_f32_16x16x32_bf16, so the unpack is paid once per weight and up
// to four stacked 16-row A tiles (MT = 1, 2, 4) share it: a routed
// expert's bank is read once per layer at any M <= 64.
//
//  - A side: x (gate/up) or act[e] (down) is staged in LDS in k-tiles of
//    512 k (256 at MT = 4) with a 16-byte row pad (the layout of gemm_m16's generic
//    kernel), only the M live rows; rows past M hold whatever LDS held,
//    and feed C rows that are never stored.
//  - B side: weights go from global memory straight into fragment shape.
//    In the pack_int4_mfma chunk-quad layout a lane's 16-byte load holds
//    its 8-element slices of four K=32 chunks: four MFMAs per load and
//    stacked tile, nibbles dequantised in registers to bf16(q*s) by the
//    deq4 of gemm_m16 (common.h). A tile's loads are all issued before
//    the x staging, so both round trips overlap.
//  - gate/up: a wave holds the 16 gate columns and the matching 16 up
//    columns of its strip, one A fragment read feeds both, and the GLU is
//    applied to the accumulators (same C layout) before the bf16 store.
//  - expert skip: every wave reads column e of we (M <= 64 values, one per
//    lane) and the block leaves when all are zero. Nothing data-dependent
//    happens on the host, so the pair is hipGraph-capturable.
//  - down combine: the experts are cut into NG contiguous groups
//    (gridDim.y). A block walks its group's routed experts in ascending
//    order, adds we[m,e] * (act[e,m] . Wd[e] + b[e]) into registers for
//    the rows with we != 0 only (a skipped expert's garbage or NaN act row
//    is multiplied but never added), and stores its [M, H] slice with
//    plain stores. A combine launch sums, per token, the slices of the
//    groups that hold one of the token's experts, ascending: no atomics,
//    no zeroed output, a token without experts gets exact zeros, and a
//    token's bits depend on its own routing only. NG = min(E, 8 *
//    ceil(64 / M)): at batch 1 every routed expert gets blocks of its own,
//    at batch 64 the slices stay a few MB against a bank of 100 MB+.
//
// Filling the machine: with KS = 1 a block's four waves take four strips
// (64 columns) over the whole K; a narrow bank then gives too few blocks
// (Qwen3-30B-A3B down at batch 1: 8 experts x 32 blocks on 256 CUs). With
// KS = 4 the four waves share ONE strip, wave w taking the quads
// q % 4 == w of every tile, and the partial accumulators are summed
// through LDS in wave order (fixed, so bits repeat). The launcher takes
// KS = 4 when KS = 1 would start fewer than kFillBlocks blocks, counting
// min(groups, 2 * M) routed experts (the host cannot know the routing),
// and only for M <= 32: at MT = 4 a tile holds two quads. Measurements in
// profiles/r10_moe_int4.md; DNET_MOE_INT4_KS = 1 / 4 (or
// moe_int4_force_ks) forces either.
#include "moe_common.h"

namespace dnet {

using i32x4 = __attribute__((ext_vector_type(4))) int;

constexpr int kFillBlocks = 512;

// we[:, e] != 0 anywhere? Same answer in every wave of the block.
__device__ __forceinline__ bool int4_expert_routed(const float* __restrict__ we,
                                                   const int M, const int E,
                                                   const int e,
                                                   const int lane) {
  const bool r = lane < M && we[(int64_t)lane * E + e] != 0.f;
  return __ballot(r) != 0ull;
}

// LDS image of one k-tile: 16 * MT rows of kXT k (512, or 256 at MT = 4)
// and a 16-byte pad, 17 to 34 KB.
template <int MT>
struct Int4Lds {
  static constexpr int kXT = MT == 4 ? 256 : 512;
  static constexpr int kElems = 16 * MT * (kXT + 8);
  // the KS reduce parks 3 waves * 2 rows * MT tiles * 256 f32 here
  static_assert(kElems * 2 >= 3 * 2 * MT * 256 * 4, "reduce fits");
};

// acc[b][t] += A[M, K] . W_b[16 rows of this lane's strip, K]^T for NB
// weight rows per lane (gate and up, or one down row). a: bf16 rows of
// stride K; wrow[b]: the lane's packed row + its 16-byte slot offset;
// srow[b]: the row's scales. kpart: this wave's share of every tile's
// quads under KS. All waves of the block must call this together.
template <int MT, int KS, int NB>
__device__ __forceinline__ void int4_strip_gemm(
    const short* __restrict__ a, const int M, const int K, const int G,
    const uint8_t* const (&wrow)[NB], const short* const (&srow)[NB],
    short* x_lds, f32x4 (&acc)[NB][MT], const int kpart, const int lane) {
  constexpr int XT = Int4Lds<MT>::kXT;  // k per tile
  constexpr int SE = XT + 8;           // row stride in bf16 elems (16 B pad)
  constexpr int NQ = XT / 128;         // quads per tile
  constexpr int QW = (NQ + KS - 1) / KS;  // quads per tile and wave
  const int row = lane & 15;
  const int ks = (lane >> 4) * 8;
  for (int k0 = 0; k0 < K; k0 += XT) {
    const int tk = min(XT, K - k0);
    const int nq = tk / 128;
    i32x4 wq[NB][QW];
    float sv[NB][QW];
#pragma unroll
    for (int j = 0; j < QW; ++j) {
      const int ql = kpart + j * KS;
      const int quad = k0 / 128 + min(ql, nq - 1);  // clamped: stays in row
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        wq[b][j] = *reinterpret_cast<const i32x4*>(wrow[b] + quad * 64);
        sv[b][j] = bits2f(srow[b][(quad * 128) / G]);
      }
    }
    // raw barriers (lgkmcnt only, as gemm_m16): __syncthreads() would
    // drain the weight loads just issued before the x loads even start
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    asm volatile("s_barrier" ::: "memory");
    const int vpr = tk / 8;
    for (int idx = threadIdx.x; idx < M * vpr; idx += 256) {
      const int r = idx / vpr;
      const int vec = idx - r * vpr;
      *reinterpret_cast<short8*>(&x_lds[r * SE + vec * 8]) =
          *reinterpret_cast<const short8*>(&a[(int64_t)r * K + k0 + vec * 8]);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    asm volatile("s_barrier" ::: "memory");
#pragma unroll
    for (int j = 0; j < QW; ++j) {
      const int ql = kpart + j * KS;
      if (ql >= nq) break;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        bf16x8 bf[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          // opaque copy at the use (as gemm_m16): without it the nibbles
          // of the whole tile are extracted up front, 256 VGPRs at MT = 1
          int wc = wq[b][j][c];
          asm volatile("" : "+v"(wc));
          bf[b] = deq4(reinterpret_cast<const uint8_t*>(&wc), sv[b][j]);
        }
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          const bf16x8 af = *reinterpret_cast<const bf16x8*>(
              &x_lds[(t * 16 + row) * SE + ql * 128 + c * 32 + ks]);
#pragma unroll
          for (int b = 0; b < NB; ++b)
            acc[b][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                af, bf[b], acc[b][t], 0, 0, 0);
        }
      }
    }
  }
}

// KS = 4: waves 1..3 hand their accumulators to wave 0 through LDS (the
// x tile is dead by then); wave 0 adds them in wave order.
template <int MT, int NB>
__device__ __forceinline__ void int4_ks_reduce(f32x4 (&acc)[NB][MT],
                                               short* x_lds, const int kpart,
                                               const int lane) {
  float* red = reinterpret_cast<float*>(x_lds);
  __syncthreads();
  if (kpart > 0) {
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int t = 0; t < MT; ++t)
        *reinterpret_cast<f32x4*>(
            &red[(((kpart - 1) * NB + b) * MT + t) * 256 + lane * 4]) =
            acc[b][t];
  }
  __syncthreads();
  if (kpart == 0) {
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int t = 0; t < MT; ++t)
          acc[b][t] += *reinterpret_cast<const f32x4*>(
              &red[((p * NB + b) * MT + t) * 256 + lane * 4]);
  }
}

// grid: (strips / (4 / KS), E)
template <int MT, int KS, int GLU>
__global__ __launch_bounds__(256) void moe_int4_gateup_kernel(
    const short* __restrict__ x, const uint8_t* __restrict__ w,
    const short* __restrict__ scales, const short* __restrict__ bias,
    const float* __restrict__ we, short* __restrict__ act, const int M,
    const int K, const int I, const int E, const int G, const float alpha,
    const float limit) {
  __shared__ __attribute__((aligned(16))) short x_lds[Int4Lds<MT>::kElems];
  const int e = blockIdx.y;
  const int wave = threadIdx.x / kWave;
  const int lane = threadIdx.x & (kWave - 1);
  if (!int4_expert_routed(we, M, E, e, lane)) return;
  const int strip = blockIdx.x * (4 / KS) + wave / KS;
  const int kpart = wave % KS;
  // I % 64 == 0: every strip of the grid is a whole one
  const int col = strip * 16 + (lane & 15);
  const int64_t grow = (int64_t)e * 2 * I + col;
  const int64_t urow = grow + I;
  const int woff = (lane >> 4) * 16;
  const uint8_t* const wrow[2] = {w + grow * (K / 2) + woff,
                                  w + urow * (K / 2) + woff};
  const short* const srow[2] = {scales + grow * (K / G),
                                scales + urow * (K / G)};
  f32x4 acc[2][MT];
#pragma unroll
  for (int t = 0; t < MT; ++t)
    acc[0][t] = acc[1][t] = {0.f, 0.f, 0.f, 0.f};
  int4_strip_gemm<MT, KS, 2>(x, M, K, G, wrow, srow, x_lds, acc, kpart, lane);
  if constexpr (KS > 1) {
    int4_ks_reduce<MT, 2>(acc, x_lds, kpart, lane);
    if (kpart > 0) return;
  }
  float bg = 0.f, bu = 0.f;
  if (bias != nullptr) {
    bg = bits2f(bias[grow]);
    bu = bits2f(bias[urow]);
  }
  // C layout: column lane & 15, rows (lane >> 4) * 4 + r of each tile
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = t * 16 + (lane >> 4) * 4 + r;
      if (m < M)
        act[((int64_t)e * M + m) * I + col] = f2bits(apply_glu<GLU>(
            acc[0][t][r] + bg, acc[1][t][r] + bu, alpha, limit));
    }
}

// grid: (ceil(strips / (4 / KS)), NG); group g = experts [g * EG, ...)
template <int MT, int KS>
__global__ __launch_bounds__(256) void moe_int4_down_kernel(
    const short* __restrict__ act, const uint8_t* __restrict__ w,
    const short* __restrict__ scales, const short* __restrict__ bias,
    const float* __restrict__ we, float* __restrict__ slices, const int M,
    const int I, const int H, const int E, const int EG, const int G) {
  __shared__ __attribute__((aligned(16))) short x_lds[Int4Lds<MT>::kElems];
  const int g = blockIdx.y;
  const int wave = threadIdx.x / kWave;
  const int lane = threadIdx.x & (kWave - 1);
  const int strip = blockIdx.x * (4 / KS) + wave / KS;
  const int kpart = wave % KS;
  // H % 16 == 0, but the last block may hold strips past H: those waves
  // read a clamped row, keep the barriers and store nothing
  const bool live = strip * 16 < H;
  const int col = min(strip * 16 + (lane & 15), H - 1);
  const int woff = (lane >> 4) * 16;
  f32x4 o[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) o[t] = {0.f, 0.f, 0.f, 0.f};
  bool any = false;
  const int e_end = min(E, (g + 1) * EG);
  for (int e = g * EG; e < e_end; ++e) {
    if (!int4_expert_routed(we, M, E, e, lane)) continue;  // block-uniform
    any = true;
    const int64_t wr = (int64_t)e * H + col;
    const uint8_t* const wrow[1] = {w + wr * (I / 2) + woff};
    const short* const srow[1] = {scales + wr * (I / G)};
    f32x4 acc[1][MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[0][t] = {0.f, 0.f, 0.f, 0.f};
    int4_strip_gemm<MT, KS, 1>(act + (int64_t)e * M * I, M, I, G, wrow, srow,
                               x_lds, acc, kpart, lane);
    // under KS the bias rides with wave 0's share of the dot
    const float b =
        (bias != nullptr && kpart == 0) ? bits2f(bias[wr]) : 0.f;
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = t * 16 + (lane >> 4) * 4 + r;
        const float wme = m < M ? we[(int64_t)m * E + e] : 0.f;
        if (wme != 0.f) o[t][r] += wme * (acc[0][t][r] + b);
      }
  }
  if (!any) return;  // the combine never reads this group's slice
  if constexpr (KS > 1) {
    f32x4 o2[1][MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) o2[0][t] = o[t];
    int4_ks_reduce<MT, 1>(o2, x_lds, kpart, lane);
    if (kpart > 0) return;
#pragma unroll
    for (int t = 0; t < MT; ++t) o[t] = o2[0][t];
  }
  if (!live) return;
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = t * 16 + (lane >> 4) * 4 + r;
      if (m < M) slices[((int64_t)g * M + m) * H + col] = o[t][r];
    }
}

// out[m, :] = sum, ascending, of the slices of the groups that hold one of
// token m's experts. grid: (ceil(H / 4 / 256), M); NG <= 256.
__global__ __launch_bounds__(256) void moe_int4_combine_kernel(
    const float* __restrict__ slices, const float* __restrict__ we,
    float* __restrict__ out, const int M, const int H, const int E,
    const int EG, const int NG) {
  __shared__ int list[256];
  __shared__ int wcnt[4];
  const int m = blockIdx.y;
  const int tid = threadIdx.x;
  const int wave = tid / kWave, lane = tid & (kWave - 1);
  bool f = false;
  if (tid < NG) {
    const int e_end = min(E, (tid + 1) * EG);
    for (int e = tid * EG; e < e_end; ++e)
      f |= we[(int64_t)m * E + e] != 0.f;
  }
  const unsigned long long bal = __ballot(f);
  if (lane == 0) wcnt[wave] = __popcll(bal);
  __syncthreads();
  int base = 0, n = 0;
  for (int v = 0; v < 4; ++v) {
    if (v < wave) base += wcnt[v];
    n += wcnt[v];
  }
  if (f) list[base + __popcll(bal & ((1ull << lane) - 1ull))] = tid;
  __syncthreads();
  const int h4 = blockIdx.x * 256 + tid;
  if (h4 >= H / 4) return;
  const float4* sl = reinterpret_cast<const float4*>(slices);
  float4 s = {0.f, 0.f, 0.f, 0.f};
  for (int i = 0; i < n; i += 4) {  // four loads in flight, adds in order
    float4 t[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (i + u < n)
        t[u] = sl[((int64_t)list[i + u] * M + m) * (H / 4) + h4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (i + u < n) slice_add(s, t[u]);
  }
  reinterpret_cast<float4*>(out)[(int64_t)m * (H / 4) + h4] = s;
}

// waves per strip: 4 when one strip per wave would leave CUs empty
// 0 = by shape; 1 / 4 forced (benchmarks, and tests of the path the small
// test shapes would not pick). Process-wide, read at launch.
static int g_int4_ks = []() {
  const char* e = getenv("DNET_MOE_INT4_KS");
  return e ? atoi(e) : 0;
}();
void moe_int4_force_ks(int64_t ks) { g_int4_ks = (int)ks; }

static int int4_pick_ks(int64_t n_cols, int64_t groups, int64_t M) {
  const int forced = g_int4_ks;
  if (M > 32) return 1;
  if (forced == 1 || forced == 4) return forced;
  const int64_t routed = std::min<int64_t>(groups, 2 * M);
  return cdiv(n_cols, 64) * routed < kFillBlocks ? 4 : 1;
}

static void int4_check_bank(const torch::Tensor& w,
                            const c10::optional<torch::Tensor>& scales,
                            int64_t rows, int64_t K, int64_t group) {
  DNET_CHECK(K % 128 == 0 && group > 0 && group % 128 == 0 && K % group == 0,
             "moe int4: inner dim and group must be multiples of 128");
  DNET_CHECK(w.scalar_type() == torch::kByte && w.is_contiguous() &&
                 w.size(1) == rows && w.size(2) == K / 2,
             "moe int4: bank shape");
  DNET_CHECK(scales.has_value() &&
                 scales->scalar_type() == torch::kBFloat16 &&
                 scales->is_contiguous() && scales->size(0) == w.size(0) &&
                 scales->size(1) == rows && scales->size(2) == K / group,
             "moe int4: scales shape");
}

void moe_int4_gateup(torch::Tensor x, torch::Tensor w,
                     c10::optional<torch::Tensor> scales,
                     c10::optional<torch::Tensor> bias, torch::Tensor we,
                     torch::Tensor act, int64_t group, int64_t glu,
                     double alpha, double limit) {
  const int64_t M = x.size(0), K = x.size(1);
  const int64_t E = w.size(0), I = w.size(1) / 2;
  DNET_CHECK(M >= 1 && M <= 64, "moe int4: 1 <= M <= 64");
  DNET_CHECK(I % 128 == 0, "moe int4: I must be a multiple of 128");
  int4_check_bank(w, scales, 2 * I, K, group);
  DNET_CHECK(x.scalar_type() == torch::kBFloat16 && x.is_contiguous() &&
                 act.is_contiguous() && act.size(0) == E &&
                 act.size(1) == M && act.size(2) == I, "moe_gateup shape");
  DNET_CHECK(we.is_contiguous() && we.scalar_type() == torch::kFloat &&
                 we.size(0) == M && we.size(1) == E, "we shape");
  if (bias.has_value())
    DNET_CHECK(bias->is_contiguous() && bias->numel() == E * 2 * I, "bias");
  const short* bptr =
      bias.has_value() ? (const short*)bias->data_ptr() : nullptr;
  auto stream = current_stream();
  const int ks = int4_pick_ks(I, E, M);
  const dim3 grid((unsigned)(I / 16 / (4 / ks)), (unsigned)E);
  auto launch = [&](auto mtc, auto ksc, auto gluc) {
    hipLaunchKernelGGL(
        (moe_int4_gateup_kernel<decltype(mtc)::value, decltype(ksc)::value,
                                decltype(gluc)::value>),
        grid, dim3(256), 0, stream, (const short*)x.data_ptr(),
        (const uint8_t*)w.data_ptr(), (const short*)scales->data_ptr(), bptr,
        (const float*)we.data_ptr(), (short*)act.data_ptr(), (int)M, (int)K,
        (int)I, (int)E, (int)group, (float)alpha, (float)limit);
  };
  auto with_glu = [&](auto mtc, auto ksc) {
    if (glu == 1)
      launch(mtc, ksc, std::integral_constant<int, 1>{});
    else
      launch(mtc, ksc, std::integral_constant<int, 0>{});
  };
  using one = std::integral_constant<int, 1>;
  using two = std::integral_constant<int, 2>;
  using four = std::integral_constant<int, 4>;
  if (M > 32) with_glu(four{}, one{});
  else if (M > 16) { if (ks == 4) with_glu(two{}, four{}); else with_glu(two{}, one{}); }
  else { if (ks == 4) with_glu(one{}, four{}); else with_glu(one{}, one{}); }
}

void moe_int4_down(torch::Tensor act, torch::Tensor w,
                   c10::optional<torch::Tensor> scales,
                   c10::optional<torch::Tensor> bias, torch::Tensor we,
                   torch::Tensor out, int64_t group) {
  const int64_t E = w.size(0), H = w.size(1);
  const int64_t M = act.size(1), I = act.size(2);
  DNET_CHECK(M >= 1 && M <= 64, "moe int4: 1 <= M <= 64");
  DNET_CHECK(H % 16 == 0, "moe int4: H must be a multiple of 16");
  int4_check_bank(w, scales, H, I, group);
  DNET_CHECK(act.scalar_type() == torch::kBFloat16 && act.is_contiguous() &&
                 act.size(0) == E, "moe_down act shape");
  DNET_CHECK(out.is_contiguous() && out.scalar_type() == torch::kFloat &&
                 out.size(0) == M && out.size(1) == H, "moe_down out f32");
  DNET_CHECK(we.is_contiguous() && we.scalar_type() == torch::kFloat &&
                 we.size(0) == M && we.size(1) == E, "we shape");
  if (bias.has_value())
    DNET_CHECK(bias->is_contiguous() && bias->numel() == E * H, "bias");
  const short* bptr =
      bias.has_value() ? (const short*)bias->data_ptr() : nullptr;
  // expert groups (see the header): a function of E and M alone
  const int64_t ng0 =
      std::min<int64_t>(std::min<int64_t>(E, 8 * cdiv(64, M)), 256);
  const int64_t EG = cdiv(E, ng0);
  const int64_t NG = cdiv(E, EG);
  auto slices = torch::empty({NG, M, H}, out.options());
  auto stream = current_stream();
  const int ks = int4_pick_ks(H, NG, M);
  const dim3 grid((unsigned)cdiv(H / 16, 4 / ks), (unsigned)NG);
  auto launch = [&](auto mtc, auto ksc) {
    hipLaunchKernelGGL(
        (moe_int4_down_kernel<decltype(mtc)::value, decltype(ksc)::value>),
        grid, dim3(256), 0, stream, (const short*)act.data_ptr(),
        (const uint8_t*)w.data_ptr(), (const short*)scales->data_ptr(), bptr,
        (const float*)we.data_ptr(), (float*)slices.data_ptr(), (int)M,
        (int)I, (int)H, (int)E, (int)EG, (int)group);
  };
  using one = std::integral_constant<int, 1>;
  using two = std::integral_constant<int, 2>;
  using four = std::integral_constant<int, 4>;
  if (M > 32) launch(four{}, one{});
  else if (M > 16) { if (ks == 4) launch(two{}, four{}); else launch(two{}, one{}); }
  else { if (ks == 4) launch(one{}, four{}); else launch(one{}, one{}); }
  hipLaunchKernelGGL(moe_int4_combine_kernel,
                     dim3((unsigned)cdiv(H / 4, 256), (unsigned)M), dim3(256),
                     0, stream, (const float*)slices.data_ptr(),
                     (const float*)we.data_ptr(), (float*)out.data_ptr(),
                     (int)M, (int)H, (int)E, (int)EG, (int)NG);
}

}  // namespace dnet
