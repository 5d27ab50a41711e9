// Flash-decode over the latent (absorbed) MLA KV cache, gfx950 only.
//
//   o_lat[b,h,:] = softmax(scale * (q_lat[b,h,:] . ckv[b,:len,:]^T
//                                   + q_pe[b,h,:] . kpe[b,:len,:]^T))
//                  @ ckv[b,:len,:]
//
// One KV "head" of width 576 = 512 latent + 64 rope is shared by every
// query head, and the value is the first 512 columns of the same row. The
// query heads are the 16-wide dimension of v_mfma_f32_16x16x32_bf16: one
// wave owns one 16-head tile, up to 4 tiles (64 heads) share a block and
// with it every staged chunk of the latent. (A wave needs 72 VGPRs of Q
// fragments and 128 of accumulator; 8 waves per block would cap it at 256
// registers and the compiler spills there, so more than 64 heads take a
// second block per batch row.)
//
// Data movement per 64-position chunk:
//   HBM -> LDS once, row-major [64][576] (pitch 584).
//   QK^T reads it as the A operand (positions are the M rows, 8 contiguous
//   d per lane), with the Q fragments, held in registers for the whole
//   kernel, as B: the MFMA yields S^T[pos][head], so a lane holds the
//   scores of ONE head (lane & 15) at positions hi*4 .. hi*4+3 of each
//   16-position tile (hi = lane >> 4). The softmax row reductions are
//   in-lane plus two xor-shuffles over hi, and two such tiles are already
//   the A operand of the PV product (8 k-slots per lane) without a trip
//   through LDS: k-slot hi*8+e stands for position (e/4)*16 + hi*4 + e%4
//   of the 32-position step.
//   PV reads the SAME row-major tile through the LDS transpose read
//   (ds_read_b64_tr_b16): within a 16-lane group lane j hands in the
//   address of 4 contiguous columns of row j/4 and lane i receives
//   column i of the four rows — 4 consecutive positions of one dv column.
//   Two reads (16 rows apart) make the bf16x8 B operand in the k-slot
//   order above. There is no transposed copy and no second global read.
//
// Few heads (1 or 2 tiles): two waves per tile, each owning 32 positions
// of every chunk with an independent online-softmax state, merged once at
// the end through the freed staging LDS.
//
// Split-S like attn_decode: grid (B * head-tile groups, splits); split y
// takes chunks y, y+splits, ... of ceil(len/64); partials go to
// [B, nh, splits, 512+2] f32 (max at [512], sum at [513]) and
// attn_combine<512> merges them in index order. splits == 1 normalises
// and stores bf16 directly. Rows >= len are never read.
#include "common.h"

namespace dnet {

void attn_combine(torch::Tensor partials, c10::optional<torch::Tensor> sinks,
                  torch::Tensor out, int64_t splits);

namespace {

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using i16x4 = __attribute__((ext_vector_type(4))) short;

constexpr int kLora = 512;            // latent width = value width
constexpr int kRope = 64;
constexpr int kRow = kLora + kRope;   // 576
constexpr int kPitch = kRow + 8;      // LDS row pitch, bf16 elems (292 dwords)
constexpr int kMlaChunk = 64;
constexpr int kDC = kRow / 32;        // 18 QK k-steps
constexpr int kNV = kLora / 16;       // 32 PV n-tiles
constexpr int kVecRow = kRow / 8;     // 72 16-byte vectors per row
constexpr int kStageBytes = kMlaChunk * kPitch * 2;   // 74752
constexpr int kMaxTiles = 4;          // head tiles per block

// 4 positions x 1 dv column out of a row-major LDS tile (see the header).
__device__ __forceinline__ i16x4 lds_read_tr16(const short* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) i16x4*)p);
}

// NT head tiles x PS position slices = NT * PS waves.
template <int NT, int PS>
__global__ __launch_bounds__(NT * PS * 64) void mla_decode_kernel(
    const short* __restrict__ q_lat, const short* __restrict__ q_pe,
    const short* __restrict__ ckv, const short* __restrict__ kpe,
    const int* __restrict__ lens, short* __restrict__ out,
    float* __restrict__ partials, const int nh, const int groups,
    const int S, const int64_t ckv_bs, const int64_t kpe_bs, const float scale,
    const int splits) {
  constexpr int NTHR = NT * PS * 64;
  constexpr int NP = kMlaChunk / PS;   // positions of a chunk per wave
  constexpr int NQ = NP / 16;          // score tiles per wave
  constexpr int NK = NP / 32;          // PV k-steps per wave
  extern __shared__ __attribute__((aligned(16))) char smem[];
  short* kv_lds = reinterpret_cast<short*>(smem);   // [64][kPitch]

  const int b = blockIdx.x / groups;
  const int grp = blockIdx.x % groups;
  const int split = blockIdx.y;
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int r = lane & 15;
  const int hi = lane >> 4;
  const int tile = wave / PS;
  const int ps = wave % PS;
  const int head0 = (grp * NT + tile) * 16;
  // a tile past nh (ragged last group) still stages and syncs; it
  // computes on a clamped head and stores nothing
  const int len = min(lens[b], S);   // never past the allocation

  // Q fragments: lane holds Q[head0 + r][cc*32 + hi*8 .. +8]; rows >= nh
  // duplicate head nh-1 (never stored, softmax is per head)
  const int qh = min(head0 + r, nh - 1);
  bf16x8 qf[kDC];
  {
    const short* ql = q_lat + ((int64_t)b * nh + qh) * kLora;
    const short* qp = q_pe + ((int64_t)b * nh + qh) * kRope;
#pragma unroll
    for (int cc = 0; cc < kLora / 32; ++cc)
      qf[cc] = *reinterpret_cast<const bf16x8*>(&ql[cc * 32 + hi * 8]);
#pragma unroll
    for (int cc = 0; cc < kRope / 32; ++cc)
      qf[kLora / 32 + cc] =
          *reinterpret_cast<const bf16x8*>(&qp[cc * 32 + hi * 8]);
  }

  f32x4 acc[kNV];   // O[head = head0 + hi*4 + j][dv = n*16 + r]
#pragma unroll
  for (int n = 0; n < kNV; ++n) acc[n] = {0.f, 0.f, 0.f, 0.f};
  float m_run = -1e30f;   // head head0 + r (same in the 4 lanes r + 16*hi)
  float l_run = 0.f;      // this lane's share; summed over hi at the end

  const short* ckv_b = ckv + (int64_t)b * ckv_bs;
  const short* kpe_b = kpe + (int64_t)b * kpe_bs;
  const int nchunks = (len + kMlaChunk - 1) / kMlaChunk;
  for (int c = split; c < nchunks; c += splits) {
    const int s0 = c * kMlaChunk;
    const int valid = min(kMlaChunk, len - s0);
    __syncthreads();   // previous chunk's readers are done
    // stage rows [s0, s0 + valid) of ckv | kpe; dead rows become zeros
    // (p = 0 times a NaN there would poison the accumulator)
    constexpr int NVEC = kMlaChunk * kVecRow;
    constexpr int U = 3;
#pragma unroll 1
    for (int i0 = threadIdx.x; i0 < NVEC; i0 += NTHR * U) {
      short8 t[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = i0 + u * NTHR;
        const int sr = i / kVecRow;
        const int col = (i % kVecRow) * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) t[u].x[j] = 0;
        if (i < NVEC && sr < valid) {
          const int64_t row = s0 + sr;
          t[u] = (col < kLora)
              ? *reinterpret_cast<const short8*>(&ckv_b[row * kLora + col])
              : *reinterpret_cast<const short8*>(
                    &kpe_b[row * kRope + col - kLora]);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = i0 + u * NTHR;
        if (i < NVEC)
          *reinterpret_cast<short8*>(
              &kv_lds[(i / kVecRow) * kPitch + (i % kVecRow) * 8]) = t[u];
      }
    }
    __syncthreads();

    const int pbase = ps * NP;
    if (pbase >= valid) continue;   // wave-uniform: nothing live in my slice

    // S^T[pos][head]: sc[t][j] = score(pos pbase + t*16 + hi*4 + j, head r)
    f32x4 sc[NQ];
#pragma unroll
    for (int t = 0; t < NQ; ++t) {
      sc[t] = {0.f, 0.f, 0.f, 0.f};
      const short* krow = &kv_lds[(pbase + t * 16 + r) * kPitch + hi * 8];
#pragma unroll
      for (int cc = 0; cc < kDC; ++cc) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(&krow[cc * 32]);
        sc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[cc], sc[t], 0,
                                                        0, 0);
        // keep the scheduler from hoisting every LDS read of the unrolled
        // loop to the top: it costs registers and buys nothing
        if (cc % 6 == 5) __builtin_amdgcn_sched_barrier(0);
      }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < NQ; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool dead = pbase + t * 16 + hi * 4 + j >= valid;
        sc[t][j] = dead ? -INFINITY : sc[t][j] * scale;
        mx = fmaxf(mx, sc[t][j]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mn = fmaxf(m_run, mx);   // finite: position pbase is live
    const float corr = __expf(m_run - mn);
    m_run = mn;
    float ls = 0.f;
#pragma unroll
    for (int t = 0; t < NQ; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sc[t][j] = __expf(sc[t][j] - mn);   // -inf -> exactly 0
        ls += sc[t][j];
      }
    l_run = l_run * corr + ls;
    // the accumulator rows are heads hi*4 + j: fetch their factors
    float cj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) cj[j] = __shfl(corr, hi * 4 + j, 64);
#pragma unroll
    for (int n = 0; n < kNV; ++n)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[n][j] *= cj[j];

#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
      union { bf16x8 v; short s[8]; } pf;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        pf.s[j] = f2bits(sc[2 * ks][j]);
        pf.s[4 + j] = f2bits(sc[2 * ks + 1][j]);
      }
      // lane j of a 16-group: row hi*4 + j/4, columns (j%4)*4 .. +4
      const short* vp = &kv_lds[(pbase + ks * 32 + hi * 4 + (r >> 2)) * kPitch
                                + (r & 3) * 4];
#pragma unroll
      for (int n = 0; n < kNV; ++n) {
        union { bf16x8 v; i16x4 h[2]; } vf;
        vf.h[0] = lds_read_tr16(vp + n * 16);
        vf.h[1] = lds_read_tr16(vp + 16 * kPitch + n * 16);
        acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf.v, vf.v, acc[n],
                                                         0, 0, 0);
        if (n % 4 == 3) __builtin_amdgcn_sched_barrier(0);
      }
    }
  }

  l_run += __shfl_xor(l_run, 16, 64);
  l_run += __shfl_xor(l_run, 32, 64);

  if (PS > 1) {
    // merge the two position slices of a tile: slice 1 parks its state in
    // the staging LDS, slice 0 folds it in
    static_assert(PS <= 2, "merge is written for two slices");
    static_assert(PS == 1 || NT * (16 * kLora + 32) * 4 <= kStageBytes,
                  "merge area must fit in the staging LDS");
    float* mrg = reinterpret_cast<float*>(smem) + tile * (16 * kLora + 32);
    float* mml = mrg + 16 * kLora;
    __syncthreads();
    if (ps == 1) {
#pragma unroll
      for (int n = 0; n < kNV; ++n)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          mrg[(hi * 4 + j) * kLora + n * 16 + r] = acc[n][j];
      if (hi == 0) {
        mml[r] = m_run;
        mml[16 + r] = l_run;
      }
    }
    __syncthreads();
    if (ps == 1) return;
    const float m1 = mml[r], l1 = mml[16 + r];
    const float M = fmaxf(m_run, m1);
    const float w0 = __expf(m_run - M), w1 = __expf(m1 - M);
    l_run = l_run * w0 + l1 * w1;
    m_run = M;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float a0 = __shfl(w0, hi * 4 + j, 64);
      const float a1 = __shfl(w1, hi * 4 + j, 64);
#pragma unroll
      for (int n = 0; n < kNV; ++n)
        acc[n][j] = acc[n][j] * a0
                    + mrg[(hi * 4 + j) * kLora + n * 16 + r] * a1;
    }
  }

  if (partials != nullptr) {
    if (hi == 0 && head0 + r < nh) {
      float* prow = partials
          + (((int64_t)b * nh + head0 + r) * splits + split) * (kLora + 2);
      prow[kLora] = m_run;
      prow[kLora + 1] = l_run;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int head = head0 + hi * 4 + j;
      if (head >= nh) continue;
      float* prow = partials
          + (((int64_t)b * nh + head) * splits + split) * (kLora + 2);
#pragma unroll
      for (int n = 0; n < kNV; ++n) prow[n * 16 + r] = acc[n][j];
    }
    return;
  }
  const float inv = (l_run > 0.f) ? 1.f / l_run : 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float ij = __shfl(inv, hi * 4 + j, 64);
    const int head = head0 + hi * 4 + j;
    if (head >= nh) continue;
    short* orow = out + ((int64_t)b * nh + head) * kLora;
#pragma unroll
    for (int n = 0; n < kNV; ++n) orow[n * 16 + r] = f2bits(acc[n][j] * ij);
  }
}

template <int NT, int PS>
void launch(dim3 grid, hipStream_t stream, const short* q_lat,
            const short* q_pe, const short* ckv, const short* kpe,
            const int* lens, short* out, float* partials, int nh, int groups,
            int S, int64_t ckv_bs, int64_t kpe_bs, float scale, int splits) {
  // 73 KB of dynamic LDS: above the 64 KB default, below the CU's 160 KB
  static const bool raised = []() {
    DNET_CHECK_HIP(hipFuncSetAttribute(
        reinterpret_cast<const void*>(&mla_decode_kernel<NT, PS>),
        hipFuncAttributeMaxDynamicSharedMemorySize, kStageBytes));
    return true;
  }();
  (void)raised;
  hipLaunchKernelGGL((mla_decode_kernel<NT, PS>), grid, dim3(NT * PS * 64),
                     kStageBytes, stream, q_lat, q_pe, ckv, kpe, lens, out,
                     partials, nh, groups, S, ckv_bs, kpe_bs, scale, splits);
}

}  // namespace

// q_lat [B,nh,512], q_pe [B,nh,64] contiguous bf16; ckv [B,S,512],
// kpe [B,S,64] bf16 with contiguous rows and any batch stride; lens [B]
// int32; out [B,nh,512] bf16. splits > 1 needs partials of
// B*nh*splits*514 f32 and finishes with attn_combine.
void mla_decode(torch::Tensor q_lat, torch::Tensor q_pe, torch::Tensor ckv,
                torch::Tensor kpe, torch::Tensor lens, torch::Tensor out,
                double scale, c10::optional<torch::Tensor> partials,
                int64_t splits) {
  const int64_t B = q_lat.size(0), nh = q_lat.size(1);
  DNET_CHECK(q_lat.dim() == 3 && q_lat.size(2) == kLora && q_pe.dim() == 3
                 && q_pe.size(0) == B && q_pe.size(1) == nh
                 && q_pe.size(2) == kRope, "q_lat [B,nh,512], q_pe [B,nh,64]");
  DNET_CHECK(ckv.dim() == 3 && ckv.size(0) == B && ckv.size(2) == kLora
                 && kpe.dim() == 3 && kpe.size(0) == B
                 && kpe.size(1) == ckv.size(1) && kpe.size(2) == kRope,
             "ckv [B,S,512], kpe [B,S,64]");
  DNET_CHECK(q_lat.dtype() == torch::kBFloat16
                 && q_pe.dtype() == torch::kBFloat16
                 && ckv.dtype() == torch::kBFloat16
                 && kpe.dtype() == torch::kBFloat16
                 && out.dtype() == torch::kBFloat16, "bf16 tensors");
  DNET_CHECK(q_lat.is_contiguous() && q_pe.is_contiguous()
                 && out.is_contiguous(), "q/out contiguous");
  DNET_CHECK(ckv.stride(2) == 1 && ckv.stride(1) == kLora
                 && kpe.stride(2) == 1 && kpe.stride(1) == kRope,
             "cache rows contiguous");
  DNET_CHECK(ckv.stride(0) % 8 == 0 && kpe.stride(0) % 8 == 0,
             "cache batch stride 16-byte aligned");
  DNET_CHECK(lens.dtype() == torch::kInt32 && lens.numel() == B
                 && lens.is_contiguous(), "lens [B] int32");
  DNET_CHECK(out.size(0) == B && out.size(1) == nh && out.size(2) == kLora,
             "out [B,nh,512]");
  DNET_CHECK(nh >= 1 && splits >= 1 && splits <= 65535, "nh, splits");
  if (B == 0) return;
  float* pp = nullptr;
  if (splits > 1) {
    DNET_CHECK(partials.has_value()
                   && partials->dtype() == torch::kFloat32
                   && partials->is_contiguous()
                   && partials->numel() >= B * nh * splits * (kLora + 2),
               "split-S partials scratch required");
    pp = (float*)partials->data_ptr();
  }
  const int tiles = cdiv(nh, 16);
  const int groups = cdiv(tiles, kMaxTiles);
  const int nt = cdiv(tiles, groups);   // balanced: 5 tiles -> 3 + 2
  const dim3 grid((unsigned)(B * groups), (unsigned)splits);
  auto stream = current_stream();
#define MLA_LAUNCH(NT, PS)                                                   \
  launch<NT, PS>(grid, stream, (const short*)q_lat.data_ptr(),               \
                 (const short*)q_pe.data_ptr(), (const short*)ckv.data_ptr(),\
                 (const short*)kpe.data_ptr(), (const int*)lens.data_ptr(),  \
                 (short*)out.data_ptr(), pp, (int)nh, groups,                \
                 (int)ckv.size(1), ckv.stride(0), kpe.stride(0),             \
                 (float)scale, (int)splits)
  switch (nt) {
    case 1: MLA_LAUNCH(1, 2); break;
    case 2: MLA_LAUNCH(2, 2); break;
    case 3: MLA_LAUNCH(3, 1); break;
    default: MLA_LAUNCH(4, 1); break;
  }
#undef MLA_LAUNCH
  if (splits > 1) attn_combine(*partials, c10::nullopt, out, splits);
}

}  // namespace dnet
