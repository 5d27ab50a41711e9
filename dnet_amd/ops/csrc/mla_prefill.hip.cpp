// Flash-prefill over the latent (absorbed) MLA KV cache, gfx950 only.
//
//   o_lat[b,t,h,:] = softmax(scale * (q_lat[b,t,h,:] . ckv[b,:n,:]^T
//                                     + q_pe[b,t,h,:] . kpe[b,:n,:]^T))
//                    @ ckv[b,:n,:]            n = q_off + t + 1
//
// A continuation chunk in absorbed form is the decode problem with more
// rows: all T x nh query rows of a batch entry attend one shared 576-wide
// stream (512 latent + 64 rope) whose first 512 columns are the value.
// mla_decode gives every 16-head tile a block and a staged copy of its
// own; here the query rows of several tokens share one block, so a staged
// chunk feeds up to 64 MFMA rows whatever the head count.
//
// Work split
//   The 16-wide dimension of v_mfma_f32_16x16x32_bf16 is 16 heads of ONE
//   token, so the causal bound n is wave-uniform. Work items are (token,
//   head tile) pairs, token-major; a block takes 4 consecutive items, one
//   wave each: 4 consecutive tokens with 16 heads, 4 head tiles of one
//   token with 128 heads, a mix in between (40 heads: 3 tiles, a block
//   spans two tokens). Heads past nh are clamped to nh-1 and never stored.
//   Grid (B * item groups, splits).
//
// Few items (T * ceil(nh/16) < 4, e.g. T = 1, nh = 16): the block still
//   has 4 waves and the ones without an item only stage. Decode's
//   arrangement (two position slices per tile, merged at the end) needs
//   the same 72 Q + 128 accumulator registers per wave, so it frees
//   nothing; the idle waves keep the staging at 256 threads and the kernel
//   at one instantiation. T = 1 belongs to mla_decode anyway.
//
// Data movement per 64-position chunk (as in mla_decode.hip.cpp, whose
// header explains the fragment layouts and why 8 waves per block spill):
//   HBM -> LDS once, row-major [64][576], pitch 584. QK^T reads it as the
//   A operand against the Q fragments, held in registers for the whole
//   kernel: S^T[pos][head], a lane holds one head's scores at 4 positions
//   of each 16-position tile, and two such tiles are the A operand of PV
//   without a trip through LDS. PV reads the SAME tile through the LDS
//   transpose read (ds_read_b64_tr_b16). No transposed copy, no second
//   global read.
//
// Chunk loop: to the block's largest n. Rows at or past it are staged as
//   zeros (0 x NaN would poison the accumulator) and rows >= q_off + T
//   are never read. A wave whose item has n <= s0 stages, takes the
//   barriers and skips the math: its running max and sum stay untouched.
//   Positions in [n, s0 + 64) are masked to -inf per item.
//
// Split-S: split y takes chunks y, y + splits, ...; partials go to
//   [B, T, nh, splits, 514] f32 (max at [512], sum at [513]), decode's
//   layout over B*T rows, merged by attn_combine<512> in index order. An
//   item with no chunk in a split writes the empty state (max -1e30, sum
//   0, zeros). splits == 1 normalises and stores bf16 directly.
#include "common.h"

namespace dnet {

void attn_combine(torch::Tensor partials, c10::optional<torch::Tensor> sinks,
                  torch::Tensor out, int64_t splits);

namespace {

using i16x4 = __attribute__((ext_vector_type(4))) short;

constexpr int kLora = 512;            // latent width = value width
constexpr int kRope = 64;
constexpr int kRow = kLora + kRope;   // 576
constexpr int kPitch = kRow + 8;      // LDS row pitch, bf16 elems (292 dwords)
constexpr int kChunk = 64;
constexpr int kDC = kRow / 32;        // 18 QK k-steps
constexpr int kNV = kLora / 16;       // 32 PV n-tiles
constexpr int kVecRow = kRow / 8;     // 72 16-byte vectors per row
constexpr int kStageBytes = kChunk * kPitch * 2;   // 74752
constexpr int kItems = 4;             // items (waves) per block
constexpr int kThreads = kItems * 64;
constexpr int kNQ = kChunk / 16;      // score tiles per chunk
constexpr int kNK = kChunk / 32;      // PV k-steps per chunk

// 4 positions x 1 dv column out of a row-major LDS tile: within a 16-lane
// group lane j hands in the address of 4 contiguous columns of row j/4 and
// lane i receives column i of the four rows.
__device__ __forceinline__ i16x4 lds_read_tr16(const short* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) i16x4*)p);
}

__global__ __launch_bounds__(kThreads) void mla_prefill_kernel(
    const short* __restrict__ q_lat, const short* __restrict__ q_pe,
    const short* __restrict__ ckv, const short* __restrict__ kpe,
    short* __restrict__ out, float* __restrict__ partials, const int T,
    const int nh, const int tiles, const int groups, const int q_off,
    const int64_t ckv_bs, const int64_t kpe_bs, const float scale,
    const int splits) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  short* kv_lds = reinterpret_cast<short*>(smem);   // [64][kPitch]

  const int b = blockIdx.x / groups;
  const int grp = blockIdx.x % groups;
  const int split = blockIdx.y;
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int r = lane & 15;
  const int hi = lane >> 4;

  const int nitems = T * tiles;
  const int item = grp * kItems + wave;
  const bool live = item < nitems;          // wave-uniform
  const int it = min(item, nitems - 1);     // idle waves load a valid Q
  const int t = it / tiles;
  const int head0 = (it % tiles) * 16;
  const int n = live ? q_off + t + 1 : 0;   // idle: every chunk is skipped
  // items are token-major, so the block's last live item has its largest n
  const int n_max = q_off + min(grp * kItems + kItems - 1, nitems - 1) / tiles
                    + 1;

  // Q fragments: lane holds Q[head0 + r][cc*32 + hi*8 .. +8]; rows >= nh
  // duplicate head nh-1 (never stored, softmax is per head)
  const int qh = min(head0 + r, nh - 1);
  const int64_t qrow = ((int64_t)b * T + t) * nh;
  bf16x8 qf[kDC];
  {
    const short* ql = q_lat + (qrow + qh) * kLora;
    const short* qp = q_pe + (qrow + qh) * kRope;
#pragma unroll
    for (int cc = 0; cc < kLora / 32; ++cc)
      qf[cc] = *reinterpret_cast<const bf16x8*>(&ql[cc * 32 + hi * 8]);
#pragma unroll
    for (int cc = 0; cc < kRope / 32; ++cc)
      qf[kLora / 32 + cc] =
          *reinterpret_cast<const bf16x8*>(&qp[cc * 32 + hi * 8]);
  }

  f32x4 acc[kNV];   // O[head = head0 + hi*4 + j][dv = nn*16 + r]
#pragma unroll
  for (int nn = 0; nn < kNV; ++nn) acc[nn] = {0.f, 0.f, 0.f, 0.f};
  float m_run = -1e30f;   // head head0 + r (same in the 4 lanes r + 16*hi)
  float l_run = 0.f;      // this lane's share; summed over hi at the end

  const short* ckv_b = ckv + (int64_t)b * ckv_bs;
  const short* kpe_b = kpe + (int64_t)b * kpe_bs;
  const int nchunks = (n_max + kChunk - 1) / kChunk;   // block-uniform
  for (int c = split; c < nchunks; c += splits) {
    const int s0 = c * kChunk;
    const int valid = min(kChunk, n_max - s0);
    __syncthreads();   // previous chunk's readers are done
    // stage rows [s0, s0 + valid) of ckv | kpe; the rest become zeros
    constexpr int NVEC = kChunk * kVecRow;
    constexpr int U = 3;
    static_assert(NVEC % (kThreads * U) == 0, "staging covers the tile");
#pragma unroll 1
    for (int i0 = threadIdx.x; i0 < NVEC; i0 += kThreads * U) {
      short8 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = i0 + u * kThreads;
        const int sr = i / kVecRow;
        const int col = (i % kVecRow) * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[u].x[j] = 0;
        if (sr < valid) {
          const int64_t row = s0 + sr;
          v[u] = (col < kLora)
              ? *reinterpret_cast<const short8*>(&ckv_b[row * kLora + col])
              : *reinterpret_cast<const short8*>(
                    &kpe_b[row * kRope + col - kLora]);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = i0 + u * kThreads;
        *reinterpret_cast<short8*>(
            &kv_lds[(i / kVecRow) * kPitch + (i % kVecRow) * 8]) = v[u];
      }
    }
    __syncthreads();

    if (n <= s0) continue;   // wave-uniform: my item ends before this chunk

    // S^T[pos][head]: sc[q][j] = score(pos s0 + q*16 + hi*4 + j, head r)
    f32x4 sc[kNQ];
#pragma unroll
    for (int q = 0; q < kNQ; ++q) {
      sc[q] = {0.f, 0.f, 0.f, 0.f};
      const short* krow = &kv_lds[(q * 16 + r) * kPitch + hi * 8];
#pragma unroll
      for (int cc = 0; cc < kDC; ++cc) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(&krow[cc * 32]);
        sc[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[cc], sc[q], 0,
                                                        0, 0);
        // keep the scheduler from hoisting every LDS read of the unrolled
        // loop to the top: it costs registers and buys nothing
        if (cc % 6 == 5) __builtin_amdgcn_sched_barrier(0);
      }
    }
    const int nloc = n - s0;   // >= 1: position s0 is live
    float mx = -INFINITY;
#pragma unroll
    for (int q = 0; q < kNQ; ++q)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool dead = q * 16 + hi * 4 + j >= nloc;
        sc[q][j] = dead ? -INFINITY : sc[q][j] * scale;
        mx = fmaxf(mx, sc[q][j]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mn = fmaxf(m_run, mx);   // finite
    const float corr = __expf(m_run - mn);
    m_run = mn;
    float ls = 0.f;
#pragma unroll
    for (int q = 0; q < kNQ; ++q)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sc[q][j] = __expf(sc[q][j] - mn);   // -inf -> exactly 0
        ls += sc[q][j];
      }
    l_run = l_run * corr + ls;
    // the accumulator rows are heads hi*4 + j: fetch their factors
    float cj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) cj[j] = __shfl(corr, hi * 4 + j, 64);
#pragma unroll
    for (int nn = 0; nn < kNV; ++nn)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[nn][j] *= cj[j];

#pragma unroll
    for (int ks = 0; ks < kNK; ++ks) {
      // k-slot hi*8 + e stands for position (e/4)*16 + hi*4 + e%4 of the
      // 32-position step, in P and in V alike
      union { bf16x8 v; short s[8]; } pf;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        pf.s[j] = f2bits(sc[2 * ks][j]);
        pf.s[4 + j] = f2bits(sc[2 * ks + 1][j]);
      }
      // lane j of a 16-group: row hi*4 + j/4, columns (j%4)*4 .. +4
      const short* vp = &kv_lds[(ks * 32 + hi * 4 + (r >> 2)) * kPitch
                                + (r & 3) * 4];
#pragma unroll
      for (int nn = 0; nn < kNV; ++nn) {
        union { bf16x8 v; i16x4 h[2]; } vf;
        vf.h[0] = lds_read_tr16(vp + nn * 16);
        vf.h[1] = lds_read_tr16(vp + 16 * kPitch + nn * 16);
        acc[nn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf.v, vf.v, acc[nn],
                                                          0, 0, 0);
        if (nn % 4 == 3) __builtin_amdgcn_sched_barrier(0);
      }
    }
  }

  if (!live) return;
  l_run += __shfl_xor(l_run, 16, 64);
  l_run += __shfl_xor(l_run, 32, 64);

  if (partials != nullptr) {
    if (hi == 0 && head0 + r < nh) {
      float* prow = partials
          + ((qrow + head0 + r) * splits + split) * (kLora + 2);
      prow[kLora] = m_run;
      prow[kLora + 1] = l_run;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int head = head0 + hi * 4 + j;
      if (head >= nh) continue;
      float* prow = partials + ((qrow + head) * splits + split) * (kLora + 2);
#pragma unroll
      for (int nn = 0; nn < kNV; ++nn) prow[nn * 16 + r] = acc[nn][j];
    }
    return;
  }
  const float inv = (l_run > 0.f) ? 1.f / l_run : 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float ij = __shfl(inv, hi * 4 + j, 64);
    const int head = head0 + hi * 4 + j;
    if (head >= nh) continue;
    short* orow = out + (qrow + head) * kLora;
#pragma unroll
    for (int nn = 0; nn < kNV; ++nn)
      orow[nn * 16 + r] = f2bits(acc[nn][j] * ij);
  }
}

}  // namespace

// q_lat [B,T,nh,512], q_pe [B,T,nh,64] contiguous bf16; ckv [B,S,512],
// kpe [B,S,64] bf16 with contiguous rows and any 16-byte-aligned batch
// stride; out [B,T,nh,512] bf16; token t attends rows [0, q_off + t + 1).
// splits > 1 needs partials of B*T*nh*splits*514 f32 and finishes with
// attn_combine.
void mla_prefill(torch::Tensor q_lat, torch::Tensor q_pe, torch::Tensor ckv,
                 torch::Tensor kpe, torch::Tensor out, int64_t q_off,
                 double scale, c10::optional<torch::Tensor> partials,
                 int64_t splits) {
  DNET_CHECK(q_lat.dim() == 4 && q_pe.dim() == 4, "q_lat, q_pe 4-d");
  const int64_t B = q_lat.size(0), T = q_lat.size(1), nh = q_lat.size(2);
  DNET_CHECK(q_lat.size(3) == kLora && q_pe.size(0) == B && q_pe.size(1) == T
                 && q_pe.size(2) == nh && q_pe.size(3) == kRope,
             "q_lat [B,T,nh,512], q_pe [B,T,nh,64]");
  DNET_CHECK(ckv.dim() == 3 && ckv.size(0) == B && ckv.size(2) == kLora
                 && kpe.dim() == 3 && kpe.size(0) == B
                 && kpe.size(1) == ckv.size(1) && kpe.size(2) == kRope,
             "ckv [B,S,512], kpe [B,S,64]");
  DNET_CHECK(q_lat.dtype() == torch::kBFloat16
                 && q_pe.dtype() == torch::kBFloat16
                 && ckv.dtype() == torch::kBFloat16
                 && kpe.dtype() == torch::kBFloat16
                 && out.dtype() == torch::kBFloat16, "bf16 tensors");
  DNET_CHECK(q_lat.is_cuda() && q_pe.is_cuda() && ckv.is_cuda()
                 && kpe.is_cuda() && out.is_cuda(), "device tensors");
  DNET_CHECK(q_lat.is_contiguous() && q_pe.is_contiguous()
                 && out.is_contiguous(), "q/out contiguous");
  DNET_CHECK(ckv.stride(2) == 1 && ckv.stride(1) == kLora
                 && kpe.stride(2) == 1 && kpe.stride(1) == kRope,
             "cache rows contiguous");
  DNET_CHECK(ckv.stride(0) % 8 == 0 && kpe.stride(0) % 8 == 0,
             "cache batch stride 16-byte aligned");
  DNET_CHECK(out.dim() == 4 && out.size(0) == B && out.size(1) == T
                 && out.size(2) == nh && out.size(3) == kLora,
             "out [B,T,nh,512]");
  DNET_CHECK(nh >= 1 && splits >= 1 && splits <= 65535, "nh, splits");
  DNET_CHECK(q_off >= 0 && q_off + T <= ckv.size(1),
             "q_off + T within the cache");
  if (B == 0 || T == 0) return;
  float* pp = nullptr;
  if (splits > 1) {
    DNET_CHECK(partials.has_value()
                   && partials->dtype() == torch::kFloat32
                   && partials->is_cuda() && partials->is_contiguous()
                   && partials->numel() >= B * T * nh * splits * (kLora + 2),
               "split-S partials scratch required");
    pp = (float*)partials->data_ptr();
  }
  const int tiles = cdiv(nh, 16);
  const int64_t groups = (T * tiles + kItems - 1) / kItems;
  DNET_CHECK(B * groups < (int64_t)1 << 31, "grid too large");
  // 73 KB of dynamic LDS: above the 64 KB default, below the CU's 160 KB
  static const bool raised = []() {
    DNET_CHECK_HIP(hipFuncSetAttribute(
        reinterpret_cast<const void*>(&mla_prefill_kernel),
        hipFuncAttributeMaxDynamicSharedMemorySize, kStageBytes));
    return true;
  }();
  (void)raised;
  hipLaunchKernelGGL(mla_prefill_kernel,
                     dim3((unsigned)(B * groups), (unsigned)splits),
                     dim3(kThreads), kStageBytes, current_stream(),
                     (const short*)q_lat.data_ptr(),
                     (const short*)q_pe.data_ptr(),
                     (const short*)ckv.data_ptr(),
                     (const short*)kpe.data_ptr(), (short*)out.data_ptr(), pp,
                     (int)T, (int)nh, tiles, (int)groups, (int)q_off,
                     ckv.stride(0), kpe.stride(0), (float)scale, (int)splits);
  if (splits > 1)
    attn_combine(*partials, c10::nullopt, out.view({B * T, nh, kLora}),
                 splits);
}

}  // namespace dnet
