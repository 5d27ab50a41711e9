// MFMA decode GEMM: out[M,N] = x[M,K] @ W[N,K]^T (+bias), M <= 64 per pass.
//
// The scalar GEMV (gemv.hip.cpp) is VALU-bound at M>=4: every weight element
// costs ~2 VALU ops per output row. Here one v_mfma_f32_16x16x32_bf16
// covers a 16(M)x16(N)x32(K) tile; MT in {1,2,4} stacks up to 4 M-tiles per
// wave so ONE weight read (and for int8 ONE in-register dequant) serves up
// to 64 batch rows — decode batching at constant weight traffic. Fragment
// layout for 16x16x32 (cdna_hip_programming.md §3): lane l holds
// A[row=l&15][k=(l>>4)*8+j], B[col=l&15][k=(l>>4)*8+j],
// C[col=l&15][row=(l>>4)*4+r].
//
// x is staged tile-wise into LDS with coalesced full-line loads (direct
// fragment-shaped x reads touch 16 scattered rows per instruction, up to
// +45% — guide §5 M=256 GEMM row). int8 weights use the chunk-pair packed
// layout (pack_int8_mfma) so each lane loads 16 B contiguous (full 64 B
// HBM bursts).
//
// Wave tile: 16 N-columns; block = 4 waves = 64 columns; gridDim.y = SPLITK
// K-splits. Split s stores its whole [M,N] f32 tile with plain stores into
// slice s of a partials buffer laid out [sk][M][N]; whoever reads the
// result (the convert/bias kernel, or the fused rope / rmsnorm / resid-add
// / swiglu consumers) sums slices 0..sk-1 in that fixed order. No atomics,
// nothing to zero beforehand, and two launches give the same bits.
#include "common.h"

namespace dnet {

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ bf16x8 deq8(const int8_t* q, const float s) {
  bf16x8 b;
#pragma unroll
  for (int j = 0; j < 8; ++j) b[j] = (__bf16)((float)q[j] * s);
  return b;
}

// 4 packed nibble-bytes (offset-8) -> 8 bf16 values * scale
__device__ __forceinline__ bf16x8 deq4(const uint8_t* qb, const float s) {
  bf16x8 b;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int byte = qb[j];
    b[2 * j] = (__bf16)((float)((byte & 0xF) - 8) * s);
    b[2 * j + 1] = (__bf16)((float)((byte >> 4) - 8) * s);
  }
  return b;
}

// Opt-in reproducible split-k (set_splitk_exact, OFF by default; the
// default path stores the raw f32 partials). When on, every partial is
// rounded to a fixed 2^-16 grid before it is stored. Sums of grid values
// stay exactly representable in f32 while their magnitude is below 2^8, so
// the additions are exact and the total does not depend on the order in
// which the partials are added. The slices are summed in a fixed order, so
// the default path is run-to-run reproducible too; this mode additionally
// keeps the bits of builds that combined the splits in arrival order
// (f32 atomics). The price is an absolute precision floor: each
// partial carries up to 2^-17 of rounding error and one below 2^-17 is
// flushed to zero, so the mode is meant for O(1) activations (synthetic
// benchmark runs), not for general use. Sums beyond 2^8 are still correct
// but no longer order-independent; magnitudes from 2^7 up pass unchanged.
__device__ __forceinline__ float splitk_grid(const float v) {
  return rintf(v * 65536.0f) * (1.0f / 65536.0f);
}

// QBITS: 16 = bf16 weights, 8 = packed int8 (pack_int8_mfma chunk-pair
// layout), 4 = packed int4 (pack_int4_mfma chunk-quad layout).
// MT: number of stacked 16-row A tiles (M <= 16*MT).
template <int QBITS, int MT>
__global__ void gemm_m16_kernel(const short* __restrict__ x,
                                const void* __restrict__ w,
                                const short* __restrict__ scales,
                                const short* __restrict__ bias,
                                short* __restrict__ out,        // SPLITK==1
                                float* __restrict__ out_f32,    // SPLITK>1
                                const int M, const int K, const int N,
                                const int G, const int splitk,
                                const int exact) {
  constexpr int XT = 1024 / MT;        // k per x tile (LDS ~33 KB, 4 blocks/CU)
  constexpr int SE = XT + 8;           // row stride in bf16 elems (16B pad)
  __shared__ short x_lds[16 * MT * SE];
  const int wave = threadIdx.x / kWave;
  const int lane = threadIdx.x & (kWave - 1);
  const int n0 = (blockIdx.x * 4 + wave) * 16;
  // Block-wide barriers: OOB waves must stay alive; their stores are
  // skipped at the end.
  const int row = lane & 15;          // A row within a tile, B col
  const int ks = (lane >> 4) * 8;     // k-offset of this lane's 8-elem slice
  const int n_w = min(n0 + row, N - 1);     // this lane's W row

  const int pairs = K / 64;
  int p_begin, p_end;
  if (QBITS == 4) {
    // partition at quad (128-k) granularity so every split starts on an
    // even pair (the int4 layout packs four chunks per lane load)
    const int quads = K / 128;
    const int qq = quads / splitk;
    p_begin = blockIdx.y * qq * 2;
    p_end = (blockIdx.y == splitk - 1) ? quads * 2 : p_begin + qq * 2;
  } else {
    const int pp = pairs / splitk;
    p_begin = blockIdx.y * pp;
    p_end = (blockIdx.y == splitk - 1) ? pairs : p_begin + pp;
  }
  const int woff = (lane >> 4) * 16;

  f32x4 acc[MT][2];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int u = 0; u < 2; ++u) acc[t][u] = {0.f, 0.f, 0.f, 0.f};

  const int8_t* wrow_q = (const int8_t*)w + (int64_t)n_w * K;
  const uint8_t* wrow_q4 = (const uint8_t*)w + (int64_t)n_w * (K / 2);
  const short* wrow_b = (const short*)w + (int64_t)n_w * K;
  const short* srow = QBITS < 16 ? scales + (int64_t)n_w * (K / G) : nullptr;

  for (int k0 = p_begin * 64; k0 < p_end * 64; k0 += XT) {
    const int tk = min(XT, p_end * 64 - k0);
    // raw barrier (lgkmcnt only): __syncthreads() would wait vmcnt(0) and
    // drain the in-flight weight stream at EVERY x-tile boundary — at MT=4
    // (XT=256) that is a full memory-pipeline restart every 4 pairs
    // (guide §6: counted waits, not vmcnt(0), across barriers)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    asm volatile("s_barrier" ::: "memory");
    for (int idx = threadIdx.x; idx < 16 * MT * (tk / 8); idx += 256) {
      const int r = idx / (tk / 8);
      const int vec = idx % (tk / 8);
      // rows >= M read a clamped row; their C rows are never stored
      *reinterpret_cast<short8*>(&x_lds[r * SE + vec * 8]) =
          *reinterpret_cast<const short8*>(
              &x[(int64_t)min(r, M - 1) * K + k0 + vec * 8]);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    asm volatile("s_barrier" ::: "memory");
    const short* arow = &x_lds[row * SE];
    int pl = 0;
    const int pl_end = tk / 64;
    for (; pl + 4 <= pl_end; pl += 4) {  // 4 pairs, all weight loads first
      int4 wq8[4];
      int4 wq4[2];
      bf16x8 wb[4][2];
      float sv[4];
      if (QBITS == 8) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int p = (k0 / 64) + pl + u;
          wq8[u] = *reinterpret_cast<const int4*>(&wrow_q[p * 64 + woff]);
          sv[u] = bits2f(srow[(p * 64) / G]);
        }
      } else if (QBITS == 4) {
#pragma unroll
        for (int v = 0; v < 2; ++v) {
          const int quad = ((k0 / 64) + pl) / 2 + v;
          wq4[v] = *reinterpret_cast<const int4*>(&wrow_q4[quad * 64 + woff]);
          sv[v] = bits2f(srow[(quad * 128) / G]);
        }
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int p = (k0 / 64) + pl + u;
          wb[u][0] = *reinterpret_cast<const bf16x8*>(&wrow_b[p * 64 + ks]);
          wb[u][1] = *reinterpret_cast<const bf16x8*>(
              &wrow_b[p * 64 + 32 + ks]);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        bf16x8 b0, b1;
        if (QBITS == 8) {
          const int8_t* q8 = reinterpret_cast<const int8_t*>(&wq8[u]);
          b0 = deq8(q8, sv[u]);
          b1 = deq8(q8 + 8, sv[u]);
        } else if (QBITS == 4) {
          const uint8_t* q4 =
              reinterpret_cast<const uint8_t*>(&wq4[u / 2]) + (u & 1) * 8;
          b0 = deq4(q4, sv[u / 2]);
          b1 = deq4(q4 + 4, sv[u / 2]);
        } else {
          b0 = wb[u][0];
          b1 = wb[u][1];
        }
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          const short* at = arow + t * 16 * SE;
          const bf16x8 a0 =
              *reinterpret_cast<const bf16x8*>(&at[(pl + u) * 64 + ks]);
          const bf16x8 a1 =
              *reinterpret_cast<const bf16x8*>(&at[(pl + u) * 64 + 32 + ks]);
          acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a0, b0, acc[t][0], 0, 0, 0);
          acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a1, b1, acc[t][1], 0, 0, 0);
        }
      }
    }
    for (; pl < pl_end; ++pl) {
      const int p = (k0 / 64) + pl;
      bf16x8 b0, b1;
      if (QBITS == 8) {
        const int4 wq = *reinterpret_cast<const int4*>(&wrow_q[p * 64 + woff]);
        const int8_t* q8 = reinterpret_cast<const int8_t*>(&wq);
        const float sv = bits2f(srow[(p * 64) / G]);
        b0 = deq8(q8, sv);
        b1 = deq8(q8 + 8, sv);
      } else if (QBITS == 4) {
        const int quad = p / 2;
        const int half = p & 1;
        const int2 wq = *reinterpret_cast<const int2*>(
            &wrow_q4[quad * 64 + woff + half * 8]);
        const uint8_t* q4 = reinterpret_cast<const uint8_t*>(&wq);
        const float sv = bits2f(srow[(quad * 128) / G]);
        b0 = deq4(q4, sv);
        b1 = deq4(q4 + 4, sv);
      } else {
        b0 = *reinterpret_cast<const bf16x8*>(&wrow_b[p * 64 + ks]);
        b1 = *reinterpret_cast<const bf16x8*>(&wrow_b[p * 64 + 32 + ks]);
      }
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const short* at = arow + t * 16 * SE;
        const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(&at[pl * 64 + ks]);
        const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(&at[pl * 64 + 32 + ks]);
        acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, acc[t][0],
                                                            0, 0, 0);
        acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1, acc[t][1],
                                                            0, 0, 0);
      }
    }
  }

  // C write: lane covers col = n0 + (lane&15), rows (lane>>4)*4 + 0..3 of
  // each stacked tile.
  const int n = n0 + (lane & 15);
  if (n >= N) return;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const f32x4 a2 = acc[t][0] + acc[t][1];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = t * 16 + (lane >> 4) * 4 + r;
      if (m >= M) continue;
      if (splitk > 1) {
        // split s owns slice s of the [sk][M][N] partials: a plain store,
        // zeros included when this split had no k of its own
        out_f32[((int64_t)blockIdx.y * M + m) * N + n] =
            exact ? splitk_grid(a2[r]) : a2[r];
      } else {
        float v = a2[r];
        if (bias != nullptr) v += bits2f(bias[n]);
        out[(int64_t)m * N + n] = f2bits(v);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Streamed int8/int4 schedule: a two-stage software pipeline over XT-k
// x tiles (profiles/r03_gemm_pipeline.md).
//
//   prologue: stage tile 0 (global_load_lds DMA) + load its weights, drain
//   per tile i:
//     raw s_barrier (lgkmcnt only)  — publishes tile i (every wave drained
//                                     its share of the DMA before arriving)
//                                     and retires tile i-1's readers
//     issue tile i+1: x DMA into the OTHER image buffer, weights + scales
//                     by plain loads into a second register set
//     consume tile i from LDS/registers: A fragments of pair u+1 are
//                     requested before the MFMAs of pair u, the dequant of
//                     pair u+1 runs beside them (counted lgkmcnt waits)
//     s_waitcnt vmcnt(0)            — tile i+1's DMA and weights, one drain
//
// So a wave's global round trip overlaps its own MFMA work, one barrier
// per tile replaces two, and a span remainder (64/128/192 k) runs through
// the same stages as a short last tile with its pairs predicated by a
// block-uniform count.
//
// The weight loads are plain C++ loads: hipcc counts them itself, so the
// values may live across the loop back-edge (an inline-asm load may not:
// hipcc treats asm outputs as ready when the statement ends, and an
// in-flight destination can then be copied or reused — measured garbage
// and page faults in round 2). sched_barrier(0) fences keep the loads in
// front of the consume and their first use behind it.
//
// Every wait hipcc has to know about is the s_waitcnt BUILTIN, not inline
// asm, and the DMA is issued from inline asm, not the builtin (it has no
// register destination, so nothing in flight escapes the statement):
// hipcc keeps its own counters, and both a wait it cannot see and an
// LDS-DMA it can see make it turn the counted lgkmcnt waits of the consume
// back into lgkmcnt(0) between the MFMAs (see stage_tile and the kernel).
// The tile loop is unrolled by two so the register sets swap without
// copies.
//
// glds writes LDS at (wave-uniform base + lane*16), so an image is
// UNPADDED (16*MT rows x XT/8 16B-chunks); bank conflicts on the 16-lane
// fragment reads are killed by an XOR swizzle applied on the SOURCE
// address instead of row padding (guide §5 rule 21): source chunk c lands
// at image chunk c ^ (row & 15) — the 16 reader lanes (rows 0..15, same
// c) then touch 16 different 16B slots = all 64 LDS banks.
// ---------------------------------------------------------------------------

using i32x4 = __attribute__((ext_vector_type(4))) int;

// s_waitcnt immediate (gfx9 encoding): vmcnt(0), expcnt and lgkmcnt free
constexpr int kWaitVm0 = 0x0F70;
// lgkmcnt(0), vmcnt and expcnt free
constexpr int kWaitLgkm0 = 0xC07F;

// One tile's weights and scales. G is compile-time via dispatch (the host
// streams only G in {64,128} and requires every split start to be
// G-aligned, so pair u of a tile reads scale u*64/G).
template <int QBITS, int G, int XT>
struct WSet {
  static constexpr int NW = QBITS == 8 ? XT / 64 : XT / 128;
  static constexpr int NS = XT / G;
  i32x4 w[NW];
  unsigned s[NS];
};

// Issue one tile's weight + scale loads (plain loads, no wait here). wb is
// the lane's row pointer (n_w row + woff) advanced to the tile; sb points
// at the tile's first scale. A short tile (FULL = false) loads only what
// its np pairs cover: the rest would lie past the row's end.
template <int QBITS, int G, int XT, bool FULL>
__device__ __forceinline__ void wset_load(WSet<QBITS, G, XT>& o,
                                          const char* wb,
                                          const unsigned short* sb,
                                          const int np) {
  constexpr int PPW = QBITS == 8 ? 1 : 2;  // pairs per 16-byte load
#pragma unroll
  for (int v = 0; v < WSet<QBITS, G, XT>::NW; ++v) {
    if (FULL || v * PPW < np)
      o.w[v] = *reinterpret_cast<const i32x4*>(wb + v * 64);
    else
      o.w[v] = i32x4{0, 0, 0, 0};
  }
#pragma unroll
  for (int j = 0; j < WSet<QBITS, G, XT>::NS; ++j)
    o.s[j] = (FULL || j * G < np * 64) ? (unsigned)sb[j] : 0u;
}

// Stage one x tile into an image. xk = x + tile start k (block-uniform);
// offb[g] is the per-lane source BYTE offset of this wave's g-th 1 KB
// slice (row clamp, swizzle: k-invariant, computed once per kernel).
//
// The DMA is issued from inline asm (it has no register destination, so
// nothing in flight can escape the statement). Through the builtin hipcc
// books every global_load_lds as a pending access to BOTH counters and
// then turns each later wait into lgkmcnt(0)/vmcnt(0) until both have
// drained: with a DMA in flight across the consume, that put a full
// lgkmcnt(0) between the MFMAs again. LDS address = m0 + lane*16.
template <int MT, int XT, bool GLDS>
__device__ __forceinline__ void stage_tile(const short* __restrict__ xk,
                                           short* img,
                                           const unsigned (&offb)[MT * XT / 128]) {
  constexpr int NSG = MT * XT / 128;  // 1 KB slices per wave
  const int wavei = (int)threadIdx.x >> 6, lanei = (int)threadIdx.x & 63;
  if constexpr (GLDS) {
    const unsigned base = __builtin_amdgcn_readfirstlane(
        (unsigned)(unsigned long)(__attribute__((address_space(3))) short*)img +
        (unsigned)wavei * NSG * 1024u);
#pragma unroll
    for (int g = 0; g < NSG; ++g)
      asm volatile(
          "s_mov_b32 m0, %0\n\t"
          "s_nop 0\n\t"
          "global_load_lds_dwordx4 %1, %2"
          :
          : "s"(base + g * 1024u), "v"(offb[g]), "s"(xk)
          : "memory");
    // DS ops bound-check against m0 on gfx9-family
    asm volatile("s_mov_b32 m0, -1" ::: "memory");
  } else {
    // debug/fallback: same swizzled image via plain loads + ds_write
#pragma unroll
    for (int g = 0; g < NSG; ++g)
      *reinterpret_cast<short8*>(&img[((wavei * NSG + g) * 64 + lanei) * 8]) =
          *reinterpret_cast<const short8*>((const char*)xk + offb[g]);
  }
}

// dequant + MFMA for one tile from already-final weight registers. The A
// fragments of pair u+1 are requested before pair u's MFMAs, so only the
// first pair's reads are waited on cold.
template <int QBITS, int MT, int G, int XT, bool FULL>
__device__ __forceinline__ void consume_tile(const WSet<QBITS, G, XT>& ws,
                                             const short* img,
                                             f32x4 (&acc)[MT][2],
                                             const int row, const int ln4,
                                             const int np) {
  constexpr int PT = XT / 64;
  const short* rb = img + row * XT;
  int v = ln4 ^ row;  // image chunk of source chunk c is c ^ row
  // opaque: keeps the 2*PT swizzled read addresses of BOTH images from
  // being hoisted out of the tile loop and held in registers throughout
  asm volatile("" : "+v"(v));
  bf16x8 a[2][MT][2];
  bf16x8 b[2][2];
  auto frag = [&](const int u, const int s) __attribute__((always_inline)) {
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      a[s][t][0] = *reinterpret_cast<const bf16x8*>(
          &rb[t * 16 * XT + ((u * 8) ^ v) * 8]);
      a[s][t][1] = *reinterpret_cast<const bf16x8*>(
          &rb[t * 16 * XT + ((u * 8 + 4) ^ v) * 8]);
    }
  };
  auto deq = [&](const int u, const int s) __attribute__((always_inline)) {
    const float sv = bits2f((short)ws.s[u * 64 / G]);
    // opaque copy right at the use: without it the optimizer extracts the
    // bytes of the whole register set a tile early (+48 VGPRs and spills)
    i32x4 wq = ws.w[QBITS == 8 ? u : u / 2];
    asm volatile("" : "+v"(wq));
    if (QBITS == 8) {
      const int8_t* q8 = reinterpret_cast<const int8_t*>(&wq);
      b[s][0] = deq8(q8, sv);
      b[s][1] = deq8(q8 + 8, sv);
    } else {
      const uint8_t* q4 = reinterpret_cast<const uint8_t*>(&wq) + (u & 1) * 8;
      b[s][0] = deq4(q4, sv);
      b[s][1] = deq4(q4 + 4, sv);
    }
  };
  frag(0, 0);
  __builtin_amdgcn_sched_barrier(0);
  deq(0, 0);
#pragma unroll
  for (int u = 0; u < PT; ++u) {
    if (!FULL && u >= np) break;  // block-uniform
    const int s = u & 1;
    if (u + 1 < PT && (FULL || u + 1 < np)) frag(u + 1, s ^ 1);
    __builtin_amdgcn_sched_barrier(0);
    if (u + 1 < PT) deq(u + 1, s ^ 1);
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          a[s][t][0], b[s][0], acc[t][0], 0, 0, 0);
      acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          a[s][t][1], b[s][1], acc[t][1], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// XT: k per x tile; MINW: min waves per EU hint. Together with the LDS
// size (two images) they pick the occupancy point per MT tier
// (profiles/r03_gemm_pipeline.md).
template <int QBITS, int MT, int G, int XT, int MINW, bool GLDS = true>
__global__ __launch_bounds__(256, MINW) void gemm_m16_stream_kernel(
    const short* __restrict__ x, const void* __restrict__ w,
    const short* __restrict__ scales, const short* __restrict__ bias,
    short* __restrict__ out, float* __restrict__ out_f32, const int M,
    const int K, const int N, const int splitk, const int exact) {
  using WS = WSet<QBITS, G, XT>;
  constexpr int PT = XT / 64;
  constexpr int CPR = XT / 8;         // 16-byte chunks per image row
  constexpr int NSG = MT * XT / 128;  // 1 KB staging slices per wave
  // two unpadded, swizzled glds images
  constexpr int TILE = 16 * MT * XT;
  __shared__ short x_lds[2 * TILE];
  short* const x_img0 = x_lds;
  short* const x_img1 = x_lds + TILE;
  const int wave = threadIdx.x / kWave;
  const int lane = threadIdx.x & (kWave - 1);
  const int n0 = (blockIdx.x * 4 + wave) * 16;
  const int row = lane & 15;
  const int ln4 = lane >> 4;
  const int n_w = min(n0 + row, N - 1);

  const int pairs = K / 64;
  int p_begin, p_end;
  if (QBITS == 4) {
    const int quads = K / 128;
    const int qq = quads / splitk;
    p_begin = blockIdx.y * qq * 2;
    p_end = (blockIdx.y == splitk - 1) ? quads * 2 : p_begin + qq * 2;
  } else {
    const int pp = pairs / splitk;
    p_begin = blockIdx.y * pp;
    p_end = (blockIdx.y == splitk - 1) ? pairs : p_begin + pp;
  }
  const int woff = ln4 * 16;

  f32x4 acc[MT][2];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int u = 0; u < 2; ++u) acc[t][u] = {0.f, 0.f, 0.f, 0.f};

  // bytes per k: int8 1, int4 1/2
  const char* wrow = (const char*)w +
                     (int64_t)n_w * (QBITS == 8 ? K : K / 2) + woff;
  const unsigned short* srow =
      (const unsigned short*)scales + (int64_t)n_w * (K / G);

  const int kbeg = p_begin * 64, kend = p_end * 64;
  const int nfull = (kend - kbeg) / XT;
  const int rem = (kend - kbeg) - nfull * XT;  // 0, or 64..XT-64
  const int ntiles = nfull + (rem > 0 ? 1 : 0);

  // k-invariant staging source offsets (rows >= M read a clamped row;
  // their C rows are never stored)
  unsigned offb[NSG];
#pragma unroll
  for (int g = 0; g < NSG; ++g) {
    const int L = (wave * NSG + g) * 64 + lane;  // image chunk
    const int r = L / CPR;
    const int cs8 = ((L % CPR) ^ (r & 15)) * 8;  // source k (swizzle)
    offb[g] = 2u * (unsigned)(min(r, M - 1) * K + cs8);
  }

  // issue tile i: x image + weights. A short last tile clamps the source
  // k into the tile (image columns past it hold junk and are never read)
  // and loads only the pairs it has.
  auto issue = [&](const int i, short* img, WS& dst)
      __attribute__((always_inline)) {
    const int k0 = kbeg + i * XT;
    const char* wb = wrow + (QBITS == 8 ? k0 : k0 / 2);
    if (i < nfull) {
      stage_tile<MT, XT, GLDS>(x + k0, img, offb);
      wset_load<QBITS, G, XT, true>(dst, wb, srow + k0 / G, PT);
    } else {
      unsigned offp[NSG];
#pragma unroll
      for (int g = 0; g < NSG; ++g) {
        const int L = (wave * NSG + g) * 64 + lane;
        const int r = L / CPR;
        const int cs8 = ((L % CPR) ^ (r & 15)) * 8;
        offp[g] = 2u * (unsigned)(min(r, M - 1) * K + min(cs8, rem - 8));
      }
      stage_tile<MT, XT, GLDS>(x + k0, img, offp);
      wset_load<QBITS, G, XT, false>(dst, wb, srow + k0 / G, rem / 64);
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  // one pipeline step: publish tile i, put tile i+1 in flight, consume i
  auto step = [&](const int i, const short* img, short* img_next, WS& cur,
                  WS& nxt) __attribute__((always_inline)) {
    // raw barrier (lgkmcnt only): __syncthreads() would add a vmcnt(0)
    // (the wait is the builtin so that hipcc's own counters see it: after
    // an inline-asm wait it still believes the previous tile's reads are
    // pending and turns every counted lgkmcnt in the consume into 0)
    __builtin_amdgcn_s_waitcnt(kWaitLgkm0);
    asm volatile("s_barrier" ::: "memory");
    if (i + 1 < ntiles) issue(i + 1, img_next, nxt);
    if (i < nfull)
      consume_tile<QBITS, MT, G, XT, true>(cur, img, acc, row, ln4, PT);
    else
      consume_tile<QBITS, MT, G, XT, false>(cur, img, acc, row, ln4,
                                             rem / 64);
    __builtin_amdgcn_sched_barrier(0);
    // the DMA has no register destination for hipcc to wait on. The
    // builtin, not inline asm: hipcc then knows the DMA has landed and
    // does not drain vmcnt again before the next tile's first ds_read
    __builtin_amdgcn_s_waitcnt(kWaitVm0);
  };

  if (ntiles > 0) {  // block-uniform (a forced deep split can be empty)
    WS wa, wb2;
#pragma unroll
    for (int v = 0; v < WS::NW; ++v) wb2.w[v] = i32x4{0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < WS::NS; ++j) wb2.s[j] = 0u;
    issue(0, x_img0, wa);
    __builtin_amdgcn_s_waitcnt(kWaitVm0);
    for (int i = 0; i < ntiles; i += 2) {
      step(i, x_img0, x_img1, wa, wb2);
      if (i + 1 < ntiles) step(i + 1, x_img1, x_img0, wb2, wa);
    }
  }

  const int n = n0 + (lane & 15);
  if (n >= N) return;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const f32x4 a2 = acc[t][0] + acc[t][1];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = t * 16 + (lane >> 4) * 4 + r;
      if (m >= M) continue;
      if (splitk > 1) {
        // split s owns slice s of the [sk][M][N] partials: a plain store,
        // zeros included when this split had no k of its own
        out_f32[((int64_t)blockIdx.y * M + m) * N + n] =
            exact ? splitk_grid(a2[r]) : a2[r];
      } else {
        float v = a2[r];
        if (bias != nullptr) v += bits2f(bias[n]);
        out[(int64_t)m * N + n] = f2bits(v);
      }
    }
  }
}

__global__ void f32_to_bf16_bias_kernel(const float* __restrict__ in,
                                        const short* __restrict__ bias,
                                        short* __restrict__ out,
                                        const int64_t total, const int N,
                                        const int splits) {
  // in: [splits][total] partial slices, summed in slice order; read only
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    float v = sum_slices(in + i, total, splits);
    if (bias != nullptr) v += bits2f(bias[i % N]);
    out[i] = f2bits(v);
  }
}

// reproducible split-k (see splitk_grid); process-wide, read at launch —
// set it before graphs are captured
static bool g_splitk_exact = false;
void set_splitk_exact(bool on) { g_splitk_exact = on; }

// partial_elems: capacity of the [sk][M][N] partials buffer in f32.
static int pick_splitk(int64_t N, int64_t K, int64_t M, int64_t partial_elems,
                       int min_pairs, int g_align) {
  // Target ~1024 blocks (~4 blocks / 16 waves per CU) so HBM latency is
  // covered by wave overlap; each split keeps >= 8 K-chunk-pairs of work.
  static const int forced = []() {
    const char* e = getenv("DNET_GEMM_SPLITK");  // debug/bench override
    return e ? atoi(e) : 0;
  }();
  const int blocks = (int)((N + 63) / 64);
  if (forced > 0) {
    // every split needs a slice of its own: fall back to a shallower split
    int sk = (K / 64) < forced ? 1 : forced;
    while (sk > 1 && sk * M * N > partial_elems) sk /= 2;
    return sk;
  }
  int sk = 1;
  while (sk < 32 && blocks * sk < 1024 &&
         (K / 64) / (sk * 2) >= min_pairs &&
         ((K / 64) / (sk * 2)) * 64 % g_align == 0)  // split starts G-aligned
    sk *= 2;
  // Measured (profiles/r02, sk sweep): a split span that is not a
  // multiple of 256 pushes its remainder through the serial tail path;
  // on SHORT spans that tail dominates (qkv K=5120 sk=8: span 640,
  // 20% tail, 27.7us vs 23.6us at sk=4). Halve sk when the tail is
  // >=15% of the span, the halved span is tail-free, and the halved
  // grid still covers the chip (o N=5120 shows 320 blocks is too few).
  if (sk > 1) {
    const int64_t span = ((K / 64) / sk) * 64;
    const int64_t span2 = ((K / 64) / (sk / 2)) * 64;
    if (span % 256 != 0 && (double)(span % 256) / span >= 0.15 &&
        span2 % 256 == 0 && span2 % g_align == 0 &&
        blocks * (sk / 2) >= 440)
      sk /= 2;
  }
  // one [M,N] slice per split (a doubled span stays G-aligned). The loop
  // above ends with blocks * sk < 2048, so sk * N < 131072 and 64 rows
  // need fewer than 8.4 M elements.
  while (sk > 1 && sk * M * N > partial_elems) sk /= 2;
  return sk;
}

// Returns the number of splits left un-combined in the partials buffer
// (the caller's next kernel sums them), or 0 when `out` holds the result.
static int launch_m16(torch::Tensor x, torch::Tensor w,
                      c10::optional<torch::Tensor> scales,
                      c10::optional<torch::Tensor> bias, torch::Tensor out,
                      c10::optional<torch::Tensor> partials, int group,
                      int64_t m0, int M, int bits, bool defer_combine) {
  const int64_t K = x.size(1), N = w.size(0);
  auto stream = current_stream();
  const int64_t partial_elems = partials.has_value() ? partials->numel() : 0;
  // the streamed schedule tolerates short splits (one combined round
  // trip per 4-pair tile), so quantized paths split deeper to fill the
  // 256 CUs on small-N shapes (qkv/o run at <2 blocks/CU otherwise)
  const int sk = pick_splitk(N, K, M, partial_elems, bits < 16 ? 4 : 8,
                             bits < 16 ? std::max<int>((int)group, 64) : 64);
  const short* bptr = bias.has_value() ? (const short*)bias->data_ptr() : nullptr;
  const dim3 grid((unsigned)((N + 63) / 64), sk);
  const int exact = g_splitk_exact ? 1 : 0;
  const short* xp = (const short*)x.data_ptr() + m0 * K;
  short* op = (short*)out.data_ptr() + m0 * N;
  float* fp = nullptr;
  if (sk > 1) {
    // Every split stores its whole [M,N] slice, so the buffer needs no
    // zeroing before the launch and nobody has to clean up after it.
    TORCH_CHECK(partials.has_value() &&
                    partials->numel() >= (int64_t)sk * M * N,
                "split-k partials buffer required");
    fp = (float*)partials->data_ptr();
  }
  const short* sp = bits < 16 ? (const short*)scales->data_ptr() : nullptr;
  const short* bp1 = sk > 1 ? nullptr : bptr;
#define LAUNCH(QQ, TT)                                                      \
  hipLaunchKernelGGL((gemm_m16_kernel<QQ, TT>), grid, dim3(256), 0, stream, \
                     xp, w.data_ptr(), sp, bp1, op, fp, M, (int)K, (int)N,  \
                     group, sk, exact)
  static const bool noglds = getenv("DNET_GEMM_NOGLDS") != nullptr;
#define LAUNCH_STREAM(QQ, TT, GG, XT, MW)                                   \
  do {                                                                      \
    if (noglds)                                                             \
      hipLaunchKernelGGL(                                                   \
          (gemm_m16_stream_kernel<QQ, TT, GG, XT, 2, false>), grid,         \
          dim3(256), 0, stream, xp, w.data_ptr(), sp, bp1, op, fp, M,       \
          (int)K, (int)N, sk, exact);                                       \
    else                                                                    \
      hipLaunchKernelGGL(                                                   \
          (gemm_m16_stream_kernel<QQ, TT, GG, XT, MW, true>), grid,         \
          dim3(256), 0, stream, xp, w.data_ptr(), sp, bp1, op, fp, M,       \
          (int)K, (int)N, sk, exact);                                       \
  } while (0)
  // occupancy point per MT tier (profiles/r03_gemm_pipeline.md)
  // occupancy point per MT tier (profiles/r03_gemm_pipeline.md): 256-k
  // tiles everywhere; two 32 KB images leave MT4 two blocks per CU
#define LAUNCH_STREAM_T(QQ, TT, GG) \
  LAUNCH_STREAM(QQ, TT, GG, 256, (TT == 4 ? 2 : TT == 2 ? 3 : 4))
#define LAUNCH_STREAM_G8(TT)                                                \
  do {                                                                      \
    if (group == 64) LAUNCH_STREAM_T(8, TT, 64);                            \
    else LAUNCH_STREAM_T(8, TT, 128);                                       \
  } while (0)
#define LAUNCH_STREAM_G4(TT) LAUNCH_STREAM_T(4, TT, 128)
  // the streamed counted-vmcnt schedule needs a compile-time scale count
  // per 256-k tile; other group sizes fall back to the generic kernel
  // G must divide every tile start (k0 is any multiple of 64 under
  // split-k partitioning, and the in-tile scale index u*NSC/4 assumes
  // k0 % G == 0), so only G <= 128 streams; G=256 falls back
  // additionally every split start kbeg = by*(pairs/sk)*64 must be
  // G-aligned (the in-tile scale index assumes k0 % G == 0)
  const bool split_aligned =
      group > 0 && (sk == 1 || ((K / 64 / sk) * 64) % group == 0);
  const bool can_stream =
      split_aligned && ((bits == 8 && (group == 64 || group == 128)) ||
                        (bits == 4 && group == 128));
  static const bool nostream = getenv("DNET_GEMM_NOSTREAM") != nullptr;
  const bool use_stream = can_stream && !nostream;
  if (bits == 8) {
    if (M > 32) { if (use_stream) LAUNCH_STREAM_G8(4); else LAUNCH(8, 4); }
    else if (M > 16) { if (use_stream) LAUNCH_STREAM_G8(2); else LAUNCH(8, 2); }
    else { if (use_stream) LAUNCH_STREAM_G8(1); else LAUNCH(8, 1); }
  } else if (bits == 4) {
    if (M > 32) { if (use_stream) LAUNCH_STREAM_G4(4); else LAUNCH(4, 4); }
    else if (M > 16) { if (use_stream) LAUNCH_STREAM_G4(2); else LAUNCH(4, 2); }
    else { if (use_stream) LAUNCH_STREAM_G4(1); else LAUNCH(4, 1); }
  } else {
    if (M > 32) LAUNCH(16, 4);
    else if (M > 16) LAUNCH(16, 2);
    else LAUNCH(16, 1);
  }
#undef LAUNCH
#undef LAUNCH_STREAM
#undef LAUNCH_STREAM_T
#undef LAUNCH_STREAM_G8
#undef LAUNCH_STREAM_G4
  if (sk > 1) {
    // defer_combine: the caller's next kernel sums the f32 slices itself
    // — skip the convert/bias pass
    if (defer_combine && bptr == nullptr) return sk;
    const int64_t total = (int64_t)M * N;
    const int cgrid = (int)std::min<int64_t>((total + 255) / 256, 2048);
    hipLaunchKernelGGL(f32_to_bf16_bias_kernel, dim3(cgrid), dim3(256), 0,
                       stream, fp, bptr, op, total, (int)N, sk);
  }
  return 0;
}

// Would gemm_m16(defer_combine=true) actually defer for this shape?
// (Pure: lets callers decide between the fused-consumer and the
// bias-in-combine paths BEFORE launching.)
bool gemm_m16_will_defer(int64_t M, int64_t N, int64_t K, int64_t group,
                         int64_t bits, int64_t partial_elems) {
  if (M > 64 || M <= 2) return false;
  const int sk = pick_splitk(N, K, M, partial_elems, bits < 16 ? 4 : 8,
                             bits < 16 ? std::max<int>((int)group, 64) : 64);
  return sk > 1;
}

// Returns 0 when `out` holds the result, else the number of split-k
// slices the deferred result occupies in `partials` ([sk][M][N] f32): the
// caller hands that count to the consumer kernel.
int64_t gemm_m16(torch::Tensor x, torch::Tensor w,
                 c10::optional<torch::Tensor> scales,
                 c10::optional<torch::Tensor> bias, torch::Tensor out,
                 c10::optional<torch::Tensor> partials, int64_t group,
                 bool packed, int64_t bits, bool defer_combine) {
  const int64_t M = x.size(0), K = x.size(1), N = w.size(0);
  DNET_CHECK(K % 64 == 0, "K % 64 == 0 required for the MFMA path");
  DNET_CHECK(out.size(0) == M && out.size(1) == N, "shape");
  DNET_CHECK(x.is_contiguous() && w.is_contiguous() && out.is_contiguous(), "contig");
  if (bits == 16) {
    DNET_CHECK(w.size(1) == K, "w shape");
  } else {
    DNET_CHECK(packed, "quantized MFMA path expects the packed weight layout");
    DNET_CHECK(scales.has_value() && scales->is_contiguous(), "scales");
    DNET_CHECK(group % 64 == 0 && K % group == 0, "group align");
    if (bits == 8) DNET_CHECK(w.size(1) == K, "w shape (int8)");
    if (bits == 4) {
      DNET_CHECK(w.size(1) == K / 2 && K % 128 == 0 && group % 128 == 0,
                 "w shape / align (int4)");
    }
  }
  // defer only meaningful for the single-chunk (M <= 64) decode path:
  // multiple chunks could pick different sk and leave a mixed state
  const bool defer = defer_combine && M <= 64 && !bias.has_value();
  int64_t deferred = 0;
  int64_t m0 = 0;
  while (m0 < M) {
    const int mt = (int)std::min<int64_t>(M - m0, 64);
    deferred = launch_m16(x, w, scales, bias, out, partials, (int)group, m0,
                          mt, (int)bits, defer);
    m0 += mt;
  }
  return deferred;
}

}  // namespace dnet
