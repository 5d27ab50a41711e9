// Token-routed grouped-expert MoE for prefill-sized batches (T > 64 rows):
// sort the routed (token, expert) pairs by expert on the device, run the
// gate/up and down projections as MFMA GEMMs over each expert's gathered
// rows, and sum every token's expert outputs in a fixed order. No host
// sync, no atomics; a token's bits do not depend on the other tokens of
// the call.
//
// Plan (moe_route, two launches). A pair (t, e) is routed iff we[t,e] != 0.
// Routed pairs get slots in (e ascending, t ascending) order:
//   counts[E], offsets[E+1]      per-expert slot ranges
//   slot_token[slots_cap]        slot -> token (-1 past the live slots)
//   token_slots[T, topk]         token -> its slots, e ascending, -1 = none
//   tiles[tiles_cap, 3], ntiles  (expert, first slot, rows <= 64) work list
// Launch 1 counts the non-zeros of every expert column per 256-token block
// (one ballot + popcount per wave and expert). Launch 2 turns the block
// counts into per-expert offsets (LDS block scan) and per-block bases, and
// every thread (= token) walks its row: the slot of (t, e) is
// base[e] + earlier waves' counts + popcount(ballot below this lane).
// Positions come from prefix sums only, so the order is fixed.
//
// GEMM (one kernel body, two epilogues). A block owns one tile of up to 64
// rows of one expert (4 stacked 16-row A tiles) and a strip of output
// columns; blocks past ntiles exit at once. The A rows (x gathered through
// slot_token for gate/up, contiguous act slots for down) are staged 256 k
// at a time into LDS with 16 B row loads and a padded row stride; dead
// rows read a clamped live row and are never stored. The weight loads of
// up to four 64-k pairs are issued together and consumed before the next
// group; nothing is prefetched across a tile boundary (the barriers are
// the raw lgkmcnt-only form of gemm_m16, which leaves that open). Each
// wave holds two sets of 16 weight rows (gate and up columns i, or down
// columns h and h+16), so one A fragment read feeds two MFMAs. Weights
// come straight from global memory in fragment shape
// (v_mfma_f32_16x16x32_bf16: lane l holds row l&15, k-slice l>>4):
//   bf16   16 B per lane and 32-k chunk
//   int8   pack_int8_mfma chunk-pair rows, 16 B per lane and 64-k pair,
//          dequantised in registers to bf16(q*s)
//   mxfp4  row-major nibble rows: a 64-k pair is 32 B = two 16 B blocks of
//          32 values; lane slice s loads the 8 B at pair*32 + s*8, i.e.
//          half (s&1) of block pair*2 + (s>>1): 16 consecutive k, one e8m0
//          scale. The MFMA contracts over k in any order, so step c (0/1)
//          takes k = pair*64 + s*16 + c*8 + j from the lane's bytes and the
//          A fragment is read from LDS at the same k. Values are converted
//          by v_cvt_scalef32_pk_bf16_fp4 with the f32 scale (e8m0 << 23):
//          the exact e2m1 * 2^(e8m0-127), the value moe.hip.cpp's
//          mxfp4_val builds, for e8m0 in 1..254 (the checkpoints' range);
//          e8m0 = 0 gives a zero scale, not 2^-127.
// K is never split, so the accumulation order of a row is fixed.
//
// gate/up epilogue: bias + GLU from the accumulators -> act[slot, I] bf16.
// down epilogue: y[slot, H] = we[t,e] * (acc + bias) f32, plain stores.
// Combine: out[t] = sum of y over token_slots[t] in order (zeros if none).
#include "moe_common.h"

namespace dnet {

using i32x4 = __attribute__((ext_vector_type(4))) int;
using i32x2 = __attribute__((ext_vector_type(2))) int;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;

constexpr int kRouteThreads = 256;
constexpr int kRouteWaves = kRouteThreads / kWave;
constexpr int kRouteMaxE = 4 * kRouteThreads;   // 4 scan entries per thread
constexpr int kTileRows = 64;

// wcnt[w * E + e] = non-zeros of column e among wave w's 64 tokens
__device__ __forceinline__ void route_wave_counts(const float* __restrict__ row,
                                                  const bool live, const int E,
                                                  int* wcnt) {
  const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
  for (int e = 0; e < E; ++e) {
    const unsigned long long m = __ballot(live && row[e] != 0.f);
    if (lane == 0) wcnt[wave * E + e] = __popcll(m);
  }
}

__global__ __launch_bounds__(kRouteThreads) void moe_route_count_kernel(
    const float* __restrict__ we, int* __restrict__ blockcnt, const int T,
    const int E) {
  extern __shared__ int smem[];
  const int t = blockIdx.x * kRouteThreads + threadIdx.x;
  route_wave_counts(we + (int64_t)min(t, T - 1) * E, t < T, E, smem);
  __syncthreads();
  for (int e = threadIdx.x; e < E; e += kRouteThreads) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < kRouteWaves; ++w) c += smem[w * E + e];
    blockcnt[blockIdx.x * E + e] = c;
  }
}

// exclusive prefix of v over the block's threads (thread order); total out
__device__ __forceinline__ int block_excl_scan(const int v, int* s,
                                               int& total) {
  const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
  int inc = v;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const int n = __shfl_up(inc, off, kWave);
    if (lane >= off) inc += n;
  }
  if (lane == kWave - 1) s[wave] = inc;
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < kRouteWaves; ++w) {
    if (w < wave) base += s[w];
    total += s[w];
  }
  __syncthreads();
  return base + inc - v;
}

__global__ __launch_bounds__(kRouteThreads) void moe_route_fill_kernel(
    const float* __restrict__ we, const int* __restrict__ blockcnt,
    int* __restrict__ counts, int* __restrict__ offsets,
    int* __restrict__ slot_token, int* __restrict__ token_slots,
    int* __restrict__ tiles, int* __restrict__ ntiles, const int T,
    const int E, const int topk, const int slots_cap, const int tiles_cap) {
  extern __shared__ int smem[];
  int* wcnt = smem;                       // [kRouteWaves][E]
  int* base = smem + kRouteWaves * E;     // [E] first slot of (block, e)
  int* scan = base + E;                   // [kRouteWaves]
  const int nb = gridDim.x, b = blockIdx.x;
  // thread i owns experts 4i..4i+3: column totals over all blocks, and the
  // part that belongs to earlier token blocks
  int tot[4], before[4], sum = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = threadIdx.x * 4 + i;
    tot[i] = before[i] = 0;
    if (e < E)
      for (int bb = 0; bb < nb; ++bb) {
        const int c = blockcnt[bb * E + e];
        tot[i] += c;
        if (bb < b) before[i] += c;
      }
    sum += tot[i];
  }
  int live;
  int off = block_excl_scan(sum, scan, live);
  int eoff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = threadIdx.x * 4 + i;
    eoff[i] = off;
    if (e < E) base[e] = off + before[i];
    off += tot[i];
  }
  const int t = b * kRouteThreads + threadIdx.x;
  const float* row = we + (int64_t)min(t, T - 1) * E;
  route_wave_counts(row, t < T, E, wcnt);
  __syncthreads();
  {
    const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    int j = 0;
    for (int e = 0; e < E; ++e) {
      const bool nz = t < T && row[e] != 0.f;
      const unsigned long long m = __ballot(nz);
      if (!nz) continue;
      int slot = base[e] + __popcll(m & ((1ull << lane) - 1ull));
      for (int w = 0; w < wave; ++w) slot += wcnt[w * E + e];
      // more than topk non-zeros in a row breaks the caller's promise;
      // stay inside the buffers
      if (slot < slots_cap) {
        slot_token[slot] = t;
        if (j < topk) token_slots[(int64_t)t * topk + j] = slot;
        ++j;
      }
    }
    if (t < T)
      for (; j < topk; ++j) token_slots[(int64_t)t * topk + j] = -1;
  }
  if (b != 0) return;
  // block 0: counts, offsets, dead slots and the tile work list
  live = min(live, slots_cap);
  int nt[4], ntsum = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = threadIdx.x * 4 + i;
    const int s0 = min(eoff[i], slots_cap);
    const int s1 = min(eoff[i] + tot[i], slots_cap);
    nt[i] = (s1 - s0 + kTileRows - 1) / kTileRows;
    ntsum += nt[i];
    if (e < E) {
      counts[e] = tot[i];
      offsets[e] = eoff[i];
    }
    if (e == E - 1) offsets[E] = eoff[i] + tot[i];
  }
  int ntot;
  int ti = block_excl_scan(ntsum, scan, ntot);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = threadIdx.x * 4 + i;
    const int s0 = min(eoff[i], slots_cap);
    const int s1 = min(eoff[i] + tot[i], slots_cap);
    for (int k = 0; k < nt[i]; ++k, ++ti) {
      if (ti >= tiles_cap) break;
      tiles[ti * 3 + 0] = e;
      tiles[ti * 3 + 1] = s0 + k * kTileRows;
      tiles[ti * 3 + 2] = min(kTileRows, s1 - s0 - k * kTileRows);
    }
  }
  ntot = min(ntot, tiles_cap);
  if (threadIdx.x == 0) ntiles[0] = ntot;
  for (int i = ntot + threadIdx.x; i < tiles_cap; i += kRouteThreads) {
    tiles[i * 3 + 0] = 0;
    tiles[i * 3 + 1] = 0;
    tiles[i * 3 + 2] = 0;
  }
  for (int i = live + threadIdx.x; i < slots_cap; i += kRouteThreads)
    slot_token[i] = -1;
}

// 8 e2m1 nibbles (k ascending from the low nibble) * 2^(ebits-127) -> bf16
__device__ __forceinline__ bf16x8 deq_mxfp4(const unsigned q, const int ebits) {
  const float sc = __uint_as_float((unsigned)ebits << 23);
  const bf16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, sc, 0);
  const bf16x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, sc, 1);
  const bf16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, sc, 2);
  const bf16x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, sc, 3);
  return bf16x8{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}

// QMODE: 0 = bf16, 1 = int8 (pack_int8_mfma rows), 2 = mxfp4.
// DOWN = 0: a = x [T, K], the bank is [E, 2*NC, K] (gate rows then up rows),
//           act[slot, NC] = glu(gate, up); a wave owns 16 columns.
// DOWN = 1: a = act [slots_cap, K], the bank is [E, NC, K],
//           y[slot, NC] = we[t, e] * (a . w + bias); a wave owns 32 columns.
template <int QMODE, int DOWN, int GLU>
__global__ __launch_bounds__(256, 2) void moe_rows_gemm_kernel(
    const short* __restrict__ a, const void* __restrict__ w,
    const void* __restrict__ scales, const short* __restrict__ bias,
    const int* __restrict__ slot_token, const int* __restrict__ tiles,
    const int* __restrict__ ntiles, const float* __restrict__ we,
    short* __restrict__ act, float* __restrict__ y, const int K, const int NC,
    const int E, const int G, const float alpha, const float limit) {
  constexpr int MT = 4;                // stacked 16-row A tiles
  constexpr int XT = 256;              // k per staged tile
  constexpr int SE = XT + 8;           // row stride in bf16 elems (16 B pad)
  __shared__ short a_lds[16 * MT * SE];   // 33 KB: 4 blocks fit a CU's LDS
  __shared__ int rowsrc[16 * MT];
  const int tile = blockIdx.y;
  if (tile >= ntiles[0]) return;       // block-uniform
  const int e = tiles[tile * 3 + 0];
  const int first = tiles[tile * 3 + 1];
  const int rows = tiles[tile * 3 + 2];
  const int wave = threadIdx.x / kWave;
  const int lane = threadIdx.x & (kWave - 1);
  const int col = lane & 15;
  const int sl = lane >> 4;            // k-slice of this lane
  if (threadIdx.x < 16 * MT) {
    // rows past the tile's end read its last live row; never stored
    const int slot = first + min((int)threadIdx.x, rows - 1);
    rowsrc[threadIdx.x] = DOWN ? slot : slot_token[slot];
  }
  // this lane's two weight rows (a wave past NC keeps the barriers and
  // reads clamped rows; it stores nothing)
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
  // per-lane byte offset inside a 64-k pair, and the A k-offsets of the
  // two MFMA steps of a pair
  const int a0off = QMODE == 2 ? sl * 16 : sl * 8;
  const int a1off = QMODE == 2 ? sl * 16 + 8 : sl * 8 + 32;
  const char* wp[2];
  const short* s8[2];
  const uint8_t* s4[2];
#pragma unroll
  for (int z = 0; z < 2; ++z) {
    if (QMODE == 0) {
      wp[z] = (const char*)w + wr[z] * K * 2 + sl * 16;
    } else if (QMODE == 1) {
      wp[z] = (const char*)w + wr[z] * K + sl * 16;
      s8[z] = (const short*)scales + wr[z] * (K / G);
    } else {
      wp[z] = (const char*)w + wr[z] * (K / 2) + sl * 8;
      s4[z] = (const uint8_t*)scales + wr[z] * (K / 32) + (sl >> 1);
    }
  }

  f32x4 acc[MT][2];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int z = 0; z < 2; ++z) acc[t][z] = {0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < K; k0 += XT) {
    const int tk = min(XT, K - k0);
    const int vecs = tk / 8;
    // raw barriers (lgkmcnt only), as in gemm_m16; no weight load is in
    // flight here (each group's loads are consumed inside the pl loop)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    asm volatile("s_barrier" ::: "memory");
    for (int idx = threadIdx.x; idx < 16 * MT * vecs; idx += 256) {
      const int r = idx / vecs;
      const int vec = idx - r * vecs;
      *reinterpret_cast<short8*>(&a_lds[r * SE + vec * 8]) =
          *reinterpret_cast<const short8*>(
              &a[(int64_t)rowsrc[r] * K + k0 + vec * 8]);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    asm volatile("s_barrier" ::: "memory");
    const short* arow = &a_lds[col * SE];
    const int pl_end = tk / 64;
    for (int pl = 0; pl < pl_end; pl += 4) {
      const int np = min(4, pl_end - pl);    // block-uniform
      // all weight loads of up to 4 pairs first
      bf16x8 rb[4][2][2];
      i32x4 rq[4][2];
      i32x2 rm[4][2];
      float sc[4][2];
      int eb[4][2];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (u >= np) break;
        const int p = k0 / 64 + pl + u;
#pragma unroll
        for (int z = 0; z < 2; ++z) {
          if (QMODE == 0) {
            rb[u][z][0] = *reinterpret_cast<const bf16x8*>(wp[z] + p * 128);
            rb[u][z][1] =
                *reinterpret_cast<const bf16x8*>(wp[z] + p * 128 + 64);
          } else if (QMODE == 1) {
            rq[u][z] = *reinterpret_cast<const i32x4*>(wp[z] + p * 64);
            sc[u][z] = bits2f(s8[z][(p * 64) / G]);
          } else {
            rm[u][z] = *reinterpret_cast<const i32x2*>(wp[z] + p * 32);
            eb[u][z] = s4[z][p * 2];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (u >= np) break;
        bf16x8 b[2][2];
#pragma unroll
        for (int z = 0; z < 2; ++z) {
          if (QMODE == 0) {
            b[z][0] = rb[u][z][0];
            b[z][1] = rb[u][z][1];
          } else if (QMODE == 1) {
            const int8_t* q8 = reinterpret_cast<const int8_t*>(&rq[u][z]);
            b[z][0] = deq8(q8, sc[u][z]);
            b[z][1] = deq8(q8 + 8, sc[u][z]);
          } else {
            b[z][0] = deq_mxfp4((unsigned)rm[u][z][0], eb[u][z]);
            b[z][1] = deq_mxfp4((unsigned)rm[u][z][1], eb[u][z]);
          }
        }
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          const short* at = arow + t * 16 * SE + (pl + u) * 64;
          const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(&at[a0off]);
          const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(&at[a1off]);
          acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a0, b[0][0], acc[t][0], 0, 0, 0);
          acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a0, b[1][0], acc[t][1], 0, 0, 0);
          acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a1, b[0][1], acc[t][0], 0, 0, 0);
          acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a1, b[1][1], acc[t][1], 0, 0, 0);
        }
      }
    }
  }

  // C: lane covers column (lane&15), rows (lane>>4)*4 + 0..3 of each tile
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

// out[t, :] = y[s0, :] + y[s1, :] + ... over token_slots[t] in order
__global__ __launch_bounds__(256) void moe_rows_combine_kernel(
    const float* __restrict__ y, const int* __restrict__ token_slots,
    float* __restrict__ out, const int H, const int topk) {
  const int t = blockIdx.x;
  const int* ts = token_slots + (int64_t)t * topk;
  for (int h = threadIdx.x * 4; h < H; h += 256 * 4) {
    float4 v = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < topk; ++j) {
      const int s = ts[j];
      if (s < 0) break;                // slots are packed at the front
      const float4 p = *reinterpret_cast<const float4*>(&y[(int64_t)s * H + h]);
      if (j == 0) v = p;
      else slice_add(v, p);
    }
    *reinterpret_cast<float4*>(&out[(int64_t)t * H + h]) = v;
  }
}

// the combine launch, shared with moe_rows_int4.hip.cpp (checked tensors)
void moe_rows_combine(const torch::Tensor& y, const torch::Tensor& token_slots,
                      torch::Tensor& out, hipStream_t stream) {
  hipLaunchKernelGGL(moe_rows_combine_kernel, dim3((unsigned)out.size(0)),
                     dim3(256), 0, stream, (const float*)y.data_ptr(),
                     (const int*)token_slots.data_ptr(),
                     (float*)out.data_ptr(), (int)out.size(1),
                     (int)token_slots.size(1));
}

static bool is_i32(const torch::Tensor& t) {
  return t.scalar_type() == torch::kInt && t.is_contiguous();
}

void moe_route(torch::Tensor we, torch::Tensor blockcnt, torch::Tensor counts,
               torch::Tensor offsets, torch::Tensor slot_token,
               torch::Tensor token_slots, torch::Tensor tiles,
               torch::Tensor ntiles, int64_t topk) {
  const int64_t T = we.size(0), E = we.size(1);
  const int nb = cdiv(T, kRouteThreads);
  DNET_CHECK(we.scalar_type() == torch::kFloat && we.is_contiguous(), "we f32");
  DNET_CHECK(T > 0 && E > 0 && E <= kRouteMaxE && topk > 0, "moe_route shape");
  DNET_CHECK(is_i32(blockcnt) && is_i32(counts) && is_i32(offsets) &&
                 is_i32(slot_token) && is_i32(token_slots) && is_i32(tiles) &&
                 is_i32(ntiles), "plan tensors are contiguous int32");
  DNET_CHECK(blockcnt.numel() >= nb * E && counts.numel() == E &&
                 offsets.numel() == E + 1 && token_slots.numel() == T * topk &&
                 tiles.dim() == 2 && tiles.size(1) == 3 && ntiles.numel() == 1,
             "plan shapes");
  auto stream = current_stream();
  hipLaunchKernelGGL(moe_route_count_kernel, dim3(nb), dim3(kRouteThreads),
                     kRouteWaves * E * sizeof(int), stream,
                     (const float*)we.data_ptr(), (int*)blockcnt.data_ptr(),
                     (int)T, (int)E);
  hipLaunchKernelGGL(moe_route_fill_kernel, dim3(nb), dim3(kRouteThreads),
                     ((kRouteWaves + 1) * E + kRouteWaves) * sizeof(int),
                     stream, (const float*)we.data_ptr(),
                     (const int*)blockcnt.data_ptr(), (int*)counts.data_ptr(),
                     (int*)offsets.data_ptr(), (int*)slot_token.data_ptr(),
                     (int*)token_slots.data_ptr(), (int*)tiles.data_ptr(),
                     (int*)ntiles.data_ptr(), (int)T, (int)E, (int)topk,
                     (int)slot_token.numel(), (int)tiles.size(0));
}

// Checks one bank against the inner dim K; returns QMODE.
static int rows_bank_mode(const torch::Tensor& w,
                          const c10::optional<torch::Tensor>& scales,
                          const c10::optional<torch::Tensor>& bias, int64_t K,
                          int64_t group, bool packed) {
  const int64_t E = w.size(0), N = w.size(1);
  DNET_CHECK(w.dim() == 3 && w.is_contiguous() && K % 64 == 0, "bank / K % 64");
  if (bias.has_value())
    DNET_CHECK(bias->is_contiguous() && bias->numel() == E * N &&
                   bias->scalar_type() == torch::kBFloat16, "bank bias");
  if (w.scalar_type() == torch::kBFloat16) {
    DNET_CHECK(w.size(2) == K, "bf16 bank shape");
    return 0;
  }
  DNET_CHECK(scales.has_value() && scales->is_contiguous(), "bank scales");
  if (w.scalar_type() == torch::kChar) {
    DNET_CHECK(packed && group > 0 && group % 64 == 0 && K % group == 0 &&
                   w.size(2) == K, "int8 bank: packed layout, group % 64");
    DNET_CHECK(scales->scalar_type() == torch::kBFloat16 &&
                   scales->numel() == E * N * (K / group), "int8 scales");
    return 1;
  }
  DNET_CHECK(w.scalar_type() == torch::kByte && w.size(2) == K / 2 &&
                 scales->scalar_type() == torch::kByte &&
                 scales->numel() == E * N * (K / 32), "mxfp4 bank shape");
  return 2;
}

template <int DOWN>
static void launch_rows_gemm(int mode, int glu, dim3 grid, hipStream_t stream,
                             const short* a, const void* w, const void* sp,
                             const short* bp, const int* st, const int* tl,
                             const int* nt, const float* we, short* act,
                             float* y, int K, int NC, int E, int G,
                             float alpha, float limit) {
#define ROWS_LAUNCH(QQ, GG)                                                   \
  hipLaunchKernelGGL((moe_rows_gemm_kernel<QQ, DOWN, GG>), grid, dim3(256),  \
                     0, stream, a, w, sp, bp, st, tl, nt, we, act, y, K, NC, \
                     E, G, alpha, limit)
#define ROWS_MODE(GG)              \
  do {                             \
    if (mode == 0) ROWS_LAUNCH(0, GG); \
    else if (mode == 1) ROWS_LAUNCH(1, GG); \
    else ROWS_LAUNCH(2, GG);       \
  } while (0)
  if (!DOWN && glu == 1) ROWS_MODE(1);
  else ROWS_MODE(0);
#undef ROWS_MODE
#undef ROWS_LAUNCH
}

void moe_rows_gateup(torch::Tensor x, torch::Tensor w,
                     c10::optional<torch::Tensor> scales,
                     c10::optional<torch::Tensor> bias,
                     torch::Tensor slot_token, torch::Tensor tiles,
                     torch::Tensor ntiles, torch::Tensor act, int64_t group,
                     bool packed, int64_t glu, double alpha, double limit) {
  const int64_t K = x.size(1), E = w.size(0), I = w.size(1) / 2;
  DNET_CHECK(x.scalar_type() == torch::kBFloat16 && x.is_contiguous(), "x");
  const int mode = rows_bank_mode(w, scales, bias, K, group, packed);
  DNET_CHECK(w.size(1) == 2 * I && I % 64 == 0, "I % 64");
  DNET_CHECK(is_i32(slot_token) && is_i32(tiles) && is_i32(ntiles) &&
                 tiles.size(0) <= 65535, "plan");
  DNET_CHECK(act.scalar_type() == torch::kBFloat16 && act.is_contiguous() &&
                 act.size(0) == slot_token.numel() && act.size(1) == I, "act");
  const dim3 grid((unsigned)(I / 64), (unsigned)tiles.size(0));
  launch_rows_gemm<0>(
      mode, (int)glu, grid, current_stream(), (const short*)x.data_ptr(),
      w.data_ptr(), scales.has_value() ? scales->data_ptr() : nullptr,
      bias.has_value() ? (const short*)bias->data_ptr() : nullptr,
      (const int*)slot_token.data_ptr(), (const int*)tiles.data_ptr(),
      (const int*)ntiles.data_ptr(), nullptr, (short*)act.data_ptr(), nullptr,
      (int)K, (int)I, (int)E, (int)std::max<int64_t>(group, 64), (float)alpha,
      (float)limit);
}

void moe_rows_down(torch::Tensor act, torch::Tensor w,
                   c10::optional<torch::Tensor> scales,
                   c10::optional<torch::Tensor> bias, torch::Tensor we,
                   torch::Tensor slot_token, torch::Tensor token_slots,
                   torch::Tensor tiles, torch::Tensor ntiles, torch::Tensor y,
                   torch::Tensor out, int64_t group, bool packed) {
  const int64_t I = act.size(1), E = w.size(0), H = w.size(1);
  const int64_t T = we.size(0);
  DNET_CHECK(act.scalar_type() == torch::kBFloat16 && act.is_contiguous() &&
                 act.size(0) == slot_token.numel(), "act");
  const int mode = rows_bank_mode(w, scales, bias, I, group, packed);
  DNET_CHECK(H % 64 == 0, "H % 64");
  DNET_CHECK(we.scalar_type() == torch::kFloat && we.is_contiguous() &&
                 we.size(1) == E, "we");
  DNET_CHECK(is_i32(slot_token) && is_i32(token_slots) && is_i32(tiles) &&
                 is_i32(ntiles) && tiles.size(0) <= 65535 &&
                 token_slots.dim() == 2 && token_slots.size(0) == T, "plan");
  DNET_CHECK(y.scalar_type() == torch::kFloat && y.is_contiguous() &&
                 y.size(0) == slot_token.numel() && y.size(1) == H, "y");
  DNET_CHECK(out.scalar_type() == torch::kFloat && out.is_contiguous() &&
                 out.size(0) == T && out.size(1) == H, "out");
  auto stream = current_stream();
  const dim3 grid((unsigned)cdiv(H, 128), (unsigned)tiles.size(0));
  launch_rows_gemm<1>(
      mode, 0, grid, stream, (const short*)act.data_ptr(), w.data_ptr(),
      scales.has_value() ? scales->data_ptr() : nullptr,
      bias.has_value() ? (const short*)bias->data_ptr() : nullptr,
      (const int*)slot_token.data_ptr(), (const int*)tiles.data_ptr(),
      (const int*)ntiles.data_ptr(), (const float*)we.data_ptr(), nullptr,
      (float*)y.data_ptr(), (int)I, (int)H, (int)E,
      (int)std::max<int64_t>(group, 64), 0.f, 0.f);
  moe_rows_combine(y, token_slots, out, stream);
}

}  // namespace dnet
