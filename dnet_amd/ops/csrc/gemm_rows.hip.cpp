// Fused-dequant MFMA prefill GEMM for int8 / int4 dense linears, M > 64:
//   out[M,N] bf16 = x[M,K] bf16 @ W[N,K]^T (+ bias[N])
// straight from the packed bytes the decode GEMM (gemm_m16.hip.cpp) reads:
//   int8  pack_int8_mfma chunk-pair rows, bf16 scales [N, K/G],
//         K % 64 == 0, G % 64 == 0: 16 B per lane and 64-k pair
//   int4  pack_int4_mfma chunk-quad nibble rows, bf16 scales [N, K/G],
//         K % 128 == 0, G % 128 == 0: 16 B per lane and 128-k quad
// The weight matrix is read once per 128-row M tile and never written back
// as bf16 (the dequant + hipBLASLt path moves 5 bytes per int8 weight).
//
// Contract (that of gemm_m16): every weight enters as bf16(q * s) (deq8 /
// deq4 of common.h), products accumulate in f32 through
// v_mfma_f32_16x16x32_bf16, the bias is added in f32 and the output is
// rounded to bf16 once. K is never split: an output element is ONE
// accumulator that takes the 32-k chunks in ascending order, so two
// launches give the same bits, and the bits of a row depend on neither M,
// the other rows of the call nor the tile shape picked below (a C row of
// an MFMA depends on its own A row alone).
//
// Block tile: 128 rows x (64 * NZ) columns, NZ in {1, 2}, 4 waves side by
// side along N. A wave owns all 128 rows (8 stacked 16-row A tiles) of
// 16 * NZ columns: acc[8][NZ] f32x4 = 64 accumulator VGPRs at NZ = 2, and
// per 32-k chunk 8 A fragment reads feed 8 * NZ MFMAs. The waves are NOT
// arranged 2 x 2 over 64 x 64 sub-tiles: there every weight is dequantised
// by two waves (int8: ~2.5 VALU per weight, 128 weights per lane and 128 k
// against 64 MFMAs, which makes the VALU the longer pipe), and the cure,
// bf16 B fragments staged once per block through LDS, reads as many LDS
// bytes per MFMA as this layout does and writes them on top. Here a weight
// is dequantised once per block, in the registers of the one wave that
// multiplies by it, and feeds 8 MFMAs; the price is that each wave reads
// the whole x tile from LDS (8 KB per 16 MFMAs at NZ = 2). Only this
// variant was built and measured (profiles/r12_gemm_rows.md).
// NZ = 1 halves the block's columns for grids that would otherwise leave
// most of the 256 CUs idle (M = 128, N = 4096 is 32 blocks at NZ = 2).
//
// x: 128 rows x 128 k per stage, 16 B coalesced row loads (16 threads per
// 256 B row segment) into LDS rows of 128 + 8 elements; the pad spreads
// the 16 rows of a fragment read over the banks. Two images (69.6 KB, one
// dynamic __shared__ object, two blocks per CU): the global loads of stage
// i + 1 are issued before stage i is consumed, held in registers and
// written to the other image afterwards. One barrier per stage, the raw
// s_barrier behind an lgkmcnt-only wait as in gemm_m16 (__syncthreads()
// would drain vmcnt and with it the weight stream). Rows >= M read row
// M - 1 and are never stored; a short last stage (int8, K % 128 == 64)
// clamps its source k into the row.
//
// W: fetched from global memory in fragment shape (lane l: column l & 15,
// k-slice l >> 4), the loads and scales of stage i + 1 issued together
// with the x loads before stage i is consumed (two register sets, the
// stage loop unrolled by two). Columns >= N read row N - 1 and are never
// stored; no address is formed from an unclamped index.
//
// Grid: 1-D. Work item L = ntile * mtiles + mtile, so the M tiles of one
// weight strip are neighbours. Consecutive block ids are dealt round-robin
// to the 8 XCDs, each with an L2 of its own, so block b takes
// L = (b % 8) * ceil(items / 8) + b / 8: neighbouring items run on the
// same XCD and the strip is fetched from HBM once.
//
// Resources (hipcc -O3 --offload-arch=gfx950,
// -Rpass-analysis=kernel-resource-usage), launch bounds (256, 2), no
// scratch and no spills in any instantiation; 69632 B of dynamic LDS hold
// every one at two blocks per CU = 2 waves per SIMD, whatever the VGPR
// count alone would allow:
//   int8 NZ=2  202 VGPRs (2 waves/SIMD)   int8 NZ=1  128 VGPRs (4)
//   int4 NZ=2  168 VGPRs (3)              int4 NZ=1  112 VGPRs (4)
// The file is built with packed f32 ops left on (not in _NO_PACKED_F32 of
// build.py, like gemm_m16): its only f32 VALU arithmetic is q * s and
// acc + bias, single IEEE operations whose bits do not depend on pairing.
#include "common.h"

namespace dnet {

using i32x4 = __attribute__((ext_vector_type(4))) int;

constexpr int kRowsBM = 128;                // rows per block tile
constexpr int kRowsMT = kRowsBM / 16;       // stacked 16-row A tiles
constexpr int kRowsKT = 128;                // k per stage
constexpr int kRowsSE = kRowsKT + 8;        // LDS row stride (16 B pad)
constexpr int kRowsImg = kRowsBM * kRowsSE; // one x image, bf16 elements
constexpr int kRowsLds = 2 * kRowsImg * (int)sizeof(short);
constexpr int kRowsXV = kRowsBM * (kRowsKT / 8) / 256;  // 16 B loads/thread
constexpr int kRowsXcds = 8;
// s_waitcnt immediate (gfx9 encoding): lgkmcnt(0), vmcnt and expcnt free
constexpr int kRowsWaitLgkm0 = 0xC07F;

// One stage's weights of a lane: NZ column sets, 128 k each.
template <int QBITS, int NZ>
struct RowsWSet {
  static constexpr int NL = QBITS == 8 ? 2 : 1;   // 16 B loads per column
  i32x4 q[NZ][NL];
  unsigned short s[NZ][NL];
};

template <int QBITS, int NZ>
__global__ __launch_bounds__(256, 2) void gemm_rows_kernel(
    const short* __restrict__ x, const void* __restrict__ w,
    const short* __restrict__ scales, const short* __restrict__ bias,
    short* __restrict__ out, const int M, const int K, const int N,
    const int G, const int mtiles, const int items) {
  using WS = RowsWSet<QBITS, NZ>;
  extern __shared__ __attribute__((aligned(16))) char gemm_rows_smem[];
  short* const img0 = reinterpret_cast<short*>(gemm_rows_smem);
  short* const img1 = img0 + kRowsImg;
  const int per = (items + kRowsXcds - 1) / kRowsXcds;
  const int item = ((int)blockIdx.x % kRowsXcds) * per +
                   (int)blockIdx.x / kRowsXcds;
  if (item >= items) return;           // block-uniform
  const int m0 = (item % mtiles) * kRowsBM;
  const int wave = threadIdx.x / kWave;
  const int lane = threadIdx.x & (kWave - 1);
  const int col = lane & 15;
  const int sl = lane >> 4;            // k-slice of this lane
  const int n0 = (item / mtiles) * (64 * NZ) + wave * (16 * NZ);

  // this lane's NZ weight rows (a wave past N keeps the barriers, reads
  // row N - 1 and stores nothing)
  const char* wp[NZ];
  const unsigned short* sp[NZ];
#pragma unroll
  for (int z = 0; z < NZ; ++z) {
    const int64_t n_w = min(n0 + z * 16 + col, N - 1);
    wp[z] = (const char*)w + n_w * (QBITS == 8 ? K : K / 2) + sl * 16;
    sp[z] = (const unsigned short*)scales + n_w * (K / G);
  }
  // x staging: load v of a thread is chunk (tid & 15) of row v * 16 +
  // tid / 16, so 16 threads read one 256 B row segment
  const int xc = (threadIdx.x & 15) * 8;
  const int xr0 = threadIdx.x >> 4;
  // (block-uniform 64-bit base + 32-bit offsets inside the 128-row tile:
  // at most 127 * K + K - 8, which the host keeps below 2^31 by K < 2^24)
  const short* const xblk = x + (int64_t)m0 * K;
  int xoff[kRowsXV];
#pragma unroll
  for (int v = 0; v < kRowsXV; ++v)
    xoff[v] = min(v * 16 + xr0, M - 1 - m0) * K;

  f32x4 acc[kRowsMT][NZ];
#pragma unroll
  for (int t = 0; t < kRowsMT; ++t)
#pragma unroll
    for (int z = 0; z < NZ; ++z) acc[t][z] = {0.f, 0.f, 0.f, 0.f};

  const int nst = (K + kRowsKT - 1) / kRowsKT;

  // issue the loads of stage i: its x rows and its weights + scales. A
  // short stage (64 k) clamps the x source into the row (those image
  // columns are never read) and loads its one pair only.
  auto issue = [&](const int i, i32x4 (&xr)[kRowsXV], WS& ws)
      __attribute__((always_inline)) {
    const int k0 = i * kRowsKT;
    const int tk = min(kRowsKT, K - k0);
    const int kx = k0 + min(xc, tk - 8);
#pragma unroll
    for (int v = 0; v < kRowsXV; ++v)
      xr[v] = *reinterpret_cast<const i32x4*>(xblk + (xoff[v] + kx));
#pragma unroll
    for (int z = 0; z < NZ; ++z) {
      if (QBITS == 8) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          if (u * 64 < tk) {
            ws.q[z][u] =
                *reinterpret_cast<const i32x4*>(wp[z] + (k0 + u * 64));
            ws.s[z][u] = sp[z][(k0 + u * 64) / G];
          } else {
            ws.q[z][u] = i32x4{0, 0, 0, 0};
            ws.s[z][u] = 0;
          }
        }
      } else {
        ws.q[z][0] = *reinterpret_cast<const i32x4*>(wp[z] + k0 / 2);
        ws.s[z][0] = sp[z][k0 / G];
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  auto store = [&](const i32x4 (&xr)[kRowsXV], short* img)
      __attribute__((always_inline)) {
#pragma unroll
    for (int v = 0; v < kRowsXV; ++v)
      *reinterpret_cast<i32x4*>(&img[(v * 16 + xr0) * kRowsSE + xc]) = xr[v];
  };
  // dequant + MFMA of one stage: chunk c is k = c * 32 .. c * 32 + 31
  auto consume = [&](const int i, const short* img, const WS& ws)
      __attribute__((always_inline)) {
    const int nch = min(kRowsKT, K - i * kRowsKT) / 32;   // block-uniform
    const short* arow = img + col * kRowsSE + sl * 8;
#pragma unroll
    for (int c = 0; c < kRowsKT / 32; ++c) {
      if (c >= nch) break;
      bf16x8 b[NZ];
#pragma unroll
      for (int z = 0; z < NZ; ++z) {
        if (QBITS == 8) {
          // opaque copy at the use: otherwise the bytes of the whole set
          // are extracted a stage early and held in registers (gemm_m16)
          i32x4 wq = ws.q[z][c >> 1];
          asm volatile("" : "+v"(wq));
          const int8_t* q8 = reinterpret_cast<const int8_t*>(&wq);
          b[z] = deq8(q8 + (c & 1) * 8, bits2f((short)ws.s[z][c >> 1]));
        } else {
          i32x4 wq = ws.q[z][0];
          asm volatile("" : "+v"(wq));
          const uint8_t* q4 = reinterpret_cast<const uint8_t*>(&wq);
          b[z] = deq4(q4 + c * 4, bits2f((short)ws.s[z][0]));
        }
      }
#pragma unroll
      for (int t = 0; t < kRowsMT; ++t) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(
            &arow[t * 16 * kRowsSE + c * 32]);
#pragma unroll
        for (int z = 0; z < NZ; ++z)
          acc[t][z] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[z],
                                                              acc[t][z], 0, 0, 0);
      }
    }
  };
  // one pipeline step: publish stage i, put stage i + 1 in flight,
  // consume stage i, then hand stage i + 1's x rows to the other image
  i32x4 xr[kRowsXV];
  auto step = [&](const int i, const short* img, short* img_next,
                  const WS& cur, WS& nxt) __attribute__((always_inline)) {
    // every wave's image writes have landed (lgkmcnt) before it arrives,
    // and the readers of the image written below have finished with it
    __builtin_amdgcn_s_waitcnt(kRowsWaitLgkm0);
    asm volatile("s_barrier" ::: "memory");
    const bool more = i + 1 < nst;     // block-uniform
    if (more) issue(i + 1, xr, nxt);
    consume(i, img, cur);
    __builtin_amdgcn_sched_barrier(0);
    if (more) store(xr, img_next);
  };

  WS wa, wb;
  issue(0, xr, wa);
  store(xr, img0);
  for (int i = 0; i < nst; i += 2) {
    step(i, img0, img1, wa, wb);
    if (i + 1 < nst) step(i + 1, img1, img0, wb, wa);
  }

  // C: lane covers column (lane & 15) of each column set, rows
  // (lane >> 4) * 4 + 0..3 of each stacked tile
#pragma unroll
  for (int z = 0; z < NZ; ++z) {
    const int n = n0 + z * 16 + col;
    if (n >= N) continue;
    const float bz = bias != nullptr ? bits2f(bias[n]) : 0.f;
#pragma unroll
    for (int t = 0; t < kRowsMT; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + t * 16 + sl * 4 + r;
        if (m < M) out[(int64_t)m * N + n] = f2bits(acc[t][z][r] + bz);
      }
    }
  }
}

template <int QBITS, int NZ>
static void gemm_rows_launch(unsigned grid, hipStream_t stream,
                             const short* x, const void* w, const short* sc,
                             const short* bias, short* out, int M, int K,
                             int N, int G, int mtiles, int items) {
  static const bool raised = []() {
    DNET_CHECK_HIP(hipFuncSetAttribute(
        reinterpret_cast<const void*>(&gemm_rows_kernel<QBITS, NZ>),
        hipFuncAttributeMaxDynamicSharedMemorySize, kRowsLds));
    return true;
  }();
  (void)raised;
  hipLaunchKernelGGL((gemm_rows_kernel<QBITS, NZ>), dim3(grid), dim3(256),
                     kRowsLds, stream, x, w, sc, bias, out, M, K, N, G,
                     mtiles, items);
}

void gemm_rows(torch::Tensor x, torch::Tensor w, torch::Tensor scales,
               c10::optional<torch::Tensor> bias, torch::Tensor out,
               int64_t group, int64_t bits) {
  DNET_CHECK(x.is_cuda() && w.is_cuda() && scales.is_cuda() && out.is_cuda(),
             "gemm_rows: device tensors");
  DNET_CHECK(x.dim() == 2 && w.dim() == 2 && out.dim() == 2 &&
                 scales.dim() == 2, "gemm_rows: 2-D tensors");
  const int64_t M = x.size(0), K = x.size(1), N = w.size(0);
  DNET_CHECK(bits == 8 || bits == 4, "gemm_rows: bits is 8 or 4");
  DNET_CHECK(M > 64 && N > 0 && K > 0, "gemm_rows: M > 64");
  DNET_CHECK(x.scalar_type() == torch::kBFloat16 && x.is_contiguous(),
             "gemm_rows: x is contiguous bf16");
  DNET_CHECK(out.scalar_type() == torch::kBFloat16 && out.is_contiguous() &&
                 out.size(0) == M && out.size(1) == N,
             "gemm_rows: out is contiguous bf16 [M, N]");
  const int64_t align = bits == 8 ? 64 : 128;
  DNET_CHECK(group > 0 && K % align == 0 && group % align == 0 &&
                 K % group == 0,
             "gemm_rows: K and group alignment (int8 64, int4 128)");
  DNET_CHECK(w.is_contiguous() &&
                 w.scalar_type() == (bits == 8 ? torch::kChar : torch::kByte) &&
                 w.size(1) == (bits == 8 ? K : K / 2),
             "gemm_rows: packed weights [N, K] int8 or [N, K/2] uint8");
  DNET_CHECK(scales.scalar_type() == torch::kBFloat16 &&
                 scales.is_contiguous() && scales.size(0) == N &&
                 scales.size(1) == K / group, "gemm_rows: scales bf16 [N, K/G]");
  if (bias.has_value())
    DNET_CHECK(bias->is_cuda() && bias->scalar_type() == torch::kBFloat16 &&
                   bias->is_contiguous() && bias->numel() == N,
               "gemm_rows: bias bf16 [N]");
  // the kernel's 32-bit x offsets span the 128 rows of one M tile
  // (127 * K + k < 2^31 needs K < 2^24); everything else goes through int64
  DNET_CHECK(M < (1 << 30) && N < (1 << 30) && K < (1 << 24),
             "gemm_rows: dims (K < 2^24)");
  const int mtiles = cdiv(M, kRowsBM);
  // 128-column blocks when they give every CU two blocks, else 64
  const int nz = (int64_t)mtiles * cdiv(N, 128) >= 512 ? 2 : 1;
  const int64_t items64 = (int64_t)mtiles * cdiv(N, 64 * nz);
  DNET_CHECK(items64 < (1 << 30), "gemm_rows: grid");
  const int items = (int)items64;
  const unsigned grid = (unsigned)(cdiv(items, kRowsXcds) * kRowsXcds);
  auto stream = current_stream();
  const short* bp =
      bias.has_value() ? (const short*)bias->data_ptr() : nullptr;
#define ROWS_GEMM(QQ, ZZ)                                                     \
  gemm_rows_launch<QQ, ZZ>(grid, stream, (const short*)x.data_ptr(),          \
                           w.data_ptr(), (const short*)scales.data_ptr(), bp, \
                           (short*)out.data_ptr(), (int)M, (int)K, (int)N,    \
                           (int)group, mtiles, items)
  if (bits == 8) {
    if (nz == 2) ROWS_GEMM(8, 2); else ROWS_GEMM(8, 1);
  } else {
    if (nz == 2) ROWS_GEMM(4, 2); else ROWS_GEMM(4, 1);
  }
#undef ROWS_GEMM
}

}  // namespace dnet
