// Fused RMSNorm (+ optional residual add) for bf16 rows, f32 accumulation.
//
// y = (x / rms(x)) * w         (residual == nullptr)
// r = r + x; y = (r / rms(r)) * w   (fused residual update, in-place on r)
//
// MI355X-native: memory-bound; vectorized short8 (16 B/lane) loads
// (cdna_hip_programming.md G13: scalar bf16 loads are ~2x slower), one
// workgroup per row, grid-stride over rows.
#include "common.h"

namespace dnet {

// F32X: x comes from the UN-COMBINED f32 split-k partials of the
// producing GEMM (o/down projection): `splits` slices of [T,H], summed
// here in slice order and only read — the f32->bf16 combine kernel
// disappears from the decode chain. splits == 1 is the one legacy mode:
// a single [T,H] f32 buffer that is read and then re-zeroed, kept for
// callers that fill such a buffer themselves and expect it back zeroed.
template <bool HAS_RES, bool F32X = false>
__global__ void rmsnorm_kernel(const short* __restrict__ x,
                               short* __restrict__ res,  // in/out residual
                               const short* __restrict__ w,
                               short* __restrict__ y,
                               const int H, const float eps, const int T,
                               float* __restrict__ xf = nullptr,
                               const int splits = 1) {
  __shared__ float scratch[16];
  const int vecs = H / 8;  // H % 8 == 0 enforced on host
  for (int row = blockIdx.x; row < T; row += gridDim.x) {
    const short8* xv = reinterpret_cast<const short8*>(x + (int64_t)row * H);
    short8* rv = HAS_RES ? reinterpret_cast<short8*>(res + (int64_t)row * H) : nullptr;
    float ss = 0.f;
    for (int i = threadIdx.x; i < vecs; i += blockDim.x) {
      short8 v;
      if (F32X) {
        float* xr = xf + (int64_t)row * H + i * 8;
        const int64_t slice = (int64_t)T * H;
        const float* const src2[2] = {xr, xr + 4};
        float4 ab[2];
        sum_slices_multi<float4, 2>(src2, slice, splits, ab);
        const float4 a = ab[0], bq = ab[1];
        if (splits == 1) {
          reinterpret_cast<float4*>(xr)[0] = make_float4(0.f, 0.f, 0.f, 0.f);
          reinterpret_cast<float4*>(xr)[1] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const float av[8] = {a.x, a.y, a.z, a.w, bq.x, bq.y, bq.z, bq.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) v.x[j] = f2bits(av[j]);
      } else {
        v = xv[i];
      }
      if (HAS_RES) {
        short8 rr = rv[i];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float f = bits2f(v.x[j]) + bits2f(rr.x[j]);
          v.x[j] = f2bits(f);
        }
        rv[i] = v;  // residual stream updated in bf16
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = bits2f(v.x[j]);
        ss += f * f;
      }
    }
    ss = block_reduce_sum(ss, scratch);
    const float scale = rsqrtf(ss / (float)H + eps);
    const short8* src = HAS_RES ? rv : xv;
    const short8* wv = reinterpret_cast<const short8*>(w);
    short8* yv = reinterpret_cast<short8*>(y + (int64_t)row * H);
    for (int i = threadIdx.x; i < vecs; i += blockDim.x) {
      short8 v = src[i];
      short8 ww = wv[i];
      short8 out;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        out.x[j] = f2bits(bits2f(v.x[j]) * scale * bits2f(ww.x[j]));
      yv[i] = out;
    }
    __syncthreads();
  }
}

// rmsnorm_kernel<true, true> for splits > 1 and H <= 8192: the same
// arithmetic in the same order, spread over more waves. There a thread
// walks its 8-element vectors t, t + 256, t + 512, ... one after the other
// and every step waits for 2 * splits loads; a row of 5120 at 8 slices is
// three such round trips on 4 waves of one CU. Here the block has one
// 256-thread group per step, so all of a row's loads are in flight at
// once. Group g sums the slices of vector t + 256 g, adds the residual and
// keeps the rounded sum in registers for the output; groups > 0 pass their
// 8 values through LDS to group 0, which folds the squares in exactly the
// order the one-group kernel does (own vector first, then g = 1, 2, ...),
// so both kernels give the same bits. block_reduce_sum adds the other
// groups' zeros to that sum, which changes nothing.
__global__ __launch_bounds__(1024) void rmsnorm_slices_kernel(
    const float* __restrict__ xf, short* __restrict__ res,
    const short* __restrict__ w, short* __restrict__ y, const int H,
    const float eps, const int T, const int splits) {
  __shared__ float red[16];
  __shared__ float vals[3][8][256];  // [group - 1][element][thread]
  const int vecs = H / 8;
  const int g = threadIdx.x >> 8, t = threadIdx.x & 255;
  const int groups = blockDim.x >> 8;
  const int i = g * 256 + t;
  const bool act = i < vecs;
  const int64_t slice = (int64_t)T * H;
  for (int row = blockIdx.x; row < T; row += gridDim.x) {
    short8 v;
    float f[8];
    if (act) {
      const float* xr = xf + (int64_t)row * H + i * 8;
      const float* const src2[2] = {xr, xr + 4};
      float4 ab[2];
      sum_slices_multi<float4, 2>(src2, slice, splits, ab);
      const float av[8] = {ab[0].x, ab[0].y, ab[0].z, ab[0].w,
                           ab[1].x, ab[1].y, ab[1].z, ab[1].w};
      short8* rv = reinterpret_cast<short8*>(res + (int64_t)row * H);
      const short8 rr = rv[i];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        // two roundings, as in rmsnorm_kernel: the projection, then the sum
        v.x[j] = f2bits(bits2f(f2bits(av[j])) + bits2f(rr.x[j]));
        f[j] = bits2f(v.x[j]);
        if (g > 0) vals[g - 1][j][t] = f[j];
      }
      rv[i] = v;  // residual stream updated in bf16
    }
    __syncthreads();
    float ss = 0.f;
    if (g == 0) {
      if (act) {
#pragma unroll
        for (int j = 0; j < 8; ++j) ss += f[j] * f[j];
      }
      for (int gg = 1; gg < groups; ++gg) {
        if (gg * 256 + t < vecs) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float fv = vals[gg - 1][j][t];
            ss += fv * fv;
          }
        }
      }
    }
    ss = block_reduce_sum(ss, red);
    const float scale = rsqrtf(ss / (float)H + eps);
    if (act) {
      const short8 ww = reinterpret_cast<const short8*>(w)[i];
      short8 out;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        out.x[j] = f2bits(f[j] * scale * bits2f(ww.x[j]));
      reinterpret_cast<short8*>(y + (int64_t)row * H)[i] = out;
    }
    __syncthreads();
  }
}

// h += x where x is the sum of the `splits` f32 split-k slices (read
// only; splits == 1: the legacy read-and-re-zero mode, see
// rmsnorm_kernel): the final residual update of a decode window whose
// last down-projection was left deferred.
__global__ void resid_add_f32_kernel(short* __restrict__ h,
                                     float* __restrict__ xf,
                                     const int64_t total, const int splits) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float v = sum_slices(xf + i, total, splits);
    if (splits == 1) xf[i] = 0.f;
    h[i] = f2bits(bits2f(h[i]) + v);
  }
}

void resid_add_f32(torch::Tensor h, torch::Tensor xf, int64_t splits) {
  const int64_t total = h.numel();
  DNET_CHECK(h.is_contiguous() && xf.is_contiguous(), "contig");
  DNET_CHECK(splits >= 1 && xf.numel() >= splits * total,
             "partials too small");
  auto stream = current_stream();
  const int grid = (int)std::min<int64_t>((total + 255) / 256, 2048);
  hipLaunchKernelGGL(resid_add_f32_kernel, dim3(grid), dim3(256), 0, stream,
                     (short*)h.data_ptr(), (float*)xf.data_ptr(), total,
                     (int)splits);
}

// Split-k-fused variant: x is the sum of `splits` f32 partial slices.
void rmsnorm_f32(torch::Tensor xf, torch::Tensor residual, torch::Tensor w,
                 torch::Tensor y, double eps, int64_t splits) {
  const int64_t H = residual.size(-1);
  const int64_t T = residual.numel() / H;
  DNET_CHECK(H % 8 == 0, "H % 8");
  DNET_CHECK(splits >= 1 && xf.numel() >= splits * T * H,
             "partials too small");
  DNET_CHECK(residual.is_contiguous() && y.is_contiguous() &&
                 w.is_contiguous() && xf.is_contiguous(), "contig");
  auto stream = current_stream();
  const int grid = (int)std::min<int64_t>(T, 2048);
  const int64_t groups = (H / 8 + 255) / 256;
  if (splits > 1 && groups <= 4) {
    hipLaunchKernelGGL(rmsnorm_slices_kernel, dim3(grid),
                       dim3((unsigned)(256 * groups)), 0, stream,
                       (const float*)xf.data_ptr(),
                       (short*)residual.data_ptr(),
                       (const short*)w.data_ptr(), (short*)y.data_ptr(),
                       (int)H, (float)eps, (int)T, (int)splits);
    return;
  }
  hipLaunchKernelGGL((rmsnorm_kernel<true, true>), dim3(grid), dim3(256), 0,
                     stream, nullptr, (short*)residual.data_ptr(),
                     (const short*)w.data_ptr(), (short*)y.data_ptr(),
                     (int)H, (float)eps, (int)T, (float*)xf.data_ptr(),
                     (int)splits);
}

// y = rmsnorm(x) * w ; if residual is given: residual += x (in place), then
// y = rmsnorm(residual) * w.
void rmsnorm(torch::Tensor x, c10::optional<torch::Tensor> residual,
             torch::Tensor w, torch::Tensor y, double eps) {
  DNET_CHECK(x.is_cuda() && x.dtype() == torch::kBFloat16, "x must be bf16 on GPU");
  const int64_t H = x.size(-1);
  const int64_t T = x.numel() / H;
  DNET_CHECK(H % 8 == 0, "H must be a multiple of 8");
  DNET_CHECK(x.is_contiguous() && y.is_contiguous() && w.is_contiguous(), "contiguous");
  auto stream = current_stream();
  const int block = 256;
  const int grid = std::min<int64_t>(T, 2048);
  if (residual.has_value()) {
    DNET_CHECK(residual->is_contiguous(), "residual contiguous");
    hipLaunchKernelGGL(rmsnorm_kernel<true>, dim3(grid), dim3(block), 0, stream,
                       (const short*)x.data_ptr(), (short*)residual->data_ptr(),
                       (const short*)w.data_ptr(), (short*)y.data_ptr(),
                       (int)H, (float)eps, (int)T);
  } else {
    hipLaunchKernelGGL(rmsnorm_kernel<false>, dim3(grid), dim3(block), 0, stream,
                       (const short*)x.data_ptr(), nullptr,
                       (const short*)w.data_ptr(), (short*)y.data_ptr(),
                       (int)H, (float)eps, (int)T);
  }
}

}  // namespace dnet
