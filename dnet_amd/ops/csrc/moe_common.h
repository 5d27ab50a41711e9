// Helpers shared by the grouped MoE kernels (moe.hip.cpp: M <= 64 rows,
// moe_int4.hip.cpp: its MFMA pair for int4 banks, moe_rows.hip.cpp:
// token-routed MFMA path, moe_rows_int4.hip.cpp: that path for int4 banks).
#pragma once

#include "common.h"

namespace dnet {

// GLU = 0: silu(g) * u   GLU = 1: gpt-oss clamped (u+1) * g * sigmoid(g*a)
template <int GLU>
__device__ __forceinline__ float apply_glu(float g, float u, const float alpha,
                                           const float limit) {
  if (GLU == 1) {
    g = fminf(g, limit);
    u = fminf(fmaxf(u, -limit), limit);
    return (u + 1.f) * g / (1.f + __expf(-g * alpha));
  }
  return g / (1.f + __expf(-g)) * u;
}

// int4 (uint8 nibbles in the pack_int4_mfma layout + bf16 group scales)
// banks: the MFMA pair of moe_int4.hip.cpp, reached through moe_gateup /
// moe_down. `out` need not be zeroed.
void moe_int4_gateup(torch::Tensor x, torch::Tensor w,
                     c10::optional<torch::Tensor> scales,
                     c10::optional<torch::Tensor> bias, torch::Tensor we,
                     torch::Tensor act, int64_t group, int64_t glu,
                     double alpha, double limit);
void moe_int4_down(torch::Tensor act, torch::Tensor w,
                   c10::optional<torch::Tensor> scales,
                   c10::optional<torch::Tensor> bias, torch::Tensor we,
                   torch::Tensor out, int64_t group);

void moe_int4_force_ks(int64_t ks);

// out[t, :] = sum of y over token_slots[t] in order (moe_rows.hip.cpp);
// the launch that ends moe_rows_down and moe_rows_int4_down.
void moe_rows_combine(const torch::Tensor& y, const torch::Tensor& token_slots,
                      torch::Tensor& out, hipStream_t stream);

// uint8 banks come in two formats, told apart by the scales: bf16 group
// scales = int4, e8m0 uint8 block scales = mxfp4.
inline bool moe_bank_is_int4(const torch::Tensor& w,
                             const c10::optional<torch::Tensor>& scales) {
  return w.scalar_type() == torch::kByte && scales.has_value() &&
         scales->scalar_type() == torch::kBFloat16;
}

}  // namespace dnet
