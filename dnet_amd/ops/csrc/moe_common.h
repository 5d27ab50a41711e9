// Helpers shared by the grouped MoE kernels (moe.hip.cpp: M <= 64 rows,
// moe_rows.hip.cpp: token-routed MFMA path).
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

}  // namespace dnet
