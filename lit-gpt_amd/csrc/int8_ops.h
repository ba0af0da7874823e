// Device helpers shared by the LLM.int8 kernels (gemv_int8.hip, gemm_int8.hip): one definition of the rounding and
// of the dequantization constant, so the decode and prefill paths produce the same bits.
#pragma once
#include "common.h"

namespace lga {

// clamp(rint(x * inv), -127, 127), round to nearest even; inv = 127 / absmax in fp32 (0 for an all-zero row)
__device__ __forceinline__ int q8(float x, float inv) {
  return (int)fminf(fmaxf(rintf(mul_rn(x, inv)), -127.0f), 127.0f);
}
__device__ __forceinline__ float q8_inv(float absmax) { return absmax > 0.0f ? 127.0f / absmax : 0.0f; }
// signed byte b (0..3) of w as float
__device__ __forceinline__ float sbyte(uint32_t w, int b) { return (float)((int)(w << (24 - 8 * b)) >> 24); }

constexpr float kInt8C = (float)(1.0 / 16129.0);  // 1 / 127^2

// float(acc) * ((s_x * s_w) * C), every operation fp32 in this association
__device__ __forceinline__ float int8_main(int acc, float sx, float sw) {
  return mul_rn((float)acc, mul_rn(mul_rn(sx, sw), kInt8C));
}

}  // namespace lga
