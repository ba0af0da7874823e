// Device helpers of the fp8 (OCP e4m3) KV cache: the row quantizer and the two expansions the attention kernels use.
//
// The format: a row is the 128 bf16 values of one (slot, query group, position) of K or V, held by a
// 16-lane row group at 8 values per lane. amax = max |x_i| = m 2^E with m in [0.5, 1); the scale is s = 2^e with
// e = E - 9 when m <= 0.875, else E - 8 (the smallest power of two with amax / s <= 448), clamped to [-126, 127];
// amax = 0 gives s = 1. code_i = e4m3(x_i / s), round to nearest even; nothing saturates. x_i / s is exact (a power
// of two) and so is float(code_i) * s in bf16.
#pragma once
#include "decode_ops.h"

namespace lga {

typedef float f32x2_t __attribute__((ext_vector_type(2)));

// max over the 16 lanes of a row group (a DPP row), in every lane of it
__device__ __forceinline__ uint32_t row_group_umax16(uint32_t v) {
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false));
  return v;
}

// The scale rule on the row's largest bf16 magnitude (its 15 bits a16 = biased exponent << 7 | 7 mantissa bits):
// amax = 1.f 2^(be - 127) = m 2^(be - 126), and m <= 0.875 <=> 1.f <= 1.75 <=> f <= 0x60. Returns s, 1 / s in inv.
// (A finite bf16 has be <= 254, so e <= 120 and 1 / s = 2^-e is a normal fp32.)
__device__ __forceinline__ float kv8_scale(uint32_t a16, float& inv) {
  int e = 0;
  if (a16 != 0) {
    e = (int)(a16 >> 7) - 126 - ((a16 & 0x7Fu) <= 0x60u ? 9 : 8);
    e = min(max(e, -126), 127);
  }
  inv = __uint_as_float((uint32_t)(127 - e) << 23);
  return __uint_as_float((uint32_t)(127 + e) << 23);
}

// Quantize the 8 bf16 values this lane holds of a row spread over its 16-lane row group (all 16 lanes active):
// returns the 8 codes (value i in byte i) and the row's scale in every lane.
__device__ __forceinline__ uint2 kv8_quantize8(const uint4 x, float& scale) {
  const uint32_t d[4] = {x.x, x.y, x.z, x.w};
  uint32_t mx = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) mx = max(mx, max(d[i] & 0x7FFFu, (d[i] >> 16) & 0x7FFFu));
  mx = row_group_umax16(mx);
  float inv;
  scale = kv8_scale(mx, inv);
  int w[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    w[i] = __builtin_amdgcn_cvt_pk_fp8_f32(bflo(d[2 * i]) * inv, bfhi(d[2 * i]) * inv, 0, false);
    w[i] = __builtin_amdgcn_cvt_pk_fp8_f32(bflo(d[2 * i + 1]) * inv, bfhi(d[2 * i + 1]) * inv, w[i], true);
  }
  return make_uint2((uint32_t)w[0], (uint32_t)w[1]);
}

// 8 codes -> 8 packed bf16 (unscaled: every e4m3 value is exact in bf16; the row scale is applied to the score)
__device__ __forceinline__ uint4 kv8_bf16x8(const uint2 c) {
  return make_uint4(__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c.x, 1.0f, false)),
                    __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c.x, 1.0f, true)),
                    __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c.y, 1.0f, false)),
                    __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c.y, 1.0f, true)));
}

// 8 codes -> 8 fp32 (unscaled)
__device__ __forceinline__ void kv8_f32x8(const uint2 c, float* f) {
  const f32x2_t a = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.x, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.x, true);
  const f32x2_t p = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.y, false), q = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.y, true);
  f[0] = a.x, f[1] = a.y, f[2] = b.x, f[3] = b.y;
  f[4] = p.x, f[5] = p.y, f[6] = q.x, f[7] = q.y;
}

}  // namespace lga
