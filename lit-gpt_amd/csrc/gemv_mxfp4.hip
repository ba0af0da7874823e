// MXFP4 (OCP microscaling fp4) weights, --quantize mxfp4: the weight quantizer and the batch-1 decode GEMV
//   y[n] = sum_k x[k] * e2m1(code[n, k]) * 2^(scale[n, k / 32] - 127)   (+ the fused epilogues of gemv_bf16.hip)
//
// Format (include/litgpt_amd.h): codes (N, K / 2) uint8, two e2m1 codes per byte with the even column in
// the low nibble; scales (N, K / 32) uint8 e8m0, one per 32 consecutive weights of a row. Every dequantized weight is
// zero or a normal bf16, so the GEMV computes what lga_bf16_gemv computes on the dequantized weight, in its own order.
//
// The GEMV moves 4.25 bits per weight: the thinnest HBM stream of the project, and the most VALU and LDS work per byte.
// It is the pass skeleton (gemv_pass.h) with:
//  * A lane's 16-B load is 32 codes = exactly ONE MX block, so the chunk has one scale: the lane fetches that byte
//    itself (chunk c of row n is scales[n K/32 + c]; 64 lanes read 64 contiguous bytes; scale rows need no alignment).
//    The bytes stay raw until used (decode_ops.h).
//  * A pass is 2 chunks per lane. A Llama-2-7B row of K = 4096 is ONE pass of 2 KB, so the bytes in flight come from
//    rows: a wave owns 8 rows when the row is one pass (fc_1 || fc_2: 4 rows of each) and 4 rows when it is several
//    (fc_1 || fc_2: 2 of each). 16 x 16 B (+ 16 scale bytes) in flight per lane either way.
//  * A 16-B chunk meets 64 B of activations: FOUR planes of x, and the 64 B a lane reads serve all 8 (4) rows of the
//    wave — 8 B of LDS traffic per 16-B weight load at 8 rows.
//  * Expansion: one v_cvt_scalef32_pk_bf16_fp4 per code byte (byte select 0..3 of a dword), the block scale 2^(e - 127)
//    as its fp32 operand: two weights -> a packed bf16 pair with the scale applied, straight into v_dot2_f32_bf16.
//    16 converts + 16 dots per chunk, one VALU op per weight. The hardware returns the low nibble first (LGA_MXFP4_SWAP
//    rotates the x pairs instead, should a part return the other order).
// K limits: K % 32 == 0, K <= 32768; the RMSNorm fuses up to K = 12288 (longer rows take lga_rmsnorm first —
// Mxfp4Linear.gemv_fuses_norm).
#include "gemv_pass.h"

#ifndef LGA_MXFP4_SWAP
#define LGA_MXFP4_SWAP 0
#endif

namespace lga {

// ---------------------------------------------------------------------------------------------------- quantizer
// OCP MX v1.0 §6.3 on fp32 bits. Four lanes per 32-weight block, 8 weights per lane; 64 blocks per 256-thread workgroup.
//   e = clamp(biased exponent of amax - 2, 2, 252) (amax = 0: e = 127, all codes 0); v = |w| 2^(127 - e) < 8 (exact, or
//   an underflow far below the first tie at 0.25); magnitude code = the number of the seven round-to-nearest-even-code
//   thresholds at or below v; sign bit = the sign bit of w.
__device__ __forceinline__ uint32_t mx4_code(float w, float inv) {
  const float v = fabsf(w) * inv;
  const uint32_t m = (uint32_t)(v > 0.25f) + (uint32_t)(v >= 0.75f) + (uint32_t)(v > 1.25f) + (uint32_t)(v >= 1.75f) +
                     (uint32_t)(v > 2.5f) + (uint32_t)(v >= 3.5f) + (uint32_t)(v > 5.0f);
  return m | ((__float_as_uint(w) >> 31) << 3);
}

template <bool BF16>
__global__ void __launch_bounds__(256) mxfp4_quantize_kernel(const void* w, uint32_t* codes, uint8_t* scales,
                                                             size_t blocks) {
  const size_t b = (size_t)blockIdx.x * 64 + (threadIdx.x >> 2);
  const int sub = threadIdx.x & 3;
  const size_t bl = b < blocks ? b : blocks - 1;  // whole quads stay active for the DPP maximum
  const size_t at = bl * 32 + (size_t)sub * 8;
  float f[8];
  if (BF16) {
    unpack8(*(const uint4*)((const uint16_t*)w + at), f);
  } else {
    const float4 a = *(const float4*)((const float*)w + at), c = *(const float4*)((const float*)w + at + 4);
    f[0] = a.x, f[1] = a.y, f[2] = a.z, f[3] = a.w, f[4] = c.x, f[5] = c.y, f[6] = c.z, f[7] = c.w;
  }
  uint32_t mx = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) mx = max(mx, __float_as_uint(f[i]) & 0x7FFFFFFFu);
  mx = max(mx, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)mx, 0xB1, 0xF, 0xF, false));  // quad [1,0,3,2]
  mx = max(mx, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)mx, 0x4E, 0xF, 0xF, false));  // quad [2,3,0,1]
  const int e = mx == 0 ? 127 : min(max((int)(mx >> 23) - 2, 2), 252);
  const float inv = __uint_as_float((uint32_t)(254 - e) << 23);  // 2^(127 - e), a normal fp32
  uint32_t out = 0;
  if (mx != 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) out |= mx4_code(f[i], inv) << (4 * i);
  }
  if (b < blocks) {
    codes[b * 4 + sub] = out;
    if (sub == 0) scales[b] = (uint8_t)e;
  }
}

// ---------------------------------------------------------------------------------------------------- GEMV
// e8m0 byte -> 2^(e - 127) (the quantizer writes e in [2, 252]; e = 0 is 2^-127, a subnormal fp32)
__device__ __forceinline__ float e8m0_f32(uint32_t e) { return __uint_as_float(e ? e << 23 : 0x00400000u); }

// code byte B (0..3) of c, scaled by s, as a packed bf16 pair: (column 2 i, column 2 i + 1) of the byte's two codes
template <int B>
__device__ __forceinline__ uint32_t mx4_bf16x2(uint32_t c, float s) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, s, B));
}
__device__ __forceinline__ uint32_t mx4_xpair(uint32_t x) {  // the activation pair as the convert orders the codes
  return LGA_MXFP4_SWAP ? __builtin_amdgcn_alignbit(x, x, 16) : x;
}

// dot of code dword c (8 weights, scaled by s) against its 8 activations (xa: columns 0..3, xb: 4..7), onto d
__device__ __forceinline__ float mx4_dword_dot(uint32_t c, float s, uint32_t xa0, uint32_t xa1, uint32_t xb0,
                                               uint32_t xb1, float d) {
  d = dot2_bf16(mx4_bf16x2<0>(c, s), mx4_xpair(xa0), d);
  d = dot2_bf16(mx4_bf16x2<1>(c, s), mx4_xpair(xa1), d);
  d = dot2_bf16(mx4_bf16x2<2>(c, s), mx4_xpair(xb0), d);
  d = dot2_bf16(mx4_bf16x2<3>(c, s), mx4_xpair(xb1), d);
  return d;
}

// dot of one 32-weight block against its 32 activations: x[q] holds columns 8 q .. 8 q + 7
__device__ __forceinline__ float mx4_chunk_dot(const uint4 wv, const uint4 (&x)[4], float s) {
  float d = 0.0f;
  d = mx4_dword_dot(wv.x, s, x[0].x, x[0].y, x[0].z, x[0].w, d);
  d = mx4_dword_dot(wv.y, s, x[1].x, x[1].y, x[1].z, x[1].w, d);
  d = mx4_dword_dot(wv.z, s, x[2].x, x[2].y, x[2].z, x[2].w, d);
  d = mx4_dword_dot(wv.w, s, x[3].x, x[3].y, x[3].z, x[3].w, d);
  return d;
}

struct Mxfp4Fmt {
  static constexpr int CPT = 2, PLANES = 4, SPL = CPT;  // a chunk is one MX block: its scale byte is the lane's own
  static constexpr int MAX_K = 32768, NORM_MAX_K = 12288;
  static constexpr bool RED_ALWAYS = false, PARTNER_DPP8 = false;
  static constexpr int rows(bool dual, bool multi) { return (multi ? 4 : 8) / (dual ? 2 : 1); }
  __device__ static __forceinline__ uint32_t load_scale(const void* sc, size_t n, int K, int pass, int lane, int j) {
    const int nch = K / 32;
    return ((const uint8_t*)sc)[n * nch + min(pass * (64 * CPT) + lane + 64 * j, nch - 1)];
  }
  __device__ static __forceinline__ float scale(const uint32_t (&s)[SPL], int, int j) { return e8m0_f32(s[j]); }
  __device__ static __forceinline__ float chunk_dot(const uint4 wv, const uint4 (&x)[4], float s) {
    return mx4_chunk_dot(wv, x, s);
  }
};

template <int RPR, bool DUAL, bool NORM, bool RES, int XPT, bool MULTI>
__global__ void __launch_bounds__(256) gemv_mxfp4_kernel(GemvPassArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  gemv_pass_body<Mxfp4Fmt, RPR, DUAL, NORM, RES, XPT, MULTI>(a, smem);
}

template <bool DUAL>
static int dispatch_mx4(const GemvPassArgs& a, const char* name, hipStream_t stream) {
  return gemv_dispatch<Mxfp4Fmt, DUAL>(a, name, [&](auto c) {
    using C = decltype(c);
    gemv_launch<C::RPR, DUAL, C::CAN_NORM>(a, [&](auto norm, auto res, dim3 blocks) {
      gemv_mxfp4_kernel<C::RPR, DUAL, decltype(norm)::value, decltype(res)::value, C::XPT, C::MULTI>
          <<<blocks, 256, gemv_pass_lds<Mxfp4Fmt>(a), stream>>>(a);
    });
  });
}

int preload_mxfp4_gemv() {  // the lm_head launch of a prefill (no norm: it follows lga_rmsnorm there) and decode
  return preload(gemv_mxfp4_kernel<8, false, false, false, 2, false>) +
         preload(gemv_mxfp4_kernel<8, false, true, false, 2, false>);
}

}  // namespace lga

extern "C" int lga_mxfp4_quantize(const void* w, int w_is_bf16, uint8_t* codes, uint8_t* scales, int N, int K,
                                  hipStream_t stream) {
  LGA_CHECK_ARG(w && codes && scales, "lga_mxfp4_quantize: null pointer");
  LGA_CHECK_ARG(N > 0 && K > 0 && K % 32 == 0, "lga_mxfp4_quantize: K must be a positive multiple of 32");
  LGA_CHECK_ARG(((uintptr_t)w | (uintptr_t)codes) % 16 == 0, "lga_mxfp4_quantize: w and codes must be 16-B aligned");
  const size_t blocks = (size_t)N * (K / 32);
  const unsigned grid = (unsigned)((blocks + 63) / 64);
  if (w_is_bf16) lga::mxfp4_quantize_kernel<true><<<grid, 256, 0, stream>>>(w, (uint32_t*)codes, scales, blocks);
  else lga::mxfp4_quantize_kernel<false><<<grid, 256, 0, stream>>>(w, (uint32_t*)codes, scales, blocks);
  LGA_LAUNCH_RETURN();
}

extern "C" int lga_mxfp4_gemv(const void* x, const uint8_t* codes, const uint8_t* scales, const void* bias,
                              const void* residual, const void* norm_weight, float norm_eps, void* y, int N, int K,
                              hipStream_t stream) {
  LGA_GEMV_CHECKS("lga_mxfp4_gemv", 32, x && codes && scales && y,
                  LGA_GEMV_LIMITS("lga_mxfp4_gemv", 32768, 12288), (uintptr_t)x | (uintptr_t)codes, "x, codes");
  lga::GemvPassArgs a{(const uint16_t*)x, codes, nullptr, scales, nullptr, (const uint16_t*)bias,
                      (const uint16_t*)residual, (const uint16_t*)norm_weight, (uint16_t*)y, N, K, norm_eps};
  const int rc = lga::dispatch_mx4<false>(a, "lga_mxfp4_gemv", stream);
  if (rc) return rc;
  LGA_LAUNCH_RETURN();
}

extern "C" int lga_mxfp4_gemv_swiglu(const void* x, const uint8_t* codes1, const uint8_t* scales1,
                                     const uint8_t* codes2, const uint8_t* scales2, const void* norm_weight,
                                     float norm_eps, void* y, int N, int K, hipStream_t stream) {
  LGA_GEMV_CHECKS("lga_mxfp4_gemv_swiglu", 32, x && codes1 && scales1 && codes2 && scales2 && y,
                  LGA_GEMV_LIMITS("lga_mxfp4_gemv_swiglu", 32768, 12288),
                  (uintptr_t)x | (uintptr_t)codes1 | (uintptr_t)codes2, "x, codes");
  lga::GemvPassArgs a{(const uint16_t*)x, codes1, codes2, scales1, scales2, nullptr,
                      nullptr, (const uint16_t*)norm_weight, (uint16_t*)y, N, K, norm_eps};
  const int rc = lga::dispatch_mx4<true>(a, "lga_mxfp4_gemv_swiglu", stream);
  if (rc) return rc;
  LGA_LAUNCH_RETURN();
}

