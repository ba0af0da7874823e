// Batch-1 decode GEMV over bf16 weights: y[n] = sum_k x[k] * W[n, k]  (+ the same fused epilogues as gemv.hip)
//
// Serves BASELINE config 2 (Llama-2-7B with unquantized bf16 weights, precision bf16-true): every Linear of the
// decode step stays an nn.Linear (reference generate/base.py:128-136 without --quantize) and its one-token
// forward (`F.linear`, lit_gpt/model.py:619, :656, :712-716, :519) lands here instead of a rocBLAS GEMV.
//
// A bf16 GEMV moves 2 bytes per weight (13.2 GB per Llama-2-7B token) at ~0.5 flop/byte: a pure HBM stream on the pass
// skeleton (gemv_pass.h). A 16-B chunk is 8 weights against one uint4 of x, v_dot2c_f32_bf16 straight on the
// (w_k, w_k+1) / (x_k, x_k+1) pairs with fp32 accumulation; a pass is 8 chunks per lane (4096 columns). One pass
// (K <= 4096) runs 2 rows per wave (fc_1 || fc_2: 1 row of each); longer rows 1 row per wave, which keeps both pass
// buffers within ~64-128 VGPRs. The norm fuses at every K.
#include "gemv_pass.h"

namespace lga {

struct Bf16Fmt {
  static constexpr int CPT = 8, PLANES = 1, SPL = 0;
  static constexpr int MAX_K = 32768, NORM_MAX_K = 32768;
  static constexpr bool RED_ALWAYS = true, PARTNER_DPP8 = true;
  static constexpr int rows(bool dual, bool multi) { return multi || dual ? 1 : 2; }
  __device__ static __forceinline__ float chunk_dot(const uint4 wv, const uint4 (&x)[1], float) {
    float d = dot2_bf16(wv.x, x[0].x, 0.0f);
    d = dot2_bf16(wv.y, x[0].y, d);
    d = dot2_bf16(wv.z, x[0].z, d);
    d = dot2_bf16(wv.w, x[0].w, d);
    return d;
  }
};

template <int RPR, bool DUAL, bool NORM, bool RES, int XPT, bool MULTI>
__global__ void __launch_bounds__(256) gemv_bf16_kernel(GemvPassArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  gemv_pass_body<Bf16Fmt, RPR, DUAL, NORM, RES, XPT, MULTI>(a, smem);
}

template <bool DUAL>
static int dispatch_b(const GemvPassArgs& a, const char* name, hipStream_t stream) {
  return gemv_dispatch<Bf16Fmt, DUAL>(a, name, [&](auto c) {
    using C = decltype(c);
    gemv_launch<C::RPR, DUAL, C::CAN_NORM>(a, [&](auto norm, auto res, dim3 blocks) {
      gemv_bf16_kernel<C::RPR, DUAL, decltype(norm)::value, decltype(res)::value, C::XPT, C::MULTI>
          <<<blocks, 256, gemv_pass_lds<Bf16Fmt>(a), stream>>>(a);
    });
  });
}

}  // namespace lga

extern "C" int lga_bf16_gemv(const void* x, const void* weight, const void* bias, const void* residual,
                             const void* norm_weight, float norm_eps, void* y, int N, int K, hipStream_t stream) {
  LGA_GEMV_CHECKS("lga_bf16_gemv", 8, x && weight && y, , (uintptr_t)x | (uintptr_t)weight, "x, weight");
  lga::GemvPassArgs a{(const uint16_t*)x, (const uint8_t*)weight, nullptr, nullptr, nullptr, (const uint16_t*)bias,
                      (const uint16_t*)residual, (const uint16_t*)norm_weight, (uint16_t*)y, N, K, norm_eps};
  const int rc = lga::dispatch_b<false>(a, "lga_bf16_gemv", stream);
  if (rc) return rc;
  LGA_LAUNCH_RETURN();
}

extern "C" int lga_bf16_gemv_swiglu(const void* x, const void* weight1, const void* weight2, const void* norm_weight,
                                    float norm_eps, void* y, int N, int K, hipStream_t stream) {
  LGA_GEMV_CHECKS("lga_bf16_gemv_swiglu", 8, x && weight1 && weight2 && y, ,
                  (uintptr_t)x | (uintptr_t)weight1 | (uintptr_t)weight2, "x, weights");
  lga::GemvPassArgs a{(const uint16_t*)x, (const uint8_t*)weight1, (const uint8_t*)weight2, nullptr, nullptr, nullptr,
                      nullptr, (const uint16_t*)norm_weight, (uint16_t*)y, N, K, norm_eps};
  const int rc = lga::dispatch_b<true>(a, "lga_bf16_gemv_swiglu", stream);
  if (rc) return rc;
  LGA_LAUNCH_RETURN();
}
