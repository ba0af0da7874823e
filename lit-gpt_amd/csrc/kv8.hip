// The T-row side of the fp8 (e4m3) KV cache (the decode attention over it lives in attention.hip):
//   lga_kv8_rope_append  lga_rope_kv_append for fp8 caches — roped q to q_out, k (roped) and v quantized row by row
//                        into the code / scale arrays at cache_pos. The RoPE is the decode kernel's rope8 and the
//                        quantizer its kv8_quantize8, so a prefill row and a decode row of the same values store the
//                        same bits.
//   lga_kv8_dequantize   rows [0, n) of one slot's codes and scales -> bf16 (G, n, 128) buffers (exact), which the
//                        MFMA prefill attention then reads as a bf16 cache.
#include <algorithm>

#include "kv8_ops.h"

namespace lga {

// one 16-lane row group per head row of the (T, G, q_per_kv + 2) rows of qkv; 16 row groups per workgroup
__global__ void __launch_bounds__(256) kv8_rope_append_kernel(
    const uint16_t* __restrict__ qkv, uint16_t* __restrict__ q_out, uint8_t* __restrict__ kc, uint8_t* __restrict__ vc,
    float* __restrict__ ksc, float* __restrict__ vsc, const int64_t* __restrict__ cache_pos,
    const int64_t* __restrict__ rope_pos, const float* __restrict__ cos, const float* __restrict__ sin, int T,
    int n_head, int n_groups, int max_seq, int rope_rows) {
  constexpr int HS = 128, LPR = HS / 8;
  const int qpk = n_head / n_groups;
  const long rows = (long)T * n_groups * (qpk + 2);
  const long row = (long)blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
  if (row >= rows) return;  // (whole row groups: the DPP rows below stay fully active)
  const int sub = threadIdx.x % LPR;
  const int t = (int)(row / (n_groups * (qpk + 2))), rem = (int)(row % (n_groups * (qpk + 2)));
  const int g = rem / (qpk + 2), slot = rem % (qpk + 2);
  const long p = cache_pos[t], rp = rope_pos[t];
  if (p < 0 || p >= max_seq || rp < 0 || rp >= rope_rows) return;  // host validates; never out of bounds
  uint4 x = *(const uint4*)(qkv + ((size_t)t * (n_head + 2 * n_groups) + (size_t)g * (qpk + 2) + slot) * HS + sub * 8);
  if (slot <= qpk) {  // q heads and k
    float cs[8], sn[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      cs[i] = cos[(size_t)rp * HS + sub * 8 + i];
      sn[i] = sin[(size_t)rp * HS + sub * 8 + i];
    }
    x = rope8(x, cs, sn, sub);
  }
  if (slot < qpk) {
    *(uint4*)(q_out + ((size_t)t * n_head + (size_t)g * qpk + slot) * HS + sub * 8) = x;
    return;
  }
  float s;
  const uint2 c8 = kv8_quantize8(x, s);
  const size_t dst = (size_t)g * max_seq + p;
  *(uint2*)((slot == qpk ? kc : vc) + dst * HS + sub * 8) = c8;
  if (sub == 0) (slot == qpk ? ksc : vsc)[dst] = s;
}

// grid.y = 0: K, 1: V; a thread expands 8 codes of one row
__global__ void __launch_bounds__(256) kv8_dequantize_kernel(const uint8_t* __restrict__ kc,
                                                             const uint8_t* __restrict__ vc,
                                                             const float* __restrict__ ksc,
                                                             const float* __restrict__ vsc, uint16_t* __restrict__ ko,
                                                             uint16_t* __restrict__ vo, int n_groups, int n,
                                                             int max_seq) {
  constexpr int HS = 128, LPR = HS / 8;
  const uint8_t* codes = blockIdx.y ? vc : kc;
  const float* scales = blockIdx.y ? vsc : ksc;
  uint16_t* out = blockIdx.y ? vo : ko;
  const long total = (long)n_groups * n * LPR;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int sub = (int)(i % LPR);
    const long r = i / LPR;
    const int g = (int)(r / n), j = (int)(r % n);
    const size_t src = (size_t)g * max_seq + j;
    const uint2 c8 = *(const uint2*)(codes + src * HS + sub * 8);
    const float s = scales[src];
    float f[8];
    kv8_f32x8(c8, f);
    *(uint4*)(out + (size_t)r * HS + sub * 8) =
        make_uint4(pack2(f[0] * s, f[1] * s), pack2(f[2] * s, f[3] * s), pack2(f[4] * s, f[5] * s),
                   pack2(f[6] * s, f[7] * s));
  }
}

}  // namespace lga

extern "C" int lga_kv8_rope_append(const void* qkv, void* q_out, void* k_codes, void* v_codes, float* k_scale,
                                   float* v_scale, const int64_t* cache_pos, const int64_t* rope_pos, const float* cos,
                                   const float* sin, int rope_rows, int T, int n_head, int n_query_groups,
                                   int head_size, int rope_n_elem, int max_seq, hipStream_t stream) {
  LGA_CHECK_ARG(qkv && q_out && k_codes && v_codes && k_scale && v_scale && cache_pos && rope_pos && cos && sin,
                "lga_kv8_rope_append: null pointer");
  LGA_CHECK_ARG(T > 0 && n_query_groups > 0 && n_head > 0 && n_head % n_query_groups == 0,
                "lga_kv8_rope_append: bad head geometry");
  LGA_CHECK_ARG(head_size == 128 && rope_n_elem == 128,
                "lga_kv8_rope_append: needs head_size == rope_n_elem == 128");
  LGA_CHECK_ARG(rope_rows > 0 && max_seq > 0, "lga_kv8_rope_append: empty rope cache or kv cache");
  const long rows = (long)T * (n_head + 2 * n_query_groups);
  lga::kv8_rope_append_kernel<<<(unsigned)((rows + 15) / 16), 256, 0, stream>>>(
      (const uint16_t*)qkv, (uint16_t*)q_out, (uint8_t*)k_codes, (uint8_t*)v_codes, k_scale, v_scale, cache_pos,
      rope_pos, cos, sin, T, n_head, n_query_groups, max_seq, rope_rows);
  LGA_LAUNCH_RETURN();
}

extern "C" int lga_kv8_dequantize(const void* k_codes, const void* v_codes, const float* k_scale,
                                  const float* v_scale, void* k_out, void* v_out, int n_query_groups, int n,
                                  int head_size, int max_seq, hipStream_t stream) {
  LGA_CHECK_ARG(k_codes && v_codes && k_scale && v_scale && k_out && v_out, "lga_kv8_dequantize: null pointer");
  LGA_CHECK_ARG(head_size == 128, "lga_kv8_dequantize: needs head_size == 128");
  LGA_CHECK_ARG(n_query_groups > 0 && n > 0 && n <= max_seq, "lga_kv8_dequantize: rows must be in [1, max_seq]");
  const long chunks = (long)n_query_groups * n * 16;
  const dim3 grid((unsigned)std::min<long>((chunks + 255) / 256, 4096), 2);
  lga::kv8_dequantize_kernel<<<grid, 256, 0, stream>>>((const uint8_t*)k_codes, (const uint8_t*)v_codes, k_scale,
                                                       v_scale, (uint16_t*)k_out, (uint16_t*)v_out, n_query_groups, n,
                                                       max_seq);
  LGA_LAUNCH_RETURN();
}
