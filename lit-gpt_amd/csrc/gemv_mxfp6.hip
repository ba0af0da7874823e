// MXFP6 (OCP microscaling fp6, e2m3) weights, --quantize mxfp6: the weight quantizer and the batch-1 decode GEMV
//   y[n] = sum_k x[k] * e2m3(code[n, k]) * 2^(scale[n, k / 32] - 127)   (+ the fused epilogues of gemv_bf16.hip)
//
// Format (include/litgpt_amd.h): codes (N, 3 K / 4) uint8, a block's 32 six-bit codes in 24 consecutive
// bytes, code i in bits 6 i .. 6 i + 5 of the block's 192-bit little-endian word (the order v_cvt_scalef32_pk32_bf16_fp6
// reads from 6 consecutive dwords); scales (N, K / 32) uint8 e8m0, one per 32 consecutive weights of a row, in [4, 252].
// Every dequantized weight is zero or a normal bf16, so the GEMV computes what lga_bf16_gemv computes on the
// dequantized weight, in its own order. K % 64 == 0: a row is a run of 48-B block pairs and starts 16-B aligned.
//
// The GEMV moves 6.25 bits per weight. It is built from the pieces of the pass skeleton (gemv_pass.h: the x fetch, the
// sum of squares, normalise, the pass loop, the butterfly and the epilogues, the K classes and the launcher), with a
// body of its own, because a lane's unit is no 16-B chunk:
//  * A lane's unit is a PAIR of MX blocks: 48 B of codes as three 16-B loads (lane l of a pass holds unit l, so a wave's
//    three load instructions of a row cover 3 KB contiguous), and its two scale bytes as ONE 16-bit load (unit u of row
//    n is scales[n K/32 + 2 u], 2-B aligned as K / 32 is even). The bytes stay raw until used.
//  * A pass is one unit per lane: 64 columns per lane, 4096 per wave. A Llama-2-7B row of K = 4096 is one pass, so the
//    bytes in flight come from rows: a wave owns 8 rows when the row is one pass (fc_1 || fc_2: 4 rows of each) and 4
//    rows, double-buffered, when it is several (fc_1 || fc_2: 2 of each): 24 x 16 B (+ 8 x 2 scale bytes) in flight per
//    lane either way.
//  * A unit meets 128 B of activations: x sits in LDS as EIGHT planes (plane q = the q-th 16 B of every unit's x), so
//    each of the eight ds_read_b128 is lane-contiguous (conflict-free), and the 128 B a lane reads serve all 8 (4) rows
//    of the wave: 16 B of LDS traffic per 48 B of weights at 8 rows.
//  * Expansion: ONE v_cvt_scalef32_pk32_bf16_fp6 per block, the block scale 2^(e - 127) as its fp32 operand: 32 codes
//    in 6 VGPRs -> 16 packed bf16 pairs with the scale applied, straight into 16 v_dot2_f32_bf16. 17 VALU ops per 32
//    weights (mxfp4: 32).
// K limits: K % 64 == 0, K <= 32768; the RMSNorm fuses up to K = 12288 (longer rows take lga_rmsnorm first —
// Mxfp6Linear.gemv_fuses_norm).
#include "gemv_pass.h"

namespace lga {

typedef unsigned u32x6_t __attribute__((ext_vector_type(6)));
typedef unsigned u32x16_t __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------------------- quantizer
// OCP MX v1.0 §6.3 with the e2m3 element, on fp32 bits. Four lanes per 32-weight block, 8 weights per lane (48 bits of
// codes, three 16-bit stores); 64 blocks per 256-thread workgroup.
//   e = clamp(biased exponent of amax - 2, 4, 252) (amax = 0: e = 127, all codes 0); v = |w| 2^(127 - e) < 8 (exact, or
//   an underflow far below the first tie at 1/16). The e2m3 magnitudes are a grid of step 1/8 below 2 (codes 0..16 are
//   8 v), 1/4 in [2, 4) (codes 4 v + 8) and 1/2 in [4, 8) (codes 2 v + 16), and in each range the code's parity is the
//   grid index's: v_rndne_f32 on the grid index is round-to-nearest, ties to the even code. 7.75 and above end at code
//   31 (7.5). Sign bit (bit 5) = the sign bit of w.
__device__ __forceinline__ uint32_t mx6_code(float w, float inv) {
  const float v = fabsf(w) * inv;
  const float g = v < 2.0f ? 8.0f : (v < 4.0f ? 4.0f : 2.0f);  // v g is exact; the offset goes on after the rounding
  const uint32_t m = min((uint32_t)rintf(v * g) + (v < 2.0f ? 0u : (v < 4.0f ? 8u : 16u)), 31u);
  return m | ((__float_as_uint(w) >> 31) << 5);
}

template <bool BF16>
__global__ void __launch_bounds__(256) mxfp6_quantize_kernel(const void* w, uint16_t* codes, uint8_t* scales,
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
  const int e = mx == 0 ? 127 : min(max((int)(mx >> 23) - 2, 4), 252);
  const float inv = __uint_as_float((uint32_t)(254 - e) << 23);  // 2^(127 - e), a normal fp32
  uint64_t out = 0;
  if (mx != 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) out |= (uint64_t)mx6_code(f[i], inv) << (6 * i);
  }
  if (b < blocks) {  // the lane's 48 bits are bytes 6 sub .. 6 sub + 5 of the block's 24
    uint16_t* o = codes + b * 12 + sub * 3;
    o[0] = (uint16_t)out, o[1] = (uint16_t)(out >> 16), o[2] = (uint16_t)(out >> 32);
    if (sub == 0) scales[b] = (uint8_t)e;
  }
}

// ---------------------------------------------------------------------------------------------------- GEMV
// e8m0 byte -> 2^(e - 127) (the quantizer writes e in [4, 252]; e = 0 is 2^-127, a subnormal fp32)
__device__ __forceinline__ float mx6_e8m0_f32(uint32_t e) { return __uint_as_float(e ? e << 23 : 0x00400000u); }

// dot of one 32-weight block (6 code dwords, scaled by s) against its 32 activations: x[q] holds columns 8 q .. 8 q + 7
__device__ __forceinline__ float mx6_block_dot(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t c4,
                                               uint32_t c5, float s, const uint4& x0, const uint4& x1, const uint4& x2,
                                               const uint4& x3) {
  const u32x6_t c = {c0, c1, c2, c3, c4, c5};
  const u32x16_t p = __builtin_bit_cast(u32x16_t, __builtin_amdgcn_cvt_scalef32_pk32_bf16_fp6(c, s));
  float d = 0.0f;
  d = dot2_bf16(p[0], x0.x, d), d = dot2_bf16(p[1], x0.y, d), d = dot2_bf16(p[2], x0.z, d), d = dot2_bf16(p[3], x0.w, d);
  d = dot2_bf16(p[4], x1.x, d), d = dot2_bf16(p[5], x1.y, d), d = dot2_bf16(p[6], x1.z, d), d = dot2_bf16(p[7], x1.w, d);
  d = dot2_bf16(p[8], x2.x, d), d = dot2_bf16(p[9], x2.y, d), d = dot2_bf16(p[10], x2.z, d), d = dot2_bf16(p[11], x2.w, d);
  d = dot2_bf16(p[12], x3.x, d), d = dot2_bf16(p[13], x3.y, d), d = dot2_bf16(p[14], x3.z, d), d = dot2_bf16(p[15], x3.w, d);
  return d;
}

// what the skeleton's dispatcher, launcher and epilogues ask of a format
struct Mxfp6Fmt {
  static constexpr int MAX_K = 32768, NORM_MAX_K = 12288;
  static constexpr bool PARTNER_DPP8 = false;
  static constexpr int rows(bool dual, bool multi) { return (multi ? 4 : 8) / (dual ? 2 : 1); }
};

// the loads of one pass in flight: the unit (three 16-B loads) of row i of matrix m and its two scale bytes
template <int NM, int RPR>
struct Mx6Buf {
  uint4 w[NM][RPR][3];
  uint32_t s[NM][RPR];
};

template <int NM, int RPR>
__device__ __forceinline__ void mx6_issue(Mx6Buf<NM, RPR>& buf, const GemvPassArgs& a, const int& row0, const int& lane,
                                          int pass) {
  const int nu = a.K / 64;
  const int u = min(pass * 64 + lane, nu - 1);  // units past the row re-read its last one; never used
  const uint8_t* wm[2] = {a.w, NM == 2 ? a.w2 : a.w};
  const void* sm[2] = {a.sc, NM == 2 ? a.sc2 : a.sc};
#pragma unroll
  for (int i = 0; i < RPR; ++i)
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      const size_t n = (size_t)min(row0 + i, a.N - 1);  // rows past N re-read row N - 1; never stored
      const uint8_t* p = wm[m] + (n * nu + (size_t)u) * 48;
#pragma unroll
      for (int j = 0; j < 3; ++j) buf.w[m][i][j] = ld_nt16(p + 16 * j);
    }
#pragma unroll
  for (int i = 0; i < RPR; ++i)
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      const size_t n = (size_t)min(row0 + i, a.N - 1);
      buf.s[m][i] = ((const uint16_t*)sm[m])[n * nu + (size_t)u];
    }
}

template <int RPR, bool DUAL, bool NORM, bool RES, int XPT, bool MULTI>
__global__ void __launch_bounds__(256) gemv_mxfp6_kernel(GemvPassArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4* xl = (uint4*)smem;                       // 8 planes of nu uint4
  float* red = (float*)(smem + (size_t)a.K * 2);  // 4 (NORM only)
  constexpr int NM = DUAL ? 2 : 1;
  constexpr int R = NM * RPR;
  static_assert(R == 4 || R == 8, "row partials per lane");
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int n8 = a.K / 8, nu = a.K / 64;
  const int passes = MULTI ? (nu + 63) / 64 : 1;
  const int row0 = (blockIdx.x * 4 + wave) * RPR;

  // 1. this thread's share of x, 2. the pass-0 loads of every row of this wave
  uint4 xr[XPT], nr[XPT];
  fetch_x<NORM>(a.x, a.norm_w, t, n8, xr, nr);
  Mx6Buf<NM, RPR> wa;
  Mx6Buf<NM, MULTI ? RPR : 1> wb;
  auto issue = [&](auto& buf, int pass) { mx6_issue(buf, a, row0, lane, pass); };
  issue(wa, 0);
  uint32_t res = 0;
  if (RES) res = a.residual[min(row0 + (lane & (RPR - 1)), a.N - 1)];
  __builtin_amdgcn_sched_barrier(0);  // nothing that waits on x may move above the weight loads

  // 3. stage x into LDS (RMS-normalised when NORM) while the weights stream: uint4 u of the row is plane u % 8 of
  // unit u / 8
  float rs = 1.0f;
  if (NORM) {
    rms_wave(sum_squares(xr, t, n8), red, wave, lane);
    __syncthreads();
    rs = rms_block(red, a.K, a.eps);
  }
#pragma unroll
  for (int i = 0; i < XPT; ++i) {
    const int u = t + 256 * i;
    const uint4 v = normalise<NORM>(xr[i], nr[i], rs);
    if (u < n8) xl[(u & 7) * nu + (u >> 3)] = v;
  }
  __syncthreads();

  // 4. dot every row of this wave pass by pass, then one butterfly for all of them
  float part[R];
#pragma unroll
  for (int i = 0; i < R; ++i) part[i] = 0.0f;
  auto consume = [&](const auto& buf, int pass) {
    const int u = pass * 64 + lane;
    const bool ok = u < nu;
    const int uu = min(u, nu - 1);
    uint4 x[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) x[q] = xl[q * nu + uu];
#pragma unroll
    for (int i = 0; i < RPR; ++i)
#pragma unroll
      for (int m = 0; m < NM; ++m) {
        const uint4 w0 = buf.w[m][i][0], w1 = buf.w[m][i][1], w2 = buf.w[m][i][2];
        const uint32_t sb = buf.s[m][i];
        const float d0 = mx6_block_dot(w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, mx6_e8m0_f32(sb & 0xFFu), x[0], x[1], x[2], x[3]);
        const float d1 = mx6_block_dot(w1.z, w1.w, w2.x, w2.y, w2.z, w2.w, mx6_e8m0_f32(sb >> 8), x[4], x[5], x[6], x[7]);
        part[i * NM + m] += ok ? d0 + d1 : 0.0f;
      }
  };
  pass_loop<MULTI>(passes, wa, wb, issue, consume);
  reduce_store<Mxfp6Fmt, RPR, DUAL>(part, res, RES, a.bias, a.y, a.N, row0, lane);
}

template <bool DUAL>
static int dispatch_mx6(const GemvPassArgs& a, const char* name, hipStream_t stream) {
  return gemv_dispatch<Mxfp6Fmt, DUAL>(a, name, [&](auto c) {
    using C = decltype(c);
    gemv_launch<C::RPR, DUAL, C::CAN_NORM>(a, [&](auto norm, auto res, dim3 blocks) {
      gemv_mxfp6_kernel<C::RPR, DUAL, decltype(norm)::value, decltype(res)::value, C::XPT, C::MULTI>
          <<<blocks, 256, (size_t)a.K * 2 + (a.norm_w ? 16 : 0), stream>>>(a);
    });
  });
}

int preload_mxfp6_gemv() {  // the lm_head launch of a prefill (no norm: it follows lga_rmsnorm there) and decode
  return preload(gemv_mxfp6_kernel<8, false, false, false, 2, false>) +
         preload(gemv_mxfp6_kernel<8, false, true, false, 2, false>);
}

}  // namespace lga

extern "C" int lga_mxfp6_quantize(const void* w, int w_is_bf16, uint8_t* codes, uint8_t* scales, int N, int K,
                                  hipStream_t stream) {
  LGA_CHECK_ARG(w && codes && scales, "lga_mxfp6_quantize: null pointer");
  LGA_CHECK_ARG(N > 0 && K > 0 && K % 64 == 0, "lga_mxfp6_quantize: K must be a positive multiple of 64");
  LGA_CHECK_ARG(((uintptr_t)w | (uintptr_t)codes) % 16 == 0, "lga_mxfp6_quantize: w and codes must be 16-B aligned");
  const size_t blocks = (size_t)N * (K / 32);
  const unsigned grid = (unsigned)((blocks + 63) / 64);
  if (w_is_bf16) lga::mxfp6_quantize_kernel<true><<<grid, 256, 0, stream>>>(w, (uint16_t*)codes, scales, blocks);
  else lga::mxfp6_quantize_kernel<false><<<grid, 256, 0, stream>>>(w, (uint16_t*)codes, scales, blocks);
  LGA_LAUNCH_RETURN();
}

extern "C" int lga_mxfp6_gemv(const void* x, const uint8_t* codes, const uint8_t* scales, const void* bias,
                              const void* residual, const void* norm_weight, float norm_eps, void* y, int N, int K,
                              hipStream_t stream) {
  LGA_GEMV_CHECKS("lga_mxfp6_gemv", 64, x && codes && scales && y,
                  LGA_GEMV_LIMITS("lga_mxfp6_gemv", 32768, 12288), (uintptr_t)x | (uintptr_t)codes, "x, codes");
  LGA_CHECK_ARG((uintptr_t)scales % 2 == 0, "lga_mxfp6_gemv: scales must be 2-B aligned");
  lga::GemvPassArgs a{(const uint16_t*)x, codes, nullptr, scales, nullptr, (const uint16_t*)bias,
                      (const uint16_t*)residual, (const uint16_t*)norm_weight, (uint16_t*)y, N, K, norm_eps};
  const int rc = lga::dispatch_mx6<false>(a, "lga_mxfp6_gemv", stream);
  if (rc) return rc;
  LGA_LAUNCH_RETURN();
}

extern "C" int lga_mxfp6_gemv_swiglu(const void* x, const uint8_t* codes1, const uint8_t* scales1,
                                     const uint8_t* codes2, const uint8_t* scales2, const void* norm_weight,
                                     float norm_eps, void* y, int N, int K, hipStream_t stream) {
  LGA_GEMV_CHECKS("lga_mxfp6_gemv_swiglu", 64, x && codes1 && scales1 && codes2 && scales2 && y,
                  LGA_GEMV_LIMITS("lga_mxfp6_gemv_swiglu", 32768, 12288),
                  (uintptr_t)x | (uintptr_t)codes1 | (uintptr_t)codes2, "x, codes");
  LGA_CHECK_ARG(((uintptr_t)scales1 | (uintptr_t)scales2) % 2 == 0, "lga_mxfp6_gemv_swiglu: scales must be 2-B aligned");
  lga::GemvPassArgs a{(const uint16_t*)x, codes1, codes2, scales1, scales2, nullptr,
                      nullptr, (const uint16_t*)norm_weight, (uint16_t*)y, N, K, norm_eps};
  const int rc = lga::dispatch_mx6<true>(a, "lga_mxfp6_gemv_swiglu", stream);
  if (rc) return rc;
  LGA_LAUNCH_RETURN();
}
