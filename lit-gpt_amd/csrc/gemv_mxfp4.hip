// MXFP4 (OCP microscaling fp4) weights, --quantize mxfp4: the weight quantizer and the batch-1 decode GEMV
//   y[n] = sum_k x[k] * e2m1(code[n, k]) * 2^(scale[n, k / 32] - 127)   (+ the fused epilogues of gemv_bf16.hip)
//
// Format (include/litgpt_amd.h): codes (N, K / 2) uint8, two e2m1 codes per byte with the even column in
// the low nibble; scales (N, K / 32) uint8 e8m0, one per 32 consecutive weights of a row. Every dequantized weight is
// zero or a normal bf16, so the GEMV computes what lga_bf16_gemv computes on the dequantized weight, in its own order.
//
// The GEMV moves 4.25 bits per weight: the thinnest HBM stream of the project, and the most VALU and LDS work per byte.
//  * A lane's 16-B load is 32 codes = exactly ONE MX block, so the chunk has one scale: the lane fetches that byte
//    itself (chunk c of row n is scales[n K/32 + c]; 64 lanes read 64 contiguous bytes; scale rows need no alignment).
//    The bytes stay raw until used (decode_ops.h) and are issued behind the code loads of their pass.
//  * A pass covers 4096 columns of a row: lane l holds the chunks l and l + 64 (a wave instruction reads 1 KB
//    contiguous of one row). A Llama-2-7B row of K = 4096 is ONE pass of 2 KB, so the bytes in flight come from rows:
//    a wave owns 8 rows when the row is one pass (fc_1 || fc_2: 4 rows of each) and 4 rows when it is several
//    (double-buffered passes, the next pass's loads issued before this pass's math; fc_1 || fc_2: 2 of each).
//    16 x 16 B (+ 16 scale bytes) in flight per lane either way.
//  * A 16-B chunk meets 64 B of activations. x is staged in LDS as FOUR planes, plane q holding the q-th 16 B of every
//    64-B chunk: the four ds_read_b128 of a chunk are each lane-contiguous (conflict-free), and the 64 B a lane reads
//    serve all 8 (4) rows of the wave — 8 B of LDS traffic per 16-B weight load at 8 rows.
//  * Expansion: one v_cvt_scalef32_pk_bf16_fp4 per code byte (byte select 0..3 of a dword), the block scale 2^(e - 127)
//    as its fp32 operand: two weights -> a packed bf16 pair with the scale applied, straight into v_dot2_f32_bf16.
//    16 converts + 16 dots per chunk, one VALU op per weight. The hardware returns the low nibble first (LGA_MXFP4_SWAP
//    rotates the x pairs instead, should a part return the other order).
//  * Every code and scale load of pass 0 is issued before the fused RMSNorm stages x. One transposed butterfly reduces
//    the 8 (4) row partials; bias / residual / SwiGLU epilogues with lga_bf16_gemv's bf16 rounding points.
// K limits: K % 32 == 0, K <= 32768; the RMSNorm fuses up to K = 12288 (kMx4NormMaxK; longer rows take lga_rmsnorm
// first — Mxfp4Linear.gemv_fuses_norm).
#include "decode_ops.h"

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
struct GemvMx4Args {
  const uint16_t* x;         // [K] bf16
  const uint8_t* w;          // [N][K / 2] e2m1 code pairs
  const uint8_t* w2;         // dual: fc_2
  const uint8_t* sc;         // [N][K / 32] e8m0
  const uint8_t* sc2;        // dual
  const uint16_t* bias;      // [N] or null
  const uint16_t* residual;  // [N] or null
  const uint16_t* norm_w;    // [K] or null (fused RMSNorm)
  uint16_t* y;               // [N]
  int N, K;
  float eps;
};

constexpr int MCPT = 2;            // 16-B chunks (MX blocks) per lane per row per pass
constexpr int MPASS = 64 * MCPT;   // chunks per pass (4096 columns)
constexpr int kMx4NormMaxK = 12288;
constexpr int kMx4MaxK = 32768;

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

template <int RPR, bool DUAL, bool NORM, bool RES, int XPT, bool MULTI>
__global__ void __launch_bounds__(256) gemv_mxfp4_kernel(GemvMx4Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4* xl = (uint4*)smem;                        // four planes of K / 32 uint4: chunk c = xl[q nch + c], q = 0..3
  float* red = (float*)(smem + (size_t)a.K * 2);   // 4 (NORM only)
  constexpr int NM = DUAL ? 2 : 1;
  constexpr int R = NM * RPR;                      // values per lane entering the butterfly
  static_assert(R == 4 || R == 8, "row partials per lane");
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int n8 = a.K / 8, nch = a.K / 32, kb = a.K / 2;
  const int passes = MULTI ? (nch + MPASS - 1) / MPASS : 1;
  const int row0 = (blockIdx.x * 4 + wave) * RPR;
  const uint8_t* wm[2] = {a.w, DUAL ? a.w2 : a.w};
  const uint8_t* sm[2] = {a.sc, DUAL ? a.sc2 : a.sc};

  // 1. activation (and norm weight) share of this thread: uint4 t, t + 256, ... (clamped, branch-free)
  uint4 xr[XPT], nr[XPT];
#pragma unroll
  for (int i = 0; i < XPT; ++i) {
    const int u = min(t + 256 * i, n8 - 1);
    xr[i] = ((const uint4*)a.x)[u];
    if (NORM) nr[i] = ((const uint4*)a.norm_w)[u];
  }
  // 2. pass-0 loads of every row of this wave: the code chunks, then each chunk's scale byte (rows past N re-read row
  //    N - 1, chunks past the row re-read its last one; neither is ever used)
  uint4 wa[NM][RPR][MCPT];
  uint4 wb[NM][MULTI ? RPR : 1][MULTI ? MCPT : 1];
  uint32_t sa[NM][RPR][MCPT], sb[NM][MULTI ? RPR : 1][MULTI ? MCPT : 1];
  auto issue = [&](auto& buf, auto& sbuf, int pass) {
#pragma unroll
    for (int j = 0; j < MCPT; ++j) {
      const int c = min(pass * MPASS + lane + 64 * j, nch - 1);
#pragma unroll
      for (int i = 0; i < RPR; ++i)
#pragma unroll
        for (int m = 0; m < NM; ++m) {
          const size_t n = (size_t)min(row0 + i, a.N - 1);
          buf[m][i][j] = ld_nt16(wm[m] + n * kb + (size_t)c * 16);
        }
    }
#pragma unroll
    for (int j = 0; j < MCPT; ++j) {
      const int c = min(pass * MPASS + lane + 64 * j, nch - 1);
#pragma unroll
      for (int i = 0; i < RPR; ++i)
#pragma unroll
        for (int m = 0; m < NM; ++m) {
          const size_t n = (size_t)min(row0 + i, a.N - 1);
          sbuf[m][i][j] = sm[m][n * nch + c];
        }
    }
  };
  issue(wa, sa, 0);
  uint32_t res = 0;
  if (RES) res = a.residual[min(row0 + (lane & (RPR - 1)), a.N - 1)];
  __builtin_amdgcn_sched_barrier(0);  // nothing that waits on x may move above the weight loads

  // 3. stage x into LDS (RMS-normalised when NORM) while the weights stream
  float rs = 1.0f;
  if (NORM) {
    float ss = 0.0f;
#pragma unroll
    for (int i = 0; i < XPT; ++i) {
      const bool ok = t + 256 * i < n8;
      const uint32_t d[4] = {xr[i].x, xr[i].y, xr[i].z, xr[i].w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float lo = ok ? bflo(d[q]) : 0.0f, hi = ok ? bfhi(d[q]) : 0.0f;
        ss = fmaf(lo, lo, ss);
        ss = fmaf(hi, hi, ss);
      }
    }
    ss = wave_sum_uniform(ss);
    if (lane == 0) red[wave] = ss;
    __syncthreads();
    rs = 1.0f / sqrtf(((red[0] + red[1]) + (red[2] + red[3])) / (float)a.K + a.eps);
  }
#pragma unroll
  for (int i = 0; i < XPT; ++i) {
    const int u = t + 256 * i;
    uint32_t d[4] = {xr[i].x, xr[i].y, xr[i].z, xr[i].w};
    if (NORM) {  // bf16(w * (x * rs)), two elements per instruction
      const uint32_t nw[4] = {nr[i].x, nr[i].y, nr[i].z, nr[i].w};
#pragma unroll
      for (int q = 0; q < 4; ++q)
        d[q] = pack2(__fmul_rn(bflo(nw[q]), __fmul_rn(bflo(d[q]), rs)),
                     __fmul_rn(bfhi(nw[q]), __fmul_rn(bfhi(d[q]), rs)));
    }
    if (u < n8) xl[(u & 3) * nch + (u >> 2)] = make_uint4(d[0], d[1], d[2], d[3]);
  }
  __syncthreads();

  // 4. dot every row of this wave pass by pass, then one butterfly for all of them
  float part[R];
#pragma unroll
  for (int i = 0; i < R; ++i) part[i] = 0.0f;
  auto consume = [&](const auto& buf, const auto& sbuf, int pass) {
#pragma unroll
    for (int j = 0; j < MCPT; ++j) {
      const int c = pass * MPASS + lane + 64 * j;
      const bool ok = c < nch;
      const int cc = min(c, nch - 1);
      const uint4 x[4] = {xl[cc], xl[nch + cc], xl[2 * nch + cc], xl[3 * nch + cc]};
#pragma unroll
      for (int i = 0; i < RPR; ++i)
#pragma unroll
        for (int m = 0; m < NM; ++m) {
          const float d = mx4_chunk_dot(buf[m][i][j], x, e8m0_f32(sbuf[m][i][j]));
          part[i * NM + m] += ok ? d : 0.0f;
        }
    }
  };
  if constexpr (MULTI) {
    for (int p = 0; p < passes; p += 2) {
      if (p + 1 < passes) issue(wb, sb, p + 1);
      consume(wa, sa, p);
      if (p + 1 < passes) {
        if (p + 2 < passes) issue(wa, sa, p + 2);
        consume(wb, sb, p + 1);
      }
    }
  } else {
    consume(wa, sa, 0);
  }
  const float tot = butterfly<R>(part, lane);
  const int vi = bfly_index<R>(lane);  // value index held by this lane
  constexpr int GROUP = 64 / R;        // lanes per value after the butterfly
  if (DUAL) {
    // value index = 2 * row + matrix: the fc_2 partner of a row sits in the lane whose value index differs in bit 0
    constexpr int PD = R == 8 ? 8 : 16;
    const float other = __shfl_xor(tot, PD);
    const int row = row0 + (vi >> 1);
    if ((lane & (GROUP - 1)) == 0 && (vi & 1) == 0 && row < a.N) {
      const float g = round_bf(silu_f(round_bf(tot)));  // silu(bf16(fc_1 x)) -> bf16
      a.y[row] = f2bf(__fmul_rn(g, round_bf(other)));   // * bf16(fc_2 x)
    }
  } else {
    const uint32_t rv = RES ? (uint32_t)__shfl(res, vi) : 0u;  // residual of row vi sits in lane vi
    const int row = row0 + vi;
    float o = tot;
    if (RES) {
      o = round_bf(a.bias ? o + bf2f(a.bias[min(row, a.N - 1)]) : o) + __uint_as_float(rv << 16);
    } else if (a.bias) {
      o += bf2f(a.bias[min(row, a.N - 1)]);
    }
    if ((lane & (GROUP - 1)) == 0 && row < a.N) a.y[row] = f2bf(o);
  }
}

template <int RPR, bool DUAL, int XPT, bool MULTI, bool CAN_NORM>
static void launch_mx4(const GemvMx4Args& a, hipStream_t stream) {
  const int waves = (a.N + RPR - 1) / RPR;
  const dim3 blocks((waves + 3) / 4);
  const bool norm = a.norm_w != nullptr, res = a.residual != nullptr;
  const size_t lds = (size_t)a.K * 2 + (norm ? 16 : 0);
  if constexpr (CAN_NORM) {
    if (norm) {
      if (DUAL || !res) gemv_mxfp4_kernel<RPR, DUAL, true, false, XPT, MULTI><<<blocks, 256, lds, stream>>>(a);
      else gemv_mxfp4_kernel<RPR, DUAL, true, true, XPT, MULTI><<<blocks, 256, lds, stream>>>(a);
      return;
    }
  }
  if (DUAL || !res) gemv_mxfp4_kernel<RPR, DUAL, false, false, XPT, MULTI><<<blocks, 256, lds, stream>>>(a);
  else gemv_mxfp4_kernel<RPR, DUAL, false, true, XPT, MULTI><<<blocks, 256, lds, stream>>>(a);
}

template <bool DUAL>
static void dispatch_mx4(const GemvMx4Args& a, hipStream_t stream) {
  constexpr int RS = DUAL ? 4 : 8, RM = DUAL ? 2 : 4;  // rows per wave (of each matrix): one pass / several
  if (a.K / 32 <= MPASS) launch_mx4<RS, DUAL, 2, false, true>(a, stream);              // K <= 4096
  else if (a.K <= kMx4NormMaxK) launch_mx4<RM, DUAL, 6, true, true>(a, stream);        // K <= 12288
  else launch_mx4<RM, DUAL, 16, true, false>(a, stream);                               // K <= 32768, no norm
}

int preload_mxfp4_gemv() {  // the lm_head launch of a prefill (no norm: it follows lga_rmsnorm there) and decode
  return preload(gemv_mxfp4_kernel<8, false, false, false, 2, false>) +
         preload(gemv_mxfp4_kernel<8, false, true, false, 2, false>);
}

}  // namespace lga

#define LGA_MXFP4_GEMV_CHECKS(name)                                                                            \
  LGA_CHECK_ARG(N > 0 && K > 0 && K % 32 == 0, name ": K must be a positive multiple of 32");                  \
  LGA_CHECK_ARG(K <= lga::kMx4MaxK, name ": K > 32768 is not supported");                                      \
  LGA_CHECK_ARG(!norm_weight || K <= lga::kMx4NormMaxK, name ": the fused RMSNorm takes K <= 12288")

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
  LGA_CHECK_ARG(x && codes && scales && y, "lga_mxfp4_gemv: null pointer");
  LGA_MXFP4_GEMV_CHECKS("lga_mxfp4_gemv");
  LGA_CHECK_ARG(((uintptr_t)x | (uintptr_t)codes | (uintptr_t)(norm_weight ? norm_weight : x)) % 16 == 0,
                "lga_mxfp4_gemv: x, codes and norm_weight must be 16-B aligned");
  lga::GemvMx4Args a{(const uint16_t*)x, codes, nullptr, scales, nullptr, (const uint16_t*)bias,
                     (const uint16_t*)residual, (const uint16_t*)norm_weight, (uint16_t*)y, N, K, norm_eps};
  lga::dispatch_mx4<false>(a, stream);
  LGA_LAUNCH_RETURN();
}

extern "C" int lga_mxfp4_gemv_swiglu(const void* x, const uint8_t* codes1, const uint8_t* scales1,
                                     const uint8_t* codes2, const uint8_t* scales2, const void* norm_weight,
                                     float norm_eps, void* y, int N, int K, hipStream_t stream) {
  LGA_CHECK_ARG(x && codes1 && scales1 && codes2 && scales2 && y, "lga_mxfp4_gemv_swiglu: null pointer");
  LGA_MXFP4_GEMV_CHECKS("lga_mxfp4_gemv_swiglu");
  LGA_CHECK_ARG(((uintptr_t)x | (uintptr_t)codes1 | (uintptr_t)codes2 |
                 (uintptr_t)(norm_weight ? norm_weight : x)) % 16 == 0,
                "lga_mxfp4_gemv_swiglu: x, codes and norm_weight must be 16-B aligned");
  lga::GemvMx4Args a{(const uint16_t*)x, codes1, codes2, scales1, scales2, nullptr,
                     nullptr, (const uint16_t*)norm_weight, (uint16_t*)y, N, K, norm_eps};
  lga::dispatch_mx4<true>(a, stream);
  LGA_LAUNCH_RETURN();
}
