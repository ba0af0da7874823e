// fp8 (OCP e4m3) weights, --quantize fp8-g128: the weight quantizer and the batch-1 decode GEMV
//   y[n] = sum_k x[k] * float(code[n, k]) * s[n, k / 128]   (+ the fused epilogues of gemv_bf16.hip)
//
// Format (include/litgpt_amd.h): codes (N, K) uint8 e4m3fn and scales (N, K / 128) bf16, every scale a
// power of two chosen by the fp8 KV cache's rule (kv8_ops.h) on each run of 128 weights of a row. float(code) * s is
// exact in bf16, so the GEMV computes what lga_bf16_gemv computes on the dequantized weight, in its own order.
//
// The GEMV moves 1 byte per weight (+ 2 bytes per 128): a pure HBM stream at half of bf16's bytes.
//  * A lane's 16-B load is 16 weights of ONE scale group (8 lanes per group). A pass covers 4096 columns of a row:
//    lane l reads the chunks l, l + 64, l + 128, l + 192, so each wave instruction is 1 KB contiguous of one row.
//  * A wave owns 4 rows when the row is one pass (K <= 4096; fc_1 || fc_2: 2 rows of each) and 2 rows when it is
//    several (double-buffered passes, the next pass's loads issued before this pass's math): 16 x 16 B in flight per
//    lane either way, the bf16 kernel's figure at half the bytes per weight. The x chunk a lane reads from LDS
//    (32 B) serves all rows of the wave.
//  * The 32 scales of a (row, pass) are ONE 2-byte load per lane (lane & 31 -> group), issued behind the weights;
//    the chunk's scale comes from lane (l >> 3) + 8 j by ds_bpermute. They stay raw bits until used (decode_ops.h).
//  * Every weight (and scale) load of pass 0 is issued before the fused RMSNorm stages x in LDS. x is staged as two
//    planes (the first and second 16 B of every 32-B chunk), so both ds_read_b128 of a chunk are lane-contiguous.
//  * Expansion (LGA_FP8_EXPAND): 0 — codes -> packed bf16 unscaled (v_cvt_scalef32_pk_bf16_fp8, scale operand 1.0,
//    the KV cache's form) into v_dot2_f32_bf16, the group scale applied once per 16-weight chunk in fp32 (exact: a
//    power of two); 1 — codes -> fp32 (v_cvt_pk_f32_fp8), fp32 FMAs, the scale once per chunk; 2 — the scaled
//    conversion straight into v_dot2_f32_bf16. All three are exact expansions; DESIGN §4.5g has the measurements.
//  * One transposed butterfly reduces the row partials; bias / residual / SwiGLU epilogues with lga_bf16_gemv's
//    bf16 rounding points.
// K limits: K % 128 == 0, K <= 32768; the RMSNorm fuses up to K = 12288 (kFp8NormMaxK; longer rows take
// lga_rmsnorm first — Fp8Linear.gemv_fuses_norm).
#include "kv8_ops.h"

#ifndef LGA_FP8_EXPAND
#define LGA_FP8_EXPAND 0
#endif

namespace lga {

// ---------------------------------------------------------------------------------------------------- quantizer
// one 16-lane row group per 128-weight group, 8 weights per lane; 16 groups per 256-thread workgroup
template <bool BF16>
__global__ void __launch_bounds__(256) fp8_quantize_kernel(const void* w, uint8_t* codes, uint16_t* scales,
                                                           size_t groups) {
  const size_t g = (size_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int sub = threadIdx.x & 15;
  const size_t gl = g < groups ? g : groups - 1;  // whole row groups stay active for the DPP maximum
  const size_t at = gl * 128 + (size_t)sub * 8;
  uint4 v;
  if (BF16) {
    v = *(const uint4*)((const uint16_t*)w + at);
  } else {  // the format quantizes the bf16 rounding of the weight
    const float4 a = *(const float4*)((const float*)w + at), b = *(const float4*)((const float*)w + at + 4);
    v = make_uint4(pack2(a.x, a.y), pack2(a.z, a.w), pack2(b.x, b.y), pack2(b.z, b.w));
  }
  float s;
  const uint2 c = kv8_quantize8(v, s);
  if (g < groups) {
    *(uint2*)(codes + at) = c;
    if (sub == 0) scales[g] = (uint16_t)(__float_as_uint(s) >> 16);  // a power of two: exact in bf16
  }
}

// ---------------------------------------------------------------------------------------------------- GEMV
struct GemvF8Args {
  const uint16_t* x;         // [K] bf16
  const uint8_t* w;          // [N][K] e4m3 codes
  const uint8_t* w2;         // dual: fc_2 [N][K]
  const uint16_t* sc;        // [N][K / 128] bf16 scales
  const uint16_t* sc2;       // dual
  const uint16_t* bias;      // [N] or null
  const uint16_t* residual;  // [N] or null
  const uint16_t* norm_w;    // [K] or null (fused RMSNorm)
  uint16_t* y;               // [N]
  int N, K;
  float eps;
};

constexpr int FCPT = 4;            // 16-B chunks per lane per row per pass
constexpr int FPASS = 64 * FCPT;   // chunks per pass (4096 columns, 32 scale groups)
constexpr int kFp8NormMaxK = 12288;
constexpr int kFp8MaxK = 32768;

__device__ __forceinline__ uint32_t fp8_bf16x2(uint32_t c, float s, bool hi) {
  return hi ? __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c, s, true))
            : __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c, s, false));
}

// dot of one 16-weight chunk against its 16 activations (x0: k 0..7, x1: k 8..15), times the group scale
__device__ __forceinline__ float fp8_chunk_dot(const uint4 wv, const uint4 x0, const uint4 x1, float s) {
  const uint32_t c[4] = {wv.x, wv.y, wv.z, wv.w};
  const uint32_t xp[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
  float d = 0.0f;
#if LGA_FP8_EXPAND == 1
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[q], false);
    const f32x2_t hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[q], true);
    d = fmaf(lo.x, bflo(xp[2 * q]), d);
    d = fmaf(lo.y, bfhi(xp[2 * q]), d);
    d = fmaf(hi.x, bflo(xp[2 * q + 1]), d);
    d = fmaf(hi.y, bfhi(xp[2 * q + 1]), d);
  }
  return d * s;
#else
  const float cs = LGA_FP8_EXPAND == 2 ? s : 1.0f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    d = dot2_bf16(fp8_bf16x2(c[q], cs, false), xp[2 * q], d);
    d = dot2_bf16(fp8_bf16x2(c[q], cs, true), xp[2 * q + 1], d);
  }
  return LGA_FP8_EXPAND == 2 ? d : d * s;
#endif
}

template <int RPR, bool DUAL, bool NORM, bool RES, int XPT, bool MULTI>
__global__ void __launch_bounds__(256) gemv_fp8_kernel(GemvF8Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4* xl = (uint4*)smem;                        // two planes of K / 16 uint4: chunk c = xl[c], xl[n16 + c]
  float* red = (float*)(smem + (size_t)a.K * 2);   // 4 (NORM only)
  constexpr int NM = DUAL ? 2 : 1;
  constexpr int R = NM * RPR;                      // values per lane entering the butterfly
  static_assert(R == 2 || R == 4, "row partials per lane");
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int n8 = a.K / 8, n16 = a.K / 16, ng = a.K / 128;
  const int passes = MULTI ? (n16 + FPASS - 1) / FPASS : 1;
  const int row0 = (blockIdx.x * 4 + wave) * RPR;
  const uint8_t* wm[2] = {a.w, DUAL ? a.w2 : a.w};
  const uint16_t* sm[2] = {a.sc, DUAL ? a.sc2 : a.sc};

  // 1. activation (and norm weight) share of this thread: uint4 t, t + 256, ... (clamped, branch-free)
  uint4 xr[XPT], nr[XPT];
#pragma unroll
  for (int i = 0; i < XPT; ++i) {
    const int u = min(t + 256 * i, n8 - 1);
    xr[i] = ((const uint4*)a.x)[u];
    if (NORM) nr[i] = ((const uint4*)a.norm_w)[u];
  }
  // 2. pass-0 loads of every row of this wave: the codes, then the pass's 32 scales (rows past N re-read row N - 1,
  //    chunks and groups past the row re-read its last one; neither is ever used)
  uint4 wa[NM][RPR][FCPT];
  uint4 wb[NM][MULTI ? RPR : 1][MULTI ? FCPT : 1];
  uint32_t sa[NM][RPR], sb[NM][MULTI ? RPR : 1];
  auto issue = [&](auto& buf, auto& sbuf, int pass) {
#pragma unroll
    for (int j = 0; j < FCPT; ++j) {
      const int c = min(pass * FPASS + lane + 64 * j, n16 - 1);
#pragma unroll
      for (int i = 0; i < RPR; ++i)
#pragma unroll
        for (int m = 0; m < NM; ++m) {
          const size_t n = (size_t)min(row0 + i, a.N - 1);
          buf[m][i][j] = ld_nt16(wm[m] + n * a.K + (size_t)c * 16);
        }
    }
    const int g = min(pass * (FPASS / 8) + (lane & 31), ng - 1);
#pragma unroll
    for (int i = 0; i < RPR; ++i)
#pragma unroll
      for (int m = 0; m < NM; ++m) {
        const size_t n = (size_t)min(row0 + i, a.N - 1);
        sbuf[m][i] = sm[m][n * ng + g];
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
    if (u < n8) xl[(u & 1) * n16 + (u >> 1)] = make_uint4(d[0], d[1], d[2], d[3]);
  }
  __syncthreads();

  // 4. dot every row of this wave pass by pass, then one butterfly for all of them
  float part[R];
#pragma unroll
  for (int i = 0; i < R; ++i) part[i] = 0.0f;
  auto consume = [&](const auto& buf, const auto& sbuf, int pass) {
#pragma unroll
    for (int j = 0; j < FCPT; ++j) {
      const int c = pass * FPASS + lane + 64 * j;
      const bool ok = c < n16;
      const int cc = min(c, n16 - 1);
      const uint4 x0 = xl[cc], x1 = xl[n16 + cc];
      const int src = (lane >> 3) + 8 * j;  // the lane holding this chunk's group scale
#pragma unroll
      for (int i = 0; i < RPR; ++i)
#pragma unroll
        for (int m = 0; m < NM; ++m) {
          const float s = __uint_as_float((uint32_t)__shfl((int)sbuf[m][i], src) << 16);
          const float d = fp8_chunk_dot(buf[m][i][j], x0, x1, s);
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
    constexpr int PD = R == 4 ? 16 : 32;
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
static void launch_f8(const GemvF8Args& a, hipStream_t stream) {
  const int waves = (a.N + RPR - 1) / RPR;
  const dim3 blocks((waves + 3) / 4);
  const bool norm = a.norm_w != nullptr, res = a.residual != nullptr;
  const size_t lds = (size_t)a.K * 2 + (norm ? 16 : 0);
  if constexpr (CAN_NORM) {
    if (norm) {
      if (DUAL || !res) gemv_fp8_kernel<RPR, DUAL, true, false, XPT, MULTI><<<blocks, 256, lds, stream>>>(a);
      else gemv_fp8_kernel<RPR, DUAL, true, true, XPT, MULTI><<<blocks, 256, lds, stream>>>(a);
      return;
    }
  }
  if (DUAL || !res) gemv_fp8_kernel<RPR, DUAL, false, false, XPT, MULTI><<<blocks, 256, lds, stream>>>(a);
  else gemv_fp8_kernel<RPR, DUAL, false, true, XPT, MULTI><<<blocks, 256, lds, stream>>>(a);
}

template <bool DUAL>
static void dispatch_f8(const GemvF8Args& a, hipStream_t stream) {
  const int n16 = a.K / 16;
  constexpr int RS = DUAL ? 2 : 4, RM = DUAL ? 1 : 2;  // rows per wave (of each matrix): one pass / several
  if (n16 <= FPASS) launch_f8<RS, DUAL, 2, false, true>(a, stream);                  // K <= 4096
  else if (a.K <= kFp8NormMaxK) launch_f8<RM, DUAL, 6, true, true>(a, stream);       // K <= 12288
  else launch_f8<RM, DUAL, 16, true, false>(a, stream);                              // K <= 32768, no norm
}

// ---------------------------------------------------------------------------------------------------- rows GEMV
// Y (M, N) = X (M, K) W'^T for M = 2..8 activation rows in ONE pass over the weights (batched decode, the speculative
// verify window). Row r has the bits gemv_fp8_kernel gives for x[r]: the same three dispatch classes and rows per
// wave, the same lane -> chunk mapping, scale hand-off, per-lane accumulation order, butterfly and epilogues.
//  * MT in {2, 4, 8} is the template row count (M rounded up; rows past M re-read row M - 1 and are never stored),
//    so the partials part[MT][R] are registers.
//  * A chunk's 16 codes are expanded ONCE, to 8 packed-bf16 registers per weight row of the wave (8 R registers),
//    and every activation row's 32 B of x (two ds_read_b128) are dotted against all of them: neither the expansion
//    nor the LDS read is repeated per (weight row, activation row) pair.
//  * x lives in LDS one PASS at a time: the 4096 columns of the MT rows, each row as the one-row kernel's two planes
//    (MT x 8 KB, 64 KB at MT = 8; whole rows of K = 11008 would not fit). A pass's x (M x 8 KB of an L2-resident
//    block) is fetched into registers BEFORE the weight loads of the same pass are issued: vmcnt retires in order, so
//    staging pass p + 1 waits for nothing younger than its own x, and the weights of p + 1 stay in flight across the
//    barriers and the math of pass p.
//  * Fused RMSNorm: every row's 1 / rms by the one-row recipe (thread t owns uint4 t + 256 i, fma in that order,
//    wave_sum_uniform, (red0 + red1) + (red2 + red3)) in a prologue, kept in MT registers; the pass staging
//    normalises what it fetched with the same two roundings. The prologue's x is held in registers across the
//    weight issue where it fits (MT x XPT <= 24 uint4); at MT = 8 with several passes it runs before the weights.
//    Its 16 MT bytes of LDS alias the x planes (one more barrier), so no launch asks for more than 64 KB.
struct GemvF8RowsArgs {
  GemvF8Args g;  // x (M, K), residual (M, N), y (M, N)
  int M;
};

__device__ __forceinline__ void fp8_expand(const uint4 wv, uint32_t (&e)[8]) {
  const uint32_t c[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    e[2 * q] = fp8_bf16x2(c[q], 1.0f, false);
    e[2 * q + 1] = fp8_bf16x2(c[q], 1.0f, true);
  }
}

// fp8_chunk_dot's dot2 chain (its LGA_FP8_EXPAND == 0 form) on an expanded chunk, before the scale
__device__ __forceinline__ float fp8_expanded_dot(const uint32_t (&e)[8], const uint4 x0, const uint4 x1) {
  const uint32_t xp[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
  float d = 0.0f;
#pragma unroll
  for (int q = 0; q < 8; ++q) d = dot2_bf16(e[q], xp[q], d);
  return d;
}

template <int MT, int RPR, bool DUAL, bool NORM, int XPT, bool MULTI>
__global__ void __launch_bounds__(256) gemv_fp8_rows_kernel(GemvF8RowsArgs ra) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const GemvF8Args& a = ra.g;
  uint4* xl = (uint4*)smem;    // [MT][2 planes][pc]: chunk c of row r = xl[2 r pc + c], xl[(2 r + 1) pc + c]
  float* red = (float*)smem;   // [MT][4] (NORM prologue only, before the first staging)
  constexpr int NM = DUAL ? 2 : 1;
  constexpr int R = NM * RPR;
  constexpr bool HOLD = MT * XPT <= 24;  // the prologue's x stays in registers across the weight issue
  static_assert(R == 2 || R == 4, "row partials per lane");
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int n8 = a.K / 8, n16 = a.K / 16, ng = a.K / 128;
  const int pc = min(n16, FPASS);
  const int passes = MULTI ? (n16 + FPASS - 1) / FPASS : 1;
  const int row0 = (blockIdx.x * 4 + wave) * RPR;
  const uint8_t* wm[2] = {a.w, DUAL ? a.w2 : a.w};
  const uint16_t* sm[2] = {a.sc, DUAL ? a.sc2 : a.sc};
  const uint4* xg[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) xg[m] = (const uint4*)(a.x + (size_t)min(m, ra.M - 1) * a.K);

  // 1. sum of squares of every activation row: this thread's share
  float ss[MT], rs[MT];
  auto square = [&](const uint4 v, bool ok, float s) {
    const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float lo = ok ? bflo(d[q]) : 0.0f, hi = ok ? bfhi(d[q]) : 0.0f;
      s = fmaf(lo, lo, s);
      s = fmaf(hi, hi, s);
    }
    return s;
  };
  auto finish_norm = [&]() {
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const float s = wave_sum_uniform(ss[m]);
      if (lane == 0) red[m * 4 + wave] = s;
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < MT; ++m)
      rs[m] = 1.0f / sqrtf(((red[m * 4] + red[m * 4 + 1]) + (red[m * 4 + 2] + red[m * 4 + 3])) / (float)a.K + a.eps);
    __syncthreads();  // red aliases the x planes
  };
  uint4 xr[NORM && HOLD ? MT : 1][NORM && HOLD ? XPT : 1];
  if constexpr (NORM && HOLD) {
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int i = 0; i < XPT; ++i) xr[m][i] = xg[m][min(t + 256 * i, n8 - 1)];
  } else if constexpr (NORM) {
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      uint4 v[XPT];
#pragma unroll
      for (int i = 0; i < XPT; ++i) v[i] = xg[m][min(t + 256 * i, n8 - 1)];
      ss[m] = 0.0f;
#pragma unroll
      for (int i = 0; i < XPT; ++i) ss[m] = square(v[i], t + 256 * i < n8, ss[m]);
    }
    finish_norm();
  }

  // 2. x (and norm weight) of a pass into registers: uint4 t, t + 256 of the pass's 512 (clamped, branch-free)
  uint4 xs[MT][2], xn[2];
  auto fetch = [&](int pass) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int u = min(pass * (2 * FPASS) + t + 256 * i, n8 - 1);
      if (NORM) xn[i] = ((const uint4*)a.norm_w)[u];
#pragma unroll
      for (int m = 0; m < MT; ++m) xs[m][i] = xg[m][u];
    }
  };
  auto stage = [&](int pass) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int ul = t + 256 * i;
      const bool ok = pass * (2 * FPASS) + ul < n8;
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        uint32_t d[4] = {xs[m][i].x, xs[m][i].y, xs[m][i].z, xs[m][i].w};
        if (NORM) {  // bf16(w * (x * rs)), as the one-row kernel
          const uint32_t nw[4] = {xn[i].x, xn[i].y, xn[i].z, xn[i].w};
#pragma unroll
          for (int q = 0; q < 4; ++q)
            d[q] = pack2(__fmul_rn(bflo(nw[q]), __fmul_rn(bflo(d[q]), rs[m])),
                         __fmul_rn(bfhi(nw[q]), __fmul_rn(bfhi(d[q]), rs[m])));
        }
        if (ok) xl[(2 * m + (ul & 1)) * pc + (ul >> 1)] = make_uint4(d[0], d[1], d[2], d[3]);
      }
    }
  };
  fetch(0);

  // 3. the weight and scale loads of a pass, issued once for all M rows (gemv_fp8_kernel's, clamped the same way)
  uint4 wa[NM][RPR][FCPT];
  uint4 wb[NM][MULTI ? RPR : 1][MULTI ? FCPT : 1];
  uint32_t sa[NM][RPR], sb[NM][MULTI ? RPR : 1];
  auto issue = [&](auto& buf, auto& sbuf, int pass) {
#pragma unroll
    for (int j = 0; j < FCPT; ++j) {
      const int c = min(pass * FPASS + lane + 64 * j, n16 - 1);
#pragma unroll
      for (int i = 0; i < RPR; ++i)
#pragma unroll
        for (int m = 0; m < NM; ++m) {
          const size_t n = (size_t)min(row0 + i, a.N - 1);
          buf[m][i][j] = ld_nt16(wm[m] + n * a.K + (size_t)c * 16);
        }
    }
    const int g = min(pass * (FPASS / 8) + (lane & 31), ng - 1);
#pragma unroll
    for (int i = 0; i < RPR; ++i)
#pragma unroll
      for (int m = 0; m < NM; ++m) {
        const size_t n = (size_t)min(row0 + i, a.N - 1);
        sbuf[m][i] = sm[m][n * ng + g];
      }
  };
  issue(wa, sa, 0);
  uint32_t res[MT];
  if (!DUAL && a.residual) {
#pragma unroll
    for (int m = 0; m < MT; ++m)
      res[m] = a.residual[(size_t)min(m, ra.M - 1) * a.N + min(row0 + (lane & (RPR - 1)), a.N - 1)];
  }
  __builtin_amdgcn_sched_barrier(0);  // nothing that waits on x may move above the weight loads

  if constexpr (NORM && HOLD) {
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      ss[m] = 0.0f;
#pragma unroll
      for (int i = 0; i < XPT; ++i) ss[m] = square(xr[m][i], t + 256 * i < n8, ss[m]);
    }
    finish_norm();
  }

  // 4. pass by pass: stage the pass's x, fetch the next pass's x and then issue its weights, dot
  float part[MT][R];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int i = 0; i < R; ++i) part[m][i] = 0.0f;
  auto consume = [&](const auto& buf, const auto& sbuf, int pass) {
#pragma unroll
    for (int j = 0; j < FCPT; ++j) {
      const int c = pass * FPASS + lane + 64 * j;
      const bool ok = c < n16;
      const int cl = min(c, n16 - 1) - pass * FPASS;
      const int src = (lane >> 3) + 8 * j;  // the lane holding this chunk's group scale
      uint32_t e[R][8];
      float s[R];
#pragma unroll
      for (int i = 0; i < RPR; ++i)
#pragma unroll
        for (int m = 0; m < NM; ++m) {
          fp8_expand(buf[m][i][j], e[i * NM + m]);
          s[i * NM + m] = __uint_as_float((uint32_t)__shfl((int)sbuf[m][i], src) << 16);
        }
#pragma unroll
      for (int r = 0; r < MT; ++r) {
        const uint4 x0 = xl[2 * r * pc + cl], x1 = xl[(2 * r + 1) * pc + cl];
#pragma unroll
        for (int v = 0; v < R; ++v) {
          const float d = fp8_expanded_dot(e[v], x0, x1) * s[v];
          part[r][v] += ok ? d : 0.0f;
        }
      }
    }
  };
  for (int p = 0; p < passes; p += 2) {
    stage(p);
    if constexpr (MULTI) {
      if (p + 1 < passes) {
        fetch(p + 1);
        issue(wb, sb, p + 1);
      }
    }
    __syncthreads();
    consume(wa, sa, p);
    if constexpr (MULTI) {
      if (p + 1 < passes) {
        __syncthreads();
        stage(p + 1);
        if (p + 2 < passes) {
          fetch(p + 2);
          issue(wa, sa, p + 2);
        }
        __syncthreads();
        consume(wb, sb, p + 1);
        if (p + 2 < passes) __syncthreads();
      }
    }
  }

  // 5. gemv_fp8_kernel's butterfly and epilogue, row by row
  const int vi = bfly_index<R>(lane);
  constexpr int GROUP = 64 / R;
#pragma unroll
  for (int r = 0; r < MT; ++r) {
    if (r >= ra.M) break;
    const float tot = butterfly<R>(part[r], lane);
    uint16_t* y = a.y + (size_t)r * a.N;
    if (DUAL) {
      constexpr int PD = R == 4 ? 16 : 32;
      const float other = __shfl_xor(tot, PD);
      const int row = row0 + (vi >> 1);
      if ((lane & (GROUP - 1)) == 0 && (vi & 1) == 0 && row < a.N) {
        const float g = round_bf(silu_f(round_bf(tot)));
        y[row] = f2bf(__fmul_rn(g, round_bf(other)));
      }
    } else {
      const int row = row0 + vi;
      float o = tot;
      if (a.residual) {
        const uint32_t rv = (uint32_t)__shfl(res[r], vi);
        o = round_bf(a.bias ? o + bf2f(a.bias[min(row, a.N - 1)]) : o) + __uint_as_float(rv << 16);
      } else if (a.bias) {
        o += bf2f(a.bias[min(row, a.N - 1)]);
      }
      if ((lane & (GROUP - 1)) == 0 && row < a.N) y[row] = f2bf(o);
    }
  }
}

template <int MT, int RPR, bool DUAL, int XPT, bool MULTI, bool CAN_NORM>
static void launch_f8_rows(const GemvF8RowsArgs& ra, hipStream_t stream) {
  const int waves = (ra.g.N + RPR - 1) / RPR;
  const dim3 blocks((waves + 3) / 4);
  const size_t lds = (size_t)MT * (ra.g.K < FPASS * 16 ? ra.g.K : FPASS * 16) * 2;  // at most 64 KB
  if constexpr (CAN_NORM) {
    if (ra.g.norm_w) {
      gemv_fp8_rows_kernel<MT, RPR, DUAL, true, XPT, MULTI><<<blocks, 256, lds, stream>>>(ra);
      return;
    }
  }
  gemv_fp8_rows_kernel<MT, RPR, DUAL, false, 0, MULTI><<<blocks, 256, lds, stream>>>(ra);
}

template <int MT, bool DUAL>
static void dispatch_f8_rows_mt(const GemvF8RowsArgs& ra, hipStream_t stream) {  // dispatch_f8's classes
  constexpr int RS = DUAL ? 2 : 4, RM = DUAL ? 1 : 2;
  if (ra.g.K / 16 <= FPASS) launch_f8_rows<MT, RS, DUAL, 2, false, true>(ra, stream);
  else if (ra.g.K <= kFp8NormMaxK) launch_f8_rows<MT, RM, DUAL, 6, true, true>(ra, stream);
  else launch_f8_rows<MT, RM, DUAL, 6, true, false>(ra, stream);
}

template <bool DUAL>
static void dispatch_f8_rows(const GemvF8RowsArgs& ra, hipStream_t stream) {
  if (ra.M == 1) dispatch_f8<DUAL>(ra.g, stream);
  else if (ra.M == 2) dispatch_f8_rows_mt<2, DUAL>(ra, stream);
  else if (ra.M <= 4) dispatch_f8_rows_mt<4, DUAL>(ra, stream);
  else dispatch_f8_rows_mt<8, DUAL>(ra, stream);
}

int preload_fp8_gemv() {  // the lm_head launch of a prefill (no norm: it follows lga_rmsnorm there) and decode
  return preload(gemv_fp8_kernel<4, false, false, false, 2, false>) +
         preload(gemv_fp8_kernel<4, false, true, false, 2, false>);
}

}  // namespace lga

#define LGA_FP8_GEMV_CHECKS(name)                                                                              \
  LGA_CHECK_ARG(N > 0 && K > 0 && K % 128 == 0, name ": K must be a positive multiple of 128");                \
  LGA_CHECK_ARG(K <= lga::kFp8MaxK, name ": K > 32768 is not supported");                                      \
  LGA_CHECK_ARG(!norm_weight || K <= lga::kFp8NormMaxK, name ": the fused RMSNorm takes K <= 12288")

extern "C" int lga_fp8_quantize(const void* w, int w_is_bf16, uint8_t* codes, void* scales, int N, int K,
                                hipStream_t stream) {
  LGA_CHECK_ARG(w && codes && scales, "lga_fp8_quantize: null pointer");
  LGA_CHECK_ARG(N > 0 && K > 0 && K % 128 == 0, "lga_fp8_quantize: K must be a positive multiple of 128");
  LGA_CHECK_ARG(((uintptr_t)w | (uintptr_t)codes) % 16 == 0, "lga_fp8_quantize: w and codes must be 16-B aligned");
  const size_t groups = (size_t)N * (K / 128);
  const unsigned blocks = (unsigned)((groups + 15) / 16);
  if (w_is_bf16) lga::fp8_quantize_kernel<true><<<blocks, 256, 0, stream>>>(w, codes, (uint16_t*)scales, groups);
  else lga::fp8_quantize_kernel<false><<<blocks, 256, 0, stream>>>(w, codes, (uint16_t*)scales, groups);
  LGA_LAUNCH_RETURN();
}

extern "C" int lga_fp8_gemv(const void* x, const uint8_t* codes, const void* scales, const void* bias,
                            const void* residual, const void* norm_weight, float norm_eps, void* y, int N, int K,
                            hipStream_t stream) {
  LGA_CHECK_ARG(x && codes && scales && y, "lga_fp8_gemv: null pointer");
  LGA_FP8_GEMV_CHECKS("lga_fp8_gemv");
  LGA_CHECK_ARG(((uintptr_t)x | (uintptr_t)codes | (uintptr_t)(norm_weight ? norm_weight : x)) % 16 == 0,
                "lga_fp8_gemv: x, codes and norm_weight must be 16-B aligned");
  lga::GemvF8Args a{(const uint16_t*)x, codes, nullptr, (const uint16_t*)scales, nullptr, (const uint16_t*)bias,
                    (const uint16_t*)residual, (const uint16_t*)norm_weight, (uint16_t*)y, N, K, norm_eps};
  lga::dispatch_f8<false>(a, stream);
  LGA_LAUNCH_RETURN();
}

extern "C" int lga_fp8_gemv_swiglu(const void* x, const uint8_t* codes1, const void* scales1, const uint8_t* codes2,
                                   const void* scales2, const void* norm_weight, float norm_eps, void* y, int N,
                                   int K, hipStream_t stream) {
  LGA_CHECK_ARG(x && codes1 && scales1 && codes2 && scales2 && y, "lga_fp8_gemv_swiglu: null pointer");
  LGA_FP8_GEMV_CHECKS("lga_fp8_gemv_swiglu");
  LGA_CHECK_ARG(((uintptr_t)x | (uintptr_t)codes1 | (uintptr_t)codes2 |
                 (uintptr_t)(norm_weight ? norm_weight : x)) % 16 == 0,
                "lga_fp8_gemv_swiglu: x, codes and norm_weight must be 16-B aligned");
  lga::GemvF8Args a{(const uint16_t*)x, codes1, codes2, (const uint16_t*)scales1, (const uint16_t*)scales2, nullptr,
                    nullptr, (const uint16_t*)norm_weight, (uint16_t*)y, N, K, norm_eps};
  lga::dispatch_f8<true>(a, stream);
  LGA_LAUNCH_RETURN();
}

extern "C" int lga_fp8_gemv_rows(const void* x, const uint8_t* codes, const void* scales, const void* bias,
                                 const void* residual, const void* norm_weight, float norm_eps, void* y, int M, int N,
                                 int K, hipStream_t stream) {
  LGA_CHECK_ARG(x && codes && scales && y, "lga_fp8_gemv_rows: null pointer");
  LGA_CHECK_ARG(M >= 1 && M <= 8, "lga_fp8_gemv_rows: M must be 1..8 rows");
  LGA_FP8_GEMV_CHECKS("lga_fp8_gemv_rows");
  LGA_CHECK_ARG(((uintptr_t)x | (uintptr_t)codes | (uintptr_t)(norm_weight ? norm_weight : x)) % 16 == 0,
                "lga_fp8_gemv_rows: x, codes and norm_weight must be 16-B aligned");
  lga::GemvF8RowsArgs a{{(const uint16_t*)x, codes, nullptr, (const uint16_t*)scales, nullptr, (const uint16_t*)bias,
                         (const uint16_t*)residual, (const uint16_t*)norm_weight, (uint16_t*)y, N, K, norm_eps}, M};
  lga::dispatch_f8_rows<false>(a, stream);
  LGA_LAUNCH_RETURN();
}

extern "C" int lga_fp8_gemv_swiglu_rows(const void* x, const uint8_t* codes1, const void* scales1,
                                        const uint8_t* codes2, const void* scales2, const void* norm_weight,
                                        float norm_eps, void* y, int M, int N, int K, hipStream_t stream) {
  LGA_CHECK_ARG(x && codes1 && scales1 && codes2 && scales2 && y, "lga_fp8_gemv_swiglu_rows: null pointer");
  LGA_CHECK_ARG(M >= 1 && M <= 8, "lga_fp8_gemv_swiglu_rows: M must be 1..8 rows");
  LGA_FP8_GEMV_CHECKS("lga_fp8_gemv_swiglu_rows");
  LGA_CHECK_ARG(((uintptr_t)x | (uintptr_t)codes1 | (uintptr_t)codes2 |
                 (uintptr_t)(norm_weight ? norm_weight : x)) % 16 == 0,
                "lga_fp8_gemv_swiglu_rows: x, codes and norm_weight must be 16-B aligned");
  lga::GemvF8RowsArgs a{{(const uint16_t*)x, codes1, codes2, (const uint16_t*)scales1, (const uint16_t*)scales2,
                         nullptr, nullptr, (const uint16_t*)norm_weight, (uint16_t*)y, N, K, norm_eps}, M};
  lga::dispatch_f8_rows<true>(a, stream);
  LGA_LAUNCH_RETURN();
}
