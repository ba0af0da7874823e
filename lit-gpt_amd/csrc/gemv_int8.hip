// Batch-1 decode GEMV over LLM.int8 weights (--quantize bnb.int8): int8 [N][K] + fp32 row absmax, the activation
// row quantized per call with the outlier columns (|x| >= threshold) kept in bf16 (include/litgpt_amd.h has the
// arithmetic). Structure follows gemv_bf16.hip — a pure weight stream in 16-B chunks (16 weights each), the weight
// loads of pass 0 issued before anything waits on x:
//  * prologue (while the weights stream): optional RMSNorm, then ONE more block reduction gives s_x = max |x| over
//    the non-outlier columns and whether any outlier exists; LDS then holds the int8 image of x (0 in outlier
//    columns), the bf16 row, and one outlier bit per column;
//  * dot: v_dot4 on packed int8 (4 per chunk and row), exact int32 accumulation, an integer transposed butterfly;
//  * outlier columns: a chunk whose 16 mask bits are not all zero takes a rare branch that adds x[j] * (q * s_w/127)
//    from the weight bytes the lane already holds — any number of outlier columns, none to all K; the branch is
//    skipped block-wide when the row has no outlier;
//  * epilogue: float(acc) * ((s_x * s_w) / 16129) + outliers + bias, residual, SwiGLU with the bf16 rounding points
//    of the other Linears.
#include "decode_ops.h"
#include "int8_ops.h"

namespace lga {

struct GemvI8Args {
  const uint16_t* x;         // [K] bf16
  const int8_t* w;           // [N][K] int8
  const int8_t* w2;          // dual: fc_2
  const float* sw;           // [N] row absmax
  const float* sw2;          // dual: fc_2
  const uint16_t* bias;      // [N] or null
  const uint16_t* residual;  // [N] or null
  const uint16_t* norm_w;    // [K] or null (fused RMSNorm)
  uint16_t* y;               // [N]
  int N, K;
  float eps, thr;
};

#define LGA_DPPI(v, ctrl) __builtin_amdgcn_update_dpp(0, v, ctrl, 0xF, 0xF, false)

// decode_ops.h butterfly<R> on int32 partials (the integer sum must stay exact: |acc| reaches K * 127^2 > 2^24)
template <int R>
__device__ __forceinline__ int butterfly_i(int* a, int lane) {
  constexpr int L = R == 8 ? 3 : (R == 4 ? 2 : 1);
#pragma unroll
  for (int lev = 0; lev < L; ++lev) {
    const int D = 32 >> lev;
    const int n = R >> (lev + 1);
    const bool h = lane & D;
#pragma unroll
    for (int i = 0; i < n; ++i) {
      int lo = a[i], hi = a[i + n];
      asm volatile("" : "+v"(lo), "+v"(hi));  // keep the pair in registers (see butterfly<R>)
      const int send = h ? lo : hi, keep = h ? hi : lo;
      int recv;
      if (D == 8) recv = LGA_DPPI(send, 0x128);
      else recv = __shfl_xor(send, D);
      a[i] = keep + recv;
    }
  }
  int d = a[0];
  d += LGA_DPPI(d, 0xB1);
  d += LGA_DPPI(d, 0x4E);
  d += LGA_DPPI(d, 0x141);
  if (R <= 4) d += LGA_DPPI(d, 0x140);
  if (R <= 2) d += __shfl_xor(d, 16);
  return d;
}

template <int RPR, bool DUAL, bool NORM, bool RES, int XPT, int CPT, bool MULTI>
__global__ void __launch_bounds__(256) gemv_int8_kernel(GemvI8Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int K = a.K;
  uint4* xq = (uint4*)smem;                                       // K int8: the quantized row
  uint4* xb = (uint4*)(smem + (size_t)K);                         // K bf16: the row itself (outlier columns)
  unsigned char* om = smem + (size_t)K * 3;                       // K / 8 bytes: outlier bit per column
  float* red = (float*)(smem + (size_t)K * 3 + ((K / 8 + 15) & ~15));  // 12
  constexpr int NM = DUAL ? 2 : 1;
  constexpr int R = NM * RPR;
  constexpr int RB = R < 2 ? 2 : R;
  constexpr int PASSC = 64 * CPT;  // chunks per pass
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int n8 = K / 8, n16 = K / 16;
  const int passes = MULTI ? (n16 + PASSC - 1) / PASSC : 1;
  const int row0 = (blockIdx.x * 4 + wave) * RPR;
  const int8_t* wm[2] = {a.w, DUAL ? a.w2 : a.w};
  const float* sm[2] = {a.sw, DUAL ? a.sw2 : a.sw};

  // 1. activation (and norm weight) share of this thread: uint4 t, t+256, ... (clamped, branch-free)
  uint4 xr[XPT], nr[XPT];
#pragma unroll
  for (int i = 0; i < XPT; ++i) {
    const int u = min(t + 256 * i, n8 - 1);
    xr[i] = ((const uint4*)a.x)[u];
    if (NORM) nr[i] = ((const uint4*)a.norm_w)[u];
  }
  // row scales of this wave's rows (tiny, ahead of the weight stream so no later wait drains it)
  float sws[RB];
#pragma unroll
  for (int i = 0; i < RB; ++i) sws[i] = 0.0f;
#pragma unroll
  for (int i = 0; i < RPR; ++i)
#pragma unroll
    for (int m = 0; m < NM; ++m) sws[i * NM + m] = sm[m][min(row0 + i, a.N - 1)];
  // 2. pass-0 weight loads of every row of this wave (rows past N re-read row N-1; never stored)
  static_assert(R >= 1 && R <= 8, "row partials per lane");
  uint4 wa[NM][RPR][CPT];
  uint4 wb[NM][MULTI ? RPR : 1][MULTI ? CPT : 1];
  auto issue = [&](auto& buf, int pass) {
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
      const int c = min(pass * PASSC + lane + 64 * j, n16 - 1);
#pragma unroll
      for (int i = 0; i < RPR; ++i)
#pragma unroll
        for (int m = 0; m < NM; ++m) {
          const size_t n = (size_t)min(row0 + i, a.N - 1);
          buf[m][i][j] = ld_nt16(wm[m] + n * K + (size_t)c * 16);
        }
    }
  };
  issue(wa, 0);
  uint32_t res = 0;
  if (RES) res = a.residual[min(row0 + (lane & (RPR - 1)), a.N - 1)];
  __builtin_amdgcn_sched_barrier(0);  // nothing that waits on x may move above the weight loads

  // 3. RMSNorm (optional), outlier columns and s_x, then the int8 image of x into LDS while the weights stream
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
    rs = 1.0f / sqrtf(((red[0] + red[1]) + (red[2] + red[3])) / (float)K + a.eps);
  }
  float amax = 0.0f;
  uint64_t obits = 0;  // 8 outlier bits per uint4 of this thread
#pragma unroll
  for (int i = 0; i < XPT; ++i) {
    const bool ok = t + 256 * i < n8;
    uint32_t d[4] = {xr[i].x, xr[i].y, xr[i].z, xr[i].w};
    if (NORM) {  // bf16(w * (x * rs)), two elements per instruction
      const uint32_t nw[4] = {nr[i].x, nr[i].y, nr[i].z, nr[i].w};
#pragma unroll
      for (int q = 0; q < 4; ++q)
        d[q] = pack2(__fmul_rn(bflo(nw[q]), __fmul_rn(bflo(d[q]), rs)),
                     __fmul_rn(bfhi(nw[q]), __fmul_rn(bfhi(d[q]), rs)));
      xr[i] = make_uint4(d[0], d[1], d[2], d[3]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float lo = fabsf(bflo(d[q])), hi = fabsf(bfhi(d[q]));
      const bool olo = ok && a.thr > 0.0f && lo >= a.thr, ohi = ok && a.thr > 0.0f && hi >= a.thr;
      obits |= (uint64_t)(olo ? 1u : 0u) << (8 * i + 2 * q);
      obits |= (uint64_t)(ohi ? 1u : 0u) << (8 * i + 2 * q + 1);
      amax = fmaxf(amax, (ok && !olo) ? lo : 0.0f);
      amax = fmaxf(amax, (ok && !ohi) ? hi : 0.0f);
    }
  }
  static_assert(XPT <= 8, "obits is 64 bits");
  amax = wave_max(amax);
  const bool wany = __any(obits != 0);
  if (lane == 0) {
    red[4 + wave] = amax;
    red[8 + wave] = wany ? 1.0f : 0.0f;
  }
  __syncthreads();
  const float sx = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
  const bool anyout = (red[8] + red[9]) + (red[10] + red[11]) > 0.0f;  // block-uniform
  const float inv = q8_inv(sx);
#pragma unroll
  for (int i = 0; i < XPT; ++i) {
    const int u = t + 256 * i;
    const uint32_t d[4] = {xr[i].x, xr[i].y, xr[i].z, xr[i].w};
    const uint32_t ob = (uint32_t)(obits >> (8 * i)) & 0xFFu;
    uint32_t pk[2] = {0u, 0u};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int lo = (ob >> (2 * q)) & 1u ? 0 : q8(bflo(d[q]), inv);
      const int hi = (ob >> (2 * q + 1)) & 1u ? 0 : q8(bfhi(d[q]), inv);
      pk[q >> 1] |= ((uint32_t)lo & 0xFFu) << (16 * (q & 1));
      pk[q >> 1] |= ((uint32_t)hi & 0xFFu) << (16 * (q & 1) + 8);
    }
    if (u < n8) {
      ((uint2*)xq)[u] = make_uint2(pk[0], pk[1]);
      xb[u] = xr[i];
      om[u] = (unsigned char)ob;
    }
  }
  __syncthreads();

  // 4. dot every row of this wave pass by pass
  int acc[RB];
  float outp[RB];
#pragma unroll
  for (int i = 0; i < RB; ++i) {
    acc[i] = 0;
    outp[i] = 0.0f;
  }
  auto consume = [&](const auto& buf, int pass) {
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
      const int c = pass * PASSC + lane + 64 * j;
      const bool ok = c < n16;
      const int cc = min(c, n16 - 1);
      const uint4 xv = xq[cc];
#pragma unroll
      for (int i = 0; i < RPR; ++i)
#pragma unroll
        for (int m = 0; m < NM; ++m) {
          const uint4 wv = buf[m][i][j];
          int d = __builtin_amdgcn_sdot4((int)wv.x, (int)xv.x, 0, false);
          d = __builtin_amdgcn_sdot4((int)wv.y, (int)xv.y, d, false);
          d = __builtin_amdgcn_sdot4((int)wv.z, (int)xv.z, d, false);
          d = __builtin_amdgcn_sdot4((int)wv.w, (int)xv.w, d, false);
          acc[i * NM + m] += ok ? d : 0;
        }
      if (anyout) {
        const uint32_t mk = ok ? (uint32_t)((const uint16_t*)om)[cc] : 0u;
        if (mk) {  // rare: this chunk holds outlier columns; the other columns contribute x = 0
          const uint4 b0 = xb[2 * cc], b1 = xb[2 * cc + 1];
          const uint32_t xw[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
          float xo[16];
#pragma unroll
          for (int b = 0; b < 16; ++b)
            xo[b] = (mk >> b) & 1u ? ((b & 1) ? bfhi(xw[b >> 1]) : bflo(xw[b >> 1])) : 0.0f;
#pragma unroll
          for (int i = 0; i < RPR; ++i)
#pragma unroll
            for (int m = 0; m < NM; ++m) {
              const uint4 wv = buf[m][i][j];
              const uint32_t ww[4] = {wv.x, wv.y, wv.z, wv.w};
              const float s127 = mul_rn(sws[i * NM + m], 1.0f / 127.0f);
              float o = outp[i * NM + m];
#pragma unroll
              for (int b = 0; b < 16; ++b) o = fmaf(xo[b], mul_rn(sbyte(ww[b >> 2], b & 3), s127), o);
              outp[i * NM + m] = o;
            }
        }
      }
    }
  };
  if constexpr (MULTI) {
    for (int p = 0; p < passes; p += 2) {
      if (p + 1 < passes) issue(wb, p + 1);
      consume(wa, p);
      if (p + 1 < passes) {
        if (p + 2 < passes) issue(wa, p + 2);
        consume(wb, p + 1);
      }
    }
  } else {
    consume(wa, 0);
  }

  // 5. one integer butterfly for all rows of the wave; the outlier partials only when the row has outliers
  const int vi = bfly_index<RB>(lane);  // value index held by this lane
  float swv = sws[0], outv = 0.0f;
  if (anyout) {
#pragma unroll
    for (int k = 0; k < R; ++k) outp[k] = wave_sum(outp[k]);
    outv = outp[0];
  }
#pragma unroll
  for (int k = 1; k < RB; ++k) {
    swv = vi == k ? sws[k] : swv;
    outv = vi == k ? outp[k] : outv;
  }
  const int tot = butterfly_i<RB>(acc, lane);
  constexpr int GROUP = 64 / RB;  // lanes per value after the butterfly
  const float mainv = int8_main(tot, sx, swv);
  float o = add_rn(mainv, outv);
  if (DUAL) {
    // value index = 2*row + matrix: the fc_2 partner of a row sits in the lane whose value index differs in bit 0
    constexpr int PD = RB == 8 ? 8 : (RB == 4 ? 16 : 32);
    const float mine = round_bf(o);
    const float other = PD == 8 ? LGA_DPP(mine, 0x128) : __shfl_xor(mine, PD);
    const int row = row0 + (vi >> 1);
    if ((lane & (GROUP - 1)) == 0 && (vi & 1) == 0 && row < a.N) {
      const float g = round_bf(silu_f(mine));       // silu(bf16(fc_1 x)) -> bf16
      a.y[row] = f2bf(__fmul_rn(g, other));          // * bf16(fc_2 x)
    }
  } else {
    const uint32_t rv = RES ? (uint32_t)__shfl(res, vi) : 0u;  // residual of row vi sits in lane vi
    const int row = row0 + vi;
    if (a.bias) o = add_rn(o, bf2f(a.bias[min(row, a.N - 1)]));
    if (RES) o = round_bf(o) + __uint_as_float(rv << 16);
    if ((lane & (GROUP - 1)) == 0 && vi < RPR && row < a.N) a.y[row] = f2bf(o);
  }
}

template <int RPR, bool DUAL, int XPT, int CPT, bool MULTI>
static void launch_i8(const GemvI8Args& a, hipStream_t stream) {
  const int waves = (a.N + RPR - 1) / RPR;
  const dim3 blocks((waves + 3) / 4);
  const size_t lds = (size_t)a.K * 3 + ((a.K / 8 + 15) & ~15) + 12 * 4;
  const bool norm = a.norm_w != nullptr, res = a.residual != nullptr;
  if (DUAL) {
    if (norm) gemv_int8_kernel<RPR, DUAL, true, false, XPT, CPT, MULTI><<<blocks, 256, lds, stream>>>(a);
    else gemv_int8_kernel<RPR, DUAL, false, false, XPT, CPT, MULTI><<<blocks, 256, lds, stream>>>(a);
  } else if (norm) {
    if (res) gemv_int8_kernel<RPR, DUAL, true, true, XPT, CPT, MULTI><<<blocks, 256, lds, stream>>>(a);
    else gemv_int8_kernel<RPR, DUAL, true, false, XPT, CPT, MULTI><<<blocks, 256, lds, stream>>>(a);
  } else {
    if (res) gemv_int8_kernel<RPR, DUAL, false, true, XPT, CPT, MULTI><<<blocks, 256, lds, stream>>>(a);
    else gemv_int8_kernel<RPR, DUAL, false, false, XPT, CPT, MULTI><<<blocks, 256, lds, stream>>>(a);
  }
}

template <bool DUAL>
static int dispatch_i8(const GemvI8Args& a, hipStream_t stream) {
  const int n16 = a.K / 16;
  // the same 16-B loads in flight per wave as the bf16 kernel: K <= 4096 4 chunks x 4 rows (fc_1 || fc_2: 2 rows of
  // each), K <= 8192 8 chunks x 2 rows, longer rows double-buffered passes of 4096 columns x 2 rows
  if (n16 <= 256) {
    if (DUAL) launch_i8<2, true, 2, 4, false>(a, stream);
    else launch_i8<4, false, 2, 4, false>(a, stream);
  } else if (n16 <= 512) {
    if (DUAL) launch_i8<1, true, 4, 8, false>(a, stream);
    else launch_i8<2, false, 4, 8, false>(a, stream);
  } else if (n16 <= 768) {  // K <= 12288
    if (DUAL) launch_i8<1, true, 6, 4, true>(a, stream);
    else launch_i8<2, false, 6, 4, true>(a, stream);
  } else if (n16 <= 1024) {  // K <= 16384
    if (DUAL) launch_i8<1, true, 8, 4, true>(a, stream);
    else launch_i8<2, false, 8, 4, true>(a, stream);
  } else {
    lga_set_error("lga_int8_gemv: K > 16384 is not supported");
    return (int)hipErrorInvalidValue;
  }
  return 0;
}

}  // namespace lga

extern "C" int lga_int8_gemv(const void* x, const void* qweight, const float* scales, const void* bias,
                             const void* residual, const void* norm_weight, float norm_eps, float threshold, void* y,
                             int N, int K, hipStream_t stream) {
  LGA_CHECK_ARG(x && qweight && scales && y, "lga_int8_gemv: null pointer");
  LGA_CHECK_ARG(N > 0 && K > 0 && K % 16 == 0, "lga_int8_gemv: K must be a positive multiple of 16");
  LGA_CHECK_ARG(((uintptr_t)x | (uintptr_t)qweight | (uintptr_t)(norm_weight ? norm_weight : x)) % 16 == 0,
                "lga_int8_gemv: x, qweight and norm_weight must be 16-B aligned");
  lga::GemvI8Args a{(const uint16_t*)x, (const int8_t*)qweight, nullptr, scales, nullptr, (const uint16_t*)bias,
                    (const uint16_t*)residual, (const uint16_t*)norm_weight, (uint16_t*)y, N, K, norm_eps, threshold};
  const int rc = lga::dispatch_i8<false>(a, stream);
  if (rc) return rc;
  LGA_LAUNCH_RETURN();
}

extern "C" int lga_int8_gemv_swiglu(const void* x, const void* qweight1, const float* scales1, const void* qweight2,
                                    const float* scales2, const void* norm_weight, float norm_eps, float threshold,
                                    void* y, int N, int K, hipStream_t stream) {
  LGA_CHECK_ARG(x && qweight1 && scales1 && qweight2 && scales2 && y, "lga_int8_gemv_swiglu: null pointer");
  LGA_CHECK_ARG(N > 0 && K > 0 && K % 16 == 0, "lga_int8_gemv_swiglu: K must be a positive multiple of 16");
  LGA_CHECK_ARG(((uintptr_t)x | (uintptr_t)qweight1 | (uintptr_t)qweight2 |
                 (uintptr_t)(norm_weight ? norm_weight : x)) % 16 == 0,
                "lga_int8_gemv_swiglu: x, qweights and norm_weight must be 16-B aligned");
  lga::GemvI8Args a{(const uint16_t*)x, (const int8_t*)qweight1, (const int8_t*)qweight2, scales1, scales2, nullptr,
                    nullptr, (const uint16_t*)norm_weight, (uint16_t*)y, N, K, norm_eps, threshold};
  const int rc = lga::dispatch_i8<true>(a, stream);
  if (rc) return rc;
  LGA_LAUNCH_RETURN();
}
