// The pass skeleton of the one-shot weight-stream decode GEMVs (gemv_bf16.hip, gemv_mxfp4.hip; in pieces
// gemv_int8.hip), once. DESIGN §4.1a. (gemv_fp8.hip still carries its own copy: on this skeleton two of its launches
// measured slower.)
//
//  * One wave per row slot owns RPR consecutive rows (of each matrix: fc_1 || fc_2 when DUAL). A weight row is a run of
//    16-B chunks; a "pass" is 64 * CPT of them: lane l holds the chunks l, l + 64, ..., so each wave instruction reads
//    1 KB contiguous of one row. Rows past N re-read row N - 1, chunks (and scales) past the row re-read its last one;
//    neither is ever used.
//  * The thread's share of x (and of the norm weight) is fetched first, then EVERY weight and scale load of pass 0 is
//    issued, behind a sched_barrier: nothing that waits on x may move above them. The fused RMSNorm
//    (lit_gpt/rmsnorm.py:19-25, the reference's rounding points) then stages x into LDS while the weights stream.
//  * Rows of several passes double-buffer them: the next pass's loads are issued before this pass's math (vmcnt retires
//    in order, so only the current pass is waited for).
//  * One transposed butterfly reduces all row partials of the wave; bias / residual / SwiGLU epilogues with the
//    reference's bf16 rounding points.
//
// A format is a trait struct F that says only what differs:
//   CPT                 16-B chunks per lane per row per pass
//   PLANES              uint4 of x per chunk: a chunk is 8 * PLANES columns, a row 2 K / PLANES bytes; x sits in LDS as
//                       PLANES planes (plane q = the q-th 16 B of every chunk's x), so each ds_read_b128 is
//                       lane-contiguous
//   SPL                 scale registers per lane per (row, pass): 0 none, CPT one per chunk
//   rows(dual, multi)   rows of each matrix per wave when the row is one pass / several
//   MAX_K, NORM_MAX_K   largest K, largest K whose RMSNorm fuses (the XPT = 16 class carries no norm kernels below it)
//   RED_ALWAYS          the launch asks for the 16 B of norm reduction LDS even without a norm
//   PARTNER_DPP8        the SwiGLU partner at lane distance 8 comes by DPP row_ror:8 rather than ds_swizzle
//   load_scale(sc, n, K, pass, lane, j)   raw bits of scale register j of row n                       (SPL > 0)
//   scale(s, lane, j)                     the fp32 scale of the lane's chunk j out of those registers  (SPL > 0)
//   chunk_dot(w, x, s)                    dot of one chunk against its 8 * PLANES activations (s = 1 without scales)
#pragma once
#include <cstdio>
#include <type_traits>

#include "decode_ops.h"

namespace lga {

struct GemvPassArgs {
  const uint16_t* x;         // [K] bf16
  const uint8_t* w;          // [N][2 K / PLANES] weights or codes
  const uint8_t* w2;         // dual: fc_2
  const void* sc;            // the format's scales (null: none)
  const void* sc2;           // dual
  const uint16_t* bias;      // [N] or null
  const uint16_t* residual;  // [N] or null
  const uint16_t* norm_w;    // [K] or null (fused RMSNorm)
  uint16_t* y;               // [N]
  int N, K;
  float eps;
};

// the loads of one pass in flight: chunk j of row i of matrix m, and the scale registers of that (row, pass)
template <int NM, int RPR, int CPT, int SPL>
struct PassBuf {
  uint4 w[NM][RPR][CPT];
  uint32_t s[NM][RPR][SPL < 1 ? 1 : SPL];
};

// ------------------------------------------------------------------------------------------- x: fetch, norm, staging
// activation (and norm weight) share of this thread: uint4 t, t + 256, ... (clamped, branch-free)
template <bool NORM, int XPT>
__device__ __forceinline__ void fetch_x(const uint16_t* x, const uint16_t* norm_w, int t, int n8, uint4 (&xr)[XPT],
                                        uint4 (&nr)[XPT]) {
#pragma unroll
  for (int i = 0; i < XPT; ++i) {
    const int u = min(t + 256 * i, n8 - 1);
    xr[i] = ((const uint4*)x)[u];
    if (NORM) nr[i] = ((const uint4*)norm_w)[u];
  }
}

// this thread's sum of squares, fma in a fixed order
template <int XPT>
__device__ __forceinline__ float sum_squares(const uint4 (&xr)[XPT], int t, int n8) {
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
  return ss;
}

// 1 / rms of the block's row out of the threads' sums: each wave's sum into red[wave], a barrier (the caller's), then
// the four in one order
__device__ __forceinline__ void rms_wave(float ss, float* red, int wave, int lane) {
  ss = wave_sum_uniform(ss);
  if (lane == 0) red[wave] = ss;
}
__device__ __forceinline__ float rms_block(const float* red, int K, float eps) {
  return 1.0f / sqrtf(((red[0] + red[1]) + (red[2] + red[3])) / (float)K + eps);
}

// what is staged of 8 activations: NORM bf16(w * (x * rs)), two roundings, two elements per instruction; else x
template <bool NORM>
__device__ __forceinline__ uint4 normalise(const uint4& x, const uint4& w, float rs) {
  uint32_t d[4] = {x.x, x.y, x.z, x.w};
  if (NORM) {
    const uint32_t nw[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int q = 0; q < 4; ++q)
      d[q] = pack2(__fmul_rn(bflo(nw[q]), __fmul_rn(bflo(d[q]), rs)),
                   __fmul_rn(bfhi(nw[q]), __fmul_rn(bfhi(d[q]), rs)));
  }
  return make_uint4(d[0], d[1], d[2], d[3]);
}

// uint4 u of a row of x among PLANES planes of pc chunks each
template <int PLANES>
__device__ __forceinline__ int plane_index(int u, int pc) {
  constexpr int SH = PLANES == 4 ? 2 : (PLANES == 2 ? 1 : 0);
  static_assert(PLANES == 1 << SH, "1, 2 or 4 planes");
  return (u & (PLANES - 1)) * pc + (u >> SH);
}

// ------------------------------------------------------------------------------------------- weights and scales
// The weight loads of one pass of every row of this wave; a 16-B chunk is COLS columns of a row. row0 and lane come by
// reference: by value, the compiler keeps the addresses of a whole pass live across the pass loop (20 VGPRs more in
// the bf16 kernels, an occupancy step in some)
template <int COLS, int NM, int RPR, int CPT, int SPL>
__device__ __forceinline__ void issue_codes(PassBuf<NM, RPR, CPT, SPL>& buf, const GemvPassArgs& a, const int& row0,
                                            const int& lane, int pass) {
  const int nch = a.K / COLS;
  const uint8_t* wm[2] = {a.w, NM == 2 ? a.w2 : a.w};
#pragma unroll
  for (int j = 0; j < CPT; ++j) {
    const int c = min(pass * (64 * CPT) + lane + 64 * j, nch - 1);
#pragma unroll
    for (int i = 0; i < RPR; ++i)
#pragma unroll
      for (int m = 0; m < NM; ++m) {
        const size_t n = (size_t)min(row0 + i, a.N - 1);
        buf.w[m][i][j] = ld_nt16(wm[m] + (n * nch + (size_t)c) * 16);
      }
  }
}

// the loads of one pass of a format: the chunks, then behind them the scales
template <class F, int NM, int RPR, int CPT, int SPL>
__device__ __forceinline__ void issue_pass(PassBuf<NM, RPR, CPT, SPL>& buf, const GemvPassArgs& a, const int& row0,
                                           const int& lane, int pass) {
  issue_codes<8 * F::PLANES>(buf, a, row0, lane, pass);
  if constexpr (SPL > 0) {
    const void* sm[2] = {a.sc, NM == 2 ? a.sc2 : a.sc};
#pragma unroll
    for (int j = 0; j < SPL; ++j)
#pragma unroll
      for (int i = 0; i < RPR; ++i)
#pragma unroll
        for (int m = 0; m < NM; ++m) {
          const size_t n = (size_t)min(row0 + i, a.N - 1);
          buf.s[m][i][j] = F::load_scale(sm[m], n, a.K, pass, lane, j);
        }
  }
}

// the double-buffered pass loop: issue(buf, pass) starts a pass's loads, consume(buf, pass) does its math
template <bool MULTI, class BufA, class BufB, class Issue, class Consume>
__device__ __forceinline__ void pass_loop(int passes, BufA& wa, BufB& wb, Issue issue, Consume consume) {
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
}

// ------------------------------------------------------------------------------------------- butterfly and epilogues
// R = NM * RPR partials per lane (R may be 1: the butterfly runs on RB = max(R, 2) values, the spare one zero) to y.
// res holds the residual of row (lane & (RPR - 1)); with_res may be a run-time flag.
template <class F, int RPR, bool DUAL>
__device__ __forceinline__ void reduce_store(float* part, uint32_t res, bool with_res, const uint16_t* bias,
                                             uint16_t* y, int N, int row0, int lane) {
  constexpr int R = (DUAL ? 2 : 1) * RPR;
  constexpr int RB = R < 2 ? 2 : R;
  const float tot = butterfly<RB>(part, lane);
  const int vi = bfly_index<RB>(lane);  // value index held by this lane
  constexpr int GROUP = 64 / RB;        // lanes per value after the butterfly
  if (DUAL) {
    // value index = 2 * row + matrix: the fc_2 partner of a row sits in the lane whose value index differs in bit 0
    constexpr int PD = RB == 8 ? 8 : (RB == 4 ? 16 : 32);
    const float other = PD == 8 && F::PARTNER_DPP8 ? LGA_DPP(tot, 0x128) : __shfl_xor(tot, PD);
    const int row = row0 + (vi >> 1);
    if ((lane & (GROUP - 1)) == 0 && (vi & 1) == 0 && row < N) {
      const float g = round_bf(silu_f(round_bf(tot)));  // silu(bf16(fc_1 x)) -> bf16
      y[row] = f2bf(__fmul_rn(g, round_bf(other)));     // * bf16(fc_2 x)
    }
  } else {
    const int row = row0 + vi;
    float o = tot;
    if (with_res) {
      const uint32_t rv = (uint32_t)__shfl(res, vi);  // residual of row vi sits in lane vi
      o = round_bf(bias ? o + bf2f(bias[min(row, N - 1)]) : o) + __uint_as_float(rv << 16);
    } else if (bias) {
      o += bf2f(bias[min(row, N - 1)]);
    }
    if ((lane & (GROUP - 1)) == 0 && (RB == R || vi < RPR) && row < N) y[row] = f2bf(o);
  }
}

// ------------------------------------------------------------------------------------------- the one-row kernel body
template <class F, int RPR, bool DUAL, bool NORM, bool RES, int XPT, bool MULTI>
__device__ __forceinline__ void gemv_pass_body(const GemvPassArgs& a, unsigned char* smem) {
  uint4* xl = (uint4*)smem;                        // PLANES planes of nch uint4
  float* red = (float*)(smem + (size_t)a.K * 2);   // 4 (NORM only)
  constexpr int NM = DUAL ? 2 : 1;                 // weight matrices
  constexpr int R = NM * RPR;                      // values per lane entering the butterfly
  constexpr int RB = R < 2 ? 2 : R;
  static_assert(R >= 1 && R <= 8, "row partials per lane");
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int n8 = a.K / 8, nch = a.K / (8 * F::PLANES);
  const int passes = MULTI ? (nch + 64 * F::CPT - 1) / (64 * F::CPT) : 1;
  const int row0 = (blockIdx.x * 4 + wave) * RPR;

  // 1. this thread's share of x, 2. the pass-0 loads of every row of this wave
  uint4 xr[XPT], nr[XPT];
  fetch_x<NORM>(a.x, a.norm_w, t, n8, xr, nr);
  PassBuf<NM, RPR, F::CPT, F::SPL> wa;
  PassBuf<NM, MULTI ? RPR : 1, MULTI ? F::CPT : 1, MULTI ? F::SPL : 0> wb;
  auto issue = [&](auto& buf, int pass) { issue_pass<F>(buf, a, row0, lane, pass); };
  issue(wa, 0);
  uint32_t res = 0;
  if (RES) res = a.residual[min(row0 + (lane & (RPR - 1)), a.N - 1)];
  __builtin_amdgcn_sched_barrier(0);  // nothing that waits on x may move above the weight loads

  // 3. stage x into LDS (RMS-normalised when NORM) while the weights stream
  float rs = 1.0f;
  if (NORM) {
    rms_wave(sum_squares(xr, t, n8), red, wave, lane);
    __syncthreads();
    rs = rms_block(red, a.K, a.eps);
  }
#pragma unroll
  for (int i = 0; i < XPT; ++i) {
    const int u = t + 256 * i;
    const uint4 v = normalise<NORM>(xr[i], nr[i], rs);  // (outside the branch: only the store is predicated)
    if (u < n8) xl[plane_index<F::PLANES>(u, nch)] = v;
  }
  __syncthreads();

  // 4. dot every row of this wave pass by pass, then one butterfly for all of them
  float part[RB];
#pragma unroll
  for (int i = 0; i < RB; ++i) part[i] = 0.0f;
  auto consume = [&](const auto& buf, int pass) {
#pragma unroll
    for (int j = 0; j < F::CPT; ++j) {
      const int c = pass * (64 * F::CPT) + lane + 64 * j;
      const bool ok = c < nch;
      const int cc = min(c, nch - 1);
      uint4 x[F::PLANES];
#pragma unroll
      for (int q = 0; q < F::PLANES; ++q) x[q] = xl[q * nch + cc];
#pragma unroll
      for (int i = 0; i < RPR; ++i)
#pragma unroll
        for (int m = 0; m < NM; ++m) {
          float s = 1.0f;
          if constexpr (F::SPL > 0) s = F::scale(buf.s[m][i], lane, j);
          const float d = F::chunk_dot(buf.w[m][i][j], x, s);
          part[i * NM + m] += ok ? d : 0.0f;
        }
    }
  };
  pass_loop<MULTI>(passes, wa, wb, issue, consume);
  reduce_store<F, RPR, DUAL>(part, res, RES, a.bias, a.y, a.N, row0, lane);
}

// ------------------------------------------------------------------------------------------- host side
template <class F>
static size_t gemv_pass_lds(const GemvPassArgs& a) {
  return (size_t)a.K * 2 + (F::RED_ALWAYS || a.norm_w ? 16 : 0);
}

// The launcher: NORM x RES selection. launch(norm, res, blocks) launches the caller's kernel at the two flags
// (std::true_type / std::false_type); without CAN_NORM no norm instantiation exists.
template <int RPR, bool DUAL, bool CAN_NORM, class Launch>
static void gemv_launch(const GemvPassArgs& a, Launch launch) {
  const int waves = (a.N + RPR - 1) / RPR;
  const dim3 blocks((waves + 3) / 4);
  const bool res = !DUAL && a.residual != nullptr;
  if constexpr (CAN_NORM) {
    if (a.norm_w) {
      if (res) launch(std::true_type{}, std::true_type{}, blocks);
      else launch(std::true_type{}, std::false_type{}, blocks);
      return;
    }
  }
  if (res) launch(std::false_type{}, std::true_type{}, blocks);
  else launch(std::false_type{}, std::false_type{}, blocks);
}

// a K class: rows per wave (of each matrix), uint4 of x per thread, several passes, whether the norm fuses
template <int RPR_, int XPT_, bool MULTI_, bool CAN_NORM_>
struct GemvClass {
  static constexpr int RPR = RPR_, XPT = XPT_;
  static constexpr bool MULTI = MULTI_, CAN_NORM = CAN_NORM_;
};

// The K-class dispatcher: one pass (K <= 4096) | K <= 12288 | K <= 32768; launch(GemvClass) launches the class. A
// format whose norm stops fusing below MAX_K refuses such calls in its entry points (LGA_GEMV_LIMITS).
template <class F, bool DUAL, class Launch>
static int gemv_dispatch(const GemvPassArgs& a, const char* name, Launch launch) {
  if (a.K > F::MAX_K) {
    char msg[96];
    snprintf(msg, sizeof(msg), "%s: K > %d is not supported", name, F::MAX_K);
    lga_set_error(msg);
    return (int)hipErrorInvalidValue;
  }
  constexpr int RS = F::rows(DUAL, false), RM = F::rows(DUAL, true);
  if (a.K <= 4096) launch(GemvClass<RS, 2, false, true>{});
  else if (a.K <= 12288) launch(GemvClass<RM, 6, true, true>{});
  else launch(GemvClass<RM, 16, true, (F::NORM_MAX_K > 12288)>{});
  return 0;
}

}  // namespace lga

// The extern "C" checks every GEMV entry point shares: pointers, K, the format's K limits, 16-B alignment (ptrs: the &&
// of the required pointers; limits: LGA_GEMV_LIMITS(...) or nothing; addrs: the | of the (uintptr_t) addresses besides
// norm_weight; what: their names for the message).
#define LGA_GEMV_LIMITS(name, maxk, normk)                                                                     \
  LGA_CHECK_ARG(K <= maxk, name ": K > " #maxk " is not supported");                                           \
  LGA_CHECK_ARG(!norm_weight || K <= normk, name ": the fused RMSNorm takes K <= " #normk)
#define LGA_GEMV_CHECKS(name, kstep, ptrs, limits, addrs, what)                                                \
  LGA_CHECK_ARG(ptrs, name ": null pointer");                                                                  \
  LGA_CHECK_ARG(N > 0 && K > 0 && K % kstep == 0, name ": K must be a positive multiple of " #kstep);          \
  limits;                                                                                                      \
  LGA_CHECK_ARG(((addrs) | (uintptr_t)(norm_weight ? norm_weight : x)) % 16 == 0,                              \
                name ": " what " and norm_weight must be 16-B aligned")
