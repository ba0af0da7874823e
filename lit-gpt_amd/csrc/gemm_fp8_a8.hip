// Prefill GEMM of --quantize fp8-g128-a8 on the block-scaled matrix instruction with BOTH operands e4m3:
// Y[M, N] = mx8(X)[M, K] . W'[N, K]^T (+bias) (+residual), W' the fp8-g128 weight (gemv_fp8.hip: e4m3fn codes [N][K], one
// bf16 power-of-two scale per 128 of K) and mx8 the MXFP8 rounding of gemm_mxfp4_a8.hip (lga_mx8_quantize: e4m3fn codes,
// one e8m0 byte per 32 columns). v_mfma_scale_f32_16x16x128_f8f6f4 with cbsz 0 and blgp 0 reads both code tiles as they
// lie in HBM and applies both scales itself: products of the codes are exact, accumulation is fp32, and there is no
// convert pass and no bf16 image of either operand, in LDS or in registers.
//
// MI355X design: (32 TI) x 128 output tile per 256-thread workgroup, 2 x 2 waves, each wave TI x 4 MFMAs of
// 16 x 16 x 128 per K-step (TI = 4: 128 rows; TI = 2: 64 rows for prompts of at most 64 tokens). A K-step is ONE MFMA
// depth, 128 = one weight scale group = four MX blocks of X. K % 128 == 0 (Fp8Linear's contract): there is no K tail.
//  * ONE LDS image per stage for both operands: (32 TI + 128) rows of 128 B, the X-code rows first, then the W-code
//    rows; a row is eight 16-B chunks and chunk c of row `row` lies at chunk c XOR ((row >> 1) & 7) (fa8_swz). Both
//    tiles go global -> LDS directly (global_load_lds_dwordx4), TI + 4 instructions per wave and step, each carrying 8
//    whole rows (lane -> row lane / 8, physical chunk lane % 8; the XOR is applied to the global address), two stages,
//    the next step's DMA issued before this step's MFMAs. 32 KB per stage at TI = 4 (64 KB, two workgroups per CU),
//    24 KB at TI = 2.
//  * Operand layout (fa8_fragment, the one place it is written; the same function serves A and B): the instruction's
//    lane (r, g) = (lane % 16, lane / 16) supplies, of row r of an 8-bit operand, k = 16 g .. 16 g + 15 in registers
//    0..3 and k = 64 + 16 g .. 64 + 16 g + 15 in registers 4..7: chunks g and 4 + g of the row, two ds_read_b128.
//    DESIGN §4.5j measured this for A; that B follows it is settled by the identity test of tests/test_gpu_fp8_a8.py
//    (X = I against the full-range weight: every code in every lane position of B).
//  * Banks: LDS has 64 banks of 4 B, a 256-B window of sixteen 16-B bank groups; a ds_read_b128 is served 16 lanes at a
//    time. The 16 lanes of a lane group read one logical chunk c of rows R .. R + 15, R a multiple of 16. Row parity
//    picks the half of the window (row * 128 mod 256) and c XOR ((row >> 1) & 7) the group within the half; over 16
//    consecutive rows (row >> 1) & 7 takes each of its 8 values once per parity, so the 16 lanes fall on the 16
//    distinct bank groups. A half-wave is two lane groups, each of which covers every bank group exactly once: 512 B
//    in the two passes that 512 B need, no conflict. The DMA side writes 1 KB of consecutive LDS per instruction.
//  * Scales never enter LDS, and no e8m0 copy of the weight scales exists anywhere. The weight scale group is the MFMA
//    depth, so all four lane groups of a weight row pass the SAME byte: lane (r, g) loads the 2-byte bf16 scale 2^e of
//    (its row of each of its four B fragments, step kt + 1) one step ahead (the four lane groups read one address) and
//    shifts it in a register: e8m0 = (bits >> 7) & 0xFF = e + 127, 1..254. The X scale is one byte per (row, block g),
//    loaded one step ahead as in gemm_mxfp4_a8.hip. The MFMA takes both with opsel 0.
// M and N tails: rows past M or N re-read the last row and are never stored.
// Epilogue with lga_bf16_gemm's rounding points: fp32 accumulator + bias, one bf16 rounding, then + residual.
// Not here: a split over K for short prompts, a fused fc_1 || fc_2 + SwiGLU form.
#include "kv8_ops.h"

namespace lga {

typedef int i32x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

constexpr int FA8_BN = 128, FA8_BK = 128;

struct GemmF8A8Args {
  const uint8_t* xc;    // [M][K] e4m3 codes
  const uint8_t* xs;    // [M][K / 32] e8m0
  const uint8_t* w;     // [N][K] e4m3 codes
  const uint16_t* ws;   // [N][K / 128] bf16 powers of two
  const uint16_t* bias;
  const uint16_t* residual;  // [M][N]
  uint16_t* y;               // [M][N]
  int M, N, K;
};

// byte offset of 16-B chunk c (0..7) of row `row` of a stage's image
__device__ __forceinline__ int fa8_swz(int row, int c) { return row * 128 + 16 * (c ^ ((row >> 1) & 7)); }

// the 32 bytes lane group g supplies of an 8-bit operand's row: k = 16 g .. 16 g + 15, then k = 64 + 16 g .. + 15
__device__ __forceinline__ i32x8_t fa8_fragment(const unsigned char* image, int row, int g) {
  const uint4 lo = *(const uint4*)(image + fa8_swz(row, g)), hi = *(const uint4*)(image + fa8_swz(row, 4 + g));
  return i32x8_t{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
}

__device__ __forceinline__ void fa8_dma16(const void* g, unsigned char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds(g, (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

template <int TI>
__global__ void __launch_bounds__(256) gemm_fp8_a8_kernel(GemmF8A8Args a) {
  constexpr int BM = 32 * TI, ROWS = BM + FA8_BN, STAGE = ROWS * FA8_BK;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * STAGE];  // [buf][X-code rows | W-code rows][128 B]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * FA8_BN;
  const int nk = a.K / FA8_BK;
  const int fr = lane & 15, fg = lane >> 4;

  // DMA: instruction i of this wave carries image rows 8 (wave (TI + 4) + i) .. + 7; this lane's row of it, its source
  // row (rows past M / N re-read the last one) and the logical chunk that lands at physical chunk lane % 8
  const uint8_t* src[TI + 4];
#pragma unroll
  for (int i = 0; i < TI + 4; ++i) {
    const int r = (wave * (TI + 4) + i) * 8 + (lane >> 3);
    const int lc = (lane & 7) ^ ((r >> 1) & 7);
    src[i] = (r < BM ? a.xc + (size_t)min(m0 + r, a.M - 1) * a.K
                     : a.w + (size_t)min(n0 + r - BM, a.N - 1) * a.K) + lc * 16;
  }
  // this lane's TI A rows and four B rows: where their scales lie
  const uint8_t* xs[TI];
  const uint16_t* ws[4];
#pragma unroll
  for (int i = 0; i < TI; ++i) xs[i] = a.xs + (size_t)min(m0 + wm * (16 * TI) + i * 16 + fr, a.M - 1) * (a.K / 32) + fg;
#pragma unroll
  for (int j = 0; j < 4; ++j) ws[j] = a.ws + (size_t)min(n0 + wn * 64 + j * 16 + fr, a.N - 1) * nk;
  int sa_next[TI], sb_next[4];

  auto gload = [&](int kt) {
    unsigned char* image = lds + (kt & 1) * STAGE;
#pragma unroll
    for (int i = 0; i < TI + 4; ++i) fa8_dma16(src[i] + (size_t)kt * FA8_BK, image + (wave * (TI + 4) + i) * 1024);
#pragma unroll
    for (int i = 0; i < TI; ++i) sa_next[i] = xs[i][kt * 4];
#pragma unroll
    for (int j = 0; j < 4; ++j) sb_next[j] = ws[j][kt];
  };

  f32x4_t acc[TI][4];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  gload(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    int sa[TI], sb[4];
#pragma unroll
    for (int i = 0; i < TI; ++i) sa[i] = sa_next[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) sb[j] = (sb_next[j] >> 7) & 0xFF;  // bf16 2^e -> e8m0 e + 127
    if (kt + 1 < nk) gload(kt + 1);
    const unsigned char* image = lds + (kt & 1) * STAGE;
    i32x8_t af[TI], bfr[4];
#pragma unroll
    for (int i = 0; i < TI; ++i) af[i] = fa8_fragment(image, wm * (16 * TI) + i * 16 + fr, fg);
#pragma unroll
    for (int j = 0; j < 4; ++j) bfr[j] = fa8_fragment(image, BM + wn * 64 + j * 16 + fr, fg);
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af[i], bfr[j], acc[i][j], 0, 0, 0, sa[i], 0,
                                                                     sb[j]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's LDS-direct loads (and scales) have landed
    __syncthreads();
  }

#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = n0 + wn * 64 + j * 16 + fr;
    if (n >= a.N) continue;
    const float b = a.bias ? bf2f(a.bias[n]) : 0.0f;
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm * (16 * TI) + i * 16 + fg * 4 + r;
        if (m >= a.M) continue;
        float out = acc[i][j][r] + b;
        if (a.residual) out = round_bf(out) + bf2f(a.residual[(size_t)m * a.N + n]);
        a.y[(size_t)m * a.N + n] = f2bf(out);
      }
  }
}

int preload_fp8_a8() { return preload(gemm_fp8_a8_kernel<2>) + preload(gemm_fp8_a8_kernel<4>); }

}  // namespace lga

extern "C" int lga_fp8_a8_gemm(const uint8_t* xcodes, const uint8_t* xscales, const uint8_t* codes, const void* scales,
                               const void* bias, const void* residual, void* y, int M, int N, int K,
                               hipStream_t stream) {
  LGA_CHECK_ARG(xcodes && xscales && codes && scales && y, "lga_fp8_a8_gemm: null pointer");
  LGA_CHECK_ARG(M >= 1 && N > 0, "lga_fp8_a8_gemm: needs M >= 1 rows and N > 0");
  LGA_CHECK_ARG(K > 0 && K % 128 == 0, "lga_fp8_a8_gemm: K must be a positive multiple of 128");
  LGA_CHECK_ARG(((uintptr_t)xcodes | (uintptr_t)codes) % 16 == 0,
                "lga_fp8_a8_gemm: xcodes and codes must be 16-B aligned");
  lga::GemmF8A8Args a{xcodes, xscales, codes, (const uint16_t*)scales, (const uint16_t*)bias, (const uint16_t*)residual,
                      (uint16_t*)y, M, N, K};
  const int nx = (N + lga::FA8_BN - 1) / lga::FA8_BN;
  if (M <= 64) lga::gemm_fp8_a8_kernel<2><<<dim3(nx, (M + 63) / 64), 256, 0, stream>>>(a);
  else lga::gemm_fp8_a8_kernel<4><<<dim3(nx, (M + 127) / 128), 256, 0, stream>>>(a);
  LGA_LAUNCH_RETURN();
}
