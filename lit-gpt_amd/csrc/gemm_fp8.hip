// Prefill GEMM over fp8 (e4m3) weights, --quantize fp8-g128: Y[M, N] = X[M, K] . W'[N, K]^T (+bias) (+residual) with
// W'[n, k] = float(code[n, k]) * s[n, k / 128] — exact in bf16, so this is lga_bf16_gemm's arithmetic on the
// dequantized weight without that weight ever existing in HBM (or in LDS).
//
// MI355X design: (32 TI) x 128 output tile per 256-thread workgroup, 2 x 2 waves, each wave TI x 4 tiles of
// v_mfma_f32_16x16x32_bf16 (TI = 4: 128 rows; TI = 2: 64 rows for prompts of at most 64 tokens). K-step 64 = half a
// scale group, so a weight row has ONE scale per step. Both operand tiles go global -> LDS directly
// (global_load_lds_dwordx4), double-buffered, the next step's DMA issued before this step's MFMAs:
//  * X: 128-B rows of eight 16-B chunks, chunk index XOR (row & 7) (gemm.hip's image: the 16-lane ds_read_b128 groups
//    of the A fragments are conflict-free);
//  * W: the CODES, 64-B rows of four 16-B chunks — half of the bf16 tile's DMA and LDS bytes — chunk index XOR
//    ((row >> 2) & 3). A B fragment is 8 consecutive k of one row = one ds_read_b64; 32 lanes (16 rows x 2 k-blocks)
//    read 32 distinct 8-B slots of the 256-B bank window: rows r, r + 4, r + 8, r + 12 share (row & 3) and the XOR
//    sends them to different chunks.
// The 8 codes become the bf16 B fragment in registers on the way out of LDS: four v_cvt_scalef32_pk_bf16_fp8 with the
// row's scale (a power of two, kept as raw bf16 bits per (tile row, step) in 4 registers and fetched one step ahead).
// Epilogue with lga_bf16_gemm's rounding points: fp32 accumulator + bias, one bf16 rounding, then + residual.
// Short prompts are not split over K (the grid of an M <= 64 prefill is N / 128 workgroups): DESIGN §4.5g.
#include "kv8_ops.h"

namespace lga {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

constexpr int F8_BN = 128, F8_BK = 64;
constexpr int F8_B_BYTES = F8_BN * F8_BK;  // the code tile: 8 KB

struct GemmF8Args {
  const uint16_t* x;   // [M][K] bf16
  const uint8_t* w;    // [N][K] codes
  const uint16_t* sc;  // [N][K / 128] bf16
  const uint16_t* bias;
  const uint16_t* residual;  // [M][N]
  uint16_t* y;               // [M][N]
  int M, N, K;
};

__device__ __forceinline__ int f8_swz_x(int row, int chunk) { return row * 128 + 16 * (chunk ^ (row & 7)); }
// byte offset of the 8 codes (row, k-block u of 8 in 0..7) in the code tile
__device__ __forceinline__ int f8_swz_w(int row, int u) { return row * 64 + 16 * ((u >> 1) ^ ((row >> 2) & 3)) + 8 * (u & 1); }

__device__ __forceinline__ void f8_dma16(const void* g, unsigned char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds(g, (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

template <int TI>
__global__ void __launch_bounds__(256) gemm_fp8_kernel(GemmF8Args a) {
  constexpr int BM = 32 * TI, A_BYTES = BM * 128, STAGE = A_BYTES + F8_B_BYTES;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * STAGE];  // [buf][X | codes]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * F8_BN;
  const int nk = a.K / F8_BK, ng = a.K / 128;
  const int fr = lane & 15, fk = lane >> 4;

  // this lane's four B rows (rows past N re-read row N - 1; never stored) and their scales, one step ahead
  size_t srow[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) srow[j] = (size_t)min(n0 + wn * 64 + j * 16 + fr, a.N - 1) * ng;
  uint32_t snext[4];

  auto gload = [&](int kt) {
    unsigned char* A = lds + (kt & 1) * STAGE;
    unsigned char* B = A + A_BYTES;
#pragma unroll
    for (int i = 0; i < TI; ++i) {  // 8 X rows per wave instruction: lane -> (row r0 + lane / 8, physical chunk lane % 8)
      const int r0 = (wave * TI + i) * 8, r = r0 + (lane >> 3);
      const int lc = (lane & 7) ^ (r & 7);
      f8_dma16(a.x + (size_t)min(m0 + r, a.M - 1) * a.K + kt * F8_BK + lc * 8, A + r0 * 128);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {  // 16 code rows per wave instruction: lane -> (row r0 + lane / 4, physical chunk lane % 4)
      const int r0 = (wave * 2 + i) * 16, r = r0 + (lane >> 2);
      const int lc = (lane & 3) ^ ((r >> 2) & 3);
      f8_dma16(a.w + (size_t)min(n0 + r, a.N - 1) * a.K + kt * F8_BK + lc * 16, B + r0 * 64);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) snext[j] = a.sc[srow[j] + (kt >> 1)];
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
    float s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = __uint_as_float(snext[j] << 16);
    if (kt + 1 < nk) gload(kt + 1);
    const unsigned char* A = lds + (kt & 1) * STAGE;
    const unsigned char* B = A + A_BYTES;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {  // two 32-deep MFMA k-slices per step
      bf16x8_t af[TI], bfr[4];
#pragma unroll
      for (int i = 0; i < TI; ++i) af[i] = *(const bf16x8_t*)(A + f8_swz_x(wm * (16 * TI) + i * 16 + fr, sub * 4 + fk));
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint2 c = *(const uint2*)(B + f8_swz_w(wn * 64 + j * 16 + fr, sub * 4 + fk));
        const uint4 e = make_uint4(
            __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c.x, s[j], false)),
            __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c.x, s[j], true)),
            __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c.y, s[j], false)),
            __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c.y, s[j], true)));
        bfr[j] = __builtin_bit_cast(bf16x8_t, e);
      }
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
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
        const int m = m0 + wm * (16 * TI) + i * 16 + fk * 4 + r;
        if (m >= a.M) continue;
        float out = acc[i][j][r] + b;
        if (a.residual) out = round_bf(out) + bf2f(a.residual[(size_t)m * a.N + n]);
        a.y[(size_t)m * a.N + n] = f2bf(out);
      }
  }
}

int preload_fp8_gemv();
int preload_fp8_a8();
int preload_fp8() {
  return preload(gemm_fp8_kernel<2>) + preload(gemm_fp8_kernel<4>) + preload_fp8_gemv() + preload_fp8_a8();
}

}  // namespace lga

extern "C" int lga_fp8_gemm(const void* x, const uint8_t* codes, const void* scales, const void* bias,
                            const void* residual, void* y, int M, int N, int K, hipStream_t stream) {
  LGA_CHECK_ARG(x && codes && scales && y, "lga_fp8_gemm: null pointer");
  LGA_CHECK_ARG(M >= 2 && N > 0, "lga_fp8_gemm: needs M >= 2 rows (one row is lga_fp8_gemv) and N > 0");
  LGA_CHECK_ARG(K > 0 && K % 128 == 0, "lga_fp8_gemm: K must be a positive multiple of 128");
  LGA_CHECK_ARG(((uintptr_t)x | (uintptr_t)codes) % 16 == 0, "lga_fp8_gemm: x and codes must be 16-B aligned");
  lga::GemmF8Args a{(const uint16_t*)x, codes, (const uint16_t*)scales, (const uint16_t*)bias,
                    (const uint16_t*)residual, (uint16_t*)y, M, N, K};
  const int nx = (N + lga::F8_BN - 1) / lga::F8_BN;
  if (M <= 64) lga::gemm_fp8_kernel<2><<<dim3(nx, (M + 63) / 64), 256, 0, stream>>>(a);
  else lga::gemm_fp8_kernel<4><<<dim3(nx, (M + 127) / 128), 256, 0, stream>>>(a);
  LGA_LAUNCH_RETURN();
}
