// Prefill GEMM over MXFP4 weights, --quantize mxfp4: Y[M, N] = X[M, K] . W'[N, K]^T (+bias) (+residual) with
// W'[n, k] = e2m1(code[n, k]) * 2^(scale[n, k / 32] - 127) — exact in bf16, so this is lga_bf16_gemm's arithmetic on
// the dequantized weight without that weight ever existing in HBM (or in LDS).
//
// MI355X design: (32 TI) x 128 output tile per 256-thread workgroup, 2 x 2 waves, each wave TI x 4 tiles of
// v_mfma_f32_16x16x32_bf16 (TI = 4: 128 rows; TI = 2: 64 rows for prompts of at most 64 tokens). One MFMA k-slice of
// 32 is exactly one MX block, so a B fragment has ONE scale. K-step 64 = two slices; K is a multiple of 32 only, so the
// last step may hold one slice: its missing half is fetched from a clamped address and never multiplied. Both operand
// tiles go global -> LDS directly (global_load_lds_dwordx4), double-buffered, the next step's DMA issued before this
// step's MFMAs:
//  * X: 128-B rows of eight 16-B chunks, chunk index XOR (row & 7) (gemm.hip's image: the 16-lane ds_read_b128 groups
//    of the A fragments are conflict-free);
//  * W: the CODES, 32-B rows of two 16-B chunks (one chunk = one MX block) — a 4 KB tile, a quarter of the bf16 tile's
//    DMA and LDS bytes, ONE DMA instruction per wave per step — chunk index XOR ((row >> 3) & 1). A B fragment is 8
//    consecutive k of one row = one ds_read_b32; the 64 lanes (16 rows x 4 k-blocks) read 64 distinct dwords of the
//    256-B bank window: rows r and r + 8 are 256 B apart and the XOR sends them to different chunks.
// The 8 codes become the bf16 B fragment in registers on the way out of LDS: four v_cvt_scalef32_pk_bf16_fp4 (byte
// select 0..3) with the block's scale 2^(e - 127); the e8m0 bytes of a lane's four rows are kept raw per (row, slice)
// in 8 registers and fetched one step ahead by byte loads (scale rows have no alignment).
// Epilogue with lga_bf16_gemm's rounding points: fp32 accumulator + bias, one bf16 rounding, then + residual.
// Short prompts are not split over K (the grid of an M <= 64 prefill is N / 128 workgroups): DESIGN §4.5i.
#include "decode_ops.h"

#ifndef LGA_MXFP4_SWAP
#define LGA_MXFP4_SWAP 0
#endif

namespace lga {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

constexpr int M4_BN = 128, M4_BK = 64;
constexpr int M4_B_BYTES = M4_BN * M4_BK / 2;  // the code tile: 4 KB

struct GemmMx4Args {
  const uint16_t* x;   // [M][K] bf16
  const uint8_t* w;    // [N][K / 2] code pairs
  const uint8_t* sc;   // [N][K / 32] e8m0
  const uint16_t* bias;
  const uint16_t* residual;  // [M][N]
  uint16_t* y;               // [M][N]
  int M, N, K;
};

__device__ __forceinline__ int m4_swz_x(int row, int chunk) { return row * 128 + 16 * (chunk ^ (row & 7)); }
// byte offset of the 8 codes (row, slice s of 32 in 0..1, k-block u of 8 in 0..3) in the code tile
__device__ __forceinline__ int m4_swz_w(int row, int s, int u) { return row * 32 + 16 * (s ^ ((row >> 3) & 1)) + 4 * u; }

__device__ __forceinline__ void m4_dma16(const void* g, unsigned char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds(g, (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

__device__ __forceinline__ uint32_t m4_pair(uint32_t p) {  // LGA_MXFP4_SWAP: the convert returned (odd, even) columns
  return LGA_MXFP4_SWAP ? __builtin_amdgcn_alignbit(p, p, 16) : p;
}

template <int TI>
__global__ void __launch_bounds__(256) gemm_mxfp4_kernel(GemmMx4Args a) {
  constexpr int BM = 32 * TI, A_BYTES = BM * 128, STAGE = A_BYTES + M4_B_BYTES;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * STAGE];  // [buf][X | codes]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * M4_BN;
  const int ng = a.K / 32, nk = (ng + 1) / 2, kb = a.K / 2;
  const int fr = lane & 15, fk = lane >> 4;

  // this lane's four B rows (rows past N re-read row N - 1; never stored) and their scale bytes, one step ahead
  size_t srow[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) srow[j] = (size_t)min(n0 + wn * 64 + j * 16 + fr, a.N - 1) * ng;
  uint32_t snext[4][2];

  auto gload = [&](int kt) {
    unsigned char* A = lds + (kt & 1) * STAGE;
    unsigned char* B = A + A_BYTES;
    const bool half = 2 * kt + 1 >= ng;  // the last step of a K that is no multiple of 64: slice 1 does not exist
#pragma unroll
    for (int i = 0; i < TI; ++i) {  // 8 X rows per wave instruction: lane -> (row r0 + lane / 8, physical chunk lane % 8)
      const int r0 = (wave * TI + i) * 8, r = r0 + (lane >> 3);
      int lc = (lane & 7) ^ (r & 7);
      if (half) lc &= 3;  // a chunk past the row re-reads one of slice 0
      m4_dma16(a.x + (size_t)min(m0 + r, a.M - 1) * a.K + kt * M4_BK + lc * 8, A + r0 * 128);
    }
    {  // 32 code rows per wave instruction: lane -> (row r0 + lane / 2, physical chunk lane % 2)
      const int r0 = wave * 32, r = r0 + (lane >> 1);
      const int lc = half ? 0 : (lane & 1) ^ ((r >> 3) & 1);
      m4_dma16(a.w + (size_t)min(n0 + r, a.N - 1) * kb + (size_t)(2 * kt + lc) * 16, B + r0 * 32);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int s = 0; s < 2; ++s) snext[j][s] = a.sc[srow[j] + min(2 * kt + s, ng - 1)];
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
    float s[4][2];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int q = 0; q < 2; ++q) s[j][q] = __uint_as_float(snext[j][q] ? snext[j][q] << 23 : 0x00400000u);
    if (kt + 1 < nk) gload(kt + 1);
    const unsigned char* A = lds + (kt & 1) * STAGE;
    const unsigned char* B = A + A_BYTES;
    const int nsub = 2 * kt + 1 < ng ? 2 : 1;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {  // two 32-deep MFMA k-slices (MX blocks) per step
      if (sub < nsub) {
        bf16x8_t af[TI], bfr[4];
#pragma unroll
        for (int i = 0; i < TI; ++i) af[i] = *(const bf16x8_t*)(A + m4_swz_x(wm * (16 * TI) + i * 16 + fr, sub * 4 + fk));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t c = *(const uint32_t*)(B + m4_swz_w(wn * 64 + j * 16 + fr, sub, fk));
          const float sj = s[j][sub];
          const uint4 e = make_uint4(
              m4_pair(__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sj, 0))),
              m4_pair(__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sj, 1))),
              m4_pair(__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sj, 2))),
              m4_pair(__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sj, 3))));
          bfr[j] = __builtin_bit_cast(bf16x8_t, e);
        }
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
      }
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

int preload_mxfp4_gemv();
int preload_mxfp4_a8();
int preload_mxfp4() {
  return preload(gemm_mxfp4_kernel<2>) + preload(gemm_mxfp4_kernel<4>) + preload_mxfp4_gemv() + preload_mxfp4_a8();
}

}  // namespace lga

extern "C" int lga_mxfp4_gemm(const void* x, const uint8_t* codes, const uint8_t* scales, const void* bias,
                              const void* residual, void* y, int M, int N, int K, hipStream_t stream) {
  LGA_CHECK_ARG(x && codes && scales && y, "lga_mxfp4_gemm: null pointer");
  LGA_CHECK_ARG(M >= 2 && N > 0, "lga_mxfp4_gemm: needs M >= 2 rows (one row is lga_mxfp4_gemv) and N > 0");
  LGA_CHECK_ARG(K > 0 && K % 32 == 0, "lga_mxfp4_gemm: K must be a positive multiple of 32");
  LGA_CHECK_ARG(((uintptr_t)x | (uintptr_t)codes) % 16 == 0, "lga_mxfp4_gemm: x and codes must be 16-B aligned");
  lga::GemmMx4Args a{(const uint16_t*)x, codes, scales, (const uint16_t*)bias, (const uint16_t*)residual,
                     (uint16_t*)y, M, N, K};
  const int nx = (N + lga::M4_BN - 1) / lga::M4_BN;
  if (M <= 64) lga::gemm_mxfp4_kernel<2><<<dim3(nx, (M + 63) / 64), 256, 0, stream>>>(a);
  else lga::gemm_mxfp4_kernel<4><<<dim3(nx, (M + 127) / 128), 256, 0, stream>>>(a);
  LGA_LAUNCH_RETURN();
}
