// Prefill GEMM over MXFP6 weights, --quantize mxfp6: Y[M, N] = X[M, K] . W'[N, K]^T (+bias) (+residual) with
// W'[n, k] = e2m3(code[n, k]) * 2^(scale[n, k / 32] - 127) — exact in bf16, so this is lga_bf16_gemm's arithmetic on
// the dequantized weight without that weight ever existing in HBM (or in LDS).
//
// MI355X design: (32 TI) x 128 output tile per 256-thread workgroup, 2 x 2 waves, each wave TI x 4 tiles of
// v_mfma_f32_16x16x32_bf16 (TI = 4: 128 rows; TI = 2: 64 rows for prompts of at most 64 tokens). The K step is 128 =
// four MX blocks = four MFMA k-slices, and the slices are cut ACROSS the blocks: the lane in k-group g (lane / 16) of a
// B fragment owns block g of its weight row, expands its 32 codes with ONE v_cvt_scalef32_pk32_bf16_fp6 (the block's
// scale 2^(e - 127) as the fp32 operand) and feeds converted columns 8 i .. 8 i + 7 to slice i. Slice i therefore
// multiplies the columns {32 g + 8 i + j}: the A fragment of lane (row, g) is read from the same columns, the 16-B
// chunk 4 g + i of the row's 256 B. Every converted value is used and a lane holds one scale per (row, step).
// K is a multiple of 64 only, so the last step may hold two blocks: its missing half is fetched from a clamped address
// and the lanes of k-groups 2 and 3 multiply zero codes.
// Both operand tiles go global -> LDS directly (global_load_lds_dwordx4), double-buffered, the next step's DMA issued
// before this step's MFMAs:
//  * X: 256-B rows of sixteen 16-B chunks, chunk index XOR (row & 15): the 16 lanes of a ds_read_b128 group (16 rows,
//    one logical chunk) read 16 distinct chunks of the 256-B bank window;
//  * W: the CODES, 96-B rows (four blocks of 24 B) of six 16-B chunks — a 12 KB tile, three DMA instructions per wave
//    per step — the chunks of rows 8..15 of every 16 rotated by one ((chunk + 1) % 6). A block is read as three
//    ds_read_b64; rows are 24 dwords apart, so rows r and r + 8 start on the same bank, and the rotation moves the
//    second onto the banks the first leaves free: the 32 lanes of a ds_read_b64 half-wave (16 rows x 2 blocks) read 32
//    distinct 8-B bank pairs.
// The e8m0 byte of a lane's block of each of its four rows is fetched one step ahead by byte loads.
// Epilogue with lga_bf16_gemm's rounding points: fp32 accumulator + bias, one bf16 rounding, then + residual.
// LDS: 2 x (32 TI x 256 + 12288) B = 88 KB (TI = 4), 56 KB (TI = 2), passed as dynamic LDS.
#include "decode_ops.h"

namespace lga {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned u32x6_t __attribute__((ext_vector_type(6)));
struct Mx6Frags {  // a converted block as the B fragments of its four slices
  bf16x8_t q[4];
};

constexpr int M6_BN = 128, M6_BK = 128;
constexpr int M6_ROW = M6_BK * 3 / 4;     // code bytes of a row of the tile: 96
constexpr int M6_B_BYTES = M6_BN * M6_ROW;  // the code tile: 12 KB
constexpr int m6_lds_bytes(int ti) { return 2 * (32 * ti * 256 + M6_B_BYTES); }

struct GemmMx6Args {
  const uint16_t* x;   // [M][K] bf16
  const uint8_t* w;    // [N][3 K / 4] codes
  const uint8_t* sc;   // [N][K / 32] e8m0
  const uint16_t* bias;
  const uint16_t* residual;  // [M][N]
  uint16_t* y;               // [M][N]
  int M, N, K;
};

__device__ __forceinline__ int m6_swz_x(int row, int chunk) { return row * 256 + 16 * (chunk ^ (row & 15)); }

__device__ __forceinline__ void m6_dma16(const void* g, unsigned char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds(g, (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

template <int TI>
__global__ void __launch_bounds__(256) gemm_mxfp6_kernel(GemmMx6Args a) {
  constexpr int BM = 32 * TI, A_BYTES = BM * 256, STAGE = A_BYTES + M6_B_BYTES;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];  // [buf][X | codes]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * M6_BN;
  const int ng = a.K / 32, nk = (ng + 3) / 4;
  const size_t kb = (size_t)a.K / 4 * 3;  // code bytes of a weight row
  const int fr = lane & 15, fk = lane >> 4;

  // this lane's four B rows (rows past N re-read row N - 1; never stored) and their scale bytes, one step ahead
  size_t srow[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) srow[j] = (size_t)min(n0 + wn * 64 + j * 16 + fr, a.N - 1) * ng;
  uint32_t snext[4];

  // the code DMA: slot s = 192 wave + 64 i + lane of the tile's 768 chunks is physical chunk s % 6 of tile row s / 6
  const uint8_t* wsrc[3];
  int wlc[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int s = wave * 192 + i * 64 + lane, r = s / 6;
    wlc[i] = (s - r * 6 + 6 - ((r >> 3) & 1)) % 6;  // logical chunk: rows 8..15 of every 16 are rotated by one
    wsrc[i] = a.w + (size_t)min(n0 + r, a.N - 1) * kb;
  }
  // the three 8-B pieces of this lane's block fk: piece q = 3 fk + t of the row's twelve is half q & 1 of chunk q >> 1
  int boff[3];
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int q = 3 * fk + t;
    boff[t] = fr * M6_ROW + 16 * (((q >> 1) + ((fr >> 3) & 1)) % 6) + 8 * (q & 1);
  }

  auto gload = [&](int kt) {
    unsigned char* A = lds + (kt & 1) * STAGE;
    unsigned char* B = A + A_BYTES;
    const bool half = 4 * kt + 2 >= ng;  // the last step of a K that is no multiple of 128: blocks 2, 3 do not exist
#pragma unroll
    for (int i = 0; i < 2 * TI; ++i) {  // 4 X rows per wave instruction: lane -> (row r0 + lane / 16, physical chunk lane % 16)
      const int r0 = (wave * 2 * TI + i) * 4, r = r0 + (lane >> 4);
      int lc = (lane & 15) ^ (r & 15);
      if (half) lc &= 7;  // a chunk past the row re-reads one of the first half
      m6_dma16(a.x + (size_t)min(m0 + r, a.M - 1) * a.K + kt * M6_BK + lc * 8, A + r0 * 256);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int lc = half ? wlc[i] % 3 : wlc[i];
      m6_dma16(wsrc[i] + (size_t)kt * M6_ROW + lc * 16, B + (wave * 192 + i * 64) * 16);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) snext[j] = a.sc[srow[j] + min(4 * kt + fk, ng - 1)];
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
    for (int j = 0; j < 4; ++j) s[j] = __uint_as_float(snext[j] ? snext[j] << 23 : 0x00400000u);
    const bool live = 4 * kt + fk < ng;  // this lane's block exists
    if (kt + 1 < nk) gload(kt + 1);
    const unsigned char* A = lds + (kt & 1) * STAGE;
    const unsigned char* B = A + A_BYTES;
    Mx6Frags bw[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned char* row = B + (wn * 64 + j * 16) * M6_ROW;
      const uint2 c0 = *(const uint2*)(row + boff[0]), c1 = *(const uint2*)(row + boff[1]),
                  c2 = *(const uint2*)(row + boff[2]);
      const u32x6_t c = {live ? c0.x : 0u, live ? c0.y : 0u, live ? c1.x : 0u,
                         live ? c1.y : 0u, live ? c2.x : 0u, live ? c2.y : 0u};
      bw[j] = __builtin_bit_cast(Mx6Frags, __builtin_amdgcn_cvt_scalef32_pk32_bf16_fp6(c, s[j]));
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {  // slice q: converted columns 8 q .. 8 q + 7 of every lane's block
      bf16x8_t af[TI];
#pragma unroll
      for (int i = 0; i < TI; ++i) af[i] = *(const bf16x8_t*)(A + m6_swz_x(wm * (16 * TI) + i * 16 + fr, 4 * fk + q));
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int i = 0; i < TI; ++i)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bw[j].q[q], acc[i][j], 0, 0, 0);
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

// dynamic LDS above 64 KB is opted into once per kernel
template <int TI>
static bool m6_lds_ready() {
  static const bool ok = hipFuncSetAttribute((const void*)gemm_mxfp6_kernel<TI>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, m6_lds_bytes(TI)) == hipSuccess;
  return ok;
}

int preload_mxfp6_gemv();
int preload_mxfp6() {
  return preload(gemm_mxfp6_kernel<2>) + preload(gemm_mxfp6_kernel<4>) + !m6_lds_ready<2>() + !m6_lds_ready<4>() +
         preload_mxfp6_gemv();
}

}  // namespace lga

extern "C" int lga_mxfp6_gemm(const void* x, const uint8_t* codes, const uint8_t* scales, const void* bias,
                              const void* residual, void* y, int M, int N, int K, hipStream_t stream) {
  LGA_CHECK_ARG(x && codes && scales && y, "lga_mxfp6_gemm: null pointer");
  LGA_CHECK_ARG(M >= 2 && N > 0, "lga_mxfp6_gemm: needs M >= 2 rows (one row is lga_mxfp6_gemv) and N > 0");
  LGA_CHECK_ARG(K > 0 && K % 64 == 0, "lga_mxfp6_gemm: K must be a positive multiple of 64");
  LGA_CHECK_ARG(((uintptr_t)x | (uintptr_t)codes) % 16 == 0, "lga_mxfp6_gemm: x and codes must be 16-B aligned");
  lga::GemmMx6Args a{(const uint16_t*)x, codes, scales, (const uint16_t*)bias, (const uint16_t*)residual,
                     (uint16_t*)y, M, N, K};
  const int nx = (N + lga::M6_BN - 1) / lga::M6_BN;
  LGA_CHECK_ARG(M <= 64 ? lga::m6_lds_ready<2>() : lga::m6_lds_ready<4>(), "lga_mxfp6_gemm: the LDS tile was refused");
  if (M <= 64) lga::gemm_mxfp6_kernel<2><<<dim3(nx, (M + 63) / 64), 256, lga::m6_lds_bytes(2), stream>>>(a);
  else lga::gemm_mxfp6_kernel<4><<<dim3(nx, (M + 127) / 128), 256, lga::m6_lds_bytes(4), stream>>>(a);
  LGA_LAUNCH_RETURN();
}
