// Prefill GEMM of --quantize mxfp4-a8 on the block-scaled matrix instruction, and the activation quantizer in front of
// it: Y[M, N] = mx8(X)[M, K] . W'[N, K]^T (+bias) (+residual), W' the mxfp4 weight (gemv_mxfp4.hip) and mx8 the MXFP8
// rounding below. v_mfma_scale_f32_16x16x128_f8f6f4 (cbsz 0: A is e4m3, blgp 4: B is e2m1) reads the e2m1 codes and both
// operands' e8m0 scale bytes as they lie in HBM: no convert pass, no bf16 image of either operand anywhere.
//
// mx8 (lga_mx8_quantize): the fp8 KV cache's rule (kv8_ops.h) on blocks of 32 consecutive columns of a row. s = 2^e the
// smallest power of two with amax / s <= 448, e clamped to [-126, 127], amax = 0 -> s = 1; codes e4m3fn(x / s), round to
// nearest even, nothing saturates; the scale is stored as the e8m0 byte e + 127 (1..254). Four lanes per block, 8
// values per lane, the maximum over a DPP quad; 64 blocks per 256-thread workgroup.
//
// The GEMM, MI355X design: (32 TI) x 128 output tile per 256-thread workgroup, 2 x 2 waves, each wave TI x 4 MFMAs of
// 16 x 16 x 128 per K-step (TI = 4: 128 rows; TI = 2: 64 rows for prompts of at most 64 tokens). A K-step is ONE MFMA
// depth, 128 = four MX blocks. The instruction's lane (r, g) = (lane % 16, lane / 16) supplies, of row r: the e2m1
// operand's block g (k = 32 g .. 32 g + 31: 16 B bytes, 4 registers); of the e4m3 operand k = 16 g .. 16 g + 15 in
// registers 0..3 and k = 64 + 16 g .. 64 + 16 g + 15 in registers 4..7 (measured on the part: the 8-bit operand is laid
// out as two K = 64 halves, so a lane's 32 A bytes are halves of blocks g / 2 and 2 + g / 2); and ONE scale byte per
// operand, that of block g, whatever codes the lane itself holds. Both code tiles go
// global -> LDS directly (global_load_lds_dwordx4), double-buffered, the next step's DMA issued before this step's MFMAs:
//  * X codes: 128-B rows of eight 16-B chunks, chunk index XOR ((row >> 1) & 7): a 16 KB tile at TI = 4. An A fragment
//    is two ds_read_b128 (chunks g and 4 + g); the 16 rows of a lane group fall on 16 distinct 16-B bank groups (row
//    parity picks the half of the 256-B window, the XOR the group within it).
//  * W codes: 64-B rows of four 16-B chunks (one chunk = one MX block), chunk index XOR ((row >> 2) & 3): an 8 KB tile,
//    two DMA instructions per wave and step. A B fragment is one ds_read_b128; 16 rows -> 16 distinct bank groups
//    (row & 3 picks the quarter of the window, the XOR the group within it).
//    24 KB per stage at TI = 4, against 36 KB per 128 of K in gemm_mxfp4.hip.
//  * Scale bytes never enter LDS: lane (r, g) loads the byte of (its row of each of its TI + 4 fragments, block g) from
//    HBM one step ahead into the low byte of a register of its own, and the MFMA takes it with opsel 0.
// K tails: K is a multiple of 32 only, so the last step may hold 1 to 3 blocks. A missing block's chunks and scale bytes
// are fetched from the row's last block (a clamped address, finite scales), and the lanes g that own a missing block
// clear their B fragment: any e4m3 code of X (the quantizer writes no NaN) times zero times two finite scales is
// exactly zero.
// M and N tails: rows past M or N re-read the last row and are never stored.
// Epilogue with lga_bf16_gemm's rounding points: fp32 accumulator + bias, one bf16 rounding, then + residual.
// Not here: a split over K for short prompts, a fused fc_1 || fc_2 + SwiGLU form.
#include "kv8_ops.h"

namespace lga {

typedef int i32x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------- quantizer
__global__ void __launch_bounds__(256) mx8_quantize_kernel(const uint16_t* x, uint2* codes, uint8_t* scales,
                                                           size_t blocks) {
  const size_t b = (size_t)blockIdx.x * 64 + (threadIdx.x >> 2);
  const int sub = threadIdx.x & 3;
  const size_t bl = b < blocks ? b : blocks - 1;  // whole quads stay active for the DPP maximum
  const uint4 v = *(const uint4*)(x + bl * 32 + (size_t)sub * 8);
  const uint32_t d[4] = {v.x, v.y, v.z, v.w};
  uint32_t mx = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) mx = max(mx, max(d[i] & 0x7FFFu, (d[i] >> 16) & 0x7FFFu));
  mx = max(mx, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)mx, 0xB1, 0xF, 0xF, false));  // quad [1,0,3,2]
  mx = max(mx, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)mx, 0x4E, 0xF, 0xF, false));  // quad [2,3,0,1]
  float inv;
  const float s = kv8_scale(mx, inv);
  int w[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    w[i] = __builtin_amdgcn_cvt_pk_fp8_f32(bflo(d[2 * i]) * inv, bfhi(d[2 * i]) * inv, 0, false);
    w[i] = __builtin_amdgcn_cvt_pk_fp8_f32(bflo(d[2 * i + 1]) * inv, bfhi(d[2 * i + 1]) * inv, w[i], true);
  }
  if (b < blocks) {
    codes[b * 4 + sub] = make_uint2((uint32_t)w[0], (uint32_t)w[1]);
    if (sub == 0) scales[b] = (uint8_t)(__float_as_uint(s) >> 23);  // e + 127
  }
}

// ---------------------------------------------------------------------------------------------------- GEMM
constexpr int A8_BN = 128, A8_BK = 128;
constexpr int A8_B_BYTES = A8_BN * A8_BK / 2;  // the W code tile: 8 KB

struct GemmMx4A8Args {
  const uint8_t* xc;   // [M][K] e4m3 codes
  const uint8_t* xs;   // [M][K / 32] e8m0
  const uint8_t* w;    // [N][K / 2] e2m1 code pairs
  const uint8_t* ws;   // [N][K / 32] e8m0
  const uint16_t* bias;
  const uint16_t* residual;  // [M][N]
  uint16_t* y;               // [M][N]
  int M, N, K;
};

// byte offset of 16-B chunk c (0..7) of X-code row `row`, and of chunk (= MX block) c (0..3) of W-code row `row`
__device__ __forceinline__ int a8_swz_x(int row, int c) { return row * 128 + 16 * (c ^ ((row >> 1) & 7)); }
__device__ __forceinline__ int a8_swz_w(int row, int c) { return row * 64 + 16 * (c ^ ((row >> 2) & 3)); }

__device__ __forceinline__ void a8_dma16(const void* g, unsigned char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds(g, (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

template <int TI>
__global__ void __launch_bounds__(256) gemm_mxfp4_a8_kernel(GemmMx4A8Args a) {
  constexpr int BM = 32 * TI, A_BYTES = BM * A8_BK, STAGE = A_BYTES + A8_B_BYTES;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * STAGE];  // [buf][X codes | W codes]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * A8_BN;
  const int ng = a.K / 32, nk = (ng + 3) / 4, kb = a.K / 2;
  const int fr = lane & 15, fk = lane >> 4;

  // this lane's TI A rows and four B rows (rows past M / N re-read the last row; never stored): their scale rows
  size_t arow[TI], brow[4];
#pragma unroll
  for (int i = 0; i < TI; ++i) arow[i] = (size_t)min(m0 + wm * (16 * TI) + i * 16 + fr, a.M - 1) * ng;
#pragma unroll
  for (int j = 0; j < 4; ++j) brow[j] = (size_t)min(n0 + wn * 64 + j * 16 + fr, a.N - 1) * ng;
  int sa_next[TI], sb_next[4];

  auto gload = [&](int kt) {
    unsigned char* A = lds + (kt & 1) * STAGE;
    unsigned char* B = A + A_BYTES;
#pragma unroll
    for (int i = 0; i < TI; ++i) {  // 8 X rows per wave instruction: lane -> (row r0 + lane / 8, physical chunk lane % 8)
      const int r0 = (wave * TI + i) * 8, r = r0 + (lane >> 3);
      const int lc = (lane & 7) ^ ((r >> 1) & 7);
      const int kc = min(kt * 8 + lc, 2 * ng - 1);  // a chunk past the row re-reads the row's last one
      a8_dma16(a.xc + (size_t)min(m0 + r, a.M - 1) * a.K + (size_t)kc * 16, A + r0 * 128);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {  // 16 W rows per wave instruction: lane -> (row r0 + lane / 4, physical chunk lane % 4)
      const int r0 = (wave * 2 + i) * 16, r = r0 + (lane >> 2);
      const int lc = (lane & 3) ^ ((r >> 2) & 3);
      const int blk = min(kt * 4 + lc, ng - 1);
      a8_dma16(a.w + (size_t)min(n0 + r, a.N - 1) * kb + (size_t)blk * 16, B + r0 * 64);
    }
    const int g = min(kt * 4 + fk, ng - 1);
#pragma unroll
    for (int i = 0; i < TI; ++i) sa_next[i] = a.xs[arow[i] + g];
#pragma unroll
    for (int j = 0; j < 4; ++j) sb_next[j] = a.ws[brow[j] + g];
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
    for (int j = 0; j < 4; ++j) sb[j] = sb_next[j];
    if (kt + 1 < nk) gload(kt + 1);
    const unsigned char* A = lds + (kt & 1) * STAGE;
    const unsigned char* B = A + A_BYTES;
    const bool live = 4 * kt + fk < ng;  // false: this lane's block lies past K (the last step of a K % 128 != 0)
    i32x8_t af[TI], bfr[4];
#pragma unroll
    for (int i = 0; i < TI; ++i) {
      const int row = wm * (16 * TI) + i * 16 + fr;
      const uint4 lo = *(const uint4*)(A + a8_swz_x(row, fk)), hi = *(const uint4*)(A + a8_swz_x(row, 4 + fk));
      af[i] = i32x8_t{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint4 c = *(const uint4*)(B + a8_swz_w(wn * 64 + j * 16 + fr, fk));
      if (!live) c = make_uint4(0, 0, 0, 0);
      bfr[j] = i32x8_t{(int)c.x, (int)c.y, (int)c.z, (int)c.w, 0, 0, 0, 0};
    }
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af[i], bfr[j], acc[i][j], 0, 4, 0, sa[i], 0, sb[j]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's LDS-direct loads (and scale bytes) have landed
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

int preload_mxfp4_a8() {
  return preload(mx8_quantize_kernel) + preload(gemm_mxfp4_a8_kernel<2>) + preload(gemm_mxfp4_a8_kernel<4>);
}

}  // namespace lga

extern "C" int lga_mx8_quantize(const void* x, uint8_t* codes, uint8_t* scales, int M, int K, hipStream_t stream) {
  LGA_CHECK_ARG(x && codes && scales, "lga_mx8_quantize: null pointer");
  LGA_CHECK_ARG(M >= 1, "lga_mx8_quantize: needs M >= 1 rows");
  LGA_CHECK_ARG(K > 0 && K % 32 == 0, "lga_mx8_quantize: K must be a positive multiple of 32");
  LGA_CHECK_ARG(((uintptr_t)x | (uintptr_t)codes) % 16 == 0, "lga_mx8_quantize: x and codes must be 16-B aligned");
  const size_t blocks = (size_t)M * (K / 32);
  lga::mx8_quantize_kernel<<<(unsigned)((blocks + 63) / 64), 256, 0, stream>>>((const uint16_t*)x, (uint2*)codes,
                                                                              scales, blocks);
  LGA_LAUNCH_RETURN();
}

extern "C" int lga_mxfp4_a8_gemm(const uint8_t* xcodes, const uint8_t* xscales, const uint8_t* w,
                                 const uint8_t* wscales, const void* bias, const void* residual, void* y, int M, int N,
                                 int K, hipStream_t stream) {
  LGA_CHECK_ARG(xcodes && xscales && w && wscales && y, "lga_mxfp4_a8_gemm: null pointer");
  LGA_CHECK_ARG(M >= 1 && N > 0, "lga_mxfp4_a8_gemm: needs M >= 1 rows and N > 0");
  LGA_CHECK_ARG(K > 0 && K % 32 == 0, "lga_mxfp4_a8_gemm: K must be a positive multiple of 32");
  LGA_CHECK_ARG(((uintptr_t)xcodes | (uintptr_t)w) % 16 == 0, "lga_mxfp4_a8_gemm: xcodes and w must be 16-B aligned");
  lga::GemmMx4A8Args a{xcodes, xscales, w, wscales, (const uint16_t*)bias, (const uint16_t*)residual, (uint16_t*)y,
                       M, N, K};
  const int nx = (N + lga::A8_BN - 1) / lga::A8_BN;
  if (M <= 64) lga::gemm_mxfp4_a8_kernel<2><<<dim3(nx, (M + 63) / 64), 256, 0, stream>>>(a);
  else lga::gemm_mxfp4_a8_kernel<4><<<dim3(nx, (M + 127) / 128), 256, 0, stream>>>(a);
  LGA_LAUNCH_RETURN();
}
