// LLM.int8 (--quantize bnb.int8) outside the decode GEMV: the weight quantizer, the prefill activation quantizer and
// the prefill GEMM on the i8 MFMA (include/litgpt_amd.h has the arithmetic).
//
// lga_int8_quantize_act runs three small launches and never talks to the host: (1) a column scan marks the outlier
// columns (col_flags, zeroed by a memset node first; every writer stores the same 1), (2) one workgroup compacts the
// flags into the ascending column list + count, (3) one workgroup per row takes s_x over the unflagged columns and
// writes the int8 row (0 in flagged columns).
//
// lga_int8_gemm: v_mfma_i32_32x32x32_i8, each wave a (32 TM) x (32 TN) tile of Y, 2 x 2 waves per workgroup. Operand
// fragments are 16 consecutive int8 of one row read straight from global memory (lane l: row l & 31, bytes
// [k0 + 16 (l >> 5), + 16)): A and B take the SAME k for the same (lane half, byte), which is all the integer sum
// needs, whatever order the instruction walks k in; the C/D map is the 32 x 32 map of every dtype (column on the
// lane, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)). The epilogue dequantizes, adds the outlier columns' term
// from the device-side list (x in bf16 against the int8 weight bytes), bias and residual. It is a plain
// register-tile kernel (no LDS staging, no split-K): prefill times are recorded in DESIGN.md, not tuned.
#include "int8_ops.h"

namespace lga {

typedef int i32x4_t __attribute__((ext_vector_type(4)));
typedef int i32x16_t __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float block_max_256(float v, float* red) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

template <bool BF16>
__global__ void __launch_bounds__(256) int8_quantize_kernel(const void* w, int8_t* q, float* s, int K) {
  __shared__ float red[4];
  const size_t base = (size_t)blockIdx.x * K;
  auto at = [&](int k) { return BF16 ? bf2f(((const uint16_t*)w)[base + k]) : ((const float*)w)[base + k]; };
  float amax = 0.0f;
  for (int k = threadIdx.x; k < K; k += 256) amax = fmaxf(amax, fabsf(at(k)));
  amax = block_max_256(amax, red);
  const float inv = q8_inv(amax);
  for (int k = threadIdx.x; k < K; k += 256) q[base + k] = (int8_t)q8(at(k), inv);
  if (threadIdx.x == 0) s[blockIdx.x] = amax;
}

constexpr int kFlagRows = 32;  // rows per workgroup of the column scan

__global__ void __launch_bounds__(256) int8_colflag_kernel(const uint16_t* x, int* flags, int M, int K, float thr) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= K) return;
  const int m1 = min(M, (int)(blockIdx.y + 1) * kFlagRows);
  bool any = false;
  for (int m = blockIdx.y * kFlagRows; m < m1; ++m) any |= fabsf(bf2f(x[(size_t)m * K + j])) >= thr;
  if (any) flags[j] = 1;
}

__global__ void __launch_bounds__(256) int8_collist_kernel(const int* flags, int* cols, int* count, int K) {
  __shared__ int cnt[256];
  const int per = (K + 255) / 256, t = threadIdx.x;
  const int j0 = min(t * per, K), j1 = min(j0 + per, K);
  int c = 0;
  for (int j = j0; j < j1; ++j) c += flags[j] != 0;
  cnt[t] = c;
  __syncthreads();
  int off = 0;
  for (int i = 0; i < t; ++i) off += cnt[i];
  for (int j = j0; j < j1; ++j)
    if (flags[j] != 0) cols[off++] = j;
  if (t == 255) *count = off;
}

__global__ void __launch_bounds__(256) int8_rowquant_kernel(const uint16_t* x, const int* flags, int8_t* xq,
                                                            float* sx, int K) {
  __shared__ float red[4];
  const size_t base = (size_t)blockIdx.x * K;
  float amax = 0.0f;
  for (int k = threadIdx.x; k < K; k += 256)
    if (!flags[k]) amax = fmaxf(amax, fabsf(bf2f(x[base + k])));
  amax = block_max_256(amax, red);
  const float inv = q8_inv(amax);
  for (int k = threadIdx.x; k < K; k += 256) xq[base + k] = flags[k] ? (int8_t)0 : (int8_t)q8(bf2f(x[base + k]), inv);
  if (threadIdx.x == 0) sx[blockIdx.x] = amax;
}

struct GemmI8Args {
  const uint16_t* x;   // [M][K] bf16 (outlier columns only)
  const int8_t* xq;    // [M][K]
  const float* sx;     // [M]
  const int* cols;     // outlier columns
  const int* count;    // [1]
  const int8_t* w;     // [N][K]
  const float* sw;     // [N]
  const uint16_t* bias;
  const uint16_t* residual;  // [M][N]
  uint16_t* y;               // [M][N]
  int M, N, K;
};

template <int TM, int TN>
__global__ void __launch_bounds__(256) int8_gemm_kernel(GemmI8Args a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int m_base = blockIdx.y * (64 * TM) + (wave >> 1) * (32 * TM);
  const int n_base = blockIdx.x * (64 * TN) + (wave & 1) * (32 * TN);
  const int K = a.K;
  // rows past M / N re-read the last row; their results are never stored
  const int8_t* ap[TM];
  const int8_t* bp[TN];
#pragma unroll
  for (int i = 0; i < TM; ++i) ap[i] = a.xq + (size_t)min(m_base + 32 * i + r, a.M - 1) * K;
#pragma unroll
  for (int j = 0; j < TN; ++j) bp[j] = a.w + (size_t)min(n_base + 32 * j + r, a.N - 1) * K;
  i32x16_t acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0;
  const i32x4_t zero = {0, 0, 0, 0};
  for (int k0 = 0; k0 < K; k0 += 32) {
    const int kk = k0 + 16 * h;
    const bool ok = kk < K;  // K % 32 == 16: the upper half of the last step is past the row
    const int kc = ok ? kk : 0;
    i32x4_t af[TM], bf[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) af[i] = *(const i32x4_t*)(ap[i] + kc);
#pragma unroll
    for (int j = 0; j < TN; ++j) bf[j] = *(const i32x4_t*)(bp[j] + kc);
#pragma unroll
    for (int i = 0; i < TM; ++i) af[i] = ok ? af[i] : zero;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[i], bf[j], acc[i][j], 0, 0, 0);
  }
  // outlier columns: x (bf16) against the weight byte, fp32, ascending column order
  float outv[TM][TN][16];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) outv[i][j][e] = 0.0f;
  float swn[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) swn[j] = a.sw[min(n_base + 32 * j + r, a.N - 1)];
  const int cnt = *a.count;
  for (int c = 0; c < cnt; ++c) {
    const int col = a.cols[c];
    float wq[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) wq[j] = mul_rn((float)bp[j][col], mul_rn(swn[j], 1.0f / 127.0f));
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int m = min(m_base + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h, a.M - 1);
        const float xv = bf2f(a.x[(size_t)m * K + col]);
#pragma unroll
        for (int j = 0; j < TN; ++j) outv[i][j][e] = fmaf(xv, wq[j], outv[i][j][e]);
      }
  }
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int m = m_base + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h;
      if (m >= a.M) continue;
      const float sxm = a.sx[m];
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int n = n_base + 32 * j + r;
        if (n >= a.N) continue;
        float o = add_rn(int8_main(acc[i][j][e], sxm, swn[j]), outv[i][j][e]);
        if (a.bias) o = add_rn(o, bf2f(a.bias[n]));
        const size_t at = (size_t)m * a.N + n;
        if (a.residual) o = round_bf(o) + bf2f(a.residual[at]);
        a.y[at] = f2bf(o);
      }
    }
}

}  // namespace lga

extern "C" int lga_int8_quantize(const void* weight, int weight_is_bf16, void* qweight, float* scales, int N, int K,
                                 hipStream_t stream) {
  LGA_CHECK_ARG(weight && qweight && scales, "lga_int8_quantize: null pointer");
  LGA_CHECK_ARG(N > 0 && K > 0 && K % 16 == 0, "lga_int8_quantize: K must be a positive multiple of 16");
  if (weight_is_bf16) lga::int8_quantize_kernel<true><<<N, 256, 0, stream>>>(weight, (int8_t*)qweight, scales, K);
  else lga::int8_quantize_kernel<false><<<N, 256, 0, stream>>>(weight, (int8_t*)qweight, scales, K);
  LGA_LAUNCH_RETURN();
}

extern "C" int lga_int8_quantize_act(const void* x, void* xq, float* sx, int* col_flags, int* cols, int* count, int M,
                                     int K, float threshold, hipStream_t stream) {
  LGA_CHECK_ARG(x && xq && sx && col_flags && cols && count, "lga_int8_quantize_act: null pointer");
  LGA_CHECK_ARG(M > 0 && K > 0 && K % 16 == 0, "lga_int8_quantize_act: K must be a positive multiple of 16");
  hipError_t e = hipMemsetAsync(col_flags, 0, (size_t)K * sizeof(int), stream);
  if (e != hipSuccess) {
    lga_set_error(hipGetErrorString(e));
    return (int)e;
  }
  if (threshold > 0.0f) {
    const dim3 grid((K + 255) / 256, (M + lga::kFlagRows - 1) / lga::kFlagRows);
    lga::int8_colflag_kernel<<<grid, 256, 0, stream>>>((const uint16_t*)x, col_flags, M, K, threshold);
  }
  lga::int8_collist_kernel<<<1, 256, 0, stream>>>(col_flags, cols, count, K);
  lga::int8_rowquant_kernel<<<M, 256, 0, stream>>>((const uint16_t*)x, col_flags, (int8_t*)xq, sx, K);
  LGA_LAUNCH_RETURN();
}

extern "C" int lga_int8_gemm(const void* x, const void* xq, const float* sx, const int* cols, const int* count,
                             const void* qweight, const float* scales, const void* bias, const void* residual, void* y,
                             int M, int N, int K, hipStream_t stream) {
  LGA_CHECK_ARG(x && xq && sx && cols && count && qweight && scales && y, "lga_int8_gemm: null pointer");
  LGA_CHECK_ARG(M >= 2 && N > 0, "lga_int8_gemm: needs M >= 2 rows (one row is lga_int8_gemv) and N > 0");
  LGA_CHECK_ARG(K > 0 && K % 16 == 0, "lga_int8_gemm: K must be a positive multiple of 16");
  LGA_CHECK_ARG(((uintptr_t)xq | (uintptr_t)qweight) % 16 == 0, "lga_int8_gemm: xq and qweight must be 16-B aligned");
  lga::GemmI8Args a{(const uint16_t*)x, (const int8_t*)xq, sx, cols, count, (const int8_t*)qweight, scales,
                    (const uint16_t*)bias, (const uint16_t*)residual, (uint16_t*)y, M, N, K};
  if (M <= 64) {
    const dim3 grid((N + 63) / 64, (M + 63) / 64);
    lga::int8_gemm_kernel<1, 1><<<grid, 256, 0, stream>>>(a);
  } else {
    const dim3 grid((N + 127) / 128, (M + 127) / 128);
    lga::int8_gemm_kernel<2, 2><<<grid, 256, 0, stream>>>(a);
  }
  LGA_LAUNCH_RETURN();
}
