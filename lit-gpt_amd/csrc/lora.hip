// LoRA adapters applied at run time (the reference's unmerged LoRALinear / LoRAQKVLinear forward, lit_gpt/lora.py:
// 170-177 and :398-433) and merged into a bf16 weight (LoRALinear.merge, :140-149).
//
// An adapter cannot be folded into a 4-bit or int8 weight without quantizing again, so on a quantized base it runs in
// every decode step, next to the base Linear's GEMV. There it is launch-bound: a Llama-2-7B q+v adapter of rank 8 is
// 128 KB of A and 196 KB of B against 26 MB of int4 qkv weight, so the whole chain — RMSNorm, down-projection,
// up-projection, scale, add to the base output, residual — is ONE launch (lga_lora_gemv).
//
// Device layout (built once by lit_gpt/lora.py attach): A (R, K) bf16; B (N, r) bf16 in output-row order; row_off (N)
// int32, the first row of A's segment that output row n uses (a fused qkv Linear has one segment of r rows per
// enabled q / k / v slot; -1 = the row has no adapter), or NULL when every row uses segment 0. r % 8 == 0 (zero
// padded), so a row of B is r / 8 16-byte chunks.
//
// Rounding points, those of the reference under bf16-true (the LoRA section):
//   x' = x or bf16(RMSNorm(x));  t_j = bf16(sum_k x'_k A[j,k]);  u_n = bf16(sum_j B[n,j] t[off_n + j]);
//   l_n = bf16(u_n * scaling);  y_n = bf16(base_n + l_n);  y_n = bf16(y_n + residual_n).
// All sums in fp32. The sum over j runs in ascending j in one fmaf chain (lora_chunk_dot) in the decode and the
// prefill kernel alike.
//
// lga_lora_gemv: every workgroup computes ALL R values of t itself (A is small and its re-reads hit L2; a second
// launch or a grid-wide hand-off would cost more than the R x K dot products), in an order that does not depend on
// the workgroup, so y does not depend on the grid. Then each thread owns 8 consecutive output rows.
//
// lga_lora_gemv_rows (batched decode): up to 8 rows, each with the adapter its device-resident id names out of a
// stacked set, or none. One more grid dimension over the rows; every workgroup runs the one-row kernel's body on its
// row (lora_gemv_body), so a row has the one-row launch's bits and depends on no other row. Rows are not grouped by
// adapter and share no A reads: at M <= 4 with the adapters in L2 the launch is latency-bound either way.
#include <cstdlib>

#include "decode_ops.h"

namespace lga {

typedef __bf16 lora_bf16x8_t __attribute__((ext_vector_type(8)));
typedef float lora_f32x16_t __attribute__((ext_vector_type(16)));

constexpr int kLoraMaxR = 192;   // rows of A (all segments)
constexpr int kLoraMaxRank = 64; // r (padded)

// u += sum over the 8 values j of one chunk of B[n][j] * t[j]: ascending j, one fmaf chain — the one definition the
// decode and the prefill kernel share, so u has the same bits in both for the same t
__device__ __forceinline__ float lora_chunk_dot(const float (&b)[8], const float* __restrict__ t, float u) {
#pragma unroll
  for (int e = 0; e < 8; ++e) u = fmaf(b[e], t[e], u);
  return u;
}

// l = bf16(bf16(u) * scaling); y = bf16(base + l) (or l); y = bf16(y + residual). has_lora false: the row passes through.
__device__ __forceinline__ float lora_epilogue(float u, float scaling, bool has_lora, bool has_base, float base,
                                               bool has_res, float res) {
  const float l = round_bf(__fmul_rn(round_bf(u), scaling));
  float y = has_base ? (has_lora ? round_bf(__fadd_rn(base, l)) : base) : (has_lora ? l : 0.0f);
  if (has_res) y = round_bf(__fadd_rn(y, res));
  return y;
}

struct LoraUpArgs {
  const uint16_t* t;         // [M][R] bf16 (prefill) — unused by the decode kernel
  const uint16_t* B;         // [N][r]
  const int32_t* row_off;    // [N] or null
  const uint16_t* base;      // [M][N] or null (may alias y)
  const uint16_t* residual;  // [M][N] or null
  uint16_t* y;               // [M][N]
  int M, N, R, r;
  float scaling;
};

// The up-projection of MT rows m0.. of the output for the 8 columns n0..n0+7 of this thread; t_lds: [MT][R] floats
// holding bf16 values. vec: N % 8 == 0 and 16-byte aligned rows, else element-wise with bounds.
template <int MT>
__device__ __forceinline__ void lora_up_columns(const LoraUpArgs& a, const float* t_lds, int m0, int n0, bool vec) {
  const int r8 = a.r / 8;
  float u[MT][8];
  int off[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int n = min(n0 + i, a.N - 1);
    off[i] = a.row_off ? a.row_off[n] : 0;
    const uint4* brow = (const uint4*)(a.B + (size_t)n * a.r);
    const float* ts = t_lds + max(off[i], 0);
#pragma unroll
    for (int m = 0; m < MT; ++m) u[m][i] = 0.0f;
    for (int c = 0; c < r8; ++c) {  // each 16-byte chunk of the row of B once, for all MT rows of t
      float b[8];
      unpack8(brow[c], b);
#pragma unroll
      for (int m = 0; m < MT; ++m) u[m][i] = lora_chunk_dot(b, ts + m * a.R + 8 * c, u[m][i]);
    }
  }
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    if (m0 + m >= a.M) break;
    const size_t row = (size_t)(m0 + m) * a.N;
    float bv[8], rv[8], yv[8];
    if (vec) {
      if (a.base) unpack8(*(const uint4*)(a.base + row + n0), bv);
      if (a.residual) unpack8(*(const uint4*)(a.residual + row + n0), rv);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const size_t e = row + min(n0 + i, a.N - 1);
        bv[i] = a.base ? bf2f(a.base[e]) : 0.0f;
        rv[i] = a.residual ? bf2f(a.residual[e]) : 0.0f;
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
      yv[i] = lora_epilogue(u[m][i], a.scaling, off[i] >= 0, a.base != nullptr, bv[i], a.residual != nullptr, rv[i]);
    if (vec) {
      *(uint4*)(a.y + row + n0) =
          make_uint4(pack2(yv[0], yv[1]), pack2(yv[2], yv[3]), pack2(yv[4], yv[5]), pack2(yv[6], yv[7]));
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (n0 + i < a.N) a.y[row + n0 + i] = f2bf(yv[i]);
    }
  }
}

// ---- decode: the whole chain in one launch ---------------------------------------------------------------------
struct LoraGemvArgs {
  const uint16_t* x;       // [K]
  const uint16_t* norm_w;  // [K] or null
  const uint16_t* A;       // [R][K]
  LoraUpArgs up;           // M = 1
  int K;
  float eps;
  int groups_per_wg;       // 8-row groups a workgroup owns (<= 1024)
};

constexpr int kGemvThreads = 1024, kGemvWaves = kGemvThreads / 64;

// The body of both decode kernels: workgroup blockIdx.x of the one-row launch on the row that ``a`` describes. ``lora``
// false (lga_lora_gemv_rows only: a row whose adapter id selects none) makes every output row an off_n < 0 row — the
// norm and the t phase are skipped and nothing of x, A or B is read.
// RB rows of A per wave and pass: 16 waves x RB rows per pass, the 8 * RB loads of an unrolled step in flight together.
// The launch is latency-bound (A comes from L2), so what counts is how few dependent rounds of loads a wave makes.
template <int RB>
__device__ __forceinline__ void lora_gemv_body(const LoraGemvArgs& a, const bool lora) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4* xl = (uint4*)smem;  // K/8 uint4: x' in bf16
  __shared__ float t_lds[kLoraMaxR];
  __shared__ float red[kGemvWaves];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n8 = a.K / 8, R = a.up.R;
  const LoraUpArgs& up = a.up;

  // 0. the epilogue's operands of this thread's 8 output rows, requested now and used last
  const int n0 = (blockIdx.x * a.groups_per_wg + tid) * 8;
  const bool owner = tid < a.groups_per_wg && n0 < up.N;
  const bool vec = owner && n0 + 8 <= up.N &&
                   (((uintptr_t)up.y | (uintptr_t)(up.base ? up.base : up.y) |
                     (uintptr_t)(up.residual ? up.residual : up.y)) & 15) == 0;
  uint4 base8 = make_uint4(0, 0, 0, 0), res8 = base8;
  int off[8];
  if (owner) {
#pragma unroll
    for (int i = 0; i < 8; ++i) off[i] = !lora ? -1 : up.row_off ? up.row_off[min(n0 + i, up.N - 1)] : 0;
    if (vec && up.base) base8 = *(const uint4*)(up.base + n0);
    if (vec && up.residual) res8 = *(const uint4*)(up.residual + n0);
  }

  // 1. x' into LDS (RMSNorm with lga_rmsnorm's rounding: fp32 sum of squares, bf16(w * (x * rs)))
  float rs = 1.0f;
  if (lora && a.norm_w) {
    float ss = 0.0f;
    for (int u = tid; u < n8; u += kGemvThreads) {
      const uint4 v = ((const uint4*)a.x)[u];
      const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        ss = fmaf(bflo(d[q]), bflo(d[q]), ss);
        ss = fmaf(bfhi(d[q]), bfhi(d[q]), ss);
      }
    }
    ss = wave_sum(ss);
    if (lane == 0) red[wave] = ss;
    __syncthreads();
    float tot = 0.0f;
#pragma unroll
    for (int w = 0; w < kGemvWaves; ++w) tot += red[w];
    rs = 1.0f / sqrtf(tot / (float)a.K + a.eps);
  }
  for (int u = tid; lora && u < n8; u += kGemvThreads) {
    const uint4 v = ((const uint4*)a.x)[u];
    uint32_t d[4] = {v.x, v.y, v.z, v.w};
    if (a.norm_w) {
      const uint4 w = ((const uint4*)a.norm_w)[u];
      const uint32_t nw[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int q = 0; q < 4; ++q)
        d[q] = pack2(__fmul_rn(bflo(nw[q]), __fmul_rn(bflo(d[q]), rs)),
                     __fmul_rn(bfhi(nw[q]), __fmul_rn(bfhi(d[q]), rs)));
    }
    xl[u] = make_uint4(d[0], d[1], d[2], d[3]);
  }
  __syncthreads();

  // 2. t: in pass p wave w takes rows (16 p + w) RB .. + RB - 1 of A; lane l the 16-byte chunks l, l + 64, ... of each
  //    row, summed in that order, then one butterfly per row. The same in every workgroup and for every RB.
  for (int j0 = wave * RB; lora && j0 < R; j0 += kGemvWaves * RB) {
    const uint4* ar[RB];
    float s[RB];
#pragma unroll
    for (int i = 0; i < RB; ++i) {
      ar[i] = (const uint4*)(a.A + (size_t)min(j0 + i, R - 1) * a.K);
      s[i] = 0.0f;
    }
#pragma unroll(RB == 1 ? 8 : 4)
    for (int c = lane; c < n8; c += 64) {
      const uint4 xv = xl[c];
#pragma unroll
      for (int i = 0; i < RB; ++i) {
        const uint4 w = ar[i][c];
        float d = dot2_bf16(w.x, xv.x, 0.0f);
        d = dot2_bf16(w.y, xv.y, d);
        d = dot2_bf16(w.z, xv.z, d);
        d = dot2_bf16(w.w, xv.w, d);
        s[i] += d;
      }
    }
#pragma unroll
    for (int i = 0; i < RB; ++i) {
      const float tot = wave_sum(s[i]);
      if (lane == 0 && j0 + i < R) t_lds[j0 + i] = round_bf(tot);
    }
  }
  __syncthreads();

  // 3. up-projection, scale, base, residual: 8 output rows per thread (the arithmetic of lora_up_columns)
  if (!owner) return;
  const int r8 = up.r / 8;
  float bv[8], rv[8], yv[8];
  if (vec) {
    unpack8(base8, bv);
    unpack8(res8, rv);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int n = min(n0 + i, up.N - 1);
    const uint4* brow = (const uint4*)(up.B + (size_t)n * up.r);
    const float* ts = t_lds + max(off[i], 0);
    float u = 0.0f;
    for (int c = 0; lora && c < r8; ++c) {
      float b[8];
      unpack8(brow[c], b);
      u = lora_chunk_dot(b, ts + 8 * c, u);
    }
    if (!vec) {
      bv[i] = up.base ? bf2f(up.base[n]) : 0.0f;
      rv[i] = up.residual ? bf2f(up.residual[n]) : 0.0f;
    }
    yv[i] = lora_epilogue(u, up.scaling, off[i] >= 0, up.base != nullptr, bv[i], up.residual != nullptr, rv[i]);
  }
  if (vec) {
    *(uint4*)(up.y + n0) = make_uint4(pack2(yv[0], yv[1]), pack2(yv[2], yv[3]), pack2(yv[4], yv[5]), pack2(yv[6], yv[7]));
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (n0 + i < up.N) up.y[n0 + i] = f2bf(yv[i]);
  }
}

template <int RB>
__global__ void __launch_bounds__(kGemvThreads) lora_gemv_kernel(LoraGemvArgs a) {
  lora_gemv_body<RB>(a, true);
}

// ---- batched decode: row m of up to 8 with the adapter adapter[m] of a stacked set, or none -------------------------
// Grid (the one-row launch's grid, M): workgroup (g, m) is lora_gemv_kernel's workgroup g on row m with adapter
// adapter[m]'s A and B, through the same body, so row m has that launch's bits. The ids are read from device memory: a
// captured launch follows them. An id outside [0, n_adapters) selects no adapter and touches neither A nor B.
struct LoraRowsArgs {
  const int32_t* adapter;  // [M]
  int n_adapters;
  long long a_stride, b_stride;  // elements between the adapters' A (R, K) / B (N, r) blocks
};

template <int RB>
__global__ void __launch_bounds__(kGemvThreads) lora_gemv_rows_kernel(LoraGemvArgs a, LoraRowsArgs rw) {
  const int m = blockIdx.y;
  const int id = rw.adapter[m];
  const bool lora = id >= 0 && id < rw.n_adapters;
  const size_t row = (size_t)m * a.up.N;
  a.x += (size_t)m * a.K;
  a.A += lora ? (size_t)id * rw.a_stride : 0;
  a.up.B += lora ? (size_t)id * rw.b_stride : 0;
  a.up.base += row;
  if (a.up.residual) a.up.residual += row;
  a.up.y += row;
  lora_gemv_body<RB>(a, lora);
}

// ---- prefill: t = bf16(X A^T) on the MFMA, then the up-projection over the base output ---------------------------
// One workgroup per 32 rows of X; its 4 waves split K in 64-element slabs (wave w: slabs w, w + 4, ...), each slab
// four v_mfma_f32_32x32x16_bf16 per 32-row tile of A. A's rows are the MFMA rows and X's rows its columns, so a
// lane ends with 4 consecutive t values of one row of X per register quad: 8-byte stores. The k order inside an MFMA
// is free as long as both operands agree: lane half h takes chunk 2 i + h of the slab, so the four loads of a row
// cover 128 contiguous bytes. The waves' partial tiles are summed through LDS in wave order.
__device__ __forceinline__ uint4 keep_if(bool ok, uint4 v) {
  return make_uint4(ok ? v.x : 0u, ok ? v.y : 0u, ok ? v.z : 0u, ok ? v.w : 0u);
}

template <int NT>
__global__ void __launch_bounds__(256) lora_down_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ A,
                                                        uint16_t* __restrict__ t, int M, int K, int R) {
  __shared__ float red[3][16][64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, q = lane & 31;
  const int n8 = K / 8, slabs = (n8 + 7) / 8;
  const int m = blockIdx.x * 32 + q;
  const uint4* xrow = (const uint4*)(x + (size_t)min(m, M - 1) * K);
  const uint4* arow[NT];
  bool aok[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    aok[j] = j * 32 + q < R;
    arow[j] = (const uint4*)(A + (size_t)min(j * 32 + q, R - 1) * K);
  }
  lora_f32x16_t acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[j][v] = 0.0f;
  for (int s = wave; s < slabs; s += 4) {
    uint4 xf[4], af[NT][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = s * 8 + 2 * i + h;
      const bool ok = c < n8;
      // (a chunk past K or a row past R: loaded from a clamped address, then zeroed word by word — a select between
      // the load and a constant uint4 becomes a load through a selected pointer with the constant in scratch)
      xf[i] = keep_if(ok, xrow[min(c, n8 - 1)]);
#pragma unroll
      for (int j = 0; j < NT; ++j) af[j][i] = keep_if(ok && aok[j], arow[j][min(c, n8 - 1)]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(lora_bf16x8_t, af[j][i]),
                                                         __builtin_bit_cast(lora_bf16x8_t, xf[i]), acc[j], 0, 0, 0);
  }
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    if (wave > 0) {
#pragma unroll
      for (int v = 0; v < 16; ++v) red[wave - 1][v][lane] = acc[j][v];
    }
    __syncthreads();
    if (wave == 0 && m < M) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        auto sum = [&](int v) { return ((acc[j][v] + red[0][v][lane]) + red[1][v][lane]) + red[2][v][lane]; };
        const int row = j * 32 + 8 * g + 4 * h;  // rows row .. row + 3 of A = t columns
        if (row < R)
          *(uint2*)(t + (size_t)m * R + row) =
              make_uint2(pack2(sum(4 * g), sum(4 * g + 1)), pack2(sum(4 * g + 2), sum(4 * g + 3)));
      }
    }
    __syncthreads();
  }
}

constexpr int kUpRows = 8;  // rows of the output per workgroup of lora_up_kernel

__global__ void __launch_bounds__(256) lora_up_kernel(LoraUpArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* t_lds = (float*)smem;  // [kUpRows][R]
  const int m0 = blockIdx.y * kUpRows;
  for (int i = threadIdx.x; i < kUpRows * a.R; i += 256) {
    const int m = min(m0 + i / a.R, a.M - 1);
    t_lds[i] = bf2f(a.t[(size_t)m * a.R + i % a.R]);
  }
  __syncthreads();
  const int n0 = (blockIdx.x * 256 + threadIdx.x) * 8;
  if (n0 >= a.N) return;
  const bool vec = a.N % 8 == 0 && (((uintptr_t)a.y | (uintptr_t)(a.base ? a.base : a.y) |
                                     (uintptr_t)(a.residual ? a.residual : a.y)) & 15) == 0;
  lora_up_columns<kUpRows>(a, t_lds, m0, n0, vec);
}

// ---- merge into a bf16 weight: W[n][k] = bf16(W + bf16(bf16(sum_j B[n][j] A[off_n + j][k]) * scaling)) ------------
__global__ void __launch_bounds__(256) lora_merge_kernel(uint16_t* __restrict__ W, const uint16_t* __restrict__ A,
                                                         const uint16_t* __restrict__ B,
                                                         const int32_t* __restrict__ row_off, float scaling, int N,
                                                         int K, int r) {
  const int n = blockIdx.y;
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int off = row_off ? row_off[n] : 0;
  if (c >= K / 8 || off < 0) return;
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.0f;
  for (int j = 0; j < r; ++j) {
    const float b = bf2f(B[(size_t)n * r + j]);
    float av[8];
    unpack8(((const uint4*)(A + (size_t)(off + j) * K))[c], av);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = fmaf(b, av[i], acc[i]);
  }
  uint4* wp = (uint4*)(W + (size_t)n * K) + c;
  float wv[8];
  unpack8(*wp, wv);
#pragma unroll
  for (int i = 0; i < 8; ++i) wv[i] = __fadd_rn(wv[i], round_bf(__fmul_rn(round_bf(acc[i]), scaling)));
  *wp = make_uint4(pack2(wv[0], wv[1]), pack2(wv[2], wv[3]), pack2(wv[4], wv[5]), pack2(wv[6], wv[7]));
}

// 8-row groups per workgroup of lga_lora_gemv: 64 (512 output rows). Every workgroup recomputes t (R x K dot products,
// A from L2), so a larger grid buys parallelism in the short up-projection only; measured at the Llama-2-7B shapes
// (tools/lora_ab.py --groups, profiles/lora_ab.txt) 64 and 128 tie and 256 / 512 are slower at every shape.
// LGA_LORA_GROUPS overrides it for that sweep.
static int lora_groups_per_wg() {
  if (const char* e = getenv("LGA_LORA_GROUPS")) {  // read per call: a captured launch keeps the grid it was given
    const int v = atoi(e);
    if (v >= 1 && v <= 1024) return v;
  }
  return 64;
}

static bool lora_ranks_ok(int R, int r) {
  return r > 0 && r % 8 == 0 && r <= kLoraMaxRank && R >= r && R % 8 == 0 && R <= kLoraMaxR;
}

}  // namespace lga

extern "C" int lga_lora_gemv(const void* x, const void* norm_weight, float norm_eps, const void* A, const void* B,
                             const int32_t* row_off, float scaling, const void* base, const void* residual, void* y,
                             int N, int K, int R, int r, hipStream_t stream) {
  LGA_CHECK_ARG(x && A && B && y, "lga_lora_gemv: null pointer");
  LGA_CHECK_ARG(N > 0 && K > 0 && K % 8 == 0 && K <= 32768,
                "lga_lora_gemv: K must be a positive multiple of 8, at most 32768");
  LGA_CHECK_ARG(lga::lora_ranks_ok(R, r), "lga_lora_gemv: needs r % 8 == 0, r <= 64, R % 8 == 0, r <= R <= 192");
  LGA_CHECK_ARG(((uintptr_t)x | (uintptr_t)A | (uintptr_t)B | (uintptr_t)(norm_weight ? norm_weight : x)) % 16 == 0,
                "lga_lora_gemv: x, norm_weight, A and B must be 16-B aligned");
  lga::LoraGemvArgs a;
  a.x = (const uint16_t*)x;
  a.norm_w = (const uint16_t*)norm_weight;
  a.A = (const uint16_t*)A;
  a.up = lga::LoraUpArgs{nullptr, (const uint16_t*)B, row_off, (const uint16_t*)base, (const uint16_t*)residual,
                         (uint16_t*)y, 1, N, R, r, scaling};
  a.K = K;
  a.eps = norm_eps;
  a.groups_per_wg = lga::lora_groups_per_wg();
  const int groups = (N + 7) / 8;
  const dim3 blocks((groups + a.groups_per_wg - 1) / a.groups_per_wg);
  const size_t lds = (size_t)K * 2;
  if (R <= 16) lga::lora_gemv_kernel<1><<<blocks, lga::kGemvThreads, lds, stream>>>(a);
  else if (R <= 32) lga::lora_gemv_kernel<2><<<blocks, lga::kGemvThreads, lds, stream>>>(a);
  else lga::lora_gemv_kernel<4><<<blocks, lga::kGemvThreads, lds, stream>>>(a);
  LGA_LAUNCH_RETURN();
}

extern "C" int lga_lora_gemv_rows(const void* x, const void* norm_weight, float norm_eps, const void* A, const void* B,
                                  const int32_t* row_off, const int32_t* adapter, int n_adapters, long long a_stride,
                                  long long b_stride, float scaling, const void* base, const void* residual, void* y,
                                  int M, int N, int K, int R, int r, hipStream_t stream) {
  LGA_CHECK_ARG(x && A && B && adapter && base && y, "lga_lora_gemv_rows: null pointer");
  LGA_CHECK_ARG(M >= 1 && M <= 8, "lga_lora_gemv_rows: M must be in 1..8");
  LGA_CHECK_ARG(n_adapters >= 1, "lga_lora_gemv_rows: n_adapters must be at least 1");
  LGA_CHECK_ARG(N > 0 && K > 0 && K % 8 == 0 && K <= 32768,
                "lga_lora_gemv_rows: K must be a positive multiple of 8, at most 32768");
  LGA_CHECK_ARG(lga::lora_ranks_ok(R, r),
                "lga_lora_gemv_rows: needs r % 8 == 0, r <= 64, R % 8 == 0, r <= R <= 192");
  LGA_CHECK_ARG(a_stride >= (long long)R * K && b_stride >= (long long)N * r && a_stride % 8 == 0 && b_stride % 8 == 0,
                "lga_lora_gemv_rows: a_stride / b_stride must be multiples of 8 elements of at least one block "
                "(R * K / N * r)");
  LGA_CHECK_ARG(((uintptr_t)x | (uintptr_t)A | (uintptr_t)B | (uintptr_t)(norm_weight ? norm_weight : x)) % 16 == 0,
                "lga_lora_gemv_rows: x, norm_weight, A and B must be 16-B aligned");
  lga::LoraGemvArgs a;
  a.x = (const uint16_t*)x;
  a.norm_w = (const uint16_t*)norm_weight;
  a.A = (const uint16_t*)A;
  a.up = lga::LoraUpArgs{nullptr, (const uint16_t*)B, row_off, (const uint16_t*)base, (const uint16_t*)residual,
                         (uint16_t*)y, 1, N, R, r, scaling};
  a.K = K;
  a.eps = norm_eps;
  a.groups_per_wg = lga::lora_groups_per_wg();
  const lga::LoraRowsArgs rw{adapter, n_adapters, a_stride, b_stride};
  const int groups = (N + 7) / 8;
  const dim3 blocks((groups + a.groups_per_wg - 1) / a.groups_per_wg, M);  // (the one-row launch's grid, M)
  const size_t lds = (size_t)K * 2;
  if (R <= 16) lga::lora_gemv_rows_kernel<1><<<blocks, lga::kGemvThreads, lds, stream>>>(a, rw);
  else if (R <= 32) lga::lora_gemv_rows_kernel<2><<<blocks, lga::kGemvThreads, lds, stream>>>(a, rw);
  else lga::lora_gemv_rows_kernel<4><<<blocks, lga::kGemvThreads, lds, stream>>>(a, rw);
  LGA_LAUNCH_RETURN();
}

extern "C" int lga_lora_down(const void* x, const void* A, void* t, int M, int K, int R, hipStream_t stream) {
  LGA_CHECK_ARG(x && A && t, "lga_lora_down: null pointer");
  LGA_CHECK_ARG(M > 0 && K > 0 && K % 8 == 0 && K <= 32768,
                "lga_lora_down: K must be a positive multiple of 8, at most 32768");
  LGA_CHECK_ARG(R > 0 && R % 8 == 0 && R <= lga::kLoraMaxR, "lga_lora_down: needs R % 8 == 0, R <= 192");
  LGA_CHECK_ARG(((uintptr_t)x | (uintptr_t)A | (uintptr_t)t) % 16 == 0,
                "lga_lora_down: x, A and t must be 16-B aligned");
  const dim3 blocks((M + 31) / 32);
  const uint16_t *xp = (const uint16_t*)x, *ap = (const uint16_t*)A;
  if (R <= 32) lga::lora_down_kernel<1><<<blocks, 256, 0, stream>>>(xp, ap, (uint16_t*)t, M, K, R);
  else if (R <= 64) lga::lora_down_kernel<2><<<blocks, 256, 0, stream>>>(xp, ap, (uint16_t*)t, M, K, R);
  else if (R <= 128) lga::lora_down_kernel<4><<<blocks, 256, 0, stream>>>(xp, ap, (uint16_t*)t, M, K, R);
  else lga::lora_down_kernel<6><<<blocks, 256, 0, stream>>>(xp, ap, (uint16_t*)t, M, K, R);
  LGA_LAUNCH_RETURN();
}

extern "C" int lga_lora_up(const void* t, const void* B, const int32_t* row_off, float scaling, const void* base,
                           const void* residual, void* y, int M, int N, int R, int r, hipStream_t stream) {
  LGA_CHECK_ARG(t && B && y, "lga_lora_up: null pointer");
  LGA_CHECK_ARG(M > 0 && N > 0 && M <= 65535 * lga::kUpRows, "lga_lora_up: M and N must be positive, M <= 524280");
  LGA_CHECK_ARG(lga::lora_ranks_ok(R, r), "lga_lora_up: needs r % 8 == 0, r <= 64, R % 8 == 0, r <= R <= 192");
  LGA_CHECK_ARG((uintptr_t)B % 16 == 0, "lga_lora_up: B must be 16-B aligned");
  const lga::LoraUpArgs a{(const uint16_t*)t, (const uint16_t*)B, row_off, (const uint16_t*)base,
                          (const uint16_t*)residual, (uint16_t*)y, M, N, R, r, scaling};
  const int groups = (N + 7) / 8;
  const dim3 blocks((groups + 255) / 256, (M + lga::kUpRows - 1) / lga::kUpRows);
  lga::lora_up_kernel<<<blocks, 256, (size_t)lga::kUpRows * R * sizeof(float), stream>>>(a);
  LGA_LAUNCH_RETURN();
}

extern "C" int lga_lora_merge(void* W, const void* A, const void* B, const int32_t* row_off, float scaling, int N,
                              int K, int R, int r, hipStream_t stream) {
  LGA_CHECK_ARG(W && A && B, "lga_lora_merge: null pointer");
  LGA_CHECK_ARG(N > 0 && K > 0 && K % 8 == 0, "lga_lora_merge: K must be a positive multiple of 8");
  LGA_CHECK_ARG(lga::lora_ranks_ok(R, r), "lga_lora_merge: needs r % 8 == 0, r <= 64, R % 8 == 0, r <= R <= 192");
  LGA_CHECK_ARG(((uintptr_t)W | (uintptr_t)A) % 16 == 0, "lga_lora_merge: W and A must be 16-B aligned");
  for (int n0 = 0; n0 < N; n0 += 32768) {  // grid.y holds at most 65535 rows (an lm_head can have more)
    const int rows = N - n0 < 32768 ? N - n0 : 32768;
    const dim3 blocks((K / 8 + 255) / 256, rows);
    lga::lora_merge_kernel<<<blocks, 256, 0, stream>>>((uint16_t*)W + (size_t)n0 * K, (const uint16_t*)A,
                                                       (const uint16_t*)B + (size_t)n0 * r,
                                                       row_off ? row_off + n0 : nullptr, scaling, rows, K, r);
  }
  LGA_LAUNCH_RETURN();
}
