// Log-likelihood scoring on the device: rows of logits reduced to what an evaluation needs, so the (rows, n) logits
// never leave the GPU (lit_gpt/score.py, eval/lm_eval_harness.py, eval/perplexity.py).
//
//   lga_token_logprobs[_f32]  logprob[r] = x[r, t_r] - (m_r + log sum_j exp(x[r, j] - m_r)),  argmax[r]
//   lga_logits_kl             kl[r] = sum_j softmax(p_r)_j (log_softmax(p_r)_j - log_softmax(q_r)_j),  agree[r]
//
// One workgroup per row, ONE pass over the row: every thread keeps a running (max, sum) pair in fp32 (online softmax,
// rescaled once per 16-B group) and its arg-max candidate; the pairs meet in a block reduction. HBM traffic is the
// rows * n * sizeof(element) bytes of the logits, read once.
//
// Fixed order. A row is cut into LOGICAL groups of 16 B (8 bf16 / 4 fp32) counted from the row's first element;
// thread t of NT owns groups t, t + NT, ... and eats them in ascending order; NT depends on n alone. So a row's result
// does not depend on the number of rows, on the row's place in the grid or on the row's address — only HOW a group
// reaches the registers does: a row that starts on a 16-B boundary loads each group with one 16-B load; any other row
// (odd n: rows start on 2-B boundaries) loads the two ALIGNED 16-B vectors a group straddles and funnel-shifts them.
// The first group and the last two groups of a row are the only ones whose aligned vectors can reach outside the row:
// they are gathered element by element under bounds tests, so nothing outside [row, row + n) is ever read.
#include <math.h>

#include <type_traits>

#include "common.h"

namespace lga {
namespace {

constexpr int kScoreMaxWaves = 16;
// Lab knobs (make lab-lib LABSRC=score LABFLAGS=...; the product build defines neither):
//   LGA_SCORE_U        16-B groups a thread of the single-row kernel has in flight (the KL kernel: half, per matrix)
//   LGA_SCORE_THREADS  one workgroup size for every n. A result's bits depend on the workgroup size, so a build with
//                      this set is comparable with itself only; the kernels need whole waves and at most 16 of them.
#ifndef LGA_SCORE_U
#define LGA_SCORE_U 4
#endif
static_assert(LGA_SCORE_U >= 2 && LGA_SCORE_U <= 16 && LGA_SCORE_U % 2 == 0, "LGA_SCORE_U: an even count in [2, 16]");
#ifdef LGA_SCORE_THREADS
static_assert(LGA_SCORE_THREADS >= 64 && LGA_SCORE_THREADS <= 1024 && LGA_SCORE_THREADS % 64 == 0,
              "LGA_SCORE_THREADS: a multiple of 64 in [64, 1024] (whole waves, 16 LDS slots, launch bounds)");
#endif
constexpr float kLog2e = 1.44269504088896340736f;

// exp(d) for d <= 0 as one v_exp_f32: the fp32 product d * log2(e) moves the exponent by at most |d| * 2^-24 (relative
// to the result), which the softmax weights (E_p |d| <= log n) keep near 1e-6 in the log of the sum
__device__ __forceinline__ float exp_fast(float d) { return __builtin_amdgcn_exp2f(d * kLog2e); }

// torch.argmax order, as sample.hip's lga_argmax: NaN above every number, ties to the lowest index
__device__ __forceinline__ void take_best(float v, int i, float& bv, int& bi) {
  const bool vn = v != v, bn = bv != bv;
  const bool t = (vn || bn) ? (vn && (!bn || i < bi)) : ((v > bv) || (v == bv && i < bi));
  bv = t ? v : bv;
  bi = t ? i : bi;
}

__device__ __forceinline__ float to_f32(uint16_t b) { return bf2f(b); }
__device__ __forceinline__ float to_f32(float f) { return f; }

__device__ __forceinline__ void unpack(const uint4& q, float (&x)[8]) {
  x[0] = bflo(q.x), x[1] = bfhi(q.x), x[2] = bflo(q.y), x[3] = bfhi(q.y);
  x[4] = bflo(q.z), x[5] = bfhi(q.z), x[6] = bflo(q.w), x[7] = bfhi(q.w);
}
__device__ __forceinline__ void unpack(const uint4& q, float (&x)[4]) {
  x[0] = __uint_as_float(q.x), x[1] = __uint_as_float(q.y), x[2] = __uint_as_float(q.z), x[3] = __uint_as_float(q.w);
}

// 16 B holding row elements [e0, e0 + P), -inf where the index falls outside [0, n): only in-row elements are read
__device__ __forceinline__ uint4 load_edge(const uint16_t* row, int n, long e0) {
  uint32_t w[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long i0 = e0 + 2 * j, i1 = i0 + 1;
    const uint32_t lo = (i0 >= 0 && i0 < n) ? row[i0] : 0xFF80u;
    const uint32_t hi = (i1 >= 0 && i1 < n) ? row[i1] : 0xFF80u;
    w[j] = lo | (hi << 16);
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ __forceinline__ uint4 load_edge(const float* row, int n, long e0) {
  uint32_t w[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long i = e0 + j;
    w[j] = (i >= 0 && i < n) ? __float_as_uint(row[i]) : 0xFF800000u;
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}
// the aligned vector that starts at row element e0 (row + e0 is 16-B aligned): one load when it lies inside the row
template <class T>
__device__ __forceinline__ uint4 load_guarded(const T* row, int n, long e0) {
  constexpr int P = 16 / sizeof(T);
  if (e0 >= 0 && e0 + P <= n) return *(const uint4*)(row + e0);
  return load_edge(row, n, e0);
}

// the 16 B that start `mis` elements into the 32 B (lo, hi); mis is the same for a whole row (a scalar branch)
__device__ __forceinline__ uint4 funnel(const uint16_t*, const uint4& lo, const uint4& hi, int mis) {
  uint32_t d0, d1, d2, d3, d4;
  switch (mis >> 1) {
    case 0: d0 = lo.x, d1 = lo.y, d2 = lo.z, d3 = lo.w, d4 = hi.x; break;
    case 1: d0 = lo.y, d1 = lo.z, d2 = lo.w, d3 = hi.x, d4 = hi.y; break;
    case 2: d0 = lo.z, d1 = lo.w, d2 = hi.x, d3 = hi.y, d4 = hi.z; break;
    default: d0 = lo.w, d1 = hi.x, d2 = hi.y, d3 = hi.z, d4 = hi.w; break;
  }
  const uint32_t by = (mis & 1) * 2;  // v_alignbyte_b32: ((high : low) >> 8 * bytes), low 32 bits
  return make_uint4(__builtin_amdgcn_alignbyte(d1, d0, by), __builtin_amdgcn_alignbyte(d2, d1, by),
                    __builtin_amdgcn_alignbyte(d3, d2, by), __builtin_amdgcn_alignbyte(d4, d3, by));
}
__device__ __forceinline__ uint4 funnel(const float*, const uint4& lo, const uint4& hi, int mis) {
  switch (mis) {
    case 0: return lo;
    case 1: return make_uint4(lo.y, lo.z, lo.w, hi.x);
    case 2: return make_uint4(lo.z, lo.w, hi.x, hi.y);
    default: return make_uint4(lo.w, hi.x, hi.y, hi.z);
  }
}

// One row as the kernels see it: `mis` elements separate the row's start from the 16-B boundary below it.
template <class T>
struct RowView {
  static constexpr int P = 16 / sizeof(T);
  const T* row;
  int n, mis, groups;
  __device__ RowView(const T* base, int r, int n_) : row(base + (size_t)r * n_), n(n_) {
    mis = (int)(((uintptr_t)row / sizeof(T)) & (P - 1));
    groups = (n - 1) / P + 1;
  }
  // groups 1 .. groups - 3: both aligned vectors lie inside the row, the loads are unconditional
  template <bool MIS>
  __device__ __forceinline__ uint4 interior(int g) const {
    const uint4* v = (const uint4*)((uintptr_t)row - (uintptr_t)mis * sizeof(T)) + g;
    if (!MIS) return v[0];
    return funnel(row, v[0], v[1], mis);
  }
  // any group, every access bounds-tested (group 0 and the last two)
  __device__ __forceinline__ uint4 edge(int g) const {
    const long e0 = (long)g * P - mis;
    const uint4 lo = load_guarded(row, n, e0);
    if (mis == 0) return lo;
    return funnel(row, lo, load_guarded(row, n, e0 + P), mis);
  }
};

struct Soft {  // running max and sum_j exp(x_j - m) of what a thread has seen
  float m = -INFINITY, s = 0.0f;
};

template <int P>
__device__ __forceinline__ float group_max(const float (&x)[P]) {
  float gm = x[0];
#pragma unroll
  for (int k = 1; k < P; ++k) gm = fmaxf(gm, x[k]);  // NaN entries are skipped here and poison the sum below
  return gm;
}

// raise the running maximum to the group's (gm); returns the factor the running sum was rescaled by (1 if unmoved)
__device__ __forceinline__ float soft_rescale(Soft& a, float gm) {
  const bool up = gm > a.m;
  const float sc = up ? exp_fast(a.m - gm) : 1.0f;  // a.m = -inf: exp2(-inf) = 0 on a sum that is still 0
  a.s *= sc;
  a.m = up ? gm : a.m;
  return sc;
}
// what the exponentials are taken against: the running maximum, or 0 while everything seen is -inf (each entry then
// adds exp(-inf) = 0, not exp(nan))
__device__ __forceinline__ float soft_base(const Soft& a) { return a.m == -INFINITY ? 0.0f : a.m; }
// adds one group; returns the group's own sum of exponentials: NaN iff the group holds a NaN or a +inf (+inf - +inf)
template <int P>
__device__ __forceinline__ float soft_add(Soft& a, const float (&x)[P], float gm) {
  soft_rescale(a, gm);
  const float mm = soft_base(a);
  float gs = 0.0f;
#pragma unroll
  for (int k = 0; k < P; ++k) gs += exp_fast(x[k] - mm);
  a.s += gs;
  return gs;
}
// The arg-max candidate of a thread, whose groups arrive in ascending index order: a group can only change it when its
// maximum beats the candidate (a tie keeps the earlier, lower index) or when it holds a NaN / +inf (gs is NaN), so the
// element-wise search runs for a handful of groups per thread.
template <int P>
__device__ __forceinline__ void best_add(const float (&x)[P], int base, float gm, float gs, float& bv, int& bi) {
  if (gm > bv || gs != gs) {
#pragma unroll
    for (int k = 0; k < P; ++k) take_best(x[k], base + k, bv, bi);  // padding (-inf, index >= n) never wins
  }
}

// Block reductions over a workgroup of up to 16 waves, every thread ending with the same value, fixed order.
struct Scratch {
  float f[kScoreMaxWaves];
  float bv[kScoreMaxWaves];
  int bi[kScoreMaxWaves];
};
__device__ __forceinline__ float block_max(float v, float* buf) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) buf[threadIdx.x >> 6] = v;
  __syncthreads();
  float m = buf[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) m = fmaxf(m, buf[w]);
  __syncthreads();
  return m;
}
__device__ __forceinline__ float block_sum(float v, float* buf) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) buf[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = buf[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) s += buf[w];
  __syncthreads();
  return s;
}
__device__ __forceinline__ int block_best(float bv, int bi, int n, Scratch& sh) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(bv, off);
    const int oi = __shfl_xor(bi, off);
    take_best(ov, oi, bv, bi);
  }
  if ((threadIdx.x & 63) == 0) {
    sh.bv[threadIdx.x >> 6] = bv;
    sh.bi[threadIdx.x >> 6] = bi;
  }
  __syncthreads();
  bv = sh.bv[0], bi = sh.bi[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) take_best(sh.bv[w], sh.bi[w], bv, bi);
  __syncthreads();
  return bi < n ? bi : 0;
}
// a thread's sum on the block's maximum M (a thread that saw nothing keeps its 0, one that saw NaN its NaN)
__device__ __forceinline__ float on_block_max(float v, float m, float M) { return m == M ? v : v * expf(m - M); }

template <class T>
__global__ void __launch_bounds__(1024) token_logprob_kernel(const T* __restrict__ logits, int n,
                                                             const int32_t* __restrict__ targets,
                                                             float* __restrict__ lp_out,
                                                             int32_t* __restrict__ am_out) {
  constexpr int P = 16 / sizeof(T), U = LGA_SCORE_U;
  __shared__ Scratch sh;
  const int r = blockIdx.x, t = threadIdx.x, nt = blockDim.x;
  const RowView<T> rv(logits, r, n);
  const int tgt = targets[r];
  float xt = __builtin_nanf("");  // a target outside [0, n) scores NaN and reads nothing
  if (t == 0 && tgt >= 0 && tgt < n) xt = to_f32(rv.row[tgt]);
  Soft a;
  float bv = -INFINITY;
  int bi = 0x7FFFFFFF;
  auto eat = [&](const uint4& q, int g) {
    float x[P];
    unpack(q, x);
    const float gm = group_max(x);
    best_add(x, g * P, gm, soft_add(a, x, gm), bv, bi);
  };
  // the bounds-tested groups (0 and the last two) are loaded ahead of the interior ones, so that their round trips
  // overlap, and eaten in their place in the ascending order; a thread owns at most one of the last two (nt >= 64)
  const uint4 none = make_uint4(0, 0, 0, 0);
  const uint4 e_first = t == 0 ? rv.edge(0) : none;
  uint4 e_tail = none;
  int g_tail = -1;
  for (int g = max(rv.groups - 2, 1); g < rv.groups; ++g)
    if (t == g % nt) e_tail = rv.edge(g), g_tail = g;
  if (t == 0) eat(e_first, 0);
  const int last = rv.groups - 3;
  auto interior = [&](auto mis_tag) {
    constexpr bool MIS = decltype(mis_tag)::value;
    for (int g0 = t == 0 ? nt : t; g0 <= last; g0 += U * nt) {
      uint4 q[U];
#pragma unroll
      for (int u = 0; u < U; ++u) q[u] = rv.template interior<MIS>(min(g0 + u * nt, last));
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (g0 + u * nt <= last) eat(q[u], g0 + u * nt);
    }
  };
  if (rv.mis == 0) interior(std::false_type{});
  else interior(std::true_type{});
  if (g_tail >= 0) eat(e_tail, g_tail);

  const float M = block_max(a.m, sh.f);
  const float S = block_sum(on_block_max(a.s, a.m, M), sh.f);
  const int best = block_best(bv, bi, n, sh);
  if (t == 0) {
    lp_out[r] = xt - (M + logf(S));
    am_out[r] = best;
  }
}

__global__ void __launch_bounds__(1024) logits_kl_kernel(const uint16_t* __restrict__ p_logits,
                                                         const uint16_t* __restrict__ q_logits, int n,
                                                         float* __restrict__ kl_out, int32_t* __restrict__ agree_out) {
  constexpr int P = 8, U = LGA_SCORE_U / 2;
  __shared__ Scratch sh;
  const int r = blockIdx.x, t = threadIdx.x, nt = blockDim.x;
  const RowView<uint16_t> rp(p_logits, r, n), rq(q_logits, r, n);
  Soft a, b;       // p's and q's running softmax
  float w = 0.0f;  // sum_j exp(p_j - a.m) (p_j - q_j), rescaled with a.s
  float pbv = -INFINITY, qbv = -INFINITY;
  int pbi = 0x7FFFFFFF, qbi = 0x7FFFFFFF;
  auto eat = [&](const uint4& vp, const uint4& vq, int g) {
    float x[P], y[P];
    unpack(vp, x);
    unpack(vq, y);
    const float gmp = group_max(x), gmq = group_max(y);
    w *= soft_rescale(a, gmp);
    const float mm = soft_base(a);
    float gs = 0.0f, gw = 0.0f;
#pragma unroll
    for (int k = 0; k < P; ++k) {
      const float e = exp_fast(x[k] - mm);
      gs += e;
      gw += e == 0.0f ? 0.0f : e * (x[k] - y[k]);  // a zero weight contributes 0 (the row padding: -inf - -inf)
    }
    a.s += gs;
    w += gw;
    best_add(x, g * P, gmp, gs, pbv, pbi);
    best_add(y, g * P, gmq, soft_add(b, y, gmq), qbv, qbi);
  };
  const uint4 none = make_uint4(0, 0, 0, 0);  // edge groups ahead of the interior ones, as in token_logprob_kernel
  const uint4 pe_first = t == 0 ? rp.edge(0) : none, qe_first = t == 0 ? rq.edge(0) : none;
  uint4 pe_tail = none, qe_tail = none;
  int g_tail = -1;
  for (int g = max(rp.groups - 2, 1); g < rp.groups; ++g)
    if (t == g % nt) pe_tail = rp.edge(g), qe_tail = rq.edge(g), g_tail = g;
  if (t == 0) eat(pe_first, qe_first, 0);
  const int last = rp.groups - 3;
  auto interior = [&](auto mis_tag) {
    constexpr bool MIS = decltype(mis_tag)::value;
    for (int g0 = t == 0 ? nt : t; g0 <= last; g0 += U * nt) {
      uint4 vp[U], vq[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        vp[u] = rp.template interior<MIS>(min(g0 + u * nt, last));
        vq[u] = rq.template interior<MIS>(min(g0 + u * nt, last));
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (g0 + u * nt <= last) eat(vp[u], vq[u], g0 + u * nt);
    }
  };
  if (rp.mis == 0 && rq.mis == 0) interior(std::false_type{});
  else interior(std::true_type{});
  if (g_tail >= 0) eat(pe_tail, qe_tail, g_tail);

  const float Mp = block_max(a.m, sh.f);
  const float Sp = block_sum(on_block_max(a.s, a.m, Mp), sh.f);
  const float Wp = block_sum(on_block_max(w, a.m, Mp), sh.f);
  const float Mq = block_max(b.m, sh.f);
  const float Sq = block_sum(on_block_max(b.s, b.m, Mq), sh.f);
  const int bp = block_best(pbv, pbi, n, sh);
  const int bq = block_best(qbv, qbi, n, sh);
  if (t == 0) {
    // sum_j p_j ((p_j - lse_p) - (q_j - lse_q)) = E_p[p_j - q_j] - (lse_p - lse_q); not clamped
    kl_out[r] = Wp / Sp - ((Mp + logf(Sp)) - (Mq + logf(Sq)));
    agree_out[r] = bp == bq;
  }
}

constexpr int kScoreMaxN = 1 << 30;
// the workgroup size is a function of n alone (the reduction order of a row must not depend on the batch)
#ifdef LGA_SCORE_THREADS  // lab builds only, see the top of the file
inline int score_threads(int, int) { return LGA_SCORE_THREADS; }
#else
inline int score_threads(int n, int per) { return (n - 1) / per + 1 >= 2048 ? 512 : 256; }
#endif

}  // namespace
}  // namespace lga

extern "C" int lga_token_logprobs(const void* logits, int rows, int n, const int32_t* targets, float* logprob_out,
                                  int32_t* argmax_out, hipStream_t stream) {
  LGA_CHECK_ARG(logits && targets && logprob_out && argmax_out, "lga_token_logprobs: null pointer");
  LGA_CHECK_ARG(rows > 0 && n > 0 && n <= lga::kScoreMaxN, "lga_token_logprobs: needs rows > 0 and 0 < n <= 2^30");
  LGA_CHECK_ARG(((uintptr_t)logits & 1) == 0, "lga_token_logprobs: logits must be 2-B aligned");
  lga::token_logprob_kernel<uint16_t><<<rows, lga::score_threads(n, 8), 0, stream>>>(
      (const uint16_t*)logits, n, targets, logprob_out, argmax_out);
  LGA_LAUNCH_RETURN();
}

extern "C" int lga_token_logprobs_f32(const float* logits, int rows, int n, const int32_t* targets,
                                      float* logprob_out, int32_t* argmax_out, hipStream_t stream) {
  LGA_CHECK_ARG(logits && targets && logprob_out && argmax_out, "lga_token_logprobs_f32: null pointer");
  LGA_CHECK_ARG(rows > 0 && n > 0 && n <= lga::kScoreMaxN,
                "lga_token_logprobs_f32: needs rows > 0 and 0 < n <= 2^30");
  LGA_CHECK_ARG(((uintptr_t)logits & 3) == 0, "lga_token_logprobs_f32: logits must be 4-B aligned");
  lga::token_logprob_kernel<float><<<rows, lga::score_threads(n, 4), 0, stream>>>(logits, n, targets, logprob_out,
                                                                                 argmax_out);
  LGA_LAUNCH_RETURN();
}

extern "C" int lga_logits_kl(const void* p_logits, const void* q_logits, int rows, int n, float* kl_out,
                             int32_t* agree_out, hipStream_t stream) {
  LGA_CHECK_ARG(p_logits && q_logits && kl_out && agree_out, "lga_logits_kl: null pointer");
  LGA_CHECK_ARG(rows > 0 && n > 0 && n <= lga::kScoreMaxN, "lga_logits_kl: needs rows > 0 and 0 < n <= 2^30");
  LGA_CHECK_ARG((((uintptr_t)p_logits | (uintptr_t)q_logits) & 1) == 0, "lga_logits_kl: logits must be 2-B aligned");
  lga::logits_kl_kernel<<<rows, lga::score_threads(n, 8), 0, stream>>>((const uint16_t*)p_logits,
                                                                       (const uint16_t*)q_logits, n, kl_out, agree_out);
  LGA_LAUNCH_RETURN();
}
