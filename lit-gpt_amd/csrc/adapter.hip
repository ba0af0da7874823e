// LLaMA-Adapter v1: the gated prefix-attention term of the reference's lit_gpt/adapter.py
// (CausalSelfAttention.scaled_dot_product_attention), applied in place to an attention result.
//
//   lga_adapter_attention   y[t, h] += g_h * softmax(scale * rope(q[t, h]) ak[g]^T) av[g]      (g = h / (H / G))
//
// ak / av (G, aT, hs) are the k / v slices of attn.attn(adapter_wte.weight): they depend on the weights alone, are
// never roped and never masked, so a query's extra work is aT (<= 64) keys. Rounding points (the reference under
// bf16-true): q^ = bf16(rope(q)) with the arithmetic of lga_rope_kv_append (x * cos + rotated * sin, no contraction);
// s_j = scale * (q^ . ak_j) in fp32; p = softmax(s) in fp32; ay = bf16(sum_j p_j av_j); t = bf16(g_h * ay);
// y = bf16(y + t).
//
// One wave per (row, head), four waves per workgroup; no splits, no workspace, no atomics: a (row, head) is summed by
// one wave in one fixed order, so its bits depend on neither T nor the grid. Lane j owns key j: its ak row (hs / 8
// 16-B chunks, held in registers) is requested at the kernel's head together with the wave's q row, the row's
// position and the head's gating factor, none of which depends on another load; the cos / sin rows are the one
// dependent round trip (behind the position). The roped q goes through LDS to every lane, p likewise. In the output
// pass a lane owns one bf16 pair of the head row: its pair of y and of the first 16 av rows are requested at the head
// too (coalesced, one dword per lane and key); only a prefix longer than 16 reads the rest once p is known.
#include "common.h"

namespace lga {

constexpr int kAdapterMaxKeys = 64;  // aT: one lane per key
constexpr int kAdapterMaxHs = 256;

// CH: 16-B chunks of a head row this instantiation holds in registers (hs <= 8 * CH). pos_mode: 0 = pos[row],
// 1 = pos[0] + row (the verify window), 2 = pos[0] for every row (samples of one prompt in lock step).
template <int CH>
__global__ void __launch_bounds__(256)
adapter_attention_kernel(const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ ak,
                         const uint16_t* __restrict__ av, const uint16_t* __restrict__ gating,
                         const float* __restrict__ cos, const float* __restrict__ sin,
                         const int64_t* __restrict__ pos, const int32_t* __restrict__ active, uint16_t* y, int T, int H,
                         int G, int hs, int n_elem, int aT, int rope_rows, int pos_mode, float scale) {
  constexpr int kDims = CH * 8;            // head dims covered
  constexpr int kQIter = kDims / 64;       // dims per lane when roping q
  constexpr int kOIter = CH > 16 ? 2 : 1;  // bf16 pairs per lane in the output pass
  constexpr int kVPre = 16;                // value rows whose pair a lane requests at the kernel's head
  __shared__ float qs[4][kDims];
  __shared__ float ps[4][kAdapterMaxKeys];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long item = (long)blockIdx.x * 4 + wave;  // (row, head), wave-uniform
  const bool in_range = item < (long)T * H;
  const int row = in_range ? (int)(item / H) : 0, h = in_range ? (int)(item % H) : 0;
  const int qpk = H / G, g = h / qpk, cph = hs >> 3, half = n_elem >> 1;

  // ---- head: every load here is independent of the others (row 0 / head 0 stand in for a wave past the end)
  const int act = active ? active[row] : 1;
  const long rp = pos_mode == 0 ? pos[row] : (pos_mode == 1 ? pos[0] + row : pos[0]);
  const uint16_t* qh = qkv + ((size_t)row * (H + 2 * G) + (size_t)g * (qpk + 2) + (h - g * qpk)) * hs;
  uint16_t xq[kQIter], xr[kQIter];
#pragma unroll
  for (int i = 0; i < kQIter; ++i) {
    const int d = lane + 64 * i;
    xq[i] = d < hs ? qh[d] : 0;
    xr[i] = d < n_elem ? qh[d < half ? d + half : d - half] : 0;
  }
  const bool key = lane < aT;
  const uint4* krow = (const uint4*)(ak + ((size_t)g * aT + (key ? lane : 0)) * hs);
  uint4 kreg[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) kreg[c] = (key && c < cph) ? krow[c] : make_uint4(0, 0, 0, 0);
  const float gh = bf2f(gating[h]);
  // the output pass's operands that depend on nothing either: the lane's y pair(s) and its pair of the first kVPre
  // value rows (the reference's default adapter_prompt_length is 10; longer prefixes load the rest after the softmax)
  const uint32_t* vrow = (const uint32_t*)(av + (size_t)g * aT * hs);
  uint32_t* yh = (uint32_t*)(y + ((size_t)row * H + h) * hs);
  const int pairs = hs >> 1;
  uint32_t y0[kOIter], vpre[kOIter][kVPre];
#pragma unroll
  for (int i = 0; i < kOIter; ++i) {
    const int pr = lane + 64 * i;
    y0[i] = pr < pairs ? yh[pr] : 0;
#pragma unroll
    for (int j = 0; j < kVPre; ++j) vpre[i][j] = (pr < pairs && j < aT) ? vrow[(size_t)j * pairs + pr] : 0;
  }

  // an idle row, or one whose position the rope tables do not hold, is left as it is (nothing below is loaded for it)
  const bool valid = in_range && act != 0 && rp >= 0 && rp < rope_rows;

  // ---- q^ = bf16(rope(q)) -> LDS
  if (valid) {
    const float* cr = cos + (size_t)rp * n_elem;
    const float* sr = sin + (size_t)rp * n_elem;
#pragma unroll
    for (int i = 0; i < kQIter; ++i) {
      const int d = lane + 64 * i;
      float v = bf2f(xq[i]);
      if (d < n_elem) {
        const float r = d < half ? -bf2f(xr[i]) : bf2f(xr[i]);
        v = round_bf(add_rn(mul_rn(v, cr[d]), mul_rn(r, sr[d])));
      }
      qs[wave][d] = v;  // (dims in hs..kDims-1 hold 0 and meet zero chunks of ak)
    }
  }
  __syncthreads();

  // ---- s_j, softmax over the aT keys (lane j = key j)
  if (valid) {
    float s = 0.0f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const uint32_t w[4] = {kreg[c].x, kreg[c].y, kreg[c].z, kreg[c].w};
      const float4 q0 = *(const float4*)&qs[wave][8 * c], q1 = *(const float4*)&qs[wave][8 * c + 4];
      s = fmaf(q0.x, bflo(w[0]), s);
      s = fmaf(q0.y, bfhi(w[0]), s);
      s = fmaf(q0.z, bflo(w[1]), s);
      s = fmaf(q0.w, bfhi(w[1]), s);
      s = fmaf(q1.x, bflo(w[2]), s);
      s = fmaf(q1.y, bfhi(w[2]), s);
      s = fmaf(q1.z, bflo(w[3]), s);
      s = fmaf(q1.w, bfhi(w[3]), s);
    }
    s = key ? s * scale : -INFINITY;
    const float m = wave_max(s);
    const float e = key ? expf(s - m) : 0.0f;
    const float l = wave_sum(e);
    ps[wave][lane] = e / l;
  }
  __syncthreads();

  // ---- ay = bf16(sum_j p_j av_j); y = bf16(y + bf16(g_h * ay)); lane = one bf16 pair of the head row
  if (valid) {
#pragma unroll
    for (int i = 0; i < kOIter; ++i) {
      const int pr = lane + 64 * i;
      if (pr < pairs) {
        float a0 = 0.0f, a1 = 0.0f;
#pragma unroll
        for (int j = 0; j < kVPre; ++j) {  // keys past aT: p_j = 0 (lanes past aT wrote it) against a zero pair
          const float p = ps[wave][j];
          a0 = fmaf(p, bflo(vpre[i][j]), a0);
          a1 = fmaf(p, bfhi(vpre[i][j]), a1);
        }
        for (int j = kVPre; j < aT; ++j) {
          const uint32_t w = vrow[(size_t)j * pairs + pr];
          const float p = ps[wave][j];
          a0 = fmaf(p, bflo(w), a0);
          a1 = fmaf(p, bfhi(w), a1);
        }
        const float t0 = round_bf(mul_rn(gh, round_bf(a0))), t1 = round_bf(mul_rn(gh, round_bf(a1)));
        yh[pr] = pack2(add_rn(bflo(y0[i]), t0), add_rn(bfhi(y0[i]), t1));
      }
    }
  }
}

}  // namespace lga

int lga::preload_adapter() {
  return lga::preload(lga::adapter_attention_kernel<8>) + lga::preload(lga::adapter_attention_kernel<16>) +
         lga::preload(lga::adapter_attention_kernel<32>);
}

extern "C" int lga_adapter_attention(const void* qkv, const void* ak, const void* av, const void* gating,
                                     const float* cos, const float* sin, int rope_rows, const int64_t* pos,
                                     int pos_mode, const int32_t* active, void* y, int T, int n_head,
                                     int n_query_groups, int head_size, int rope_n_elem, int aT, float scale,
                                     hipStream_t stream) {
  LGA_CHECK_ARG(qkv && ak && av && gating && pos && y && (rope_n_elem == 0 || (cos && sin)),
                "lga_adapter_attention: null pointer");
  LGA_CHECK_ARG(T > 0 && (long)T * n_head <= 0x7fffffffL / 4 && n_head > 0 && n_query_groups > 0 &&
                    n_head % n_query_groups == 0,
                "lga_adapter_attention: bad row count or head geometry (needs n_head % n_query_groups == 0)");
  LGA_CHECK_ARG(head_size > 0 && head_size % 8 == 0 && head_size <= lga::kAdapterMaxHs,
                "lga_adapter_attention: head_size must be a multiple of 8, at most 256");
  LGA_CHECK_ARG(rope_n_elem >= 0 && rope_n_elem % 2 == 0 && rope_n_elem <= head_size,
                "lga_adapter_attention: rope_n_elem must be even and <= head_size");
  LGA_CHECK_ARG(aT >= 1 && aT <= lga::kAdapterMaxKeys, "lga_adapter_attention: adapter_prompt_length must be 1..64");
  LGA_CHECK_ARG(rope_rows > 0 && pos_mode >= 0 && pos_mode <= 2,
                "lga_adapter_attention: rope_rows must be positive and pos_mode 0 (per row), 1 (base + row) or 2 "
                "(one position)");
  LGA_CHECK_ARG(((uintptr_t)ak % 16 | (uintptr_t)av % 4 | (uintptr_t)y % 4 | (uintptr_t)qkv % 2) == 0,
                "lga_adapter_attention: ak must be 16-B aligned, av and y 4-B aligned");
  const unsigned blocks = (unsigned)(((long)T * n_head + 3) / 4);
#define LGA_ADAPTER(CH)                                                                                          \
  lga::adapter_attention_kernel<CH><<<blocks, 256, 0, stream>>>(                                                 \
      (const uint16_t*)qkv, (const uint16_t*)ak, (const uint16_t*)av, (const uint16_t*)gating, cos, sin, pos,    \
      active, (uint16_t*)y, T, n_head, n_query_groups, head_size, rope_n_elem, aT, rope_rows, pos_mode, scale)
  if (head_size <= 64) LGA_ADAPTER(8);
  else if (head_size <= 128) LGA_ADAPTER(16);
  else LGA_ADAPTER(32);
#undef LGA_ADAPTER
  LGA_LAUNCH_RETURN();
}
