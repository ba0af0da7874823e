// The decode attention's softmax core: every piece of arithmetic that attn_body (one-row, rows, window, batch, fp8) and
// attn_shared_kernel (n samples of one prompt) have in common, written ONCE. Both kernels must give the same bits for a
// (row, head) state, so every floating-point multiply, add and multiply-add here is an explicit mul_rn / add_rn /
// __builtin_fmaf: nothing is left to -ffp-contract, and a compiler that fuses differently cannot part the two kernels
// (the forms are the ones hipcc gave attn_body when its arithmetic was still plain C++). The callers
// keep what is their own: addressing, who loads what, the cache append, the ticket protocol, their LDS arrays.
//
// A state is one query row's (m, l, o) for the QPK heads of a slice: float m[QPK], l[QPK], o[QPK][8], in log2 units,
// each lane holding the 8 columns sub * 8 .. sub * 8 + 7 of its row group's share.
#pragma once
#include "decode_ops.h"
#include "kv8_ops.h"

namespace lga {

template <bool KV8>
struct kv_regs {  // one lane's share of a K or V row in flight
  uint4 d;
};
template <>
struct kv_regs<true> {  // (fp8 caches: 8 e4m3 codes and the row's scale)
  uint2 d;
  float s;
};

// m starts at a finite floor, not -inf: every row group runs the split's step count, so one whose keys are all past
// k_end sees only masked (-inf) scores, and exp(floor - floor) = 1 keeps its (l, o) = 0 instead of NaN; a real first
// score s gives exp(kMFloor - s) = 0 exactly as exp(-inf) did
constexpr float kMFloor = -1e30f;

// Split `split` of n_splits over the keys 0..p: [k_lo, k_hi). FUSED: key p is scored from registers by the split that
// owns it (owns_new), so the cache stream stops at k_end = min(k_hi, p).
struct attn_range {
  int k_lo, k_hi, k_end;
  bool owns_new;
};
template <bool FUSED>
__device__ __forceinline__ attn_range attn_split_range(long p, int max_seq, int n_splits, int split) {
  const int L = (int)min(p + 1, (long)max_seq);  // keys 0..p (never past the cache)
  const int chunk = (L + n_splits - 1) / n_splits;
  const int k_lo = split * chunk;
  const int k_hi = min(k_lo + chunk, L);
  const bool owns_new = FUSED && p < max_seq && k_lo <= p && p < k_hi;
  return {k_lo, k_hi, FUSED ? min(k_hi, (int)p) : k_hi, owns_new};
}

// q stays packed bf16 (as the reference's bf16 q): scores are v_dot2_f32_bf16 chains — two exact bf16 products per
// instruction into an fp32 accumulator, half the VALU of unpack + fma. Interleaved A/B (tools/attn_ab.py, round 5) at
// p = 32066, 32 splits: Mixtral 34.8 -> 33.8 us, its TP = 2 rank 24.8 -> 23.5; Llama-2-7B neutral
__device__ __forceinline__ float attn_dot8(const uint4 a, const uint4 b) {
  return dot2_bf16(a.w, b.w, dot2_bf16(a.z, b.z, dot2_bf16(a.y, b.y, dot2_bf16(a.x, b.x, 0.0f))));
}

// One step = UNR keys per row group (key u is row j0 + u * RG; rows at or past k_end are masked: score -inf, e = 0):
// scores, online-softmax rescale, P.V. KV8: the row's scale multiplies the score and the P.V weight.
template <int LPR, int QPK, int UNR, int RG, bool KV8>
__device__ __forceinline__ void attn_step(float (&m)[QPK], float (&l)[QPK], float (&o)[QPK][8], const uint4 (&qp)[QPK],
                                          const kv_regs<KV8> (&kv)[UNR], const kv_regs<KV8> (&vv)[UNR], int j0,
                                          int k_end, float sl2) {
#pragma unroll
  for (int h = 0; h < QPK; ++h) {
    float s[UNR];
    float mx = m[h];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      float sd;  // whole row group active: DPP inside it
      if constexpr (KV8) sd = mul_rn(row_group_sum<LPR>(attn_dot8(qp[h], kv8_bf16x8(kv[u].d))), mul_rn(kv[u].s, sl2));
      else sd = mul_rn(row_group_sum<LPR>(attn_dot8(qp[h], kv[u].d)), sl2);
      s[u] = (j0 + u * RG < k_end) ? sd : -INFINITY;
      mx = fmaxf(mx, s[u]);
    }
    const float c = __builtin_amdgcn_exp2f(m[h] - mx);  // m = kMFloor (first step) -> 0
#pragma unroll
    for (int i = 0; i < 8; ++i) o[h][i] = mul_rn(o[h][i], c);
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const float e = __builtin_amdgcn_exp2f(s[u] - mx);  // masked keys: exp(-inf) = 0
      l[h] = u == 0 ? __builtin_fmaf(l[h], c, e) : add_rn(l[h], e);
      float vf[8];
      if constexpr (KV8) kv8_f32x8(vv[u].d, vf);
      else unpack8(vv[u].d, vf);
      float ev = e;
      if constexpr (KV8) ev = mul_rn(e, vv[u].s);
#pragma unroll
      for (int i = 0; i < 8; ++i) o[h][i] = __builtin_fmaf(ev, vf[i], o[h][i]);
    }
    m[h] = mx;
  }
}

// The new key, scored from registers by row group 0 of the owning split: kr its roped (KV8: requantized and expanded)
// row, vf its value row, ksn / vsn the KV8 row scales (1 otherwise). The score feeds the max as mul(sd, t) and the
// exponential as fma(sd, t, -mx): that asymmetry is what the compiler made of `s - mx`, and it stays.
template <int LPR, int QPK, bool KV8>
__device__ __forceinline__ void attn_new_key(float (&m)[QPK], float (&l)[QPK], float (&o)[QPK][8],
                                             const uint4 (&qp)[QPK], const uint4 kr, const float (&vf)[8], float ksn,
                                             float vsn, float sl2) {
#pragma unroll
  for (int h = 0; h < QPK; ++h) {
    const float sd = row_group_sum<LPR>(attn_dot8(qp[h], kr));
    const float t = KV8 ? mul_rn(ksn, sl2) : sl2;
    const float mx = fmaxf(m[h], mul_rn(sd, t));
    const float c = __builtin_amdgcn_exp2f(m[h] - mx);
    const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(sd, t, -mx));
    l[h] = __builtin_fmaf(l[h], c, e);
    const float ev = KV8 ? mul_rn(e, vsn) : e;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[h][i] = __builtin_fmaf(ev, vf[i], mul_rn(o[h][i], c));
    m[h] = mx;
  }
}

// One level of the wave merge: every lane takes in the state of the lane `off` away (the row groups of a wave are the
// lanes differing in the bits above log2(LPR); the caller runs off = LPR, 2 LPR, .. 32)
template <int QPK>
__device__ __forceinline__ void attn_wave_merge(float (&m)[QPK], float (&l)[QPK], float (&o)[QPK][8], int off) {
#pragma unroll
  for (int h = 0; h < QPK; ++h) {
    const float mo = __shfl_xor(m[h], off), lo = __shfl_xor(l[h], off);
    const float mn = fmaxf(m[h], mo);
    const float ca = __builtin_amdgcn_exp2f(m[h] - mn);  // m >= kMFloor: finite, never exp(-inf - -inf)
    const float cb = __builtin_amdgcn_exp2f(mo - mn);
    l[h] = __builtin_fmaf(l[h], ca, mul_rn(lo, cb));
#pragma unroll
    for (int i = 0; i < 8; ++i) o[h][i] = __builtin_fmaf(o[h][i], ca, mul_rn(__shfl_xor(o[h][i], off), cb));
    m[h] = mn;
  }
}

// The wave's merged state into LDS: smw / slw / sow are this wave's entries for the state's first head (row group 0
// stores)
template <int LPR, int QPK, int HS>
__device__ __forceinline__ void attn_stash(float* smw, float* slw, float (*sow)[HS], const float (&m)[QPK],
                                           const float (&l)[QPK], const float (&o)[QPK][8], int lane) {
  if (lane >= LPR) return;
  const int sub = lane % LPR;
#pragma unroll
  for (int h = 0; h < QPK; ++h) {
    if (lane == 0) {
      smw[h] = m[h];
      slw[h] = l[h];
    }
    *(float4*)&sow[h][sub * 8] = make_float4(o[h][0], o[h][1], o[h][2], o[h][3]);
    *(float4*)&sow[h][sub * 8 + 4] = make_float4(o[h][4], o[h][5], o[h][6], o[h][7]);
  }
}

// Block merge of one output quad: the NW waves' states of column c, output columns 4 dq .. 4 dq + 3, accumulated into
// (bm, bl, bo), which the caller starts at (-inf, 0, 0)
template <int NW, int NC, int HS>
__device__ __forceinline__ void attn_block_merge(const float (&sm)[NW][NC], const float (&sl)[NW][NC],
                                                 const float (&so)[NW][NC][HS], int c, int dq, float& bm, float& bl,
                                                 float (&bo)[4]) {
#pragma unroll
  for (int w = 0; w < NW; ++w) bm = fmaxf(bm, sm[w][c]);
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    const float cw = __builtin_amdgcn_exp2f(sm[w][c] - bm);
    bl = add_rn(bl, mul_rn(sl[w][c], cw));
    const float4 ov = *(const float4*)&so[w][c][dq * 4];
    bo[0] = __builtin_fmaf(ov.x, cw, bo[0]);
    bo[1] = __builtin_fmaf(ov.y, cw, bo[1]);
    bo[2] = __builtin_fmaf(ov.z, cw, bo[2]);
    bo[3] = __builtin_fmaf(ov.w, cw, bo[3]);
  }
}

// the normalised quad as 4 bf16 (the one division of the softmax)
__device__ __forceinline__ void attn_store_quad(uint16_t* yr, const float (&o4)[4], float l) {
  *(uint2*)yr = make_uint2(pack2(o4[0] / l, o4[1] / l), pack2(o4[2] / l, o4[3] / l));
}

// The split partials of the QPK head rows from row0 on. Per (head row, split): {m, l, 0, 0, o[HS]} fp32
template <int HS, int QPK>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t attn_ws_rsrc(float* ws, size_t row0, int n_splits) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)(ws + row0 * n_splits * (HS + 4)), (short)0,
                                           QPK * n_splits * (HS + 4) * 4, 0x00020000);
}

// Publish one quad of (head hq, split): 16-B sc1 stores (MI355X_MICROARCH.md "Valid forms" row 1; the caller drains
// and counts)
template <int HS>
__device__ __forceinline__ void attn_publish(__amdgpu_buffer_rsrc_t wrs, int hq, int dq, int n_splits, int split,
                                             float bm, float bl, const float (&bo)[4]) {
  const unsigned off = (unsigned)((hq * n_splits + split) * (HS + 4)) * 4;
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, make_float4(bo[0], bo[1], bo[2], bo[3])), wrs,
                                         off + 16 + dq * 16, 0, 16);
  if (dq == 0)
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, make_float4(bm, bl, 0.0f, 0.0f)), wrs, off, 0,
                                           16);
}

// The last arriver's combine of one quad over all splits into head row `row` of y: 8 splits per round with every load of the round in
// flight at once (sc1) and an online rescale across rounds. Split 0 always holds key 0, so the running max is finite
// after round 0; empty splits carry m = kMFloor, l = 0, o = 0 and clamped out-of-range slots are forced to m = -inf:
// both weigh 0.
template <int HS>
__device__ __forceinline__ void attn_combine(__amdgpu_buffer_rsrc_t wrs, int hq, int dq, int n_splits, uint16_t* y,
                                             size_t row) {
  const unsigned hoff = (unsigned)(hq * n_splits * (HS + 4)) * 4;
  float mx = -INFINITY, lt = 0.0f, ot[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int s0 = 0; s0 < n_splits; s0 += 8) {
    float4 ml[8], o4[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const unsigned off = hoff + (unsigned)(min(s0 + u, n_splits - 1) * (HS + 4)) * 4;
      ml[u] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(wrs, off, 0, 16));
      o4[u] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(wrs, off + 16 + dq * 16, 0, 16));
    }
    float nm = mx;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (s0 + u >= n_splits) ml[u].x = -INFINITY;
      nm = fmaxf(nm, ml[u].x);
    }
    const float c = __builtin_amdgcn_exp2f(mx - nm);  // round 0: exp(-inf) = 0
    lt = mul_rn(lt, c);
#pragma unroll
    for (int i = 0; i < 4; ++i) ot[i] = mul_rn(ot[i], c);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const float e = __builtin_amdgcn_exp2f(ml[u].x - nm);
      lt = __builtin_fmaf(ml[u].y, e, lt);
      ot[0] = __builtin_fmaf(o4[u].x, e, ot[0]);
      ot[1] = __builtin_fmaf(o4[u].y, e, ot[1]);
      ot[2] = __builtin_fmaf(o4[u].z, e, ot[2]);
      ot[3] = __builtin_fmaf(o4[u].w, e, ot[3]);
    }
    mx = nm;
  }
  attn_store_quad(y + row * HS + dq * 4, ot, lt);
}

// An idle row (batch / shared forms): the split-0 workgroups zero their QPK heads of y, nothing else is touched
template <int HS, int QPK>
__device__ __forceinline__ void attn_zero_idle(uint16_t* y_slice, int split) {
  if (split == 0 && threadIdx.x < QPK * HS / 4) *(uint2*)(y_slice + threadIdx.x * 4) = make_uint2(0u, 0u);
}

}  // namespace lga
