// Cached causal attention for decode (T = 1, split over the sequence) and prefill (T rows).
//
// Replaces CausalSelfAttention.scaled_dot_product_attention (lit_gpt/model.py:651, :658-665): SDPA of q
// against the full max_seq-long cache under the bool mask row(s) selected by input_pos (model.py:509). The
// mask allows key j for query t iff j <= input_pos[t]; this kernel reads only those keys.
//
// KV cache layout (HBM): k, v = [G][max_seq][hs] bf16 per layer (un-expanded query groups); one key row is
// hs*2 contiguous bytes, read by a "row group" of hs/8 lanes at 16 B per lane.
//
// Work decomposition: grid (splits, G, T); a 256-thread workgroup owns one (split, query group, query row) and
// all q_per_kv heads of that group (GQA/MQA read each K/V row once). The split boundaries are computed in the
// kernel from the live position (chunk = ceil((p+1)/splits)), so every split is busy whatever the context
// length and a captured HIP graph stays valid as p grows. Inside, each row group streams UNR keys per step
// (2*UNR 16-B loads in flight per lane) with an online softmax; row groups merge with shuffles, waves via LDS.
// With splits > 1 every workgroup publishes (m, l, o) write-through (sc1) and bumps a per-(t, group) counter;
// the workgroup that arrives last merges the splits and writes the bf16 output (flash-decoding combine inside
// the same launch; MI355X_MICROARCH.md "Valid forms" row 1), then re-arms the counter for the next launch.
#include <cstdlib>

#include "attn_core.h"

namespace lga {

#ifndef LGA_ATTN_PIPE
#define LGA_ATTN_PIPE 1
#endif

#ifdef LGA_ATTN_TRACE  // lab builds only (tools/attn_trace.py): per-block phase timestamps, 100 MHz clock
__device__ unsigned long long g_attn_trace[8192 * 8];
#define LGA_TRACE(i)                                                                            \
  do {                                                                                          \
    if (threadIdx.x == 0) {                                                                     \
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                              \
      g_attn_trace[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 8 + (i)] = __builtin_amdgcn_s_memrealtime(); \
    }                                                                                           \
  } while (0)
#else
#define LGA_TRACE(i) \
  do {               \
  } while (0)
#endif

// per-(t, group) arrival counters sit 256 B apart: same-line device-scope atomics serialize
constexpr int kCounterStride = 64;

// K/V rows are streamed once per step (the next step's re-read comes after ~1 GB of other traffic): nt loads
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
// (NT = false, the window kernel: the M rows of a verify window read the same K/V, so all but one read is a re-read)
template <bool NT = true>
__device__ __forceinline__ uint4 ld_kv(const uint16_t* p) {
  if constexpr (!NT) return *(const uint4*)p;
  const u32x4_t v = __builtin_nontemporal_load((const u32x4_t*)p);
  return make_uint4(v.x, v.y, v.z, v.w);
}

// KV8 (fp8 caches): a key / value row is HS e4m3 codes (8 B per lane of the same HS / 8-lane row group)
// plus one fp32 power-of-two scale; the codes expand to packed bf16 (K, for the same v_dot2 chain) and fp32 (V) in
// registers, unscaled: the row's scale multiplies the score, s_j (q . k8_j), and the P.V weight, e sv_j — exact, so
// the arithmetic is the bf16 cache's on the dequantized values.
template <bool NT = true>
__device__ __forceinline__ uint2 ld_kv8(const uint8_t* p) {
  typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
  if constexpr (!NT) return *(const uint2*)p;
  const u32x2_t v = __builtin_nontemporal_load((const u32x2_t*)p);
  return make_uint2(v.x, v.y);
}

// FUSED (decode, T = 1): q, k, v come straight from the qkv projection row; every workgroup ropes its group's
// q heads itself, and the workgroup whose split owns the new position p ropes k, appends k and v to the cache
// at p (KVCache.forward, lit_gpt/model.py:788-795) and scores that key from registers — replacing the separate
// lga_rope_kv_append launch of the decode step.
#ifndef LGA_ATTN_SOLO
#define LGA_ATTN_SOLO 1  // lab A/B: 0 = the workgroup-barrier publish for every slice width
#endif
// WINDOW (speculative verify, lga_attention_decode_window): FUSED for M rows of ONE sequence at consecutive positions;
// grid.z = row r, whose position (cache and rope) is input_pos[0] + r and whose qkv row is row r of q. Every
// workgroup is the T = 1 FUSED workgroup of its row — the row's own split boundaries, its own key scored last from
// registers by row group 0 of the owning split, the same merges and combine — so y[r] has the bits of the one-row
// launch at that position. The one difference: the roped k / v of ALL M rows are appended by window_append_kernel
// in a launch of its own BEFORE this one (row r reads the keys of rows 0..r-1 from the cache, and other workgroups
// of this launch own those positions: no store here may be depended on), so the owning workgroup does not store.
#ifndef LGA_ATTN_WIN_NT
#define LGA_ATTN_WIN_NT 0  // lab A/B: 1 = the one-row kernel's nt loads in the window kernel too
#endif

// BATCH (batched decode, lga_attention_decode_batch): B independent T = 1 FUSED workgroup sets in one launch; grid.z =
// sequence b, with its own qkv row, its own position (input_pos[b], rope_pos[b]), its own cache slot (k / v + b *
// slot_stride elements, the fp8 scale rows + b * scale_slot_stride) and its own append, exactly the one-row form's:
// no row reads what another row writes, so unlike WINDOW there is no separate append launch. Workspace and counters
// are indexed by t = b as for any multi-row launch. A row with active[b] == 0 is idle: every one of its workgroups
// returns before any K/V load, store, workspace write or counter add (the test is uniform per workgroup and sits ahead
// of every barrier, so the counter protocol of the other rows is untouched), the split-0 workgroups having zeroed
// their heads of y[b].
template <int HS, int QPK, int UNR, int NW, bool FUSED, bool PIPE, bool WINDOW = false, bool KV8 = false,
          bool BATCH = false>
__device__ __forceinline__ void attn_body(const uint16_t* __restrict__ q, uint16_t* __restrict__ kc,
                                          uint16_t* __restrict__ vc, const int64_t* __restrict__ input_pos,
                                          uint16_t* __restrict__ y, float* __restrict__ ws,
                                          unsigned* __restrict__ cnt, int n_head, int max_seq, float scale,
                                          const int64_t* __restrict__ rope_pos, const float* __restrict__ cos,
                                          const float* __restrict__ sin, int rope_rows, int hsplit,
                                          float* __restrict__ ksc = nullptr, float* __restrict__ vsc = nullptr,
                                          long slot_stride = 0, long scale_slot_stride = 0,
                                          const int* __restrict__ active = nullptr) {
  static_assert(!KV8 || (FUSED && HS == 128), "the fp8 cache serves the fused decode forms");
  static_assert(!BATCH || (FUSED && !WINDOW), "the batch form is the fused one-row form per sequence");
  constexpr int LPR = HS / 8;    // lanes per key row
  constexpr int RGW = 64 / LPR;  // row groups per wave
  constexpr int RG = NW * RGW;   // row groups per workgroup
  constexpr int NT = NW * 64;
  // blockIdx.y = (query group, head slice): with hsplit > 1 the group's QPKT heads are dealt to hsplit workgroups of
  // QPK heads each (few groups per rank: more workgroups per launch, each doing less per key)
  const int split = blockIdx.x, gy = blockIdx.y, t = blockIdx.z;
  const int g = gy / hsplit, hsi = gy % hsplit, QPKT = QPK * hsplit;
  const int n_splits = gridDim.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int rg = wave * RGW + lane / LPR;
  const int sub = lane % LPR;
  LGA_TRACE(0);
  // The two position loads sit side by side here, but hipcc does not emit them as one round trip: the wave waits for
  // the kernarg block, then for input_pos, then issues rope_pos behind a second wait, and the q and cos/sin loads
  // follow. Taking the positions, q and the RoPE tables as leading (preloaded) kernel arguments and loading q beside
  // the positions leaves one scalar wait ahead of the cos/sin loads; measured, that is 0.1 us of 10.5 per launch, inside
  // twice the A/B's own spread, so it is not in the product (profiles/attn_launch_head_ab.txt).
  static_assert(!WINDOW || FUSED, "the window form is the fused form per row");
  const long p = WINDOW ? input_pos[0] + t : input_pos[t];
  const long rp_raw = WINDOW ? p : (FUSED ? rope_pos[t] : 0);
  if (WINDOW || BATCH) q += (size_t)t * (n_head + 2 * (gridDim.y / hsplit)) * HS;  // row t of the (M, (H + 2G) hs) qkv
  if constexpr (BATCH) {
    if (active != nullptr && active[t] == 0) {  // idle row: zero y[t] (split 0), touch nothing else
      attn_zero_idle<HS, QPK>(y + ((size_t)t * n_head + (size_t)g * QPKT + hsi * QPK) * HS, split);
      return;
    }
    // sequence t's slot: KV8 codes are bytes behind the uint16_t pointers, bf16 rows are elements
    kc = KV8 ? (uint16_t*)((uint8_t*)kc + (size_t)t * slot_stride) : kc + (size_t)t * slot_stride;
    vc = KV8 ? (uint16_t*)((uint8_t*)vc + (size_t)t * slot_stride) : vc + (size_t)t * slot_stride;
    if constexpr (KV8) {
      ksc += (size_t)t * scale_slot_stride;
      vsc += (size_t)t * scale_slot_stride;
    }
  }
  const attn_range sp = attn_split_range<FUSED>(p, max_seq, n_splits, split);
  const int k_lo = sp.k_lo, k_end = sp.k_end;
  LGA_TRACE(1);
  const float* cr = nullptr;
  const float* sr = nullptr;
  if (FUSED) {
    const long rp = min(max(rp_raw, 0L), (long)rope_rows - 1);
    cr = cos + (size_t)rp * HS + sub * 8;
    sr = sin + (size_t)rp * HS + sub * 8;
  }
  const uint16_t* kbase = kc + (size_t)g * max_seq * HS + sub * 8;
  const uint16_t* vbase = vc + (size_t)g * max_seq * HS + sub * 8;
  // (KV8: the same element offsets in bytes, and the group's scale rows)
  const uint8_t* kbase8 = (const uint8_t*)kc + (size_t)g * max_seq * HS + sub * 8;
  const uint8_t* vbase8 = (const uint8_t*)vc + (size_t)g * max_seq * HS + sub * 8;
  const float* ksg = KV8 ? ksc + (size_t)g * max_seq : nullptr;
  const float* vsg = KV8 ? vsc + (size_t)g * max_seq : nullptr;
  // clamped duplicate rows (past k_end) are masked in attn_step() and hit in cache
  auto fetch = [&](kv_regs<KV8> (&kv)[UNR], kv_regs<KV8> (&vv)[UNR], int j0) {
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int j = max(min(j0 + u * RG, k_end - 1), 0);
      if constexpr (KV8) {
        kv[u].d = ld_kv8<!WINDOW || LGA_ATTN_WIN_NT>(kbase8 + (size_t)j * HS);
        vv[u].d = ld_kv8<!WINDOW || LGA_ATTN_WIN_NT>(vbase8 + (size_t)j * HS);
        kv[u].s = ksg[j];
        vv[u].s = vsg[j];
      } else {
        kv[u].d = ld_kv<!WINDOW || LGA_ATTN_WIN_NT>(kbase + (size_t)j * HS);
        vv[u].d = ld_kv<!WINDOW || LGA_ATTN_WIN_NT>(vbase + (size_t)j * HS);
      }
    }
  };
  const int j_first = k_lo + rg;

  // the q rows and the RoPE tables, then the first K/V batch (an empty split's batch re-reads row 0 and is never
  // consumed)
  uint4 qraw[QPK];
#pragma unroll
  for (int h = 0; h < QPK; ++h) {
    if (FUSED)  // qkv row layout per group: [q_0 .. q_{QPK-1}, k, v] x HS (scripts/convert_hf_checkpoint.py:181-187)
      qraw[h] = *(const uint4*)(q + ((size_t)g * (QPKT + 2) + hsi * QPK + h) * HS + sub * 8);
    else
      qraw[h] = *(const uint4*)(q + ((size_t)t * n_head + (size_t)g * QPKT + hsi * QPK + h) * HS + sub * 8);
  }
  float cs[FUSED ? 8 : 1], sn[FUSED ? 8 : 1];
  if (FUSED) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      cs[i] = cr[i];
      sn[i] = sr[i];
    }
  }
  uint4 qp[QPK];  // q stays packed bf16 (attn_dot8)
#pragma unroll
  for (int h = 0; h < QPK; ++h) qp[h] = FUSED ? rope8(qraw[h], cs, sn, sub) : qraw[h];
  // the online softmax runs in log2 units (as the prefill's flash attention): scores scaled by scale * log2(e), every
  // exponential one v_exp_f32 (exp2) instead of expf's 12-instruction range reduction — the long-context launches are
  // VALU-bound (tools/attn_pmc.py: Mixtral at p = 32066, the waves VALU-active 40 % of their cycles, 2 per SIMD);
  // the partials' m is in log2 units too (only this kernel's combine reads it)
  const float sl2 = scale * 1.4426950408889634f;
  // the first K/V batch AFTER the RoPE: issued beside q (ahead of the RoPE's wait) every split's first loads leave
  // in one burst at kernel start, measured 0.25-0.3 us slower per launch (tools/attn_ab.py, round 5)
  __builtin_amdgcn_sched_barrier(0);
  kv_regs<KV8> ka[UNR], va[UNR], kb[UNR], vb[UNR];
  if (PIPE) fetch(ka, va, j_first);
  LGA_TRACE(2);
  float m[QPK], l[QPK], o[QPK][8];
#pragma unroll
  for (int h = 0; h < QPK; ++h) {
    m[h] = kMFloor;
    l[h] = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[h][i] = 0.0f;
  }
  auto consume = [&](const kv_regs<KV8> (&kv)[UNR], const kv_regs<KV8> (&vv)[UNR], int j0) {
    attn_step<LPR, QPK, UNR, RG, KV8>(m, l, o, qp, kv, vv, j0, k_end, sl2);
  };
  if (PIPE) {
    // software pipeline: step i + 1's 2*UNR loads are issued before step i's math, so every row group keeps 2-4
    // steps of K/V in flight and a split costs one load round trip plus its streaming time (the first batch was
    // issued above, next to q)
    const int stp = RG * UNR;
    const int nst = k_end > k_lo ? (k_end - k_lo + stp - 1) / stp : 0;
    int i = 0;
    for (; i + 1 < nst; i += 2) {
      fetch(kb, vb, j_first + (i + 1) * stp);
      consume(ka, va, j_first + i * stp);
      if (i + 2 < nst) fetch(ka, va, j_first + (i + 2) * stp);
      consume(kb, vb, j_first + (i + 1) * stp);
    }
    if (i < nst) consume(ka, va, j_first + i * stp);
  } else {
    for (int j0 = j_first; j0 < k_end; j0 += RG * UNR) {
      fetch(ka, va, j0);
      consume(ka, va, j0);
    }
  }
  LGA_TRACE(3);
  if (FUSED && sp.owns_new && rg == 0) {  // the new key/value: rope k, append both to the cache, score from registers
    const uint16_t* kvrow = q + ((size_t)g * (QPKT + 2) + QPKT) * HS + sub * 8;
    uint4 kr = rope8(*(const uint4*)kvrow, cs, sn, sub);
    const uint4 vr = *(const uint4*)(kvrow + HS);
    float vf[8];
    float ksn = 1.0f, vsn = 1.0f;  // KV8: the new row's scales
    if constexpr (KV8) {
      // the row is scored as the cache holds it: quantized here (every head slice; the row group is whole), its codes
      // expanded again for the score
      const uint2 k8 = kv8_quantize8(kr, ksn), v8 = kv8_quantize8(vr, vsn);
      if (!WINDOW && hsi == 0) {  // one head slice appends
        *(uint2*)((uint8_t*)kc + ((size_t)g * max_seq + p) * HS + sub * 8) = k8;
        *(uint2*)((uint8_t*)vc + ((size_t)g * max_seq + p) * HS + sub * 8) = v8;
        if (sub == 0) {
          ksc[(size_t)g * max_seq + p] = ksn;
          vsc[(size_t)g * max_seq + p] = vsn;
        }
      }
      kr = kv8_bf16x8(k8);
      kv8_f32x8(v8, vf);
    } else {
      if (!WINDOW && hsi == 0) {  // one head slice appends; the others score the same key from their registers
        *(uint4*)(kc + ((size_t)g * max_seq + p) * HS + sub * 8) = kr;
        *(uint4*)(vc + ((size_t)g * max_seq + p) * HS + sub * 8) = vr;
      }
      unpack8(vr, vf);
    }
    attn_new_key<LPR, QPK, KV8>(m, l, o, qp, kr, vf, ksn, vsn, sl2);
  }
  // merge the RGW row groups of this wave (lanes differing in the bits above log2(LPR))
#pragma unroll
  for (int off = LPR; off < 64; off <<= 1) attn_wave_merge<QPK>(m, l, o, off);
  __shared__ float sm[NW][QPK], sl[NW][QPK];
  __shared__ __attribute__((aligned(16))) float so[NW][QPK][HS];
  __shared__ unsigned s_ticket;
  attn_stash<LPR>(sm[wave], sl[wave], so[wave], m, l, o, lane);
  __syncthreads();
  // block merge: a thread owns 4 consecutive output columns (h, 4 dq .. 4 dq + 3) of one head of the slice
  constexpr int NQ = QPK * HS / 4;
  static_assert(NQ <= NT, "one 4-column item per thread");
  const bool has_item = threadIdx.x < NQ;
  const int hq = threadIdx.x / (HS / 4), dq = threadIdx.x % (HS / 4);
  float bm = -INFINITY, bl = 0.0f, bo[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (has_item) attn_block_merge(sm, sl, so, hq, dq, bm, bl, bo);
  const size_t row0 = (size_t)t * n_head + (size_t)g * QPKT + hsi * QPK;  // first head row of this slice
  if (n_splits == 1) {
    if (has_item) attn_store_quad(y + (row0 + hq) * HS + dq * 4, bo, bl);
    return;
  }
  LGA_TRACE(4);
  // ---- publish (m, l, o), then the last-arriving split of this (t, group) merges all splits (MI355X_MICROARCH.md
  // "Valid forms" row 1: 16-B sc1 stores, every storing wave drains, a workgroup barrier, one lane's agent-scope
  // add; the last arriver's loads are sc1 too) ----
  // SOLO: every output quad sits in wave 0 (QPK * HS / 4 <= 64), so wave 0 alone stores, drains, counts and, when
  // last, combines: the same row-1 form with one storing wave, no workgroup barrier or LDS ticket on the tail
  constexpr bool SOLO = LGA_ATTN_SOLO && NQ <= 64;
  if (SOLO && wave != 0) return;
  const __amdgpu_buffer_rsrc_t wrs = attn_ws_rsrc<HS, QPK>(ws, row0, n_splits);
  if (has_item) attn_publish<HS>(wrs, hq, dq, n_splits, split, bm, bl, bo);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  unsigned* ctr = cnt + ((size_t)t * gridDim.y + gy) * kCounterStride;
  unsigned ticket;
  if constexpr (SOLO) {
    unsigned tk = 0;
    if (lane == 0) tk = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ticket = __builtin_amdgcn_readfirstlane(tk);  // lane 0's
  } else {
    __syncthreads();
    if (threadIdx.x == 0) s_ticket = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    ticket = s_ticket;
  }
  LGA_TRACE(5);
  if (ticket != (unsigned)(n_splits - 1)) return;
  if (has_item) attn_combine<HS>(wrs, hq, dq, n_splits, y, row0 + hq);  // one quad per thread
  if (threadIdx.x == 0) __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm
  LGA_TRACE(6);
}

// (BATCH sits ahead of FUSED: the mangled names of the other forms keep their <.., FUSED, PIPE, WINDOW> tail)
template <int HS, int QPK, int UNR, int NW, bool BATCH, bool FUSED, bool PIPE, bool WINDOW = false>
__global__ void __launch_bounds__(NW * 64) attn_kernel(const uint16_t* __restrict__ q, uint16_t* __restrict__ kc,
                                                   uint16_t* __restrict__ vc, const int64_t* __restrict__ input_pos,
                                                   uint16_t* __restrict__ y, float* __restrict__ ws,
                                                   unsigned* __restrict__ cnt, int n_head, int max_seq, float scale,
                                                   const int64_t* __restrict__ rope_pos, const float* __restrict__ cos,
                                                   const float* __restrict__ sin, int rope_rows, int hsplit,
                                                   long slot_stride, const int* __restrict__ active) {
  attn_body<HS, QPK, UNR, NW, FUSED, PIPE, WINDOW, false, BATCH>(q, kc, vc, input_pos, y, ws, cnt, n_head, max_seq,
                                                                 scale, rope_pos, cos, sin, rope_rows, hsplit, nullptr,
                                                                 nullptr, slot_stride, 0, active);
}

// the fp8-cache instantiations (FUSED one-row, WINDOW and BATCH): attn_kernel plus the two scale arrays
template <int HS, int QPK, int UNR, int NW, bool BATCH, bool PIPE, bool WINDOW>
__global__ void __launch_bounds__(NW * 64) attn_kernel_kv8(const uint16_t* __restrict__ q, uint8_t* __restrict__ kc,
                                                       uint8_t* __restrict__ vc, float* __restrict__ ksc,
                                                       float* __restrict__ vsc, const int64_t* __restrict__ input_pos,
                                                       uint16_t* __restrict__ y, float* __restrict__ ws,
                                                       unsigned* __restrict__ cnt, int n_head, int max_seq, float scale,
                                                       const int64_t* __restrict__ rope_pos,
                                                       const float* __restrict__ cos, const float* __restrict__ sin,
                                                       int rope_rows, int hsplit, long slot_stride,
                                                       long scale_slot_stride, const int* __restrict__ active) {
  attn_body<HS, QPK, UNR, NW, true, PIPE, WINDOW, true, BATCH>(q, (uint16_t*)kc, (uint16_t*)vc, input_pos, y, ws, cnt,
                                                               n_head, max_seq, scale, rope_pos, cos, sin, rope_rows,
                                                               hsplit, ksc, vsc, slot_stride, scale_slot_stride,
                                                               active);
}

// SHARED (n samples of one prompt, lga_attention_decode_shared): the BATCH form for B rows that sit at ONE position p
// = pos[0] and share the keys j < P = min(max(prefix_len[0], 0), p), which only slot 0 holds. grid.z = a set of R
// rows; the workgroup carries R x QPK independent (m, l, o) states, one per (row, head) pair, and every pair runs the
// op sequence of its T = 1 FUSED workgroup: the split bounds of p (one for all rows), the same key -> row group ->
// step assignment and masks, steps in ascending order, the row's own new key last from registers, the same row-group /
// wave merges, publish and combine with workspace and counters indexed by t = b. What differs is who loads: a step
// whose UNR x RG keys all lie below P is loaded ONCE from slot 0 and consumed by every pair; a step that straddles or
// lies past P is taken per row, keys < P from slot 0 and keys >= P from slot b (the same values as a slot b that held
// the prefix, so the same bits). All steps of the workgroup, shared ones first, then (row, step) in row order, form one
// pipelined item sequence: item n sits in ka / va (n even) or kb / vb (n odd) and item n + 1's loads are issued
// ahead of item n's math, across the change of row too. No state passes between workgroups. Idle rows (active[b] ==
// 0, or b >= B in the last set) are skipped; a set with no active row returns as the batch form's idle row does.
// The arithmetic of a pair is attn_body's because it is the same code: both kernels call the one softmax core
// (attn_core.h), whose every multiply-add is an explicit fma / mul_rn / add_rn, so no compiler choice can part them.
// (Left to -ffp-contract, this body's other shape once had two of them fused differently — the wave merge's l, the
// block merge's bl: one ulp apart, one output element in thousands.) tests/test_gpu_shared_attention.py holds the bits.
template <int HS, int QPK, int UNR, int NW, int R>
__global__ void __launch_bounds__(NW * 64)
    attn_shared_kernel(const uint16_t* __restrict__ q, uint16_t* __restrict__ kc, uint16_t* __restrict__ vc,
                       const int64_t* __restrict__ pos, const int64_t* __restrict__ prefix_len,
                       uint16_t* __restrict__ y, float* __restrict__ ws, unsigned* __restrict__ cnt, int n_head,
                       int max_seq, float scale, const float* __restrict__ cos, const float* __restrict__ sin,
                       int rope_rows, int hsplit, long slot_stride, const int* __restrict__ active, int B) {
  constexpr int LPR = HS / 8;
  constexpr int RGW = 64 / LPR;
  constexpr int RG = NW * RGW;
  constexpr int NT = NW * 64;
  constexpr int NP = R * QPK;  // pairs
  const int split = blockIdx.x, gy = blockIdx.y, b0 = blockIdx.z * R;
  const int g = gy / hsplit, hsi = gy % hsplit, QPKT = QPK * hsplit;
  const int n_splits = gridDim.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int rg = wave * RGW + lane / LPR;
  const int sub = lane % LPR;
  const long p = pos[0];
  const long pfx = min(max(prefix_len[0], 0L), p);
  const size_t qkv_row = (size_t)(n_head + 2 * (gridDim.y / hsplit)) * HS;
  unsigned am = 0;  // the active rows of this set, bit r = row b0 + r
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int b = b0 + r;
    if (b >= B) continue;
    if (active == nullptr || active[b] != 0) {
      am |= 1u << r;
    } else {  // idle row: zero y[b] (split 0), touch nothing else
      attn_zero_idle<HS, QPK>(y + ((size_t)b * n_head + (size_t)g * QPKT + hsi * QPK) * HS, split);
    }
  }
  if (am == 0) return;
  const attn_range sp = attn_split_range<true>(p, max_seq, n_splits, split);  // (key p is scored from registers)
  const int k_lo = sp.k_lo, k_end = sp.k_end;
  const int P = (int)min(pfx, (long)max_seq);  // (keys at or past max_seq are never loaded)
  const long rp = min(max(p, 0L), (long)rope_rows - 1);
  const float* cr = cos + (size_t)rp * HS + sub * 8;
  const float* sr = sin + (size_t)rp * HS + sub * 8;
  const uint16_t* kbase = kc + (size_t)g * max_seq * HS + sub * 8;  // slot 0
  const uint16_t* vbase = vc + (size_t)g * max_seq * HS + sub * 8;
  // one item's loads: key j comes from slot 0 below P, else from the slot `own` elements on (a shared step passes 0);
  // clamped duplicate rows (past k_end) are masked in attn_step() and hit in cache
  auto fetch = [&](kv_regs<false> (&kv)[UNR], kv_regs<false> (&vv)[UNR], int j0, size_t own) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int j = max(min(j0 + u * RG, k_end - 1), 0);
      const size_t at = (j < P ? (size_t)0 : own) + (size_t)j * HS;
      kv[u].d = ld_kv(kbase + at);
      vv[u].d = ld_kv(vbase + at);
    }
  };
  const int j_first = k_lo + rg;

  uint4 qraw[R][QPK];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int h = 0; h < QPK; ++h) {
      qraw[r][h] = make_uint4(0u, 0u, 0u, 0u);
      if (am >> r & 1)
        qraw[r][h] = *(const uint4*)(q + (size_t)(b0 + r) * qkv_row + ((size_t)g * (QPKT + 2) + hsi * QPK + h) * HS +
                                     sub * 8);
    }
  float cs[8], sn[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    cs[i] = cr[i];
    sn[i] = sr[i];
  }
  uint4 qp[R][QPK];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int h = 0; h < QPK; ++h) qp[r][h] = rope8(qraw[r][h], cs, sn, sub);
  const float sl2 = scale * 1.4426950408889634f;
  // the item sequence: ns shared steps, then the nown own steps of every active row
  const int stp = RG * UNR;
  const int nst = k_end > k_lo ? (k_end - k_lo + stp - 1) / stp : 0;
  const int ns = min(max(P - k_lo, 0) / stp, nst);  // steps i with k_lo + (i + 1) stp <= P
  const int nown = nst - ns;
  const int r_first = __builtin_ctz(am);
  auto own_of = [&](int r) { return (size_t)(b0 + r) * (size_t)slot_stride; };
  __builtin_amdgcn_sched_barrier(0);
  kv_regs<false> ka[UNR], va[UNR], kb[UNR], vb[UNR];
  if (ns > 0) fetch(ka, va, j_first, 0);
  else if (nown > 0) fetch(ka, va, j_first, own_of(r_first));
  float m[R][QPK], l[R][QPK], o[R][QPK][8];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int h = 0; h < QPK; ++h) {
      m[r][h] = kMFloor;
      l[r][h] = 0.0f;
#pragma unroll
      for (int i = 0; i < 8; ++i) o[r][h][i] = 0.0f;
    }
  // one step of one row: attn_body's, on that row's QPK states
  auto consume = [&](int r, const kv_regs<false> (&kv)[UNR], const kv_regs<false> (&vv)[UNR], int j0)
                     __attribute__((always_inline)) {
    attn_step<LPR, QPK, UNR, RG, false>(m[r], l[r], o[r], qp[r], kv, vv, j0, k_end, sl2);
  };
  int n = 0;  // items consumed so far
  // item n: issue the next item's loads (if any) into the other buffer, then the math `use` on item n's
  auto item = [&](bool has_next, int j0_next, size_t own_next, auto&& use) __attribute__((always_inline)) {
    if (n & 1) {
      if (has_next) fetch(ka, va, j0_next, own_next);
      use(kb, vb);
    } else {
      if (has_next) fetch(kb, vb, j0_next, own_next);
      use(ka, va);
    }
    ++n;
  };
  for (int i = 0; i < ns; ++i) {
    const bool more = i + 1 < ns;
    const int j0 = j_first + i * stp;
    item(more || nown > 0, j0 + stp, more ? (size_t)0 : own_of(r_first),
         [&](const kv_regs<false>(&kv)[UNR], const kv_regs<false>(&vv)[UNR]) __attribute__((always_inline)) {
#pragma unroll
           for (int r = 0; r < R; ++r)
             if (am >> r & 1) consume(r, kv, vv, j0);
         });
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (!(am >> r & 1)) continue;
    const unsigned rest = r + 1 < R ? am >> (r + 1) : 0u;
    const int r_next = rest ? r + 1 + __builtin_ctz(rest) : -1;
    for (int i = ns; i < nst; ++i) {
      const bool more = i + 1 < nst;
      const int j0 = j_first + i * stp;
      item(more || r_next >= 0, j_first + (more ? i + 1 : ns) * stp, own_of(more ? r : max(r_next, 0)),
           [&](const kv_regs<false>(&kv)[UNR], const kv_regs<false>(&vv)[UNR]) __attribute__((always_inline)) {
             consume(r, kv, vv, j0);
           });
    }
  }
  if (sp.owns_new && rg == 0) {  // every row's new key/value: rope k, append both to slot b, score from registers
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (!(am >> r & 1)) continue;
      const uint16_t* kvrow = q + (size_t)(b0 + r) * qkv_row + ((size_t)g * (QPKT + 2) + QPKT) * HS + sub * 8;
      const uint4 kr = rope8(*(const uint4*)kvrow, cs, sn, sub);
      const uint4 vr = *(const uint4*)(kvrow + HS);
      if (hsi == 0) {  // one head slice appends; the others score the same key from their registers
        *(uint4*)(kc + own_of(r) + ((size_t)g * max_seq + p) * HS + sub * 8) = kr;
        *(uint4*)(vc + own_of(r) + ((size_t)g * max_seq + p) * HS + sub * 8) = vr;
      }
      float vf[8];
      unpack8(vr, vf);
      attn_new_key<LPR, QPK, false>(m[r], l[r], o[r], qp[r], kr, vf, 1.0f, 1.0f, sl2);
    }
  }
  // merge the RGW row groups of this wave, pair by pair
#pragma unroll
  for (int off = LPR; off < 64; off <<= 1) {
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (am >> r & 1) attn_wave_merge<QPK>(m[r], l[r], o[r], off);
  }
  __shared__ float sm[NW][NP], sl[NW][NP];
  __shared__ __attribute__((aligned(16))) float so[NW][NP][HS];
  __shared__ unsigned s_ticket[R];
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (am >> r & 1)
      attn_stash<LPR>(&sm[wave][r * QPK], &sl[wave][r * QPK], &so[wave][r * QPK], m[r], l[r], o[r], lane);
  __syncthreads();
  // block merge per row: a thread owns 4 consecutive output columns of one head of the slice, as in attn_body
  constexpr int NQ = QPK * HS / 4;
  static_assert(NQ <= NT, "one 4-column item per thread and row");
  constexpr bool SOLO = LGA_ATTN_SOLO && NQ <= 64;
  if (SOLO && wave != 0) return;  // (every item sits in wave 0)
  const bool has_item = threadIdx.x < NQ;
  const int hq = threadIdx.x / (HS / 4), dq = threadIdx.x % (HS / 4);
  const size_t slice0 = (size_t)g * QPKT + hsi * QPK;  // first head of this slice
  auto ws_rsrc = [&](int r) { return attn_ws_rsrc<HS, QPK>(ws, (size_t)(b0 + r) * n_head + slice0, n_splits); };
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (!(am >> r & 1) || !has_item) continue;
    float bm = -INFINITY, bl = 0.0f, bo[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    attn_block_merge(sm, sl, so, r * QPK + hq, dq, bm, bl, bo);
    if (n_splits == 1) attn_store_quad(y + ((size_t)(b0 + r) * n_head + slice0 + hq) * HS + dq * 4, bo, bl);
    else attn_publish<HS>(ws_rsrc(r), hq, dq, n_splits, split, bm, bl, bo);  // attn_body's layout, row t = b
  }
  if (n_splits == 1) return;
  // one drain for all rows' partials, then the rows' arrival counters side by side (thread r counts for row r): the
  // last-arriving split of a (row, group) combines that row
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  auto ctr_of = [&](int r) { return cnt + ((size_t)(b0 + r) * gridDim.y + gy) * kCounterStride; };
  unsigned tk = 0;
  if constexpr (!SOLO) __syncthreads();
  if (threadIdx.x < R && (am >> threadIdx.x & 1))
    tk = __hip_atomic_fetch_add(ctr_of(threadIdx.x), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if constexpr (!SOLO) {
    if (threadIdx.x < R) s_ticket[threadIdx.x] = tk;
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (!(am >> r & 1)) continue;
    const unsigned ticket = SOLO ? (unsigned)__builtin_amdgcn_readlane((int)tk, r) : s_ticket[r];
    if (ticket != (unsigned)(n_splits - 1)) continue;
    if (has_item) attn_combine<HS>(ws_rsrc(r), hq, dq, n_splits, y, (size_t)(b0 + r) * n_head + slice0 + hq);
    if (threadIdx.x == 0) __hip_atomic_store(ctr_of(r), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm
  }
}

// The window's KV-append: roped k and v of row r into cache row pos0[0] + r of every group, with the fused kernel's
// own rope8 (and, for fp8 caches, its kv8_quantize8) on the same operands: the same bits, codes and scales it stores
// at T = 1. Grid (G, M), one wave: lanes 0..HS/8-1 (row group 0) rope k, the next HS/8 (row group 1) carry v. A row
// at or past max_seq stores nothing. KV8: kc / vc hold e4m3 codes with one scale per row in ksc / vsc (else unused).
template <bool KV8>
__global__ void __launch_bounds__(64) window_append_kernel(const uint16_t* __restrict__ qkv, void* __restrict__ kc,
                                                          void* __restrict__ vc, float* __restrict__ ksc,
                                                          float* __restrict__ vsc, const int64_t* __restrict__ pos0,
                                                          const float* __restrict__ cos, const float* __restrict__ sin,
                                                          int rope_rows, int n_head, int max_seq) {
  constexpr int HS = 128, LPR = HS / 8;
  const int g = blockIdx.x, G = gridDim.x, r = blockIdx.y, qpk = n_head / G;
  const int lane = threadIdx.x, sub = lane % LPR;
  const long p = pos0[0] + r;
  if (lane >= 2 * LPR || p < 0 || p >= max_seq) return;
  const uint16_t* kvrow = qkv + ((size_t)r * (n_head + 2 * G) + (size_t)g * (qpk + 2) + qpk) * HS + sub * 8;
  const bool is_k = lane < LPR;
  uint4 x;
  if (is_k) {
    const long rp = min(max(p, 0L), (long)rope_rows - 1);
    float cs[8], sn[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      cs[i] = cos[(size_t)rp * HS + sub * 8 + i];
      sn[i] = sin[(size_t)rp * HS + sub * 8 + i];
    }
    x = rope8(*(const uint4*)kvrow, cs, sn, sub);
  } else {
    x = *(const uint4*)(kvrow + HS);
  }
  const size_t row = (size_t)g * max_seq + p;
  if constexpr (KV8) {
    float s;
    const uint2 c8 = kv8_quantize8(x, s);
    *(uint2*)((uint8_t*)(is_k ? kc : vc) + row * HS + sub * 8) = c8;
    if (sub == 0) (is_k ? ksc : vsc)[row] = s;
  } else {
    *(uint4*)((uint16_t*)(is_k ? kc : vc) + row * HS + sub * 8) = x;
  }
}

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

// ---------------------------------------------------------------------------------------------------------------
// Prefill (T >= 16): flash attention on MFMA, swapped form (attn_prefill_pair_kernel). A wave owns 32 query rows of
// one head; key tiles of 64 rows stream through LDS. Per 32-key half-tile, S^T = K . Q^T on v_mfma_f32_32x32x16_bf16
// (A = K rows from LDS, B = this wave's Q^T held in registers), so lane l holds the scores of ONE query (l % 32)
// for 16 keys and its partner lane l ^ 32 the other 16: the online-softmax max / sum are in-lane chains plus one
// exchange. P goes to bf16 in registers and two v_permlane32_swap per 16 keys regroup it into the B operand of
// O^T += V^T . P^T, whose A operand comes straight from the row-major V image by ds_read_b64_tr_b16 (transposed
// LDS read) — no P or V^T round trip through LDS. O^T's lane also owns one query, so the rescale by
// exp(m_old - m_new) is a per-lane scalar, skipped when no row max of the wave moved. Causal masking only on the
// tiles that cross a row's position (a 32-bit compare + select per element, on those tiles only); the scores stay
// raw — the max runs on them and one fma(s, scale log2 e, -m) per element feeds v_exp_f32 (max(s) c == max(s c) for
// c > 0). Every LDS address is a per-lane base plus a compile-time offset.
// This per-wave arithmetic is round 3's (a 4-wave workgroup per 128-row query block, K / V register-staged through a
// double-buffered LDS image; no longer in the tree): Llama-2-7B, T = 2048, 64-65 us per layer =
// 529-540 TFLOP/s causal, 652-667 TFLOP/s with every row seeing all keys (tools/prefill_attn_bench.py; round 2's
// kernel: 88-90 us). Its PMC (profiles/r03c_prefill_fa_pmc.txt): MFMA busy 0.24, SQ_WAIT_ANY 30 % / SQ_WAIT_INST_ANY
// 35 % of wave cycles, L2 hit 85 % — latency inside each wave (K read -> S MFMA -> max -> exp -> P -> PV chains), not
// bandwidth; one workgroup per CU was only 19 % slower.
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef short i16x4_t __attribute__((ext_vector_type(4)));
typedef short i16x8_t __attribute__((ext_vector_type(8)));

// LDS image of a [64 keys][HS] bf16 tile: 16-B chunk ch of row r at byte r * 2HS + 16 (ch ^ sw(r)). For HS = 128
// this is cdna_hip_programming.md T10 image (b): conflict-free for both the 32x32x16 row reads (K) and the
// transposed reads (V).
template <int HS>
__device__ __forceinline__ int kv_off(int row, int ch) {
  constexpr int CH = HS / 8;
  const int sw = CH == 16 ? (((row & 3) << 2) | ((row >> 2) & 3)) : (((row & 3) << 1) | ((row >> 2) & 1));
  return row * (HS * 2) + 16 * (ch ^ sw);
}

// The paired form: one 512-thread workgroup per (head, block pair) holds query blocks hi = nblk-1-p
// (waves 0-3) and lo = p (waves 4-7) of 128 rows and streams the head's K / V ONCE for both — key tile t serves
// every wave whose rows reach it (26 % fewer L2 -> LDS bytes than a workgroup per block at T = 2048, and every SIMD
// holds one hi and one lo wave: 2 (nblk + 1) key tiles per SIMD whatever p). K / V tiles reach LDS by LDS-DMA
// (`buffer_load_dwordx4 ... lds`, range-checked: rows past the cache land as zeros) into a 4-stage ring, three tiles
// ahead of the math, with no staging registers; a raw s_barrier per tile after a counted vmcnt. The LDS reads are
// inline asm with counted lgkmcnt waits (hipcc would wait for every DMA in flight before a compiler-visible LDS
// read, not telling the stages apart).
//
// LGA_DS_READ: an LDS read at a compile-time offset (after unrolling) in inline asm; the host pass, which only
// type-checks the kernel body, cannot take the "i" operand of a non-constant expression
#ifdef __HIP_DEVICE_COMPILE__
#define LGA_DS_READ(op, dst, addr, off) \
  asm volatile(op " %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(off) : "memory")
#else
#define LGA_DS_READ(op, dst, addr, off) ((dst) = {}, (void)(addr), (void)(off))
#endif

template <int HS>
__global__ void __launch_bounds__(512, 1) attn_prefill_pair_kernel(const uint16_t* __restrict__ q,
                                                                   const uint16_t* __restrict__ kc,
                                                                   const uint16_t* __restrict__ vc,
                                                                   const int64_t* __restrict__ input_pos,
                                                                   uint16_t* __restrict__ y, int T, int n_head, int G,
                                                                   int max_seq, float scale) {
  constexpr int KT = 64;           // keys per tile
  constexpr int CH = HS / 8;       // 16-B chunks per key row
  constexpr int DK = HS / 16;      // 32x32x16 k-steps over the head dim (S^T)
  constexpr int DT = HS / 32;      // 32-row tiles of O^T
  constexpr int TB = KT * HS * 2;  // bytes of one K or V tile image
  constexpr int NS = 4;            // ring stages
  constexpr int PIECES = 2 * TB / 1024 / 8;  // 1-KB DMA pieces per wave per tile (K and V)
  static_assert(PIECES * 8 * 1024 == 2 * TB, "pieces");
  __shared__ __attribute__((aligned(1024))) unsigned char lds[NS][2][TB];  // [stage][K | V]
  __shared__ int s_pos[2][8];

  const int tid = threadIdx.x, lane = tid & 63, hh = lane >> 5, lq = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nblk = (T + 127) / 128;
  const int head = blockIdx.x % n_head, pr = blockIdx.x / n_head, g = head / (n_head / G);
  const int hi = nblk - 1 - pr, lo = pr;
  const int blk = wave < 4 ? hi : (lo < hi ? lo : -1);  // odd nblk: the middle block has no partner
  const int q0 = blk * 128 + (wave & 3) * 32;
  const int t = q0 + lq;
  const bool valid = blk >= 0 && t < T;
  const int mypos = valid ? (int)input_pos[t] : -1;
  {
    int mx = mypos, mn = valid ? mypos : INT_MAX;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mx = max(mx, __shfl_xor(mx, o));
      mn = min(mn, __shfl_xor(mn, o));
    }
    if (lane == 0) {
      s_pos[0][wave] = mx;
      s_pos[1][wave] = mn;
    }
  }
  bf16x8_t qb[DK];  // Q^T fragments (B operand): lane l holds Q[t][ks*16 + 8*hh .. +8]
  {
    const uint16_t* qr = q + ((size_t)min(max(t, 0), T - 1) * n_head + head) * HS + 8 * hh;
#pragma unroll
    for (int ks = 0; ks < DK; ++ks) qb[ks] = *(const bf16x8_t*)(qr + ks * 16);
  }
  // the Q fragments and positions are in before any DMA is counted; redefining them through an asm tells hipcc so
  // (it would otherwise wait for "their" loads — i.e. for every DMA in flight — at each use inside the loop)
#pragma unroll
  for (int ks = 0; ks < DK; ++ks) asm volatile("" : "+v"(qb[ks]));
  int mpos = mypos;
  asm volatile("" : "+v"(mpos));
  __syncthreads();
  const int wmax = s_pos[0][wave], wmin = s_pos[1][wave];
  int bmax = s_pos[0][0];
#pragma unroll
  for (int w = 1; w < 8; ++w) bmax = max(bmax, s_pos[0][w]);
  bmax = min(bmax, max_seq - 1);
  const int ntiles = (bmax + 1 + KT - 1) / KT;

  // DMA: wave w moves pieces w * PIECES .. +PIECES of the tile (K pieces first, then V); lane L of a piece lands at
  // +16 L = row r0 + L / CH, physical chunk L % CH, so it fetches logical chunk (L % CH) ^ sw(row) (kv_off's swizzle)
  const __amdgpu_buffer_rsrc_t krs =
      __builtin_amdgcn_make_buffer_rsrc((void*)(kc + (size_t)g * max_seq * HS), (short)0, max_seq * HS * 2, 0x00020000);
  const __amdgpu_buffer_rsrc_t vrs =
      __builtin_amdgcn_make_buffer_rsrc((void*)(vc + (size_t)g * max_seq * HS), (short)0, max_seq * HS * 2, 0x00020000);
  constexpr int RPP = 1024 / (HS * 2);  // key rows per piece
  // (recomputed per issue: a few VALU per tile instead of PIECES live registers)
  auto dvoff = [&](int i) -> int {
    const int piece = (wave * PIECES + i) % (TB / 1024);
    const int r = piece * RPP + lane / CH;
    const int phys = lane % CH;
    const int sw = CH == 16 ? (((r & 3) << 2) | ((r >> 2) & 3)) : (((r & 3) << 1) | ((r >> 2) & 1));
    return (r * HS + (phys ^ sw) * 8) * 2;
  };
  auto issue = [&](int tt) {  // tile tt into stage tt % NS (every wave, every tile: the vmcnt counts stay uniform)
    unsigned char* st = &lds[tt % NS][0][0];
    const int kb = tt * KT * HS * 2;
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
      const int gp = wave * PIECES + i;
      const bool isv = gp >= TB / 1024;
      unsigned char* dst = st + (isv ? TB : 0) + (gp % (TB / 1024)) * 1024;
#ifdef __HIP_DEVICE_COMPILE__  // (a device builtin: the host pass only type-checks the body)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(isv ? vrs : krs, (__attribute__((address_space(3))) void*)dst, 16,
                                               kb + dvoff(i), 0, 0, 0);
#else
      (void)dst, (void)kb, (void)isv, (void)dvoff;
#endif
    }
  };

  // LDS read addresses: K row lq (+ 32 st), chunk 2 ks + hh; V^T transposed reads (16-lane group grp, quad qq, pair pp)
  const unsigned lbase = (unsigned)(uintptr_t)&lds[0][0][0];
  unsigned koff[DK];
#pragma unroll
  for (int ks = 0; ks < DK; ++ks) koff[ks] = lbase + kv_off<HS>(lq, 2 * ks + hh);
  const int gi = lane & 15, qq = gi >> 2, pp = gi & 3, grp = lane >> 4;
  unsigned voff0[DT], voff1[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
    const int ch = ((dt * 32 + 16 * (grp & 1)) >> 3) + (pp >> 1);
    voff0[dt] = lbase + TB + kv_off<HS>(8 * (grp >> 1) + qq, ch) + 8 * (pp & 1);
    voff1[dt] = lbase + TB + kv_off<HS>(8 * (grp >> 1) + 4 + qq, ch) + 8 * (pp & 1);
  }

  f32x16_t o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.0f;
  float m = -INFINITY, l = 0.0f;
  const float sl2 = scale * 1.4426950408889634f;

  typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
  // K fragments of batch b (2 k-steps x 2 halves) of the stage at byte offset sb
  auto kread = [&](unsigned sb, int b, u32x4_t (&f)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ks = 2 * b + (j >> 1), st = j & 1;
      LGA_DS_READ("ds_read_b128", f[j], koff[ks] + sb, st * 32 * HS * 2);
    }
  };
  auto kmfma = [&](int b, const u32x4_t (&f)[4], f32x16_t (&acc)[2]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ks = 2 * b + (j >> 1), st = j & 1;
      acc[st] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, f[j]), qb[ks], acc[st], 0, 0, 0);
    }
  };
  auto vread = [&](unsigned sb, int kk, u32x2_t (&f)[DT][2]) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      LGA_DS_READ("ds_read_b64_tr_b16", f[dt][0], voff0[dt] + sb, kk * 16 * HS * 2);
      LGA_DS_READ("ds_read_b64_tr_b16", f[dt][1], voff1[dt] + sb, kk * 16 * HS * 2);
    }
  };
  // tie the fragments to a counted wait so no use moves above it
#define LGA_KW(N, f) asm volatile("s_waitcnt lgkmcnt(" #N ")" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]))
#define LGA_VW4(N, f)                                                                                             \
  asm volatile("s_waitcnt lgkmcnt(" #N ")" : "+v"(f[0][0]), "+v"(f[0][1]), "+v"(f[1][0]), "+v"(f[1][1]), "+v"(f[2][0]), \
               "+v"(f[2][1]), "+v"(f[3][0]), "+v"(f[3][1]))
#define LGA_VW2(N, f) asm volatile("s_waitcnt lgkmcnt(" #N ")" : "+v"(f[0][0]), "+v"(f[0][1]), "+v"(f[1][0]), "+v"(f[1][1]))

  // S^T = K . Q^T of the tile at sb: 16 K fragments in 4 batches of 4, one batch read ahead
  auto s_tile = [&](unsigned sb, f32x16_t (&sacc)[2]) {
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int r = 0; r < 16; ++r) sacc[st][r] = 0.0f;
    u32x4_t kf[2][4];
    kread(sb, 0, kf[0]);
#pragma unroll
    for (int b = 0; b < DK / 2; ++b) {
      if (b + 1 < DK / 2) {
        kread(sb, b + 1, kf[(b + 1) & 1]);
        LGA_KW(4, kf[b & 1]);
      } else {
        LGA_KW(0, kf[b & 1]);
      }
      kmfma(b, kf[b & 1], sacc);
    }
  };
  // the online softmax of S(t) (sacc) and O += P . V(t) from the stage at sbv
  auto pv_tile = [&](unsigned sbv, int k0, f32x16_t (&sacc)[2]) {
    u32x2_t vf[2][DT][2];
    vread(sbv, 0, vf[0]);
    if (__builtin_amdgcn_readfirstlane(k0 + KT - 1 > wmin)) {  // a row of this wave ends inside the tile
#pragma unroll
      for (int st = 0; st < 2; ++st)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (k0 + st * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh > mpos) sacc[st][r] = -INFINITY;
    }
    float tmax = -INFINITY;
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, sacc[st][r]);
    {
      const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(tmax), __float_as_uint(tmax), false, false);
      tmax = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
    }
    const float mnew = fmaxf(m, tmax * sl2);
    const float mref = mnew == -INFINITY ? 0.0f : mnew;
    if (!__all(mnew == m)) {
      const float c = __builtin_amdgcn_exp2f(m - mref);
      l *= c;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] *= c;
    }
    m = mnew;
    float rs = 0.0f;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int st = kk >> 1, r0 = 8 * (kk & 1);
      if (kk + 1 < 4) vread(sbv, kk + 1, vf[(kk + 1) & 1]);
      float x[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        x[e] = __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[st][r0 + e], sl2, -mref));
        rs += x[e];
      }
      const uint32_t w0 = pack2(x[0], x[1]), w1 = pack2(x[2], x[3]);
      const uint32_t w2 = pack2(x[4], x[5]), w3 = pack2(x[6], x[7]);
      const auto a = __builtin_amdgcn_permlane32_swap(w0, w2, false, false);
      const auto b = __builtin_amdgcn_permlane32_swap(w1, w3, false, false);
      const u32x4_t f = {a[0], b[0], a[1], b[1]};
      const bf16x8_t pb = __builtin_bit_cast(bf16x8_t, f);
      auto& cur = vf[kk & 1];
      if (kk + 1 < 4) {  // V(kk+1)'s 2 DT reads are newer than V(kk)
        if constexpr (DT == 4) LGA_VW4(8, cur); else LGA_VW2(4, cur);
      } else {
        if constexpr (DT == 4) LGA_VW4(0, cur); else LGA_VW2(0, cur);
      }
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const u32x4_t vv = {cur[dt][0][0], cur[dt][0][1], cur[dt][1][0], cur[dt][1][1]};
        o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, vv), pb, o[dt], 0, 0, 0);
      }
    }
    l += rs;
  };

  // Ring: tiles 0 .. NS-2 in flight, then per tile: wait for it (the tiles issued after it may stay in flight),
  // barrier (every wave's pieces landed; every wave done with the stage the next issue overwrites), issue tile
  // + NS - 1, math. (Round 4 also measured the lo waves half a tile behind the hi waves, so the two waves of a SIMD
  // sit in opposite phases, and a software-pipelined form with S(t + 1)'s MFMAs under tile t's softmax and P.V:
  // both slower)
#pragma unroll
  for (int i = 0; i < NS - 1; ++i)
    if (i < ntiles) issue(i);
  for (int tt = 0; tt < ntiles; ++tt) {
    const int after = min(NS - 2, ntiles - 1 - tt);  // tiles issued after tt
    if (after >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PIECES) : "memory");
    else if (after == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PIECES) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (tt + NS - 1 < ntiles) issue(tt + NS - 1);
    const int k0 = tt * KT;
    if (k0 <= wmax) {
      f32x16_t sacc[2];
      const unsigned sb = (unsigned)((tt % NS) * 2 * TB);
      s_tile(sb, sacc);
      pv_tile(sb, k0, sacc);
    }
  }
#undef LGA_KW
#undef LGA_VW4
#undef LGA_VW2
  l += __shfl_xor(l, 32);
  if (valid) {
    const float inv = 1.0f / l;
    uint16_t* yr = y + ((size_t)t * n_head + head) * HS;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        const int d = dt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
        *(uint32_t*)(yr + d) = pack2(o[dt][r] * inv, o[dt][r + 1] * inv);
      }
  }
}

// (keys in flight per row group, waves per workgroup) by q_per_kv; -D overrides are for tools/attn_sweep.py
#ifndef LGA_ATTN_Q1
#define LGA_ATTN_Q1 4, 4
#endif
#ifndef LGA_ATTN_Q1_FEW
#define LGA_ATTN_Q1_FEW 2, 8
#endif
#ifndef LGA_ATTN_Q2
#define LGA_ATTN_Q2 4, 4
#endif
#ifndef LGA_ATTN_Q4  // 8 waves (round 4, tools/attn_sweep.py 32 8 128: Mixtral at 16 splits 12.5-12.9 vs 13.7-14.1 us)
#define LGA_ATTN_Q4 2, 8
#endif
#ifndef LGA_ATTN_Q8
#define LGA_ATTN_Q8 2, 4
#endif

// rows per workgroup of the SHARED form by heads per workgroup: the largest value up to 4 (the product's MAX_BATCH; a
// row slot that stays empty still costs its registers) that compiles with no scratch. One head compiles clean beyond 4
// (R = 8 at 4 waves, R = 5 at 8 waves); 4 and 8 heads spill at R = 2. DESIGN.md 4.5f has the resource table
#ifndef LGA_SHARED_R1
#define LGA_SHARED_R1 4
#endif
#ifndef LGA_SHARED_R1_FEW
#define LGA_SHARED_R1_FEW 4
#endif
#ifndef LGA_SHARED_R2
#define LGA_SHARED_R2 4
#endif
#ifndef LGA_SHARED_R4
#define LGA_SHARED_R4 1
#endif
#ifndef LGA_SHARED_R8
#define LGA_SHARED_R8 1
#endif
static constexpr int attn_nw(int /*unr*/, int nw) { return nw; }

// One attention call as the entry points describe it. kRows: lga_attention (q (T, H, hs) already roped, no append);
// the other four are the fused decode forms on the qkv projection rows (the FUSED / WINDOW / BATCH / SHARED comments
// above).
enum AttnForm { kRows, kOne, kWindow, kBatch, kShared };
struct AttnCall {
  const char* name;  // the entry point, for its messages
  AttnForm form;
  bool kv8;  // fp8 caches: kc / vc hold codes, ksc / vsc the row scales
  int rows;  // T, 1, M or B
  const void* q;  // q, or the qkv rows of a fused form
  void *kc, *vc;
  float *ksc, *vsc;
  const int64_t *pos, *rope_pos;
  const float *cos, *sin;
  int rope_rows;
  void* y;
  float* ws;
  unsigned* cnt;
  long long slot_stride, scale_slot_stride;  // kBatch, kShared: elements between two sequences' caches / scale rows
  const int32_t* active;                     // kBatch: idle flags, may be null
  int H, G, hs, rope_n_elem, max_seq, n_splits;
  float scale;
  hipStream_t stream;
  const int64_t* prefix_len = nullptr;  // kShared: the shared prefix's length, on the device
};

// the kernel instantiation of a call, one (heads per workgroup, keys in flight, waves) configuration: hs 64 exists
// for kRows only, the fp8 kernels for the fused forms only (attn_body's static_asserts)
template <int HS, int QPK, int UNR, int NW>
static void attn_launch_cfg(const AttnCall& c, dim3 grid, int hsplit) {
  constexpr bool PIPE = LGA_ATTN_PIPE != 0;
#define LGA_BF16(BATCH, FUSED, WINDOW)                                                                             \
  attn_kernel<HS, QPK, UNR, NW, BATCH, FUSED, PIPE, WINDOW><<<grid, NW * 64, 0, c.stream>>>(                       \
      (const uint16_t*)c.q, (uint16_t*)c.kc, (uint16_t*)c.vc, c.pos, (uint16_t*)c.y, c.ws, c.cnt, c.H, c.max_seq,  \
      c.scale, c.rope_pos, c.cos, c.sin, c.rope_rows, hsplit, (long)c.slot_stride, c.active)
#define LGA_FP8(BATCH, WINDOW)                                                                                     \
  attn_kernel_kv8<HS, QPK, UNR, NW, BATCH, PIPE, WINDOW><<<grid, NW * 64, 0, c.stream>>>(                          \
      (const uint16_t*)c.q, (uint8_t*)c.kc, (uint8_t*)c.vc, c.ksc, c.vsc, c.pos, (uint16_t*)c.y, c.ws, c.cnt, c.H, \
      c.max_seq, c.scale, c.rope_pos, c.cos, c.sin, c.rope_rows, hsplit, (long)c.slot_stride,                      \
      (long)c.scale_slot_stride, c.active)
#define LGA_FUSED(BATCH, WINDOW)                    \
  do {                                              \
    if (c.kv8) LGA_FP8(BATCH, WINDOW);              \
    else LGA_BF16(BATCH, true, WINDOW);             \
    return;                                         \
  } while (0)
  if constexpr (HS == 128) {
    switch (c.form) {
      case kOne: LGA_FUSED(false, false);
      case kWindow: LGA_FUSED(false, true);
      case kBatch: LGA_FUSED(true, false);
      case kShared:  // (launched by attn_launch itself: attn_shared_kernel)
      case kRows: break;
    }
  }
  LGA_BF16(false, false, false);
#undef LGA_FUSED
#undef LGA_BF16
#undef LGA_FP8
}

// head slices per query group: split a group's heads over more workgroups while the launch would fill at most half
// the CUs (tools/attn_sweep.py, p = 2303, 16 splits: Llama-2-70B at TP = 8 — one group of 8 heads per rank — 22.5 ->
// 7.8 us with 8 slices; 70B TP = 1 23.6 -> 13.4 with 2; Mixtral 12.9 -> 10.3 with 2, Mixtral TP = 2 12.6 -> 8.3
// with 4; profiles/r04u_attn_head_slices.txt)
static int attn_hsplit(int T, int G, int qpk, int n_splits) {
  int h = 1;
  if (T == 1 && n_splits > 1)
    while (h < qpk && G * h * n_splits <= 128) h *= 2;
  if (const char* e = getenv("LGA_ATTN_HSPLIT")) {  // lab A/B
    const int v = atoi(e);
    if (v >= 1 && v <= qpk && qpk % v == 0) h = v;
  }
  return h;
}

// Every entry point below: the argument checks (nothing is dereferenced or launched before they pass), the window's
// append, the grid, the kernel.
static int attn_launch(const AttnCall& c) {
  const bool fused = c.form != kRows;
  const bool slots = c.form == kBatch || c.form == kShared;  // the caches of all slots, slot_stride apart
  const bool many = c.form == kWindow || slots;
  const int qpk = c.G > 0 ? c.H / c.G : 0;
  const long long seq_rows = (long long)c.G * c.max_seq;
  const bool ptrs = c.q && c.kc && c.vc && c.pos && c.y && (!fused || (c.rope_pos && c.cos && c.sin)) &&
                    (!c.kv8 || (c.ksc && c.vsc)) && (c.form != kShared || c.prefix_len);
  const char* bad =
      !ptrs ? "null pointer"
      : many && !(c.rows >= 1 && c.rows <= 8) ? (c.form == kWindow ? "M must be in [1, 8]" : "B must be in [1, 8]")
      : !(c.rows > 0 && c.G > 0 && c.H % c.G == 0) ? "bad head geometry"
      : fused && !(c.hs == 128 && c.rope_n_elem == 128)
          ? "needs head_size == rope_n_elem == 128 (else: rope_kv_append + attention)"
      : !fused && c.hs != 128 && c.hs != 64 ? "head_size must be 64 or 128"
      : fused && qpk != 1 && qpk != 2 && qpk != 4 && qpk != 8 ? "q_per_kv must be 1, 2, 4 or 8"
      : fused && !(c.rope_rows > 0 && c.max_seq > 0) ? "empty rope cache or kv cache"
      : !(c.n_splits >= 1 && c.n_splits <= 256) ? "n_splits must be in [1, 256]"
      : !(c.n_splits == 1 || (c.ws && c.cnt)) ? "split attention needs workspace + counters"
      : slots && c.slot_stride < seq_rows * c.hs
          ? "slot_stride below one sequence's G * max_seq * head_size elements"
      : c.form == kBatch && c.kv8 && c.scale_slot_stride < seq_rows
          ? "scale_slot_stride below one sequence's G * max_seq scales"
          : nullptr;
  if (bad) {
    char msg[160];
    snprintf(msg, sizeof msg, "%s: %s", c.name, bad);
    lga_set_error(msg);
    return (int)hipErrorInvalidValue;
  }
  if (!fused && c.rows >= 16 && c.n_splits == 1) {  // prefill: flash attention on MFMA, any heads per group
    const dim3 grid((((c.rows + 127) / 128 + 1) / 2) * c.H);
#define LGA_PREFILL(HS)                                                                                          \
  attn_prefill_pair_kernel<HS><<<grid, 512, 0, c.stream>>>((const uint16_t*)c.q, (const uint16_t*)c.kc,          \
                                                           (const uint16_t*)c.vc, c.pos, (uint16_t*)c.y, c.rows, \
                                                           c.H, c.G, c.max_seq, c.scale)
    if (c.hs == 128) LGA_PREFILL(128);
    else LGA_PREFILL(64);
#undef LGA_PREFILL
    LGA_LAUNCH_RETURN();
  }
  if (c.form == kWindow) {  // two launches on the stream: the append of all M rows, then the M-row attention
    const dim3 grid(c.G, c.rows);
    if (c.kv8)
      window_append_kernel<true><<<grid, 64, 0, c.stream>>>((const uint16_t*)c.q, c.kc, c.vc, c.ksc, c.vsc, c.pos,
                                                            c.cos, c.sin, c.rope_rows, c.H, c.max_seq);
    else
      window_append_kernel<false><<<grid, 64, 0, c.stream>>>((const uint16_t*)c.q, c.kc, c.vc, nullptr, nullptr, c.pos,
                                                             c.cos, c.sin, c.rope_rows, c.H, c.max_seq);
  }
  // a window row, a batch row: the slices of its T = 1 launch
  const int hsplit = attn_hsplit(many ? 1 : c.rows, c.G, qpk, c.n_splits);
  const dim3 grid(c.n_splits, c.G * hsplit, c.rows);
#define LGA_ATTN(QPK, CFG)                                                  \
  do {                                                                      \
    if (c.hs == 128) attn_launch_cfg<128, QPK, CFG>(c, grid, hsplit);       \
    else attn_launch_cfg<64, QPK, CFG>(c, grid, hsplit);                    \
  } while (0)
  if (c.form == kShared) {  // the same (UNR, NW) per heads-per-workgroup as below, R rows per workgroup
#define LGA_SHARED(QPK, R, CFG)                                                                                      \
  attn_shared_kernel<128, QPK, CFG, R><<<dim3(c.n_splits, c.G * hsplit, (c.rows + R - 1) / R), attn_nw(CFG) * 64, 0, \
                                         c.stream>>>(                                                                \
      (const uint16_t*)c.q, (uint16_t*)c.kc, (uint16_t*)c.vc, c.pos, c.prefix_len, (uint16_t*)c.y, c.ws, c.cnt, c.H, \
      c.max_seq, c.scale, c.cos, c.sin, c.rope_rows, hsplit, (long)c.slot_stride, c.active, c.rows)
    switch (qpk / hsplit) {
      case 1:
        if (c.G * hsplit <= 16) LGA_SHARED(1, LGA_SHARED_R1_FEW, LGA_ATTN_Q1_FEW);
        else LGA_SHARED(1, LGA_SHARED_R1, LGA_ATTN_Q1);
        break;
      case 2: LGA_SHARED(2, LGA_SHARED_R2, LGA_ATTN_Q2); break;
      case 4: LGA_SHARED(4, LGA_SHARED_R4, LGA_ATTN_Q4); break;
      default: LGA_SHARED(8, LGA_SHARED_R8, LGA_ATTN_Q8); break;  // (q_per_kv was checked above)
    }
#undef LGA_SHARED
    LGA_LAUNCH_RETURN();
  }
  switch (qpk / hsplit) {
    case 1:  // one head per group: 8 waves x 2 keys in flight when the groups are few (TP ranks: G = 4 7.9 vs 8.2 us,
             // G = 8 8.0 vs 8.7 at 16 splits; profiles/r04u_attn_head_slices.txt), else 4 x 4 (Llama-2-7B, G = 32)
      if (c.G * hsplit <= 16) LGA_ATTN(1, LGA_ATTN_Q1_FEW);
      else LGA_ATTN(1, LGA_ATTN_Q1);
      break;
    case 2: LGA_ATTN(2, LGA_ATTN_Q2); break;
    case 4: LGA_ATTN(4, LGA_ATTN_Q4); break;
    case 8: LGA_ATTN(8, LGA_ATTN_Q8); break;
    // (kRows below 16 rows only: the prefill kernel takes any q_per_kv, and the fused forms were checked above)
    default: lga_set_error("lga_attention: q_per_kv must be 1, 2, 4 or 8"); return (int)hipErrorInvalidValue;
  }
#undef LGA_ATTN
  LGA_LAUNCH_RETURN();
}

}  // namespace lga

int lga::preload_attention() {
  return lga::preload(lga::attn_prefill_pair_kernel<128>) + lga::preload(lga::attn_prefill_pair_kernel<64>);
}

// The entry points (include/litgpt_amd.h states each form's contract): fill the call, launch it.
using lga::AttnCall;

extern "C" int lga_attention(const void* q, const void* k_cache, const void* v_cache, const int64_t* input_pos,
                             void* y, float* workspace, unsigned* counters, int T, int n_head, int n_query_groups,
                             int head_size, int max_seq, int n_splits, float scale, hipStream_t stream) {
  return lga::attn_launch(AttnCall{"lga_attention", lga::kRows, false, T, q, (void*)k_cache, (void*)v_cache, nullptr,
                                   nullptr, input_pos, nullptr, nullptr, nullptr, 0, y, workspace, counters, 0, 0,
                                   nullptr, n_head, n_query_groups, head_size, 0, max_seq, n_splits, scale, stream});
}

// Decode step (T = 1) with RoPE + KV-append fused in: qkv is the fused projection row ([G][q_per_kv + 2][hs]
// bf16); q and k are roped with cos/sin row rope_pos[0], k and v are written to the caches at cache_pos[0] and
// the attention output over keys 0..cache_pos[0] lands in y ([n_head][hs]). Replaces lga_rope_kv_append +
// lga_attention for a token step; full rotary only (rope_n_elem == head_size == 128).
extern "C" int lga_attention_decode_fused(const void* qkv, void* k_cache, void* v_cache, const int64_t* cache_pos,
                                          const int64_t* rope_pos, const float* cos, const float* sin, int rope_rows,
                                          void* y, float* workspace, unsigned* counters, int n_head,
                                          int n_query_groups, int head_size, int rope_n_elem, int max_seq,
                                          int n_splits, float scale, hipStream_t stream) {
  return lga::attn_launch(AttnCall{"lga_attention_decode_fused", lga::kOne, false, 1, qkv, k_cache, v_cache, nullptr,
                                   nullptr, cache_pos, rope_pos, cos, sin, rope_rows, y, workspace, counters, 0, 0,
                                   nullptr, n_head, n_query_groups, head_size, rope_n_elem, max_seq, n_splits, scale,
                                   stream});
}

// Speculative verify window: M rows of ONE sequence at consecutive positions pos0[0] + r (cache and rope position, read
// on the device). y[r] and the caches end with the bits of M successive lga_attention_decode_fused calls with the
// same n_splits. Two launches on the stream: the append of all M rows, then the M-row attention.
extern "C" int lga_attention_decode_window(const void* qkv, void* k_cache, void* v_cache, const int64_t* pos0,
                                           const float* cos, const float* sin, int rope_rows, void* y,
                                           float* workspace, unsigned* counters, int M, int n_head,
                                           int n_query_groups, int head_size, int rope_n_elem, int max_seq,
                                           int n_splits, float scale, hipStream_t stream) {
  return lga::attn_launch(AttnCall{"lga_attention_decode_window", lga::kWindow, false, M, qkv, k_cache, v_cache,
                                   nullptr, nullptr, pos0, pos0, cos, sin, rope_rows, y, workspace, counters, 0, 0,
                                   nullptr, n_head, n_query_groups, head_size, rope_n_elem, max_seq, n_splits, scale,
                                   stream});
}

// The two decode forms over fp8 (e4m3) caches: k_codes / v_codes (G, max_seq, 128) uint8, k_scale / v_scale
// (G, max_seq) fp32 powers of two. The new row(s) are quantized on the way in and scored as the cache holds them.
extern "C" int lga_attention_decode_fused_kv8(const void* qkv, void* k_codes, void* v_codes, float* k_scale,
                                              float* v_scale, const int64_t* cache_pos, const int64_t* rope_pos,
                                              const float* cos, const float* sin, int rope_rows, void* y,
                                              float* workspace, unsigned* counters, int n_head, int n_query_groups,
                                              int head_size, int rope_n_elem, int max_seq, int n_splits, float scale,
                                              hipStream_t stream) {
  return lga::attn_launch(AttnCall{"lga_attention_decode_fused_kv8", lga::kOne, true, 1, qkv, k_codes, v_codes,
                                   k_scale, v_scale, cache_pos, rope_pos, cos, sin, rope_rows, y, workspace, counters,
                                   0, 0, nullptr, n_head, n_query_groups, head_size, rope_n_elem, max_seq, n_splits,
                                   scale, stream});
}

extern "C" int lga_attention_decode_window_kv8(const void* qkv, void* k_codes, void* v_codes, float* k_scale,
                                               float* v_scale, const int64_t* pos0, const float* cos, const float* sin,
                                               int rope_rows, void* y, float* workspace, unsigned* counters, int M,
                                               int n_head, int n_query_groups, int head_size, int rope_n_elem,
                                               int max_seq, int n_splits, float scale, hipStream_t stream) {
  return lga::attn_launch(AttnCall{"lga_attention_decode_window_kv8", lga::kWindow, true, M, qkv, k_codes, v_codes,
                                   k_scale, v_scale, pos0, pos0, cos, sin, rope_rows, y, workspace, counters, 0, 0,
                                   nullptr, n_head, n_query_groups, head_size, rope_n_elem, max_seq, n_splits, scale,
                                   stream});
}

// Batched decode step: B independent sequences in ONE launch, grid (n_splits, G * hsplit, B). Row b reads row b of
// the (B, (H + 2G) hs) qkv, sits at cache_pos[b] / rope_pos[b] and owns the cache slot k_cache + b * slot_stride,
// v_cache + b * slot_stride (strides in elements: the (B, G, max_seq, hs) cache tensor's stride(0)). Row b's y, cache
// rows (and scale rows) have the bits of lga_attention_decode_fused(_kv8) on that row and slot with the same
// n_splits; no other slot is read or written. active (B) int32 may be null (all rows active); a row with active[b]
// == 0 is idle: y[b] = 0, its slot bit-unchanged. workspace / counters as for a T = B launch.
extern "C" int lga_attention_decode_batch(const void* qkv, void* k_cache, void* v_cache, const int64_t* cache_pos,
                                          const int64_t* rope_pos, const float* cos, const float* sin, int rope_rows,
                                          void* y, float* workspace, unsigned* counters, int B, long long slot_stride,
                                          const int32_t* active, int n_head, int n_query_groups, int head_size,
                                          int rope_n_elem, int max_seq, int n_splits, float scale,
                                          hipStream_t stream) {
  return lga::attn_launch(AttnCall{"lga_attention_decode_batch", lga::kBatch, false, B, qkv, k_cache, v_cache, nullptr,
                                   nullptr, cache_pos, rope_pos, cos, sin, rope_rows, y, workspace, counters,
                                   slot_stride, 0, active, n_head, n_query_groups, head_size, rope_n_elem, max_seq,
                                   n_splits, scale, stream});
}

extern "C" int lga_attention_decode_batch_kv8(const void* qkv, void* k_codes, void* v_codes, float* k_scale,
                                              float* v_scale, const int64_t* cache_pos, const int64_t* rope_pos,
                                              const float* cos, const float* sin, int rope_rows, void* y,
                                              float* workspace, unsigned* counters, int B, long long slot_stride,
                                              long long scale_slot_stride, const int32_t* active, int n_head,
                                              int n_query_groups, int head_size, int rope_n_elem, int max_seq,
                                              int n_splits, float scale, hipStream_t stream) {
  return lga::attn_launch(AttnCall{"lga_attention_decode_batch_kv8", lga::kBatch, true, B, qkv, k_codes, v_codes,
                                   k_scale, v_scale, cache_pos, rope_pos, cos, sin, rope_rows, y, workspace, counters,
                                   slot_stride, scale_slot_stride, active, n_head, n_query_groups, head_size,
                                   rope_n_elem, max_seq, n_splits, scale, stream});
}

// n samples of one prompt: the batch form for B rows at ONE position pos[0] (cache and rope position) whose keys j <
// min(max(prefix_len[0], 0), pos[0]) only slot 0 holds; row b reads those from slot 0, the rest from slot b, and
// appends to slot b. y and row pos[0] of every slot have the bits of lga_attention_decode_batch on caches whose slot b
// holds slot 0's prefix rows, with the same n_splits. bf16 caches only.
extern "C" int lga_attention_decode_shared(const void* qkv, void* k_cache, void* v_cache, const int64_t* pos,
                                           const int64_t* prefix_len, const float* cos, const float* sin,
                                           int rope_rows, void* y, float* workspace, unsigned* counters, int B,
                                           long long slot_stride, const int32_t* active, int n_head,
                                           int n_query_groups, int head_size, int rope_n_elem, int max_seq,
                                           int n_splits, float scale, hipStream_t stream) {
  return lga::attn_launch(AttnCall{"lga_attention_decode_shared", lga::kShared, false, B, qkv, k_cache, v_cache,
                                   nullptr, nullptr, pos, pos, cos, sin, rope_rows, y, workspace, counters,
                                   slot_stride, 0, active, n_head, n_query_groups, head_size, rope_n_elem, max_seq,
                                   n_splits, scale, stream, prefix_len});
}

#ifdef LGA_ATTN_TRACE
extern "C" int lga_attn_trace_read(unsigned long long* host, int n) {
  hipError_t e = hipMemcpyFromSymbol(host, HIP_SYMBOL(lga::g_attn_trace), (size_t)n * sizeof(unsigned long long));
  void* dptr = nullptr;
  if (e == hipSuccess) e = hipGetSymbolAddress(&dptr, HIP_SYMBOL(lga::g_attn_trace));
  if (e == hipSuccess) e = hipMemset(dptr, 0, sizeof(lga::g_attn_trace));  // read-and-clear
  if (e == hipSuccess) e = hipDeviceSynchronize();
  return (int)e;
}
#endif

// fp32 partials (T * H * n_splits * (hs + 4)); the counters (T * n_head * 64 uint32: one per (row, query group, head
// slice) at a 256-B stride) must be zeroed once at allocation
extern "C" size_t lga_attention_workspace_bytes(int T, int n_head, int head_size, int n_splits) {
  return (size_t)T * n_head * (n_splits < 1 ? 1 : n_splits) * (head_size + 4) * sizeof(float);
}
