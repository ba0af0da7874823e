/*
 * litgpt_amd.h — C ABI of liblitgpt_amd.so, the MI355X (gfx950) hot path of lit_gpt's quantized decode.
 *
 * Conventions: plain device pointers + sizes, no torch types; every buffer is caller-owned
 * (kernels never allocate; scratch is passed in); all launches are asynchronous on `stream` (a hipStream_t;
 * graph-capturable); return 0 on success, otherwise a hipError_t value with a message available from
 * lga_last_error_string() (thread-local). bf16 tensors are raw uint16 bit patterns, row-major, contiguous.
 *
 * Reference interfaces replaced (file:line in /root/reference unless marked upstream):
 *   - bitsandbytes 0.41.0 (requirements-all.txt:3; upstream, not in the reference tree) reached via Lightning's
 *     BitsandbytesPrecision (generate/base.py:128-136, generate/tp.py:126-134,171,190): the ctypes C functions
 *     cquantize_blockwise_bf16_nf4 / cdequantize_blockwise_bf16_nf4 / cgemm_4bit_inference_naive_bf16
 *     (upstream names) behind Linear4bit.forward -> lga_quantize, lga_q4_gemv(_swiglu), lga_q4_gemm;
 *   - the ATen kernels lit_gpt/model.py issues on the hot path -> the remaining entry points.
 */
#ifndef LITGPT_AMD_H
#define LITGPT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* lga_stream_t; /* == hipStream_t */

/* weight formats */
#define LGA_FMT_Q4G 0 /* int4, symmetric, per-group bf16 scale = bf16(absmax/7), nibble = q + 8 */
#define LGA_FMT_NF4 1 /* bitsandbytes NF4 codebook, per-block fp32 absmax */
#define LGA_FMT_BF16 2 /* unquantized bf16 weight [N][K] (lga_q4_gemm_fused / lga_q4_gemm_swiglu only) */
#define LGA_FMT_FP4 3 /* bitsandbytes FP4 code (get_4bit_type('fp4'), "bnb.fp4"), per-block fp32 absmax */
#define LGA_FMT_INT8 4 /* LLM.int8: int8 [N][K], fp32 row absmax (the lga_int8_* entry points only) */

/* -- plumbing ---------------------------------------------------------------------------------------- */
const char* lga_last_error_string(void);
int lga_version(void);
int lga_device_info(int device, int* n_cu, char* arch_name, int arch_len);
/* builds the device objects of the prefill path's kernels (fused GEMM, flash attention, norms, RoPE, embedding,
 * lm_head GEMV, argmax) now instead of at their first launch, where the runtime spends about 0.5 ms per kernel
 * inside the first prompt (called by build_model, the model-load step; nothing is launched) */
int lga_preload_kernels(void);

/* -- quantize at load (Lightning BitsandbytesPrecision.convert_module + bnb quantize on .to(device);
 *    generate/base.py:168, generate/tp.py:171-190) ------------------------------------------------------
 * w: (N, K) fp32 (w_is_bf16 = 0) or bf16 (1). qweight: (N, K/2) bytes, byte j = k 2j (low) | 2j+1 (high).
 * scales: (N, K/group) bf16 for Q4G, fp32 for NF4 / FP4. Layout spec: oracle/quant.py. Every 4-bit entry point
 * below takes fmt 0 / 1 / 3 (FP4 runs the NF4 kernels with its own 16-entry codebook). */
int lga_quantize(const void* w, int w_is_bf16, uint8_t* qweight, void* scales, int N, int K, int group, int fmt,
                 lga_stream_t stream);
/* bitsandbytes double quantization of nf4 / fp4 statistics ("bnb.nf4-dq", "bnb.fp4-dq"; quantize_4bit(compress_statistics=True),
 * generate/base.py:105): absmax (n fp32, bnb's flattened 64-blocks, i.e. the NF4 scales of lga_quantize) is
 * replaced in place by code[q] * absmax2 + offset — q = nearest entry of `code` (the 256-entry signed dynamic
 * map, device fp32) to (absmax - offset) / absmax2 per block of 256, offset = mean(absmax) (written to
 * offset_out) — the statistic bnb's dequantize_4bit reconstructs. */
int lga_nf4_double_quant(float* absmax, long n, const float* code, float* offset_out, lga_stream_t stream);

/* -- decode GEMV, M = 1 (bnb gemv_4bit for one-token inputs; every Linear of lit_gpt/model.py:519,619,656,
 *    712-716) -----------------------------------------------------------------------------------------------
 * y[N] = x[K] . dequant(W)^T (+bias[N]) (+residual[N]); norm_weight != NULL applies RMSNorm
 * (lit_gpt/rmsnorm.py:19-25, eps = norm_eps) to x first. variant < 0 = heuristic tile choice. */
int lga_q4_gemv(const void* x, const uint8_t* qweight, const void* scales, const void* bias, const void* residual,
                const void* norm_weight, float norm_eps, void* y, int N, int K, int group, int fmt, int variant,
                lga_stream_t stream);
/* y[N] = bf16(silu(bf16(x.W1^T))) * bf16(x.W2^T) — LLaMAMLP fc_1/fc_2 + silu*mul (lit_gpt/model.py:712-715) */
int lga_q4_gemv_swiglu(const void* x, const uint8_t* qweight1, const void* scales1, const uint8_t* qweight2,
                       const void* scales2, const void* norm_weight, float norm_eps, void* y, int N, int K,
                       int group, int fmt, int variant, lga_stream_t stream);
/* -- batched decode GEMV, 1 <= M <= 8 rows (one token of each sequence of a decode batch; the reference's
 *    set_kv_cache(batch_size) / idx (B, 1) forward) ----------------------------------------------------------
 * y[M][N] from x[M][K] (residual[M][N]): the packed weights are streamed ONCE and dotted against every row while
 * they sit in registers. Row r of y is bit-identical to lga_q4_gemv (lga_q4_gemv_swiglu) on x[r], residual[r]
 * with variant -1, for every M and r: the launch takes the one-row geometry and its per-row arithmetic. Fused
 * RMSNorm: K <= 8192 (K <= 4096 for the SwiGLU pair). */
int lga_q4_gemv_rows(const void* x, const uint8_t* qweight, const void* scales, const void* bias,
                     const void* residual, const void* norm_weight, float norm_eps, void* y, int M, int N, int K,
                     int group, int fmt, lga_stream_t stream);
int lga_q4_gemv_swiglu_rows(const void* x, const uint8_t* qweight1, const void* scales1, const uint8_t* qweight2,
                            const void* scales2, const void* norm_weight, float norm_eps, void* y, int M, int N,
                            int K, int group, int fmt, lga_stream_t stream);

/* -- prefill GEMM, M > 1 (bnb dequantize_4bit + cuBLAS GEMM) -------------------------------------------- */
int lga_q4_gemm(const void* x, const uint8_t* qweight, const void* scales, const void* bias, const void* residual,
                void* y, int M, int N, int K, int group, int fmt, lga_stream_t stream);
/* The same product with the dequantization fused into a 256 x 128 MFMA tile (csrc/gemm_q4f.hip): the weight
 * is never written out in bf16. fmt 0 int4-g / 1 nf4 / 2 bf16 weights [N][K] / 3 fp4; needs N % 8 == 0, K % 64 == 0 and
 * (4-bit) a power-of-two group >= 64 dividing K (lga_q4f_fits). Numerically the bnb path: bf16(value * scale)
 * weights, fp32 accumulation, one bf16 rounding (+bias), then + residual. */
int lga_q4f_fits(int M, int N, int K, int group, int fmt);
/* Short prompts split K across workgroups: the caller passes a zero-initialised workspace of at least this many
 * bytes (0 = none needed) and keeps it for later calls (its per-tile counters are left zeroed). */
size_t lga_q4f_workspace_bytes(int M, int N, int K, int swiglu);
int lga_q4_gemm_fused(const void* x, const void* weight, const void* scales, const void* bias, const void* residual,
                      void* y, int M, int N, int K, int group, int fmt, void* workspace, size_t workspace_bytes,
                      lga_stream_t stream);
/* LLaMAMLP prefill (lit_gpt/model.py:712-716): y (M, N) = bf16(silu(bf16(x W1^T))) * bf16(x W2^T), fc_1 and fc_2
 * in one launch (each tile computes 64 columns of both and applies the product in its epilogue). */
int lga_q4_gemm_swiglu(const void* x, const void* qweight1, const void* scales1, const void* qweight2,
                       const void* scales2, void* y, int M, int N, int K, int group, int fmt, void* workspace,
                       size_t workspace_bytes, lga_stream_t stream);
/* bnb dequantize_4bit (the first half of the reference's M > 1 Linear4bit path): w (N, K) bf16 =
 * bf16(value(nibble) * scale) — the same bits lga_q4_gemm / lga_q4_gemm_fused stage, so lga_bf16_gemm over w ==
 * lga_q4_gemm (tests, tools). */
int lga_q4_dequantize(const uint8_t* qweight, const void* scales, void* w, int N, int K, int group, int fmt,
                      lga_stream_t stream);

/* -- unquantized bf16 Linears (BASELINE config 2: no --quantize, precision bf16-true; the reference runs
 *    F.linear on the bf16 nn.Linear weight, lit_gpt/model.py:619, :656, :712-716, :519) ------------------- */
/* decode GEMV y (N) = x (K) . W (N, K)^T [+bias] [+residual]; optional fused RMSNorm of x (as lga_q4_gemv) */
int lga_bf16_gemv(const void* x, const void* weight, const void* bias, const void* residual, const void* norm_weight,
                  float norm_eps, void* y, int N, int K, lga_stream_t stream);
/* y = bf16(silu(bf16(x W1^T))) * bf16(x W2^T) (LLaMAMLP, model.py:715), optional fused RMSNorm of x */
int lga_bf16_gemv_swiglu(const void* x, const void* weight1, const void* weight2, const void* norm_weight,
                         float norm_eps, void* y, int N, int K, lga_stream_t stream);
/* prefill GEMM Y (M, N) = X (M, K) . W (N, K)^T [+bias] [+residual] on MFMA; K % 32 == 0 */
int lga_bf16_gemm(const void* x, const void* weight, const void* bias, const void* residual, void* y, int M, int N,
                  int K, lga_stream_t stream);

/* -- bnb.int8 (LLM.int8, modelled on bitsandbytes Linear8bitLt(has_fp16_weights=False, threshold=6.0) with bf16 in
 *    place of fp16; the reference's --quantize bnb.int8, generate/base.py:105) ------------------------------------
 * Weights: row scale s_w[n] = max_k |W[n,k]| (fp32), q = clamp(rint(W * (127 / s_w)), -127, 127), int8 [N][K].
 * Activations (per call): column j is an outlier column iff |X[m,j]| >= threshold for any row m (threshold <= 0: no
 * column is); s_x[m] = max over the other columns, a = clamp(rint(X * (127 / s_x[m])), -127, 127), 0 in outlier
 * columns. y = bf16(float(sum_j a q) * ((s_x s_w) / 16129) + sum_{j outlier} X[m,j] * (q[n,j] * (s_w / 127)) + bias)
 * [then bf16(y + residual)]; the integer sum is exact int32. K % 16 == 0 everywhere. */
/* weight quantizer: weight [N][K] fp32 or bf16 -> qweight int8 [N][K], scales fp32 [N] */
int lga_int8_quantize(const void* weight, int weight_is_bf16, void* qweight, float* scales, int N, int K,
                      lga_stream_t stream);
/* decode GEMV y (N) = x (K) against the int8 weight; optional fused RMSNorm of x, bias, residual; K <= 16384 */
int lga_int8_gemv(const void* x, const void* qweight, const float* scales, const void* bias, const void* residual,
                  const void* norm_weight, float norm_eps, float threshold, void* y, int N, int K,
                  lga_stream_t stream);
/* y = bf16(silu(bf16(x W1^T))) * bf16(x W2^T), both matrices on one activation quantization */
int lga_int8_gemv_swiglu(const void* x, const void* qweight1, const float* scales1, const void* qweight2,
                         const float* scales2, const void* norm_weight, float norm_eps, float threshold, void* y,
                         int N, int K, lga_stream_t stream);
/* prefill activation quantizer: x [M][K] bf16 -> xq int8 [M][K], sx fp32 [M], col_flags int32 [K] (1 = outlier
 * column), cols int32 [K] (the outlier columns, ascending, first *count entries), count int32 [1]; no host sync */
int lga_int8_quantize_act(const void* x, void* xq, float* sx, int* col_flags, int* cols, int* count, int M, int K,
                          float threshold, lga_stream_t stream);
/* prefill GEMM on the i8 MFMA: Y (M, N) from xq / sx / cols / count of lga_int8_quantize_act (x: the bf16 rows, read
 * in the outlier columns only); M >= 2 */
int lga_int8_gemm(const void* x, const void* xq, const float* sx, const int* cols, const int* count,
                  const void* qweight, const float* scales, const void* bias, const void* residual, void* y, int M,
                  int N, int K, lga_stream_t stream);

/* -- LoRA adapters (the reference's lit_gpt/lora.py: the unmerged LoRALinear / LoRAQKVLinear forward :170-177,
 *    :398-433 and LoRALinear.merge :140-149, under bf16-true) --------------------------------------------------
 * Device layout, built once when the adapter is attached: A (R, K) bf16; B (N, r) bf16 in output-row order;
 * row_off (N) int32 = the first of the r rows of A that output row n uses (a fused qkv Linear: one segment of r rows
 * per enabled q / k / v slot, -1 on the rows of a slot without adapter), NULL when every row uses rows 0..r-1.
 * r % 8 == 0 and R % 8 == 0 (zero padded), r <= 64, r <= R <= 192, K % 8 == 0, K <= 32768. Per output row, with
 * fp32 sums: t_j = bf16(sum_k x'_k A[j,k]); u_n = bf16(sum_{j<r} B[n,j] t[off_n + j]); l_n = bf16(u_n * scaling);
 * y_n = bf16(base_n + l_n) (base NULL: y_n = l_n); then y_n = bf16(y_n + residual_n) where residual is given.
 * Rows with off_n < 0 pass base (+ residual) through. base may alias y. */
/* decode, M = 1, the whole chain in one launch: x' = x, or bf16(RMSNorm(x)) (as lga_q4_gemv) with norm_weight */
int lga_lora_gemv(const void* x, const void* norm_weight, float norm_eps, const void* A, const void* B,
                  const int32_t* row_off, float scaling, const void* base, const void* residual, void* y, int N,
                  int K, int R, int r, lga_stream_t stream);
/* batched decode, 1 <= M <= 8 rows, each with its own adapter out of a stacked set, in one launch. x (M, K); base
 * (required, may alias y), residual (or NULL) and y (M, N). A holds n_adapters (R, K) blocks a_stride elements apart,
 * B n_adapters (N, r) blocks b_stride elements apart (strides: multiples of 8, at least one block); row_off (N) or
 * NULL and scaling are shared by the set. adapter (M) int32 in DEVICE memory, read by the kernel, so a captured launch
 * follows a later write of the ids. Contract:
 *   - row m with adapter[m] = a in [0, n_adapters) has the bits of lga_lora_gemv(x[m], norm_weight, norm_eps,
 *     A + a * a_stride, B + a * b_stride, row_off, scaling, base[m], residual[m]) (the two kernels run one body);
 *   - a row whose id is -1, or anything else outside [0, n_adapters), passes through as that kernel's off_n < 0 rows
 *     do: y = base, then bf16(y + residual) where residual is given. Such a row reads nothing of x, A or B, so a bad
 *     id cannot read out of bounds;
 *   - no row's output depends on another row's x or id.
 * The grid is (lga_lora_gemv's grid, M); the limits on r, R and K are lga_lora_gemv's. */
int lga_lora_gemv_rows(const void* x, const void* norm_weight, float norm_eps, const void* A, const void* B,
                       const int32_t* row_off, const int32_t* adapter, int n_adapters, long long a_stride,
                       long long b_stride, float scaling, const void* base, const void* residual, void* y, int M,
                       int N, int K, int R, int r, lga_stream_t stream);
/* prefill, M > 1: t (M, R) bf16 = bf16(x A^T) on the MFMA (x already normed), then the rest of the chain per row over
 * the base output y (M, N) */
int lga_lora_down(const void* x, const void* A, void* t, int M, int K, int R, lga_stream_t stream);
int lga_lora_up(const void* t, const void* B, const int32_t* row_off, float scaling, const void* base,
                const void* residual, void* y, int M, int N, int R, int r, lga_stream_t stream);
/* in place on a bf16 weight W (N, K): W[n,k] = bf16(W[n,k] + bf16(bf16(sum_j B[n,j] A[off_n + j, k]) * scaling));
 * rows with off_n < 0 stay untouched */
int lga_lora_merge(void* W, const void* A, const void* B, const int32_t* row_off, float scaling, int N, int K,
                   int R, int r, lga_stream_t stream);

/* -- row / elementwise ops ---------------------------------------------------------------------------- */
/* RMSNorm over rows of n (lit_gpt/rmsnorm.py:19-25) */
int lga_rmsnorm(const void* x, const void* weight, void* y, int rows, int n, float eps, lga_stream_t stream);
/* RoPE (lit_gpt/model.py:641-644, 767-773) on the q and k slots of qkv (T, (H+2G)*hs) [per group g: q_per_kv
 * q heads, k, v — scripts/convert_hf_checkpoint.py:174-188 layout], cos/sin rows rope_pos[t] of (rope_rows,
 * rope_n_elem) fp32 tables; q_out (T, H, hs); k (roped) and v written to k_cache/v_cache (G, max_seq, hs) at row
 * cache_pos[t] (KVCache.forward index_copy_, lit_gpt/model.py:788-795). */
int lga_rope_kv_append(const void* qkv, void* q_out, void* k_cache, void* v_cache, const int64_t* cache_pos,
                       const int64_t* rope_pos, const float* cos, const float* sin, int rope_rows, int T, int n_head,
                       int n_query_groups, int head_size, int rope_n_elem, int max_seq, lga_stream_t stream);
/* out[t] = table[idx[t]] (nn.Embedding, lit_gpt/model.py:515) */
int lga_embedding(const void* idx, int idx_is_int64, const void* table, void* out, int T, int C, int V,
                  lga_stream_t stream);
/* y = bf16(a + b) (Block residual, lit_gpt/model.py:591-592) */
int lga_add(const void* a, const void* b, void* y, long n, lga_stream_t stream);
/* y = bf16(bf16(silu(a)) * b) (lit_gpt/model.py:715) */
int lga_swiglu(const void* a, const void* b, void* y, long n, lga_stream_t stream);
/* torch.nn.LayerNorm over rows of n (GPT-NeoX norm_class, lit_gpt/config.py:137-144; model.py:578-588):
 * fp32 mean / biased variance, y = bf16((x - mean) * rstd * weight + bias); bias may be NULL */
int lga_layernorm(const void* x, const void* weight, const void* bias, void* y, int rows, int n, float eps,
                  lga_stream_t stream);
/* y = bf16(gelu(a)) — GptNeoxMLP (lit_gpt/model.py:699-702): exact erf form, or tanh form when approximate_tanh */
int lga_gelu(const void* a, void* y, long n, int approximate_tanh, lga_stream_t stream);

/* -- attention over the KV cache (SDPA with the input_pos mask rows, lit_gpt/model.py:651,658-665) --------
 * q (T, H, hs); caches (G, max_seq, hs); query t attends keys 0..input_pos[t]; y (T, H*hs).
 * n_splits > 1 splits keys 0..input_pos[t] evenly (flash-decoding; the split merge happens in the same launch
 * by the last-arriving workgroup) and needs `workspace` of lga_attention_workspace_bytes(T, H, hs, n_splits) bytes
 * plus `counters` (T * H * 64 uint32 — one per (t, group, head slice) at a 256-B stride so the device-scope
 * atomics do not share a line; zeroed once at allocation, re-armed by the kernel; at T = 1 a group's heads may be
 * dealt to up to H/G workgroups when the groups are few).
 * head_size in {64, 128}; H/G in {1,2,4,8}; 1 <= n_splits <= 256. */
int lga_attention(const void* q, const void* k_cache, const void* v_cache, const int64_t* input_pos, void* y,
                  float* workspace, unsigned* counters, int T, int n_head, int n_query_groups, int head_size,
                  int max_seq, int n_splits, float scale, lga_stream_t stream);
size_t lga_attention_workspace_bytes(int T, int n_head, int head_size, int n_splits);
/* Decode step (T = 1) with RoPE + KV-append fused into the attention launch (apply_rope lit_gpt/model.py:641-644,
 * KVCache.forward :788-795, SDPA :651): qkv is the fused projection row ([G][q_per_kv + 2][hs], the layout of
 * CausalSelfAttention.attn); q and k are roped with row rope_pos[0] of cos/sin (rope_rows x 128 fp32); k, v are
 * stored at cache_pos[0]; y (H*hs) = attention of the roped q over keys 0..cache_pos[0]. Caches bit-identical to
 * lga_rope_kv_append; y equals lga_attention's up to fp32 summation order (the new key is scored last).
 * Requires head_size == rope_n_elem == 128. */
int lga_attention_decode_fused(const void* qkv, void* k_cache, void* v_cache, const int64_t* cache_pos,
                               const int64_t* rope_pos, const float* cos, const float* sin, int rope_rows, void* y,
                               float* workspace, unsigned* counters, int n_head, int n_query_groups, int head_size,
                               int rope_n_elem, int max_seq, int n_splits, float scale, lga_stream_t stream);
/* Speculative verify window: the decode step above for M (1..8) rows of ONE sequence at consecutive positions. qkv is
 * (M, (H + 2G) * hs), the rows qkv GEMV's output; row r sits at pos0[0] + r (cache and rope position, read on the
 * device: a captured graph stays valid as the position advances). After the call y (M, H*hs), k_cache and v_cache are
 * bit-identical to M successive lga_attention_decode_fused calls on rows 0..M-1 at those positions with the same
 * n_splits: every workgroup is the one-row kernel's workgroup of its row (own split boundaries, own key scored last
 * from registers); the roped k / v of all M rows are appended first, in a launch of their own. A row whose position
 * is >= max_seq stores nothing and its y is unspecified. workspace / counters as lga_attention's, sized for T = M.
 * Requires head_size == rope_n_elem == 128 and H/G in {1, 2, 4, 8}. */
int lga_attention_decode_window(const void* qkv, void* k_cache, void* v_cache, const int64_t* pos0, const float* cos,
                                const float* sin, int rope_rows, void* y, float* workspace, unsigned* counters, int M,
                                int n_head, int n_query_groups, int head_size, int rope_n_elem, int max_seq,
                                int n_splits, float scale, lga_stream_t stream);
/* -- fp8 (OCP e4m3) KV cache -------------------------------------------------------------------------------------
 * Per layer and slot: k_codes / v_codes (G, max_seq, 128) uint8 and k_scale / v_scale (G, max_seq) fp32. A row is the
 * 128 bf16 values the bf16 cache would hold (k after RoPE). amax = max |x_i| = m 2^E, m in [0.5, 1); the scale is
 * s = 2^e, e = E - 9 if m <= 0.875 else E - 8, clamped to [-126, 127] (the smallest power of two with amax / s <=
 * 448); amax = 0 gives s = 1. code_i = e4m3fn(x_i / s), round to nearest even; the value read back is
 * float(code_i) * s, exact in bf16. Rows with non-finite values or amax < 2^-100 are outside the contract. Every
 * attention call reads K and V as the cache holds them, the call's own rows included.
 * All four need head_size == rope_n_elem == 128; the two attention forms H/G in {1, 2, 4, 8}.
 *
 * lga_attention_decode_fused_kv8: lga_attention_decode_fused over fp8 caches; the new row's codes and scales are
 * stored at cache_pos[0] (nothing at or past max_seq) and scored from registers as stored. */
int lga_attention_decode_fused_kv8(const void* qkv, void* k_codes, void* v_codes, float* k_scale, float* v_scale,
                                   const int64_t* cache_pos, const int64_t* rope_pos, const float* cos,
                                   const float* sin, int rope_rows, void* y, float* workspace, unsigned* counters,
                                   int n_head, int n_query_groups, int head_size, int rope_n_elem, int max_seq,
                                   int n_splits, float scale, lga_stream_t stream);
/* lga_attention_decode_window over fp8 caches: y (M, H*hs), codes and scales bit-identical to M successive
 * lga_attention_decode_fused_kv8 calls with the same n_splits. */
int lga_attention_decode_window_kv8(const void* qkv, void* k_codes, void* v_codes, float* k_scale, float* v_scale,
                                    const int64_t* pos0, const float* cos, const float* sin, int rope_rows, void* y,
                                    float* workspace, unsigned* counters, int M, int n_head, int n_query_groups,
                                    int head_size, int rope_n_elem, int max_seq, int n_splits, float scale,
                                    lga_stream_t stream);
/* -- batched decode attention -------------------------------------------------------------------------------------
 * B (1..8) independent sequences in ONE launch. Row b reads row b of the (B, (H + 2G) hs) qkv, sits at cache_pos[b]
 * / rope_pos[b] and owns cache slot b: k_cache + b * slot_stride, v_cache + b * slot_stride (and for the fp8 cache
 * k_scale / v_scale + b * scale_slot_stride); strides in elements, the (B, G, max_seq, hs) tensor's stride(0), at
 * least G * max_seq * hs (G * max_seq for the scales). Row b's y (B, H*hs), cache rows and scale rows have the bits of
 * lga_attention_decode_fused(_kv8) on that row and slot with the same n_splits; no other slot is read or written. A
 * row at or past max_seq stores nothing and attends keys 0..max_seq-1. active (B) int32 may be null (every row
 * active); a row with active[b] == 0 is idle: y[b] = 0 and its slot stays bit-unchanged. workspace: lga_attention_
 * workspace_bytes(B, ...); counters B * n_head * 64 uint32, zeroed once. Same geometry limits as the fused forms. */
int lga_attention_decode_batch(const void* qkv, void* k_cache, void* v_cache, const int64_t* cache_pos,
                               const int64_t* rope_pos, const float* cos, const float* sin, int rope_rows, void* y,
                               float* workspace, unsigned* counters, int B, long long slot_stride,
                               const int32_t* active, int n_head, int n_query_groups, int head_size, int rope_n_elem,
                               int max_seq, int n_splits, float scale, lga_stream_t stream);
int lga_attention_decode_batch_kv8(const void* qkv, void* k_codes, void* v_codes, float* k_scale, float* v_scale,
                                   const int64_t* cache_pos, const int64_t* rope_pos, const float* cos,
                                   const float* sin, int rope_rows, void* y, float* workspace, unsigned* counters,
                                   int B, long long slot_stride, long long scale_slot_stride, const int32_t* active,
                                   int n_head, int n_query_groups, int head_size, int rope_n_elem, int max_seq,
                                   int n_splits, float scale, lga_stream_t stream);
/* -- shared-prompt decode attention (n samples of one prompt) ------------------------------------------------------
 * The batch form for B (1..8) rows that advance in lock step behind ONE prompt whose K / V only slot 0 holds. qkv
 * (B, (H + 2G) hs); k_cache / v_cache the whole (slots, G, max_seq, hs) bf16 tensors, slot_stride as above. pos (1)
 * int64 on the device: every row sits at p = pos[0], its cache and its rope position. prefix_len (1) int64 on the
 * device: P, used as min(max(P, 0), p). Row b scores keys j < P from slot 0 and keys P <= j < p from slot b, scores its
 * own new key from registers and appends it at row p of slot b. y[b] and row p of slot b have the bits that
 * lga_attention_decode_batch gives, with the same n_splits, on caches whose slot b holds slot 0's rows [0, P); rows
 * [0, P) of slots 1..B-1 are never read or written. Both values are read by the kernel, so a captured graph stays
 * valid as p advances and from prompt to prompt. p at or past max_seq: nothing is stored, keys 0..max_seq-1 are
 * attended. active (B) int32 may be null; a row with active[b] == 0 is idle (y[b] = 0, slot b bit-unchanged), and an
 * idle row 0 does not keep the others from reading slot 0. workspace, counters, n_splits and the geometry limits are
 * the batch form's (one workspace serves both). There is no fp8 form. */
int lga_attention_decode_shared(const void* qkv, void* k_cache, void* v_cache, const int64_t* pos,
                                const int64_t* prefix_len, const float* cos, const float* sin, int rope_rows, void* y,
                                float* workspace, unsigned* counters, int B, long long slot_stride,
                                const int32_t* active, int n_head, int n_query_groups, int head_size, int rope_n_elem,
                                int max_seq, int n_splits, float scale, lga_stream_t stream);
/* lga_rope_kv_append for fp8 caches (T rows): roped q to q_out (T, H, hs); k (roped) and v quantized into the codes
 * and scales at row cache_pos[t] — the bits the decode forms store for the same qkv row. */
int lga_kv8_rope_append(const void* qkv, void* q_out, void* k_codes, void* v_codes, float* k_scale, float* v_scale,
                        const int64_t* cache_pos, const int64_t* rope_pos, const float* cos, const float* sin,
                        int rope_rows, int T, int n_head, int n_query_groups, int head_size, int rope_n_elem,
                        int max_seq, lga_stream_t stream);
/* Rows [0, n) of every group of one slot's codes and scales -> k_out / v_out (G, n, 128) bf16 = float(code) * scale
 * (exact). The cached prefill (T > 1) expands the cache with it and runs lga_attention over the result. */
int lga_kv8_dequantize(const void* k_codes, const void* v_codes, const float* k_scale, const float* v_scale,
                       void* k_out, void* v_out, int n_query_groups, int n, int head_size, int max_seq,
                       lga_stream_t stream);
/* Greedy speculative acceptance after the window's lm_head: logits (M, n) bf16 contiguous, window (M) int32
 * (window[0] the last emitted token, window[1..] the drafts). t_r = argmax of row r in lga_argmax's order; a = the
 * largest a <= M - 1 with window[r + 1] == t_r for all r < a. out (M + 1) int32: out[0] = a, out[1..a+1] = t_0..t_a,
 * the rest -1. *token_inout = t_a (may be &window[0]), *pos_inout += a + 1 (either may be NULL). 1 <= M <= 8. */
int lga_spec_accept(const void* logits, int M, int n, const int32_t* window, int32_t* out, int32_t* token_inout,
                    int64_t* pos_inout, lga_stream_t stream);

/* -- LLaMA-Adapter v1 (lit_gpt/adapter.py CausalSelfAttention.scaled_dot_product_attention) ------------------------
 * The gated prefix-attention term, added in place to the T rows of an attention result y (T, H*hs) bf16:
 *   y[t, h] = bf16(y[t, h] + bf16(g_h * ay)),  ay = bf16(softmax(scale * q^ ak_g^T) av_g),  g = h / (H / G).
 * qkv (T, (H + 2G) * hs) is the fused projection in the per-group layout of lga_rope_kv_append, q NOT roped: the
 * kernel computes q^ = bf16(rope(q)) itself, with lga_rope_kv_append's arithmetic, from row p_t of the cos / sin
 * tables (rope_rows, rope_n_elem) fp32. ak / av (G, aT, hs) bf16 are the k / v slices of attn.attn(adapter_wte.weight),
 * un-expanded, never roped; every one of the aT keys is visible to every query (no mask). gating (H) bf16. Scores and
 * the softmax are fp32. The positions are read on the device (a captured launch follows a later write):
 *   pos_mode 0: p_t = pos[t] (T int64);  1: p_t = pos[0] + t (the verify window);  2: p_t = pos[0] (samples of one
 *   prompt in lock step).
 * active (T) int32 or NULL: a row with active[t] == 0 is skipped before anything that depends on its position is
 * loaded, and so is a row whose position is outside [0, rope_rows): y[t] keeps its bits. A row's result depends on no
 * other row, on T or on the launch grid. No workspace. bf16 only; head_size % 8 == 0, head_size <= 256; rope_n_elem
 * even, <= head_size; H % G == 0; 1 <= aT <= 64; ak 16-B aligned. */
int lga_adapter_attention(const void* qkv, const void* ak, const void* av, const void* gating, const float* cos,
                          const float* sin, int rope_rows, const int64_t* pos, int pos_mode, const int32_t* active,
                          void* y, int T, int n_head, int n_query_groups, int head_size, int rope_n_elem, int aT,
                          float scale, lga_stream_t stream);

/* -- sparse MoE (LLaMAMoE.forward, lit_gpt/model.py:727-743; Mixtral) ------------------------------------------
 * lga_moe_route: per token row of router logits [T][n_expert] bf16 -> expert_ids [T][k] int32 and probs [T][k]
 * bf16 = topk(router, k) with the CPU torch.topk order on ties (model.py:737) and
 * softmax(dim=1, dtype=float).to(bf16) (model.py:738). n_expert <= 8. */
int lga_moe_route(const void* logits, int T, int n_expert, int k, int32_t* expert_ids, void* probs,
                  lga_stream_t stream);
/* lga_moe_gate_route: one token's router gate (the 4-bit `self.gate(x)` Linear, model.py:736, optional fused
 * RMSNorm of x as lga_q4_gemv) and its routing (lga_moe_route) in one launch: expert_ids [k] int32, probs [k] bf16,
 * bit-identical to lga_q4_gemv (n_expert rows) followed by lga_moe_route. n_expert <= 8, K <= 6144. */
int lga_moe_gate_route(const void* x, const uint8_t* qweight, const void* scales, const void* norm_weight,
                       float norm_eps, int n_expert, int K, int group, int fmt, int k, int32_t* expert_ids, void* probs,
                       lga_stream_t stream);
/* Routed expert GEMVs (the per-expert `expert(x[token_idx])` calls, model.py:741-742, for one token): slot s
 * (0..n_slots-1) uses expert e = expert_ids[s], whose packed weights / scales start at qweight + e * w_stride
 * bytes / scales + e * s_stride bytes (experts stacked with a uniform stride). lga_q4_gemv_experts reads
 * x + s * x_stride and writes y[s][N]; the SwiGLU form (fc_1 / fc_2 of LLaMAMLP, model.py:712-715) shares x and
 * optionally fuses RMSNorm (norm_2) like lga_q4_gemv_swiglu. */
int lga_q4_gemv_experts(const void* x, const uint8_t* qweight, const void* scales, const int32_t* expert_ids,
                        int n_slots, int n_expert, long long w_stride, long long s_stride, int x_stride, void* y,
                        int N, int K, int group, int fmt, int variant, lga_stream_t stream);
int lga_q4_gemv_swiglu_experts(const void* x, const uint8_t* qweight1, const void* scales1, const uint8_t* qweight2,
                               const void* scales2, const int32_t* expert_ids, int n_slots, int n_expert,
                               long long w_stride, long long s_stride, const void* norm_weight, float norm_eps,
                               void* y, int N, int K, int group, int fmt, int variant, lga_stream_t stream);
/* lga_q4_gemv_experts_pair_combine: one token, k = 2, no tensor parallelism — the routed proj GEMVs of both slots
 * (x [2][K] = the slots' SwiGLU rows, experts stacked as lga_q4_gemv_experts, expert_ids [2], probs [2]) and
 * lga_moe_combine with the Block residual in one launch: y [N] = residual + sum in ascending expert id of
 * bf16(probs[s] * expert_out[s]), bit-identical to lga_q4_gemv_experts + lga_moe_combine. The second-arriving
 * workgroup of each row block combines: `scratch` [2][N] bf16 holds the first one's rows (write-through),
 * `counters` (lga_q4_gemv_experts_pair_counters(N) words, caller-zeroed once) are re-armed by the kernel. */
int lga_q4_gemv_experts_pair_supported(int N, int K, int group, int fmt);
size_t lga_q4_gemv_experts_pair_counters(int N);
int lga_q4_gemv_experts_pair_combine(const void* x, const uint8_t* qweight, const void* scales,
                                     const int32_t* expert_ids, const void* probs, const void* residual, int n_expert,
                                     long long w_stride, long long s_stride, void* y, void* scratch,
                                     unsigned* counters, int N, int K, int group, int fmt, lga_stream_t stream);
/* y[t] = residual[t] (optional) + the bf16 sum, in ascending expert order, of bf16(probs[t][s] * expert_out[t][s])
 * (the `y[token_idx] += probs * expert(...)` loop, model.py:739-742, then Block's residual add model.py:592). */
int lga_moe_combine(const void* expert_out, const void* probs, const int32_t* expert_ids, const void* residual,
                    void* y, int T, int k, int C, lga_stream_t stream);
/* Grouped sparse-MoE prefill (T > 1): replaces the per-expert loop of LLaMAMoE.forward (model.py:740-742:
 * torch.where(indices == e) per expert, then the expert MLP on the gathered rows). lga_moe_group sorts the T * k
 * (token, slot) pairs by expert on the device (stable: (token, slot) order inside an expert) into a table of
 * m-tiles of bm rows (bm 64 or 256): tiles = {n_tiles, (expert, first row, rows) x n_tiles}, capacity
 * 1 + 3 * lga_moe_group_tiles(T * k, n_expert, bm) ints; x_rows[r] = token of permuted row r, y_rows[r] =
 * token * k + slot. lga_q4_gemm_swiglu_grouped computes g[r] = bf16(silu(bf16(x[x_rows[r]] W1_e^T))) *
 * bf16(x[x_rows[r]] W2_e^T) for every permuted row r in ONE launch (the experts' weights stacked with strides
 * w_stride / s_stride bytes, as lga_q4_gemv_experts); lga_q4_gemm_grouped computes y[y_rows[r]] =
 * x[x_rows ? x_rows[r] : r] W_e^T (y_rows NULL: row r). No host synchronisation: the launches are sized by the
 * table's capacity and surplus tiles exit. */
int lga_moe_group_tiles(int rows, int n_expert, int bm);
int lga_moe_group(const int32_t* expert_ids, int T, int k, int n_expert, int bm, int32_t* tiles, int32_t* x_rows,
                  int32_t* y_rows, lga_stream_t stream);
int lga_q4_gemm_swiglu_grouped(const void* x, const void* qweight1, const void* scales1, const void* qweight2,
                               const void* scales2, long long w_stride, long long s_stride, const int32_t* tiles,
                               const int32_t* x_rows, void* y, int rows, int N, int K, int group, int fmt, int bm,
                               int n_expert, lga_stream_t stream);
int lga_q4_gemm_grouped(const void* x, const void* qweight, const void* scales, long long w_stride,
                        long long s_stride, const int32_t* tiles, const int32_t* x_rows, const int32_t* y_rows,
                        void* y, int rows, int N, int K, int group, int fmt, int bm, int n_expert,
                        lga_stream_t stream);

/* -- tensor-parallel all-reduce of decode activations (generate/tp.py:73-74 `all_reduce(outs, "sum", ranks)`,
 *    the forward hook after every attention / MLP, :53,57,70) over xGMI peer memory -----------------------------
 * Each rank owns one mailbox of lga_comm_mailbox_bytes(cap) bytes from lga_comm_alloc (uncached device memory,
 * zeroed; its 64-byte IPC handle goes to the peers, which map it with lga_comm_open). lga_allreduce_bf16:
 * y[n] = bf16(sum over ranks 0..world-1, in that order, of x_r) (+ residual[n]: y = bf16(bf16(sum) + residual),
 * the Block residual add, lit_gpt/model.py:591-592), identical bits on every rank. mailboxes: host array of world
 * device pointers (index rank = this rank's own mailbox); seq_counter: 1 uint32 zeroed once, advanced by every
 * call (the same call sequence on every rank); err: bit 0 set when a peer's flag did not arrive within 5 s
 * (results invalid). n % 8 == 0, n <= cap, world <= 8. One workgroup; graph-capturable. */
size_t lga_comm_mailbox_bytes(int cap);
int lga_comm_alloc(size_t bytes, void** ptr, void* ipc_handle);
int lga_comm_open(const void* ipc_handle, void** ptr);
int lga_comm_close(void* ptr);
int lga_comm_free(void* ptr);
int lga_allreduce_bf16(const void* x, const void* residual, void* y, int n, void* const* mailboxes, int rank,
                       int world, int cap, unsigned* seq_counter, unsigned* err, lga_stream_t stream);
/* lga_comm_trace: diagnostics of the all-reduce protocol. Every later lga_allreduce_bf16 / lga_q4_gemv_allreduce
 * launch of this process records its call into buf (n_records x 16 uint64 on the device, indexed by the call's
 * sequence number): sequence, rank, entry / flags-raised / wait-done times (s_memrealtime, 100 MHz), timeout, and
 * the peers' flag words seen when the wait ended. buf = NULL switches it off. Not part of the reference interface. */
int lga_comm_trace(void* buf, int n_records);
/* The row-parallel decode Linear and its all-reduce in ONE launch (generate/tp.py:53,57,70 hook the reduction on
 * attn.proj / mlp.proj; lit_gpt/model.py:591-592 adds the residual): y (N) = lga_allreduce_bf16 of
 * lga_q4_gemv(x, W, bias) over the ranks (+ residual), bit for bit — each workgroup pushes its partial rows into
 * every rank's mailbox, the last-arriving workgroup of the rank raises the flags, waits for the peers and sums in
 * rank order. Same mailboxes / sequence counter / error word as lga_allreduce_bf16 (calls of the two may be mixed);
 * arrive_counter: 576 uint32 (9 counters at a 256-B stride; 640 with the tagged form's) zeroed once (re-armed by the kernel). N % 8 == 0, N <= cap. Graph-capturable. */
int lga_q4_gemv_allreduce(const void* x, const uint8_t* qweight, const void* scales, const void* bias,
                          const void* residual, void* y, int N, int K, int group, int fmt, void* const* mailboxes,
                          int rank, int world, int cap, unsigned* seq_counter, unsigned* arrive_counter,
                          unsigned* err, lga_stream_t stream);
/* The same call in the tagged protocol (generate/tp.py:73-74 on multi-GPU ranks): every workgroup pushes its rows as
 * 8-byte {bf16 pair, call sequence} granules into every rank's mailbox and polls its own rows from every rank — no
 * arrival counters, flags or last-arriver sum; identical result bits. arrive_counter: 640 uint32 (words 576 / 608:
 * the launch's arrivals and the rank's call count the sequence derives from, zeroed once); seq_counter unused. The grid need not be
 * co-resident (a workgroup waits only for other ranks). Same mailboxes: lga_comm_mailbox_bytes covers both regions. */
int lga_q4_gemv_allreduce_tagged(const void* x, const uint8_t* qweight, const void* scales, const void* bias,
                                 const void* residual, void* y, int N, int K, int group, int fmt,
                                 void* const* mailboxes, int rank, int world, int cap, unsigned* seq_counter,
                                 unsigned* arrive_counter, unsigned* err, lga_stream_t stream);

/* -- greedy sampling (generate/base.py:30-47 at temperature 0): lowest index among the maxima; optionally
 *    writes the token (int32) and advances *pos_inout by one (generate/base.py:92) -------------------------- */
int lga_argmax(const void* logits, int n, int64_t* out_idx, int32_t* token_out, int64_t* pos_inout,
               lga_stream_t stream);
/* lga_argmax, then the same launch gathers row `token` of the embedding table (vocab x n_embd bf16) into emb_out
 * (n_embd bf16): the next decode step's transformer.wte(idx) (lit_gpt/model.py:515, an nn.Embedding gather),
 * bit-identical to lga_embedding of the token — one launch per step fewer. */
int lga_argmax_embed(const void* logits, int n, int64_t* out_idx, int32_t* token_out, int64_t* pos_inout,
                     const void* table, int n_embd, int vocab, void* emb_out, lga_stream_t stream);
/* lga_q4_gemv_argmax_embed: the greedy decode step's head in ONE launch — optional fused RMSNorm (ln_f), the 4-bit
 * lm_head GEMV (model.py:519; logits (N) bf16 still written), argmax (generate/base.py:30-41 at temperature 0,
 * torch.argmax order: NaN first, ties to the lowest index) and lga_argmax_embed's bookkeeping (token_out, out_idx,
 * *pos_inout += 1, the token's row of table into emb_out). Bit-identical to lga_q4_gemv + lga_argmax_embed.
 * work: lga_q4_gemv_argmax_work_bytes(N, K) bytes, zeroed once (its counters re-arm). K <= 4096. */
size_t lga_q4_gemv_argmax_work_bytes(int N, int K);
int lga_q4_gemv_argmax_embed(const void* x, const uint8_t* qweight, const void* scales, const void* norm_weight,
                             float norm_eps, void* logits, int N, int K, int group, int fmt, void* work,
                             int64_t* out_idx, int32_t* token_out, int64_t* pos_inout, const void* table, int C, int V,
                             void* emb_out, lga_stream_t stream);

/* -- temperature sampling (generate/base.py:30-41 with top_k and temperature > 0: torch.topk, scatter into -inf,
 *    softmax(logits / temperature) in the logits' dtype, torch.multinomial(probs, 1)) in ONE launch --------------
 * logits: n (<= 65536) bf16. Keeps the top_k (1..1024) largest (NaN largest, ties lowest index first),
 * x = bf16(v / temperature), p = bf16(exp(x - max) / sum); the token is the first kept index (in index order) whose
 * running fp32 sum of p divided by the total reaches u (torch's CPU inverse CDF). u = *uniform when uniform is
 * given, else a counter-based hash of (seed, *counter) in (0, 1), and *counter advances by one (device state: the
 * launch replays in a graph). Then lga_argmax's bookkeeping (out_idx, token_out, *pos_inout += 1) and, with emb_out,
 * lga_argmax_embed's row gather. kept_out (top_k int32) / probs_out (top_k bf16), optional: the kept indices in
 * index order and their probabilities. */
int lga_sample_topk(const void* logits, int n, int top_k, float temperature, const float* uniform,
                    unsigned long long seed, unsigned long long* counter, int64_t* out_idx, int32_t* token_out,
                    int64_t* pos_inout, const void* table, int n_embd, int vocab, void* emb_out, int32_t* kept_out,
                    void* probs_out, lga_stream_t stream);
/* Speculative acceptance under top-k sampling: lga_spec_accept with each row's argmax replaced by lga_sample_topk's
 * draw. logits (M, n) bf16 contiguous (rows need no alignment), window (M) int32 as in lga_spec_accept. t_r = the
 * token lga_sample_topk draws from row r at top_k / temperature under uniform[r] (uniform: M fp32), or, with uniform
 * NULL, under the uniform of draw number *counter + r. a = the largest a <= M - 1 with window[r + 1] == t_r for all
 * r < a. out (M + 1) int32 = [a, t_0..t_a, -1...], *token_inout = t_a (may be &window[0]), *pos_inout += a + 1
 * (either may be NULL), and on the counter path *counter += a + 1. Two launches: one workgroup per row writes
 * sampled (8 int32 of scratch), then one small launch does the rest. 1 <= M <= 8, n <= 65536, top_k 1..1024. */
int lga_spec_accept_sample(const void* logits, int M, int n, int top_k, float temperature, const float* uniform,
                           unsigned long long seed, unsigned long long* counter, const int32_t* window,
                           int32_t* sampled, int32_t* out, int32_t* token_inout, int64_t* pos_inout,
                           lga_stream_t stream);
/* Nucleus (top-p) sampling in ONE launch, on top of the top-k set (top_k 1..1024) or over the whole vocabulary
 * (top_k == 0). Candidates C and p as lga_sample_topk computes them over C; w = trunc(p 2^30), W = sum_C w;
 * target = clamp(ceil((double)top_p (double)W), 1, W); a value class (equal logit value, -0 == +0) is in the nucleus N
 * iff the weight of the candidates above it is < target (classes enter whole, in descending value); the token is the
 * first index of N whose running integer sum of w reaches floor((double)u (double)W') + 1, W' = sum_N w. top_p in
 * (0, 1]. u, seed / counter, the bookkeeping and the embedding gather as lga_sample_topk. Optional outputs (tests), in
 * index order over C: kept_out (|C| int32, top_k > 0 only), probs_out (|C| bf16; n entries at top_k == 0),
 * nucleus_out (|C| bytes, 1 inside N). NaN logits and candidate sets whose maximum is -inf are outside the contract. */
int lga_sample_nucleus(const void* logits, int n, int top_k, float top_p, float temperature, const float* uniform,
                       unsigned long long seed, unsigned long long* counter, int64_t* out_idx, int32_t* token_out,
                       int64_t* pos_inout, const void* table, int n_embd, int vocab, void* emb_out, int32_t* kept_out,
                       void* probs_out, uint8_t* nucleus_out, lga_stream_t stream);
/* lga_spec_accept_sample with each row drawn by lga_sample_nucleus at top_k (0: none) / top_p / temperature. */
int lga_spec_accept_sample_nucleus(const void* logits, int M, int n, int top_k, float top_p, float temperature,
                                   const float* uniform, unsigned long long seed, unsigned long long* counter,
                                   const int32_t* window, int32_t* sampled, int32_t* out, int32_t* token_inout,
                                   int64_t* pos_inout, lga_stream_t stream);

/* -- fp32 forward (the reference's --precision 32-true, generate/base.py:132; BASELINE config 1 pythia-160m fp32):
 *    float32 weights and activations, no bf16 rounding; plumbing-sized kernels (csrc/fp32.hip) -------------- */
/* y (M, N) = x (M, K) . w (N, K)^T (+ bias[N]) (+ residual (M, N)) — F.linear (lit_gpt/model.py:519,619,656,699-702) */
int lga_f32_linear(const float* x, const float* w, const float* bias, const float* residual, float* y, int M, int N,
                   int K, lga_stream_t stream);
/* torch.nn.LayerNorm over rows of n (config.py:137-144): two-pass mean / biased variance, (x - mean) * rstd * w + b */
int lga_f32_layernorm(const float* x, const float* w, const float* b, float* y, int rows, int n, float eps,
                      lga_stream_t stream);
/* F.gelu (exact erf, or tanh when approximate_tanh) — GptNeoxMLP (model.py:699-702) */
int lga_f32_gelu(const float* a, float* y, long n, int approximate_tanh, lga_stream_t stream);
/* y = a + b (the Block residual adds, model.py:584-593) */
int lga_f32_add(const float* a, const float* b, float* y, long n, lga_stream_t stream);
/* lga_rope_kv_append in fp32: apply_rope on the first rope_n_elem dims (model.py:641-644, 767-773) + KVCache.forward
 * (:788-795); caches (G, max_seq, hs) fp32 */
int lga_f32_rope_kv_append(const float* qkv, float* q_out, float* k_cache, float* v_cache, const int64_t* cache_pos,
                           const int64_t* rope_pos, const float* cos, const float* sin, int rope_rows, int T,
                           int n_head, int n_query_groups, int head_size, int rope_n_elem, int max_seq,
                           lga_stream_t stream);
/* SDPA (model.py:651, 658-665) in fp32: q (T, H, hs), caches (G, max_seq, hs), query t attends keys 0..input_pos[t];
 * y (T, H*hs). head_size <= 256, max_seq <= 32768. */
int lga_f32_attention(const float* q, const float* k_cache, const float* v_cache, const int64_t* input_pos, float* y,
                      int T, int n_head, int n_query_groups, int head_size, int max_seq, float scale,
                      lga_stream_t stream);
/* lga_argmax over fp32 logits (generate/base.py:30-47 at temperature 0) */
int lga_argmax_f32(const float* logits, int n, int64_t* out_idx, int32_t* token_out, int64_t* pos_inout,
                   lga_stream_t stream);

/* -- log-likelihood scoring (eval/lm_eval_harness.py: log_softmax over the model's full output, gathered at the
 *    continuation tokens, and the greedy match) — csrc/score.hip --------------------------------------------------
 * logits: rows x n, contiguous row-major, bf16 (2-B aligned; any n, rows need no further alignment), n <= 2^30.
 * One pass per row (running max and sum in fp32; the logits are read once), fixed reduction order per row: a row's
 * result depends on neither `rows` nor the row's position.
 *   logprob_out[r] = float(x[r, t_r]) - (m_r + log sum_j exp(float(x[r, j]) - m_r)),  m_r = max_j x[r, j]
 *   argmax_out[r]  = lga_argmax's choice for the row (torch.argmax order: NaN first, ties to the lowest index)
 * -inf entries contribute 0; a -inf target gives -inf; a row holding NaN or +inf, or all -inf, gives NaN (as
 * torch.log_softmax); a target outside [0, n) gives NaN and reads nothing. No allocation, no workspace. */
int lga_token_logprobs(const void* logits, int rows, int n, const int32_t* targets, float* logprob_out,
                       int32_t* argmax_out, lga_stream_t stream);
/* the same over fp32 logits (--precision 32-true) */
int lga_token_logprobs_f32(const float* logits, int rows, int n, const int32_t* targets, float* logprob_out,
                           int32_t* argmax_out, lga_stream_t stream);
/* Two models' logits for the same rows (bf16, rows x n each), one pass over both:
 *   kl_out[r]    = sum_j softmax(p_r)_j (log_softmax(p_r)_j - log_softmax(q_r)_j), evaluated as
 *                  E_p[p_j - q_j] - (lse(p_r) - lse(q_r)); not clamped (may be slightly negative); entries of zero
 *                  weight under p contribute 0
 *   agree_out[r] = 1 when both rows have the same argmax (rule above), else 0 */
int lga_logits_kl(const void* p_logits, const void* q_logits, int rows, int n, float* kl_out, int32_t* agree_out,
                  lga_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LITGPT_AMD_H */
