/* xllm_mi355_kv_fp8.h -- C ABI of the e4m3 paged KV cache with static per-tensor scales (kv_cache_dtype = fp8): the two KV writers,
 * decode attention over such a cache and its launch plan as a read-only query. An extension of include/xllm_mi355.h (same
 * conventions: XM_API, XM_ERR_* codes, dtype codes, XLLM_MI355_ABI_VERSION 2) exported by the same library. A header of its own for
 * the reason xllm_mi355_shared_prefix.h gives: include/, shim/ and INTEGRATION.md are pinned byte for byte by the reference-bound
 * checks of tests/test_host_abi.py; folding these declarations into include/xllm_mi355.h, and shim functions over them, belongs to
 * a change that re-records those checks.
 *
 * A static-scale fp8 checkpoint carries one f32 k_scale and one v_scale per attention layer. The cache keeps its layout
 * [n_blocks, block_size, n_kv_heads, head_dim], K and V separate, ONE byte per element: OCP e4m3fn codes, and a code c stands for
 * the value float(c) * scale. The quantisation rule is the one of xllm_mi355_static_scaled_fp8_quant:
 * e4m3fn(clamp(x * (1 / scale), +-448)), round to nearest even. Every scale is a device f32 [1]. No entry point reads a device
 * value on the host, allocates or synchronises; all are capturable into a HIP graph. */
#ifndef XLLM_MI355_KV_FP8_H_
#define XLLM_MI355_KV_FP8_H_

#include "../../include/xllm_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif

/* KV write into an e4m3 cache: byte for byte xllm_mi355_static_scaled_fp8_quant of k (k_scale) and of v (v_scale) followed by a
 * byte scatter of row t to slot slot_ids[t]. k / v: 16-bit [n_tokens, n_kv_heads, head_dim] with token strides k_stride / v_stride
 * (elements); slot < 0 and slots beyond n_blocks * block_size are skipped as xllm_mi355_reshape_paged_cache skips them.
 * NULL pointers, n_tokens < 0, n_kv_heads <= 0, head_dim <= 0, block_size <= 0: XM_ERR_INVALID; dtype other than bf16 / f16:
 * XM_ERR_UNSUPPORTED. Any alignment (16-byte loads and 8-byte stores where the rows allow them, element-wise otherwise). */
XM_API int xllm_mi355_reshape_paged_cache_kv8(const int32_t* slot_ids, const void* k, const void* v, uint8_t* k_cache,
                                              uint8_t* v_cache, const float* k_scale, const float* v_scale, int64_t n_tokens,
                                              int64_t n_kv_heads, int64_t head_dim, int64_t block_size, int64_t n_blocks,
                                              int64_t k_stride, int64_t v_stride, int dtype, void* stream);

/* RoPE on q and k in place (16-bit, bit-identical to xllm_mi355_rotary_embedding) and the KV write of the rotated k and of v into
 * an e4m3 cache: the bytes of the operator sequence rotate -> quantise -> scatter (the rotated k is rounded to 16 bits as it is
 * stored, then quantised). The arguments of xllm_mi355_rotary_embedding_and_cache plus the two scales, with its validation; dtype
 * other than bf16 / f16: XM_ERR_UNSUPPORTED. */
XM_API int xllm_mi355_rotary_embedding_and_cache_kv8(const int64_t* positions, void* q, void* k, const void* v,
                                                     const void* cos_sin_cache, const int32_t* slot_ids, uint8_t* k_cache,
                                                     uint8_t* v_cache, const float* k_scale, const float* v_scale,
                                                     int64_t n_tokens, int64_t n_q_heads, int64_t n_kv_heads, int64_t head_size,
                                                     int64_t rot_dim, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                                                     int64_t block_size, int64_t n_blocks, int is_neox, int dtype, void* stream);

/* Decode attention (one query token per sequence) over an e4m3 cache: the result is DEFINED as decode attention over the
 * dequantised cache, codes * scale. q [batch, n_q_heads, head_dim] with token stride q_stride, out [batch, n_q_heads * head_dim],
 * both bf16 or f16. The other arguments are those of the decode form of xllm_mi355_paged_attention; the workspace bound is
 * xllm_mi355_paged_attention_workspace_bytes, and split-KV degrades to the workspace given (none: one grid split).
 * Sequences of 0 tokens give zero rows; window_left follows xllm_mi355_paged_attention.
 * Validation before any device work: NULL q, caches, scales, out, kv_lens or block_table, and the scalar checks of
 * xllm_mi355_paged_attention: XM_ERR_INVALID; head_dim other than 64 / 128, n_q_heads / n_kv_heads > 16, dtype other than
 * bf16 / f16, q / caches not 16-byte aligned, q_stride % 8: XM_ERR_UNSUPPORTED. */
XM_API int xllm_mi355_paged_decode_attention_kv8(const void* q, const uint8_t* k_cache, const uint8_t* v_cache,
                                                 const float* k_scale, const float* v_scale, void* out, const int32_t* kv_lens,
                                                 const int32_t* block_table, int64_t max_blocks, int64_t batch, int64_t n_q_heads,
                                                 int64_t n_kv_heads, int64_t head_dim, int64_t block_size, int64_t n_blocks,
                                                 int64_t q_stride, int64_t max_kv_len, float scale, int64_t window_left, int dtype,
                                                 void* workspace, size_t workspace_bytes, void* stream);

/* The launch plan xllm_mi355_paged_decode_attention_kv8 takes for these scalars: launcher and query call one function
 * (kv8_plan, attention_decode_kv8.hip). No launch, no device work, no allocation. workspace_bytes: what the caller would pass
 * (0 for a NULL workspace).
 *   hpw             kv heads per workgroup (4 waves = hpw heads x 4 / hpw token sub-ranges): 1, 2 or 4
 *   nsplit_planned  grid-level split-KV count the planner asks for
 *   nsplit          the count after degradation to what workspace_bytes holds (1 = no partials, no merge launch)
 *   uniform         1: block_size % 32 == 0, a 32-token tile lives in one page (one scalar page lookup per tile);
 *                   0: gathered tiles (a page lookup per row)
 * There is one fetch layout (K straight into the MFMA operand layout, V by whole rows). Any out pointer may be NULL.
 * batch <= 0, n_q_heads <= 0, n_kv_heads <= 0, n_q_heads % n_kv_heads, block_size <= 0, max_kv_len < 0: XM_ERR_INVALID;
 * head_dim other than 64 / 128: XM_ERR_UNSUPPORTED. */
XM_API int xllm_mi355_paged_decode_kv8_plan(int64_t batch, int64_t n_q_heads, int64_t n_kv_heads, int64_t head_dim,
                                            int64_t block_size, int64_t max_kv_len, size_t workspace_bytes, int32_t* hpw,
                                            int32_t* nsplit_planned, int32_t* nsplit, int32_t* uniform);

#ifdef __cplusplus
}
#endif
#endif /* XLLM_MI355_KV_FP8_H_ */
