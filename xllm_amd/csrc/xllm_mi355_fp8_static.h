/* xllm_mi355_fp8_static.h -- C ABI of the producer-side static e4m3 quantisation of the fp8 decode layer, an extension of
 * include/xllm_mi355.h (same conventions: XM_API, XM_ERR_* codes, dtype codes, XLLM_MI355_ABI_VERSION 2) exported by the same
 * library. A header of its own for the reason xllm_mi355_shared_prefix.h gives: include/, shim/ and INTEGRATION.md are pinned byte
 * for byte by the reference-bound checks of tests/test_host_abi.py; folding these declarations into include/xllm_mi355.h, and shim
 * functions over them, belongs to a change that re-records those checks.
 *
 * A static-scale fp8 checkpoint carries one f32 input_scale per linear (the reference's layers/common/linear.cpp:130-182). With
 * the scale known before the producer runs, the quantisation of a linear's operand is element-wise (no row or tensor
 * reduction), so the kernel that produces the 16-bit value can emit e4m3 instead: the activation for down_proj, the decode
 * attention for o_proj. Both functions are DEFINED by the operator pair they replace, byte for byte. Neither reads a device
 * value on the host, allocates or synchronises; both are capturable into a HIP graph. */
#ifndef XLLM_MI355_FP8_STATIC_H_
#define XLLM_MI355_FP8_STATIC_H_

#include "../../include/xllm_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out_q[t, i] = static_scaled_fp8_quant( act_and_mul(input)[t, i] ): byte for byte what xllm_mi355_act_and_mul followed by
 * xllm_mi355_static_scaled_fp8_quant(scale) writes (the 16-bit rounding of act_and_mul happens first, then e4m3 with the
 * clamp of common.h). The 16-bit intermediate is never stored. input [n_tokens, 2*d] 16-bit, scale: device f32 [1].
 * Same envelope and act modes as xllm_mi355_act_and_mul (any d > 0, any alignment: 16-byte loads and 8-byte stores where d % 8
 * == 0 and the bases allow them, element-wise otherwise); dtype bf16 / f16, anything else XM_ERR_UNSUPPORTED.
 * NULL out_q, input or scale, n_tokens < 0, d <= 0: XM_ERR_INVALID. */
XM_API int xllm_mi355_act_and_mul_static_fp8_quant(uint8_t* out_q, const void* input, const float* scale, int64_t n_tokens,
                                                   int64_t d, int act_mode, int dtype, void* stream);

/* Decode attention whose epilogue emits the static e4m3 quantisation of its 16-bit output: byte for byte
 * xllm_mi355_paged_attention (decode form) followed by xllm_mi355_static_scaled_fp8_quant(out_scale). out (16-bit) may be
 * NULL; out_q [batch, nq*d]; out_scale: device f32 [1]. Accepts every shape, window and launch plan the decode form of
 * xllm_mi355_paged_attention accepts; workspace as there (split-KV degrades to the workspace given). Plans with one grid split
 * quantise in the attention kernel's epilogue (one launch, no workspace); split-KV plans in the merge launch.
 * Validation before any device work: NULL q, caches, out_q, out_scale, kv_lens or block_table, and the scalar checks of
 * xllm_mi355_paged_attention: XM_ERR_INVALID; dtype other than bf16 / f16, head_dim other than 64 / 128, n_q_heads / n_kv_heads
 * > 16, misaligned q / caches: XM_ERR_UNSUPPORTED. */
XM_API int xllm_mi355_paged_decode_attention_fp8(const void* q, const void* k_cache, const void* v_cache, void* out, uint8_t* out_q,
                                                 const float* out_scale, const int32_t* kv_lens, const int32_t* block_table,
                                                 int64_t max_blocks, int64_t batch, int64_t n_q_heads, int64_t n_kv_heads,
                                                 int64_t head_dim, int64_t block_size, int64_t n_blocks, int64_t q_stride,
                                                 int64_t max_kv_len, float scale, int64_t window_left, int dtype, void* workspace,
                                                 size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* XLLM_MI355_FP8_STATIC_H_ */
