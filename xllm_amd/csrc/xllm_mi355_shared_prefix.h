/* xllm_mi355_shared_prefix.h -- C ABI of shared-prefix decode attention, an extension of include/xllm_mi355.h (same conventions:
 * XM_API, XM_ERR_* codes, dtype codes, XLLM_MI355_ABI_VERSION 2) exported by the same library. It is a header of its own because
 * include/, shim/ and INTEGRATION.md are pinned byte for byte by the reference-bound checks of tests/test_host_abi.py
 * (tests/golden/reference_checks.json, re-recorded only against the reference tree): folding these declarations into
 * include/xllm_mi355.h, and the shim function over them, belongs to a change that re-records those checks. */
#ifndef XLLM_MI355_SHARED_PREFIX_H_
#define XLLM_MI355_SHARED_PREFIX_H_

#include "../../include/xllm_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Shared-prefix decode: paged decode attention for a batch in which contiguous runs of sequences ("groups") name the same
 * physical pages in the leading entries of their block-table rows (a prefix cache hit on a common system prompt, a beam fork).
 * group_cu int32 [n_groups + 1] ascending, group_cu[0] = 0, group_cu[n_groups] = batch; for group g with P =
 * group_prefix_blocks[g] the caller promises, for every member b, block_table[b, 0:P] == block_table[group_cu[g], 0:P] and
 * kv_lens[b] >= P * block_size. P = 0 (no shared stage for the group; singletons, padding rows with kv_len 0) and groups of one
 * sequence with P > 0 are allowed. The grouping only says where the bytes are: the result is DEFINED as that of
 * xllm_mi355_paged_attention in decode form (max_q_len = 1, not causal, no window) on the same tensors; out [batch, nq * d],
 * 16-bit. The shared pages are read once per (group, kv head) by a stage of their own, the rest of every sequence by the decode
 * kernel on a shifted block table, and a merge launch combines the (o, m, l) partials of both. All metadata is device memory;
 * no host synchronisation, no allocation, a fixed grid for fixed scalars (capturable). max_prefix_blocks >= every
 * group_prefix_blocks[g]. prefix_splits: token ranges of the shared stage, 0 = the plan's (at most 8; a larger value is taken as 8).
 * Validation before any device work: NULL pointers, n_groups < 1, max_prefix_blocks > max_blocks: XM_ERR_INVALID; head_dim
 * other than 64 / 128, nq / nkv > 16, dtype other than bf16 / f16: XM_ERR_UNSUPPORTED; workspace_bytes below
 * xllm_mi355_shared_prefix_decode_workspace_bytes(): XM_ERR_WORKSPACE. There is no window: a caller with a binding window uses
 * xllm_mi355_paged_attention. The plan query is read-only (no launch): rows_per_tile = (sequence, q head) rows per wave of the
 * shared stage, prefix_splits, and the suffix stage's xllm_mi355_paged_decode_plan (hpw, nsplit). Any out pointer may be NULL. */
XM_API size_t xllm_mi355_shared_prefix_decode_workspace_bytes(int64_t batch, int64_t n_q_heads, int64_t head_dim,
                                                              int64_t max_blocks, int64_t max_kv_len, int64_t n_kv_heads);
XM_API int xllm_mi355_shared_prefix_decode_plan(int64_t batch, int64_t n_q_heads, int64_t n_kv_heads, int64_t block_size,
                                                int64_t max_prefix_blocks, int64_t max_kv_len, int32_t* rows_per_tile,
                                                int32_t* prefix_splits, int32_t* suffix_hpw, int32_t* suffix_nsplit);
XM_API int xllm_mi355_paged_decode_attention_shared_prefix(
    const void* q, const void* k_cache, const void* v_cache, void* out, const int32_t* kv_lens, const int32_t* block_table,
    int64_t max_blocks, const int32_t* group_cu, const int32_t* group_prefix_blocks, int64_t n_groups, int64_t batch,
    int64_t n_q_heads, int64_t n_kv_heads, int64_t head_dim, int64_t block_size, int64_t n_blocks, int64_t q_stride,
    int64_t max_kv_len, int64_t max_prefix_blocks, float scale, int prefix_splits, int dtype, void* workspace,
    size_t workspace_bytes, void* stream);

/* HOST side: the groups the operator above takes, from a host block table [batch, max_blocks] and kv_lens [batch].
 * Deterministic, in batch order, no reordering: a run opens at row i with c = kv_lens[i] / block_size (full pages only, at most
 * max_blocks); row j joins while c' = min(c, common leading entries of rows i and j, kv_lens[j] / block_size) >=
 * min_prefix_blocks, and then c = c'. A closed run of at least min_group rows becomes one group with c prefix blocks; a shorter
 * one, or one with c < min_prefix_blocks, leaves every row a group of its own with 0. Rows with kv_len == 0 are always groups of
 * their own with 0 (and close a run). group_cu [batch + 1] and group_prefix_blocks [batch] are caller buffers; *n_groups entries
 * (+ 1) of them are written. No GPU is touched. */
XM_API int xllm_mi355_host_shared_prefix_groups(const int32_t* block_table, int64_t max_blocks, const int32_t* kv_lens,
                                                int64_t batch, int64_t block_size, int64_t min_group, int64_t min_prefix_blocks,
                                                int32_t* group_cu, int32_t* group_prefix_blocks, int32_t* n_groups);

#ifdef __cplusplus
}
#endif
#endif /* XLLM_MI355_SHARED_PREFIX_H_ */
