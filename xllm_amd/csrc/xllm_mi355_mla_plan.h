/* xllm_mi355_mla_plan.h -- the launch plan of MLA attention as a read-only query, an extension of include/xllm_mi355.h (same
 * conventions: XM_API, XM_ERR_* codes, XLLM_MI355_ABI_VERSION 2) exported by the same library. It is a header of its own because
 * include/, shim/ and INTEGRATION.md are pinned byte for byte by the reference-bound checks of tests/test_host_abi.py
 * (tests/golden/reference_checks.json, re-recorded only against the reference tree): folding this declaration into
 * include/xllm_mi355.h belongs to a change that re-records those checks. */
#ifndef XLLM_MI355_MLA_PLAN_H_
#define XLLM_MI355_MLA_PLAN_H_

#include "../../include/xllm_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The kernel and the split-KV count xllm_mi355_mla_decode (total_q_tokens = 0, `batch` sequences) or xllm_mi355_mla_prefill
 * (total_q_tokens > 0) takes for these scalars: the launchers and this query call one function (mla_plan, attention_mla.hip).
 * No launch, no device work, no allocation; it reads the switches XLLM_MI355_MLA_SPLITS / _MLA_PREFILL / _MLA_PREFILL_P through
 * the same read-once statics as the launchers. workspace_bytes is the byte count the caller would pass to the entry point (0 for
 * a NULL workspace); for the prefill form that includes the per-token index arrays in front of the partials.
 *   arm 0  mla_decode_kernel<T, false>        register-staged tiles: block_size % 64 != 0
 *   arm 1  mla_decode_dma_kernel<T, false>    LDS-DMA tiles
 *   arm 2  mla_decode_dma_kernel<T, true>     LDS-DMA tiles, non-temporal: decode form with n_heads <= 16
 *   arm 3  mla_prefill_dma_kernel<T, true>    four query tokens share a tile, one rounded P
 *   arm 4  mla_prefill_dma_kernel<T, false>   four query tokens share a tile, P = hi + lo
 * nsplit: split-KV slices per (entry, head block) AFTER degradation to what workspace_bytes holds (1 = no partials, no merge
 * launch; always 1 for arms 3 and 4). Either out pointer may be NULL.
 * batch <= 0, total_q_tokens < 0, n_heads <= 0, block_size <= 0, max_kv_len < 0: XM_ERR_INVALID; prefill form with
 * workspace_bytes below the index arrays (256-byte rounded 8 * total_q_tokens): XM_ERR_WORKSPACE, as the entry point answers. */
XM_API int xllm_mi355_mla_plan(int64_t batch, int64_t total_q_tokens, int64_t n_heads, int64_t block_size, int64_t max_kv_len,
                               size_t workspace_bytes, int32_t* arm, int32_t* nsplit);

#ifdef __cplusplus
}
#endif
#endif /* XLLM_MI355_MLA_PLAN_H_ */
