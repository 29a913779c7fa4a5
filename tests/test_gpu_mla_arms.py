"""MLA attention (xllm_amd/csrc/attention_mla.hip) on the GPU: every launch arm, length edge and rescale against TWO references.

Every test first asserts, through the read-only query xllm_mi355_mla_plan, the launch arm and the split-KV count its shape takes:
the table's (tests/_mla_cases.py) with no MLA switch in the environment; min(n, 32, what the workspace holds) splits under
XLLM_MI355_MLA_SPLITS = n; the arm XLLM_MI355_MLA_PREFILL / _PREFILL_P dictate (tests/test_zz_gpu_variants.py re-runs this file
under seven such environments). Then it runs ops.mla_decode / ops.mla_prefill into an output pre-filled with NaN (the workspace
cases use the raw ABI) on inputs whose unreadable parts are NaN: rows past kv_len in each last page, three spare blocks, every
padding table entry (pointed at a spare block; all entries stay valid ids). Live rows between one wave's causal limit and its
group's longest are this step's tokens and stay finite: that is the contract.

Bars (the project's own, none derived from the kernels), per sequence:
  * hi + lo arms (0, 1, 2, 4): assert_attn_close against the fp32-P oracle AND the dense float64 reference rounded once, rel 1e-3
    (bf16) / 2e-4 (f16), element-wise 2 bf16 ulp of the row maximum;
  * one-P arm (3): assert_p16_attention_close with float64 as the fp32-P reference and the p_round=True / "flash" oracles;
  * per (query, head) row on top: twice the oracle's own largest row distance from float64 (ROW_BAR: 2.04e-3 / 3.50e-4 hi + lo,
    9.72e-3 / 1.22e-3 one P; tests/test_mla_reference.py re-measures it);
  * exact zeros on rows with kv_len = 0 and on rows that see no key; no non-finite element anywhere.
The mask-edge cases (decode plans, causal prefill) run with q scaled by 1/8 so that every key carries weight on every head:
tests/test_mla_reference.py shows that an edge off by ONE key moves every touched (query, head) row by >= 2.4 row bars.
The references alone (CPU): oracle vs float64 uses 0.15 (bf16) / 0.26 (f16) of the relative bar, <= 0.49 / 0.12 of the
element-wise bar (0.77 on the three bf16 calls test_mla_reference.py names, where no seed keeps one rounding flip out of a row's
top binade), 0.33 of the flash bar.

Largest distances measured on the MI355X as fractions of the bars (arm: bf16 / f16):
  arm 0 (staged)    fp32 oracle rel 0.31 / 0.24, elem 0.65 / 0.08; float64 rel 0.31 / 0.17, elem 0.65 / 0.08; row 0.35 / 0.27
  arm 1 (DMA)       fp32 oracle rel 0.18 / 0.18, elem 0.62 / 0.07; float64 rel 0.17 / 0.10, elem 0.62 / 0.07; row 0.39 / 0.28
  arm 2 (DMA, NT)   fp32 oracle rel 0.18 / 0.27, elem 0.53 / 0.08; float64 rel 0.18 / 0.19, elem 0.53 / 0.08; row 0.31 / 0.27
  arm 3 (one P)     float64 0.83 / 0.33, p_round 0.62 / 0.40, flash 0.17 / 0.07; row 0.50 / 0.49
  arm 4 (hi + lo tile sharing; under XLLM_MI355_MLA_PREFILL=1 XLLM_MI355_MLA_PREFILL_P=2, every prefill call on 64-token pages)
                    fp32 oracle rel 0.16 / 0.16, elem 0.85 / 0.12; float64 rel 0.20 / 0.11, elem 0.85 / 0.11; row 0.57 / 0.37
(an element-wise figure between 0.5 and 1.0 is one bf16 rounding flip of an element in the top binade of its row).
Per-token prefill (arms 0 / 1) is bit-equal to mla_decode on the last row of each sequence; a split-KV call run twice is
bit-identical.

Scratch mutations of attention_mla.hip (arithmetic and mask changes only, applied to a copy; this file run alone), tests that fail:
  1  `>= kv_len` -> `> kv_len` in both decode kernels' partial-tile mask: 44 (every decode, split, workspace, per-token and
     decode-family rescale test)
  2  `dead ? 0 : rk` -> `rk` in write_lds (staged kernel): NONE, and none can: the clamp in load_global has already replaced a
     dead row by a copy of the last LIVE row (finite), its score is masked to -inf, so its P is exactly 0 and 0 x finite = 0.
     The zeroing is a second guard behind the clamp; the clamp itself is an address and is not mutated here. What the poison
     does hold is the clamp (a staged kernel that loaded the rows past kv_len would multiply NaN) and the DMA kernels'
     num_records zero-fill.
  3  `>= kv_w` -> `> kv_w` in the tile-sharing kernel: 12 (share_h128 causal / full, share_h20, all six share rescale cases)
  4  mla_scale_acc x 1, and x twice the factor: 4 each (share jump and staircase, both dtypes; near_miss passes, as it must: the
     lazy kernel never rescales there, nor do the flat or unit-variance calls)
  5  lazy threshold `+ 8.0f` -> `+ 1000.0f`: 3 (share jump bf16, share staircase bf16 / f16)
  6  `acc_o[i] *= alpha` dropped in both decode kernels: 44
  7  `(base + s)` -> `(s * gridDim.x + bh)` in mla_merge_kernel: 8 (the six split-KV tests, room_for_2 in both dtypes)
  8  `l > 0 ? .. : 0` -> `o / l` in the merge and the three epilogues: 28 (every call with an empty row or a row without a key)
  9  f16 tr_read with its operand pairs swapped: 9 (every f16 test of the staged kernel, the only user of MlaTraits::tr_read; the
     DMA kernels read through inline ds_read_b64_tr_b16)
No kernel bug was found: all 57 tests passed on the unmodified library on their first run. 57 tests, 9 s."""
import pytest
import torch

import _mla_cases as mc
from _mla_cases import ops_workspace, query_plan

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DT_IDS = [mc.DTNAME[d] for d in mc.DTYPES]
_WORST = {}


def _note(label, value, name):
    if value > _WORST.get(label, (-1.0, None))[0]:
        _WORST[label] = (value, name)


def _noter(arm, dt):
    return lambda label, value, name: _note((arm, mc.DTNAME[dt]) + label, value, name)


def assert_plan(case, ws_bytes, ws_splits):
    """the arm and split-KV count the library takes for this call, asserted against the table (and the switches of the environment)"""
    got = query_plan(case, ws_bytes)
    assert got == mc.expected_plan(case, ws_splits), (case["name"], got, mc.expected_plan(case, ws_splits))
    return got


def nan_out(case):
    return torch.full((case["q"].shape[0], case["H"], mc.DV), float("nan"), dtype=case["dtype"], device=DEV)


def run(case, out=None):
    """ops.mla_decode / ops.mla_prefill on the case, into an output pre-filled with NaN"""
    from xllm_amd import ops
    out = nan_out(case) if out is None else out
    c = case
    if c["decode"]:
        ops.mla_decode(c["q"].to(DEV), c["kc"].to(DEV), c["kv_lens"].to(DEV), c["block_tables"].to(DEV), mc.DV, c["scale"],
                       c["max_kv_len"], out=out)
    else:
        ops.mla_prefill(c["q"].to(DEV), c["kc"].to(DEV), c["cu_q"].to(DEV), c["kv_lens"].to(DEV), c["block_tables"].to(DEV), mc.DV,
                        c["scale"], c["max_kv_len"], is_causal=c["causal"], out=out)
    torch.cuda.synchronize()
    return out


def plan_run_check(case):
    arm, nsplit = assert_plan(case, *ops_workspace(case))
    out = run(case)
    mc.check_output(case, out, arm, _noter(arm, case["dtype"]))
    return out, arm, nsplit


@pytest.mark.parametrize("dtype", mc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("plan", mc.DECODE_PLANS, ids=[p.name for p in mc.DECODE_PLANS])
def test_decode_arm_at_every_length_edge(plan, dtype):
    plan_run_check(mc.decode_case(plan, dtype))


@pytest.mark.parametrize("dtype", mc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("plan", mc.SPLIT_PLANS, ids=[p.name for p in mc.SPLIT_PLANS])
def test_split_kv_on_a_plan_sized_by_a_bound(plan, dtype):
    """max_kv_len is a bound of 2048: slices without a tile, rows with only empty slices. Run twice: bit-identical (no atomics)"""
    c = mc.split_case(plan, dtype)
    out, _, _ = plan_run_check(c)
    again = run(c)
    assert torch.equal(out.view(torch.int16), again.view(torch.int16))


@pytest.mark.parametrize("dtype", mc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("room", [2, 0], ids=["room_for_2", "no_workspace"])
def test_split_count_degrades_to_the_workspace(room, dtype):
    """raw ABI on the dma_nt split case: the buffer has the full 32-split size, only the byte count passed shrinks (room = 0: a NULL
    pointer and 0 bytes). The NaN canary behind the passed byte count stays untouched."""
    from xllm_amd import _lib
    c = mc.split_case(mc.SPLIT_PLANS[0], dtype)
    B, H = len(c["entries"]), c["H"]
    per = mc.per_split_bytes(B, H)
    passed = room * per
    arm, nsplit = assert_plan(c, passed, room)
    assert nsplit == max(1, min(room, mc.expected_plan(c, 32)[1]))
    ws = torch.full((32 * per // 4,), float("nan"), dtype=torch.float32, device=DEV)
    canary = ws.view(torch.int32).clone()
    out = nan_out(c)
    q, kc, lens, bt = c["q"].to(DEV), c["kc"].to(DEV), c["kv_lens"].to(DEV), c["block_tables"].to(DEV)
    rc = _lib.lib().xllm_mi355_mla_decode(q.data_ptr(), kc.data_ptr(), out.data_ptr(), lens.data_ptr(), bt.data_ptr(), bt.size(1), B, H,
                                          mc.D, mc.DV, c["bs"], kc.size(0), c["max_kv_len"], c["scale"],
                                          1 if dtype == torch.bfloat16 else 2, ws.data_ptr() if room else None, passed,
                                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, rc
    mc.check_output(c, out, arm, _noter(arm, dtype))
    assert torch.equal(ws.view(torch.int32)[passed // 4:], canary[passed // 4:]), "the call wrote behind the workspace it was given"
    if nsplit > 1:
        assert not torch.equal(ws.view(torch.int32)[:passed // 4], canary[:passed // 4])


PREFILL = [(c, causal) for c in mc.PREFILL_CALLS for causal in (True, False) if causal or c.name != "share_h20"]


@pytest.mark.parametrize("dtype", mc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("call,causal", PREFILL, ids=[f"{c.name}-{'causal' if k else 'full'}" for c, k in PREFILL])
def test_prefill_arm_at_every_group_and_mask_edge(call, causal, dtype):
    plan_run_check(mc.prefill_case(call, causal, dtype))


@pytest.mark.parametrize("dtype", mc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind", sorted(mc.RESCALE_LEVELS))
@pytest.mark.parametrize("fam", mc.RESCALE_FAMILIES, ids=[f.name for f in mc.RESCALE_FAMILIES])
def test_rescale_with_a_non_zero_accumulator(fam, kind, dtype):
    plan_run_check(mc.rescale_case(fam, kind, dtype))


@pytest.mark.parametrize("dtype", mc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("call", mc.PREFILL_CALLS[:2], ids=[c.name for c in mc.PREFILL_CALLS[:2]])
def test_per_token_prefill_is_the_decode_kernel_on_the_last_rows(call, dtype):
    """the per-token prefill form IS the decode kernel (one entry per query token): bit-equal to mla_decode on the last query row
    of every sequence when both calls take a hi + lo decode arm with the same split count; otherwise (a forced tile-sharing arm, a
    forced split count that only one workspace holds) the two agree within the bars of the looser arm"""
    pre, dec = mc.last_row_decode_case(call, dtype)
    p_arm, p_split = assert_plan(pre, *ops_workspace(pre))
    d_arm, d_split = assert_plan(dec, *ops_workspace(dec))
    out_p, out_d = run(pre), run(dec)
    last = out_p[pre["cu_q"][1:].long() - 1]
    mc.check_output(dec, out_d, d_arm, _noter(d_arm, dtype))
    if p_arm in (mc.ARM_STAGED, mc.ARM_DMA) and p_split == d_split:
        assert torch.equal(last.view(torch.int16), out_d.view(torch.int16))
    else:
        mc.check_output(dec, last, p_arm if p_arm == mc.ARM_SHARE_P1 else d_arm)


def test_zz_print_the_largest_distances():
    """file order: last. The largest distance per (arm, dtype, P form, reference, kind) as a fraction of its bar, for the docstring"""
    for k in sorted(_WORST, key=str):
        print("MLA_ARMS", k, "%.3f" % _WORST[k][0], _WORST[k][1])
