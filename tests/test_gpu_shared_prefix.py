"""GPU: ops.paged_attention_shared_prefix (prologue, suffix stage = paged_decode_kernel on a shifted table, shared stage, merge)
against TWO references on the same tensors -- the dense float64 restatement of tests/_decode_cases.py rounded to the dtype, and
ops.paged_attention (the existing kernel, which the operator's result is defined as) -- both under the bar of
tests/test_gpu_decode_plans.py: relative L2 <= 1e-3 (bf16) / 2e-4 (f16) and 2 bf16 ulp of the row maximum element-wise.

Every case first asserts, through xllm_mi355_shared_prefix_decode_plan, the rows per tile and token splits of the shared stage
and the suffix stage's heads per workgroup and grid splits it is in tests/_shared_prefix_cases.py for. Inputs are poisoned
(NaN in K, Inf in V past every kv_len and in the spare blocks the table padding points at), and the workspace is filled with NaN
bit patterns before each call: a partial the call consumes but did not write shows as a non-finite output.

  case            B  nq nkv   d page  groups (members x shared pages)                 shared splits  suffix plan
  g7             24  28   4 128  128  1x0, 2x1, 3x2, 5x3, 13x1 (one row agrees beyond P)     3        hpw 1, 1 split
  g7 forced      24  ...              the same, prefix_splits = 1, 2, 5 (5 > tiles of P = 1: empty splits)
  g2_page16      40  32  16 128   16  9x1, 8x2, 1x3, 22x21 (16 ... 336 tokens)               2        hpw 2, 1 split
  d64            12  14   2  64   64  4x1, 8x5                                               2        hpw 1, 1 split
  suffix_split2   3  28   4 128  128  3x2, suffixes 2500 / 1000 / 130                        2        hpw 1, 2 splits
  b192_hpw4     192  28   4 128  128  12 groups of 16x1                                      1        hpw 4, 1 split
  singletons      8                   every row alone, no prefix, one empty row: bit-identical to ops.paged_attention
  all_prefix     24                   one group, kv_len = 2 pages everywhere (every suffix empty)
  padding_rows    9                   kv_len = 0 rows between and behind two groups"""
import os

import pytest
import torch

import _decode_cases as dc
import _shared_prefix_cases as sp
from _bars import assert_attn_close

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from xllm_amd import _lib, ops
DEV = "cuda"
_NAME = {torch.bfloat16: "bf16", torch.float16: "f16"}
_dt_ids = [_NAME[d] for d in sp.DTYPES]


def _assert_plan(c, forced_prefix=0):
    nq, nkv, d, bs = c["case"].shape
    rows, psplit, hpw, nsplit = ops.shared_prefix_decode_plan(c["B"], nq, nkv, bs, c["max_prefix_blocks"], c["max_kv_len"])
    want = c["case"].plan
    assert (rows, psplit, hpw) == want[:3], f"{c['case'].name}: the planner gives rows={rows} prefix_splits={psplit} hpw={hpw}"
    forced = os.environ.get("XLLM_MI355_DECODE_SPLITS")
    if forced is None:
        assert nsplit == want[3], f"{c['case'].name}: {nsplit} suffix splits"
    elif int(forced) > 0:
        assert nsplit == min(int(forced), 32)
    return nsplit


def _on_gpu(c):
    return [c[k].to(DEV) for k in ("q", "kc", "vc", "kv_lens", "block_tables", "group_cu", "group_prefix_blocks")]


def _poison_workspace(c):
    nq, nkv, d, bs = c["case"].shape
    need = _lib.lib().xllm_mi355_shared_prefix_decode_workspace_bytes(c["B"], nq, d, c["block_tables"].size(1), c["max_kv_len"], nkv)
    need = max(need, _lib.lib().xllm_mi355_paged_attention_workspace_bytes(c["B"], nq, d, 1, c["B"]))
    ops._attn_workspace(torch.device(DEV, torch.cuda.current_device()), need).fill_(0xFF)   # 0xFFFFFFFF: NaN as f32, -1 as int32


def _run(c, dev, prefix_splits=0):
    q, kc, vc, kv, bt, cu, pre = dev
    _poison_workspace(c)
    return ops.paged_attention_shared_prefix(q, kc, vc, kv, bt, cu, pre, c["max_kv_len"], c["max_prefix_blocks"], c["scale"],
                                             prefix_splits=prefix_splits)


def _plain(c, dev):
    q, kc, vc, kv, bt = dev[:5]
    return ops.paged_attention(q, kc, vc, None, kv, bt, 1, c["max_kv_len"], c["scale"])


def _assert_meets_both(out, c, key, dev):
    rel = dc.BAR_REL[c["dtype"]]
    ref64, plain = sp.reference(c, key), _plain(c, dev)
    for name, ref in (("float64", ref64), ("paged_attention", plain)):
        r, e = dc.distance(out, ref)
        print(f"{key}: shared-prefix vs {name} (rel L2 / bar, element-wise / bar) = {r / rel:.3f}, {e:.3f}")
    assert_attn_close(out, ref64, rel=rel)
    assert_attn_close(out, plain, rel=rel)
    assert not out[(c["kv_lens"] == 0).to(out.device)].any()
    return plain


@pytest.mark.parametrize("dtype", sp.DTYPES, ids=_dt_ids)
@pytest.mark.parametrize("name", ["g7", "g2_page16", "d64", "suffix_split2", "b192_hpw4", "all_prefix", "padding_rows"])
def test_case(name, dtype):
    key, c = sp.seeded(sp.CASE[name], dtype)
    sp.check_promise(c)
    _assert_plan(c)
    dev = _on_gpu(c)
    _assert_meets_both(_run(c, dev), c, key, dev)


@pytest.mark.parametrize("dtype", sp.DTYPES, ids=_dt_ids)
@pytest.mark.parametrize("splits", [1, 2, 5])
def test_forced_prefix_splits(splits, dtype):
    """g7 with the token splits of the shared stage forced: 5 exceeds the 4 tiles of the P = 1 groups, so their last split owns
    no tile and must still leave a partial the merge can consume"""
    key, c = sp.seeded(sp.CASE["g7"], dtype)
    _assert_plan(c)
    dev = _on_gpu(c)
    _assert_meets_both(_run(c, dev, prefix_splits=splits), c, key, dev)


@pytest.mark.parametrize("dtype", sp.DTYPES, ids=_dt_ids)
def test_singletons_without_prefix_are_the_plain_kernel_bit_for_bit(dtype):
    """no shared stage anywhere: the suffix stage is the decode kernel on the caller's own table and lengths, and with one split
    the merge reproduces its epilogue exactly"""
    key, c = sp.seeded(sp.CASE["singletons"], dtype)
    nsplit = _assert_plan(c)
    dev = _on_gpu(c)
    out = _run(c, dev)
    plain = _assert_meets_both(out, c, key, dev)
    if nsplit == 1:
        assert torch.equal(out, plain)


@pytest.mark.parametrize("dtype", sp.DTYPES, ids=_dt_ids)
def test_graph_replay_follows_rewritten_metadata(dtype):
    """one captured call; kv_lens, block_table and both group arrays are then rewritten in place with another grouping of the
    same batch (same group count: that one is a host scalar) over other cache contents, and the replay must follow them"""
    key_a, a = sp.seeded(sp.CASE["g7"], dtype)
    key_b, b = sp.seeded(sp.G7_REGROUPED, dtype)
    assert a["B"] == b["B"] and a["group_cu"].numel() == b["group_cu"].numel()
    nb, width = max(a["kc"].size(0), b["kc"].size(0)), max(a["block_tables"].size(1), b["block_tables"].size(1))
    max_kv, max_pre = max(a["max_kv_len"], b["max_kv_len"]), max(a["max_prefix_blocks"], b["max_prefix_blocks"])

    def padded(c):
        kc = torch.full((nb,) + tuple(c["kc"].shape[1:]), float("nan"), dtype=dtype)
        vc = torch.full((nb,) + tuple(c["vc"].shape[1:]), float("inf"), dtype=dtype)
        kc[:c["kc"].size(0)], vc[:c["vc"].size(0)] = c["kc"], c["vc"]
        bt = torch.zeros(c["B"], width, dtype=torch.int32)
        bt[:, :c["block_tables"].size(1)] = c["block_tables"]
        return dict(c, kc=kc, vc=vc, block_tables=bt, max_kv_len=max_kv, max_prefix_blocks=max_pre)

    a, b = padded(a), padded(b)
    _assert_plan(a)
    bufs = _on_gpu(a)
    out = torch.empty(a["B"], a["q"].size(1) * a["q"].size(2), dtype=dtype, device=DEV)
    call = lambda: ops.paged_attention_shared_prefix(*bufs, max_kv, max_pre, a["scale"], out=out)
    _poison_workspace(a)
    call()                                                              # eager once: sizes the workspace outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            call()
    torch.cuda.current_stream().wait_stream(side)
    for c, key in ((b, key_b), (a, key_a)):
        for buf, src in zip(bufs, _on_gpu(c)):
            buf.copy_(src)
        _poison_workspace(c)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        rel = dc.BAR_REL[dtype]
        assert_attn_close(out, sp.reference(c, key), rel=rel)
        assert_attn_close(out, _plain(c, bufs), rel=rel)
