"""GPU: paged_decode_kernel at every launch plan and window edge against TWO references -- the CPU oracle
(orc.paged_attention) and the dense float64 restatement of tests/_decode_cases.py rounded to the tensor dtype -- under the bars
of tests/test_gpu_parity.py::assert_attn_close: relative L2 <= 1e-3 (bf16) / 2e-4 (f16) and 2 bf16 ulp of the row maximum
element-wise.

Every test first asserts, through xllm_mi355_paged_decode_plan, the plan its case is in the table for: heads per workgroup,
the KROWS and UNIFORM kernel arms, and -- unless XLLM_MI355_DECODE_SPLITS forces one -- the grid-level split count.

  plan (tests/_decode_cases.py::PLANS)         B   nq nkv   d  page   covered by
  hpw = 4, krows = 0 (the headline plan)      192  28   4  128  128   test_plan, test_window, test_int8_entry_point
  hpw = 4, krows = 1, uniform = 0              48  32  16  128   16   test_plan, test_window
  hpw = 2, krows = 1                           96  28   4  128  128   test_plan, test_window
  hpw = 2, krows = 0, d = 64                  192  14   2   64   64   test_plan
  hpw = 4, krows = 0, d = 64, uniform = 0     192  16   4   64   16   test_plan
  hpw = 1 control                               4  28   4  128  128   test_plan, test_window
  hpw = 1, 2 grid splits (8 slots)              3  28   4  128  128   test_window_under_split_kv

All inputs are poisoned (NaN in K, Inf in V) wherever the kernel may load but must not use: past kv_len, below the window's
lower bound t_lo, in spare blocks that the table entries of pages wholly below the window point at.

Room between the two references (tests/test_decode_reference.py measures it on the CPU, over every case of the tables, and
asserts half a bar): largest relative L2 distance oracle vs float64 4.96e-05 for bf16 (0.05 of the bar; window, hpw = 1
control, W = 100) and 3.07e-05 for f16 (0.15 of the bar; split-KV, W = 100); largest element-wise distance 0.45 of the bar
for bf16 (window, headline plan, W = 5: one bf16 rounding flip next to the row maximum) and 0.09 for f16.

What these tests catch, each tried on a scratch build of attention_decode.hip:
  * the window mask of compute_tile (`tok < t_lo`) removed, or the V rows below t_lo not zeroed: every test_window with a
    binding W, test_window_under_split_kv and test_int8_entry_point[W40] fail (non-finite output);
  * the epilogue merge indexed `h_s * nsub + sb` instead of `sb * hpw + h_s`: test_plan[hpw2_krows], test_plan[hpw2_d64] and
    every test_window[hpw2_krows] fail -- the two orders agree at hpw = 4 and hpw = 1, which is all the suite reached before;
  * the zeroing of the V rows past kv_len removed ALONE: nothing fails, and nothing can -- issue_loads clamps every token index
    to kv_len - 1, so a row past kv_len never reaches a register and the tile's tail holds copies of the last valid row. With
    the clamp of the V loads removed as well, every test whose last tile is partial fails: the zeroing is the second of two
    guards, and the poisoned tails hold the pair."""
import os

import pytest
import torch

import _decode_cases as dc
from oracle import oracle as orc
from test_gpu_parity import assert_attn_close

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from xllm_amd import _lib, ops
DEV = "cuda"
_NAME = {torch.bfloat16: "bf16", torch.float16: "f16"}
_ids = lambda xs: [x.name if hasattr(x, "name") else _NAME.get(x, f"W{x}") for x in xs]


def _assert_plan(plan, max_kv_len):
    import ctypes as C
    hpw, nsplit, krows, uniform = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    rc = _lib.lib().xllm_mi355_paged_decode_plan(plan.B, plan.nkv, plan.bs, max_kv_len, C.byref(hpw), C.byref(nsplit),
                                                 C.byref(krows), C.byref(uniform))
    assert rc == 0
    assert (hpw.value, krows.value, uniform.value) == (plan.hpw, plan.krows, plan.uniform), \
        f"{plan.name}: the planner gives hpw={hpw.value} krows={krows.value} uniform={uniform.value}"
    forced = os.environ.get("XLLM_MI355_DECODE_SPLITS")
    if forced is None:
        assert nsplit.value == plan.nsplit, f"{plan.name}: {nsplit.value} splits"
    elif int(forced) > 0:
        assert nsplit.value == min(int(forced), 32)


def _on_gpu(case):
    return (case["q"].to(DEV), case["kc"].to(DEV), case["vc"].to(DEV), case["kv_lens"].to(DEV), case["block_tables"].to(DEV))


def _assert_meets_both(out, case, key):
    orc_out, ref64 = dc.references(case, key)
    rel = dc.BAR_REL[case["dtype"]]
    for name, ref in (("oracle", orc_out), ("float64", ref64)):
        print(f"{key}: kernel vs {name} (rel L2 / bar, element-wise / bar) = {dc.distance(out, ref)[0] / rel:.3f}, "
              f"{dc.distance(out, ref)[1]:.3f}")
    assert_attn_close(out, orc_out, rel=rel)
    assert_attn_close(out, ref64, rel=rel)
    assert not out[(case["kv_lens"] == 0).to(out.device)].any()


def _run_and_check(key, case):
    _assert_plan(case["plan"], case["max_kv_len"])
    q, kc, vc, kv, bt = _on_gpu(case)
    out = ops.paged_attention(q, kc, vc, None, kv, bt, 1, case["max_kv_len"], case["scale"],
                              window_left=case["window_left"])
    _assert_meets_both(out, case, key)


@pytest.mark.parametrize("dtype", dc.DTYPES, ids=_ids(dc.DTYPES))
@pytest.mark.parametrize("plan", dc.PLANS, ids=_ids(dc.PLANS))
def test_plan(plan, dtype):
    """ragged lengths 1 ... 300 and one empty row at each launch plan, poisoned tails"""
    _run_and_check(*dc.plan_case(plan, dtype))


@pytest.mark.parametrize("dtype", dc.DTYPES, ids=_ids(dc.DTYPES))
@pytest.mark.parametrize("W", dc.WINDOWS, ids=_ids(dc.WINDOWS))
@pytest.mark.parametrize("plan", dc.WINDOW_PLANS, ids=_ids(dc.WINDOW_PLANS))
def test_window(plan, W, dtype):
    """one window_left per call; the lengths of the batch put t_lo at 0, 1, on / one short of a tile boundary, on a 16-token
    page boundary inside a tile, and leave rows the window does not bind (2**40: none bound, clamped by the launcher).
    Everything below t_lo is NaN / Inf, and pages wholly below it are table entries of a poisoned spare block."""
    for key, case in dc.window_cases(plan, W, dtype):
        _run_and_check(key, case)


@pytest.mark.parametrize("dtype", dc.DTYPES, ids=_ids(dc.DTYPES))
@pytest.mark.parametrize("W", dc.SPLIT_WINDOWS, ids=_ids(dc.SPLIT_WINDOWS))
def test_window_under_split_kv(W, dtype):
    """hpw = 1 with 2 grid splits = 8 slots per (sequence, head); the window leaves the longest row 3, 5 or 34 tiles, so slots
    own no tile and the edge tile is the first live slot's"""
    _run_and_check(*dc.split_window_case(W, dtype))


@pytest.mark.parametrize("dtype", dc.DTYPES, ids=_ids(dc.DTYPES))
@pytest.mark.parametrize("W", dc.INT8_WINDOWS, ids=_ids(dc.INT8_WINDOWS))
def test_int8_entry_point(W, dtype):
    """headline plan through paged_decode_attention_int8 (the fused int8 epilogue; the finishing launch under a forced split
    count), with and without a binding window: the 16-bit output meets both references, and (q, scale) is scaled_quantize of
    that output bit for bit"""
    key, case = dc.int8_case(W, dtype)
    _assert_plan(case["plan"], case["max_kv_len"])
    q, kc, vc, kv, bt = _on_gpu(case)
    r = ops.paged_decode_attention_int8(q, kc, vc, kv, bt, case["max_kv_len"], case["scale"], window_left=W, want_16bit=True)
    assert r is not None, "the headline plan must not decline the fusion"
    oq, os_, o16 = r
    _assert_meets_both(o16, case, key)
    rq, rs = orc.scaled_quantize(o16.cpu())
    assert torch.equal(oq.cpu(), rq) and torch.equal(os_.cpu(), rs)
