"""GPU: the epilogue of paged_decode_kernel -- one pass over work items (head slot, live query head, 8 consecutive d), the
int8 form quantising from registers, 16-byte / 8-byte stores where the output bases allow them and element-wise stores in the
same loop where they do not.

The epilogue only reorders who computes what, so the checks are bit equalities wherever two paths exist for one result:

  * the int8 entry (q8, scale, 16-bit out) == paged_attention -> scaled_quantize, at the three in-workgroup merge arms the
    int8 epilogue admits (nsub = 1, 2, 4) and at group sizes G = 1, 7, 8, 16 (G = 16 fills the MFMA width: 1024 work items, four
    per thread; G = 1 leaves most threads without one);
  * outputs whose base is one element off alignment (element-wise stores) == the aligned outputs (wide stores), for the 16-bit
    store, the int8 store and the fp32 partials of the split-KV form.

The plain and split-KV arms (hpw = 2 with two head groups, hpw = 1, partials -> merge) meet the CPU oracle and the dense
float64 reference of tests/_decode_cases.py under the bars of assert_attn_close, as tests/test_gpu_decode_plans.py does.

All inputs are poisoned (tests/_decode_cases.py::poison); lengths are ragged_lens(B): 1, 31 ... 33, 63 ... 65, 127 ... 129, 257,
300 and one empty row, which must come out as zeros with scale 0. Every launch's plan is asserted first."""
import ctypes as C

import pytest
import torch

import _decode_cases as dc
from test_gpu_decode_plans import _assert_meets_both, _assert_plan, _on_gpu

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from xllm_amd import _lib, ops
DEV = "cuda"
_NAME = {torch.bfloat16: "bf16", torch.float16: "f16"}
_DT = {torch.bfloat16: 1, torch.float16: 2}    # XM_BF16, XM_F16 of include/xllm_mi355.h

# plans of the int8 epilogue: all kv heads of a token in one workgroup (nkv / hpw == 1), one grid split. B = 192 is the smallest
# batch at which decode_heads_per_wg gives hpw = 4 with nkv = 4 (and hpw = 2 with nkv = 2): B * nkv / hpw >= 192.
INT8_PLANS = [
    dc.PLAN["hpw4_headline"],                                                          # G = 7, nsub = 1, 448 items
    dc.PLAN["hpw2_d64"],                                                               # G = 7, nsub = 2, D = 64
    dc.Plan("hpw1_nkv1", 4, 7, 1, 128, 128, hpw=1, krows=0, uniform=1, nsplit=1),      # G = 7, nsub = 4, 112 items
    dc.Plan("hpw4_g1", 192, 4, 4, 128, 128, hpw=4, krows=0, uniform=1, nsplit=1),      # G = 1: 64 items
    dc.Plan("hpw4_g8", 192, 32, 4, 128, 128, hpw=4, krows=0, uniform=1, nsplit=1),     # G = 8: 512 items, two per thread
    dc.Plan("hpw4_g16", 192, 64, 4, 128, 128, hpw=4, krows=0, uniform=1, nsplit=1),    # G = 16: 1024 items, four per thread
]
_pid = lambda ps: [p.name for p in ps]
_did = lambda ds: [_NAME[d] for d in ds]


def _case(plan, dtype, window_left=-1):
    """the table's own case (and seed) where the plan is in the table, so the references are shared with the other files"""
    if window_left < 0 and plan in dc.PLANS:
        return dc.plan_case(plan, dtype)
    key = ("epilogue", plan.name, window_left, dtype)
    return key, dc.make_case(plan, dc.ragged_lens(plan.B), dtype, seed=4000 + plan.nq, window_left=window_left)


def _two_launches(case):
    """paged_attention -> scaled_quantize"""
    q, kc, vc, kv, bt = _on_gpu(case)
    o = ops.paged_attention(q, kc, vc, None, kv, bt, 1, case["max_kv_len"], case["scale"], window_left=case["window_left"])
    rq, rs = ops.scaled_quantize(o)
    return o, rq, rs


def _assert_int8_equal(case, got, want):
    (oq, os_, o16), (o, rq, rs) = got, want
    assert torch.equal(o16.view(torch.int16), o.view(torch.int16)), "16-bit output"
    assert torch.equal(os_, rs), "scale"
    assert torch.equal(oq, rq), "int8 output"
    empty = (case["kv_lens"] == 0).to(DEV)
    assert int(empty.sum()) == 1
    assert not o16[empty].any() and not oq[empty].any() and not os_[empty].any()
    assert torch.isfinite(o16.float()).all()


@pytest.mark.parametrize("dtype", dc.DTYPES, ids=_did(dc.DTYPES))
@pytest.mark.parametrize("plan", INT8_PLANS, ids=_pid(INT8_PLANS))
def test_int8_epilogue_equals_two_launches(plan, dtype):
    key, case = _case(plan, dtype)
    _assert_plan(plan, case["max_kv_len"])
    q, kc, vc, kv, bt = _on_gpu(case)
    r = ops.paged_decode_attention_int8(q, kc, vc, kv, bt, case["max_kv_len"], case["scale"], want_16bit=True)
    assert r is not None, f"{plan.name}: the int8 epilogue must take this plan"
    _assert_int8_equal(case, r, _two_launches(case))


@pytest.mark.parametrize("dtype", dc.DTYPES, ids=_did(dc.DTYPES))
def test_int8_epilogue_sliding_window(dtype):
    """window_left = 40 on the headline plan: rows of 1 ... 300 keys, most of them bound by the window, poisoned below it"""
    plan = dc.PLAN["hpw4_headline"]
    key, case = _case(plan, dtype, window_left=40)
    _assert_plan(plan, case["max_kv_len"])
    q, kc, vc, kv, bt = _on_gpu(case)
    r = ops.paged_decode_attention_int8(q, kc, vc, kv, bt, case["max_kv_len"], case["scale"], window_left=40, want_16bit=True)
    assert r is not None
    _assert_int8_equal(case, r, _two_launches(case))
    _assert_meets_both(r[2], case, key)


PLAIN_PLANS = [dc.PLAN["hpw2_krows"], dc.PLAN["hpw1_control"]]


@pytest.mark.parametrize("dtype", dc.DTYPES, ids=_did(dc.DTYPES))
@pytest.mark.parametrize("plan", PLAIN_PLANS, ids=_pid(PLAIN_PLANS))
def test_plain_epilogue_meets_both_references(plan, dtype):
    """hpw = 2 with two head groups per token (hg > 0, nsub = 2) and hpw = 1 (nsub = 4): the 16-bit store of the plain form"""
    key, case = dc.plan_case(plan, dtype)
    _assert_plan(plan, case["max_kv_len"])
    q, kc, vc, kv, bt = _on_gpu(case)
    out = ops.paged_attention(q, kc, vc, None, kv, bt, 1, case["max_kv_len"], case["scale"])
    _assert_meets_both(out, case, key)


def _split_case(dtype):
    key = ("epilogue-split", dtype)
    return key, dc.make_case(dc.SPLIT_PLAN, dc.SPLIT_LENS, dtype, seed=3000)


@pytest.mark.parametrize("dtype", dc.DTYPES, ids=_did(dc.DTYPES))
def test_partials_epilogue_meets_both_references(dtype):
    """2 grid splits x 4 sub-ranges: the workgroups leave fp32 (o, m, l) partials and paged_decode_merge_kernel finishes"""
    key, case = _split_case(dtype)
    _assert_plan(dc.SPLIT_PLAN, case["max_kv_len"])
    q, kc, vc, kv, bt = _on_gpu(case)
    out = ops.paged_attention(q, kc, vc, None, kv, bt, 1, case["max_kv_len"], case["scale"])
    _assert_meets_both(out, case, key)


def _off_by_one(shape, dtype):
    """a contiguous tensor whose base lies one element past an allocation's (at least 256-byte aligned) start"""
    n = 1
    for s in shape:
        n *= s
    t = torch.empty(n + 1, dtype=dtype, device=DEV)[1:].view(*shape)
    assert t.data_ptr() % 16 == t.element_size()
    return t


@pytest.mark.parametrize("dtype", dc.DTYPES, ids=_did(dc.DTYPES))
def test_unaligned_outputs_are_bit_equal(dtype):
    """headline plan: the plain form into a 16-bit tensor 2 bytes off, and the int8 form into an int8 tensor 1 byte off and a
    16-bit tensor 2 bytes off, against the aligned launches"""
    plan = dc.PLAN["hpw4_headline"]
    key, case = dc.plan_case(plan, dtype)
    _assert_plan(plan, case["max_kv_len"])
    q, kc, vc, kv, bt = _on_gpu(case)
    B, n = plan.B, plan.nq * plan.d
    want = _two_launches(case)
    o_off = _off_by_one((B, n), dtype)
    ops.paged_attention(q, kc, vc, None, kv, bt, 1, case["max_kv_len"], case["scale"], out=o_off)
    assert torch.equal(o_off.view(torch.int16), want[0].view(torch.int16))
    oq, o16, os_ = _off_by_one((B, n), torch.int8), _off_by_one((B, n), dtype), torch.empty(B, dtype=torch.float32, device=DEV)
    rc = _lib.lib().xllm_mi355_paged_decode_attention_int8_ws(
        q.data_ptr(), kc.data_ptr(), vc.data_ptr(), o16.data_ptr(), oq.data_ptr(), os_.data_ptr(), kv.data_ptr(), bt.data_ptr(),
        bt.size(1), B, plan.nq, plan.nkv, plan.d, plan.bs, q.stride(0), case["max_kv_len"], case["scale"], -1, _DT[dtype],
        None, 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    _assert_int8_equal(case, (oq, os_, o16), want)


@pytest.mark.parametrize("dtype", dc.DTYPES, ids=_did(dc.DTYPES))
def test_unaligned_partials_are_bit_equal(dtype):
    """split-KV plan with the workspace 4 bytes off a 16-byte boundary: element-wise partial stores, same merged output"""
    key, case = _split_case(dtype)
    plan = dc.SPLIT_PLAN
    _assert_plan(plan, case["max_kv_len"])
    q, kc, vc, kv, bt = _on_gpu(case)
    want = ops.paged_attention(q, kc, vc, None, kv, bt, 1, case["max_kv_len"], case["scale"])
    need = _lib.lib().xllm_mi355_paged_attention_workspace_bytes(plan.B, plan.nq, plan.d, 1, plan.B)
    ws = torch.empty(need + 16, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 16 == 0
    out = torch.empty(plan.B, plan.nq * plan.d, dtype=dtype, device=DEV)
    rc = _lib.lib().xllm_mi355_paged_attention(
        q.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), None, kv.data_ptr(), bt.data_ptr(), bt.size(1), plan.B,
        plan.B, plan.nq, plan.nkv, plan.d, plan.bs, kc.size(0), q.stride(0), 1, case["max_kv_len"], case["scale"], 0, -1,
        _DT[dtype], ws.data_ptr() + 4, need, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))
