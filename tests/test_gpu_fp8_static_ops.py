"""GPU: the two producer-side static e4m3 quantisations of the fp8 decode layer (xllm_amd/csrc/xllm_mi355_fp8_static.h).

Both operators are DEFINED by the operator pair they replace, so the checks are byte equalities against that pair:

  * ops.act_and_mul_static_fp8_quant == ops.act_and_mul -> ops.static_scaled_fp8_quant, at widths around the 8-element chunk
    (16, 19 = the element-wise arm, 136 = one partial batch, 2056, 18944 = the 7B width: several workgroups per row), 1 / 3 / 257
    rows, both 16-bit dtypes, every act mode, four scales (amax / 448, 1, 2^-6, and 2^-16 at which most elements saturate), an
    output one byte off its 8-byte alignment and an input one element off its 16-byte alignment;
  * ops.paged_decode_attention_fp8 == ops.paged_attention -> ops.static_scaled_fp8_quant at every launch plan of
    tests/_decode_cases.py (asserted first), the window cases and split-KV, with and without the 16-bit output (bit-equal to
    paged_attention's), with out_q one byte off alignment, at scale = amax / 448 and at 2^-8 (saturating). Poisoned caches,
    ragged lengths, the empty row comes out as zero bytes. The 16-bit output meets the bars of tests/test_gpu_decode_plans.py
    against the oracle and the dense float64 reference.

The activation is also held to float64 directly: at scale = amax / 448 nothing saturates, and the dequantised bytes of a row are
within relative L2 0.07 of act(gate) * up. e4m3 has 3 mantissa bits: half an ulp of a normal is 2^-4 = 0.0625 relative; the rest
covers the two 16-bit roundings and the subnormal floor (2^-10 * scale per element in absolute terms). A derived bound.

Both operators replay from a captured graph to the eager bytes after their inputs changed in place."""
import math

import pytest
import torch

import _decode_cases as dc
from test_gpu_decode_plans import _assert_meets_both, _assert_plan, _on_gpu

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from xllm_amd import ops
DEV = "cuda"
_NAME = {torch.bfloat16: "bf16", torch.float16: "f16"}
_did = lambda ds: [_NAME[d] for d in ds]
_pid = lambda ps: [p.name for p in ps]
U8 = torch.uint8


# ------------------------------------------------------------------------------------------------ activation
ACT_D = [16, 19, 136, 2056, 18944]
ACT_T = [1, 3, 257]
ACT_MODES = ["silu", "gelu", "gelu_tanh"]            # ops._ACT: every mode act_and_mul takes
SPIKE_GATE, SPIKE_UP = 2.0, 2.0 ** 12


def _act_input(T, d, dtype, seed, spiked=True):
    """Gaussian [T, 2 * d]. spiked: in every row three up entries are scaled by 2^12 (magnitude at least 0.5 before the scaling,
    gate set to 2: each row then holds products of several thousand, so the per-TENSOR amax / 448 scale leaves no row as a whole
    below the e4m3 subnormal floor) and three gate entries are scaled by 2^-20 (products far below that floor: they become 0)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(T, 2 * d, device=DEV, generator=g)
    if spiked:
        rows = torch.arange(T, device=DEV)
        for i in range(3):       # columns 7t + 5i + 3 (spikes) and two past each (small): distinct for every d of ACT_D
            big = (7 * rows + 5 * i + 3) % d
            u = x[rows, d + big]
            x[rows, d + big] = torch.where(u < 0, -1.0, 1.0) * u.abs().clamp_min(0.5) * SPIKE_UP    # no spike near zero
            x[rows, big] = SPIKE_GATE
            x[rows, (big + 2) % d] *= 2.0 ** -20
    return x.to(dtype)


def _two_act_launches(x, scale, mode):
    d = x.size(-1) // 2
    a16 = torch.empty(x.size(0), d, dtype=x.dtype, device=DEV)
    ops.act_and_mul(a16, x, mode)
    q = torch.empty(a16.shape, dtype=ops.FP8, device=DEV)
    ops.static_scaled_fp8_quant(q, a16, scale)
    return a16, q


def _off_by_one(shape, dtype):
    """a contiguous tensor whose base lies one element past an allocation's (at least 256-byte aligned) start"""
    n = math.prod(shape)
    t = torch.empty(n + 1, dtype=dtype, device=DEV)[1:].view(*shape)
    assert t.data_ptr() % 16 == t.element_size()
    return t


def _f32(v):
    return torch.full((1,), float(v), dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("mode", ACT_MODES)
@pytest.mark.parametrize("dtype", dc.DTYPES, ids=_did(dc.DTYPES))
def test_activation_equals_two_launches(dtype, mode):
    for d in ACT_D:
        for T in ACT_T:
            x = _act_input(T, d, dtype, seed=100 * d + T)
            a16, _ = _two_act_launches(x, _f32(1.0), mode)
            amax = float(a16.float().abs().max())
            assert math.isfinite(amax) and amax > 1000.0
            sat = None
            for name, s in (("amax/448", amax / 448.0), ("1", 1.0), ("2^-6", 2.0 ** -6), ("2^-16", 2.0 ** -16)):
                scale = _f32(s)
                _, want = _two_act_launches(x, scale, mode)
                got = ops.act_and_mul_static_fp8_quant(x, scale, mode)
                assert got.dtype == ops.FP8 and got.shape == (T, d)
                assert torch.equal(got.view(U8), want.view(U8)), (d, T, name)
                off = _off_by_one((T, d), U8)                                   # element-wise stores
                ops.act_and_mul_static_fp8_quant(x, scale, mode, out_q=off)
                assert torch.equal(off, want.view(U8)), (d, T, name, "output one byte off")
                # element-wise loads. The pair runs on the same misaligned input: act_and_mul's own element-wise arm may give a
                # zero another sign than its 16-byte arm does (f16, a gate of -0.0), so that is the reference for this call
                x_off = _off_by_one((T, 2 * d), dtype)
                x_off.copy_(x)
                _, want_off = _two_act_launches(x_off, scale, mode)
                assert torch.equal(want_off.float(), want.float()), (d, T, name, "the pair's two arms agree in value")
                assert torch.equal(ops.act_and_mul_static_fp8_quant(x_off, scale, mode).view(U8), want_off.view(U8)), (d, T, name)
                sat = float(((want.view(U8) & 0x7F) == 0x7E).float().mean())    # 0x7E = 448
            if d >= 136:
                assert sat > 0.5, f"d={d} T={T}: the smallest scale must saturate most elements, {sat:.2f} do"


def _act64(x, mode):
    d = x.size(-1) // 2
    g, u = x[:, :d].double(), x[:, d:].double()
    if mode == "silu":
        a = g / (1.0 + torch.exp(-g))
    elif mode == "gelu":
        a = 0.5 * g * (1.0 + torch.erf(g / math.sqrt(2.0)))
    else:
        a = 0.5 * g * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (g + 0.044715 * g ** 3)))
    return a * u


@pytest.mark.parametrize("spiked", [True, False], ids=["spiked", "gaussian"])
@pytest.mark.parametrize("mode", ACT_MODES)
@pytest.mark.parametrize("dtype", dc.DTYPES, ids=_did(dc.DTYPES))
def test_activation_against_float64(dtype, mode, spiked):
    worst = 0.0
    for d in ACT_D:
        for T in ACT_T:
            x = _act_input(T, d, dtype, seed=100 * d + T, spiked=spiked)
            a16, _ = _two_act_launches(x, _f32(1.0), mode)
            s = float(a16.float().abs().max()) / 448.0
            got = ops.act_and_mul_static_fp8_quant(x, _f32(s), mode)
            assert not ((got.view(U8) & 0x7F) == 0x7F).any(), "no NaN code"
            deq = got.float().double() * float(_f32(s).item())
            ref = _act64(x, mode)
            rel = (deq - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-300)
            worst = max(worst, float(rel.max()))
            print(f"act fp8 vs float64 {_NAME[dtype]} {mode} {'spiked' if spiked else 'gaussian'} d={d} T={T}: "
                  f"max row rel L2 {float(rel.max()):.4f}")
            assert float(rel.max()) <= 0.07, (d, T, float(rel.max()))
    assert worst > 0.0


# ------------------------------------------------------------------------------------------------ attention
ATTN_SCALES = ["amax/448", "2^-8"]


def _check_fp8_attention(key, case, meets=True):
    """every combination of (scale, want_16bit, aligned out_q) of one case against paged_attention -> static_scaled_fp8_quant"""
    _assert_plan(case["plan"], case["max_kv_len"])
    plan = case["plan"]
    q, kc, vc, kv, bt = _on_gpu(case)
    W = case["window_left"]
    o = ops.paged_attention(q, kc, vc, None, kv, bt, 1, case["max_kv_len"], case["scale"], window_left=W)
    assert torch.isfinite(o.float()).all()
    empty = (case["kv_lens"] == 0).to(DEV)
    n = plan.nq * plan.d
    for name in ATTN_SCALES:
        scale = _f32(float(o.float().abs().max()) / 448.0 if name == "amax/448" else 2.0 ** -8)
        want = torch.empty(o.shape, dtype=ops.FP8, device=DEV)
        ops.static_scaled_fp8_quant(want, o, scale)
        want = want.view(U8)
        if name == "2^-8" and bool((o.float().abs() > 464.0 * 2.0 ** -8).any()):     # 464: half-way past the largest e4m3
            assert ((want & 0x7F) == 0x7E).any(), "outputs beyond 448 * 2^-8 saturate"
        for want16 in (True, False):
            for aligned in (True, False):
                buf = None if aligned else _off_by_one((plan.B, n), U8)
                q8, o16 = ops.paged_decode_attention_fp8(q, kc, vc, kv, bt, case["max_kv_len"], case["scale"], scale,
                                                         window_left=W, want_16bit=want16, out_q=buf)
                what = (key, name, want16, aligned)
                assert q8.shape == (plan.B, n) and (o16 is not None) == want16
                assert torch.equal(q8.view(U8), want), what
                assert not q8.view(U8)[empty].any(), what
                if want16:
                    assert torch.equal(o16.view(torch.int16), o.view(torch.int16)), what
                    if meets and name == "amax/448" and aligned:
                        _assert_meets_both(o16, case, key)


ALL_PLANS = dc.PLANS + [dc.SPLIT_PLAN]


@pytest.mark.parametrize("dtype", dc.DTYPES, ids=_did(dc.DTYPES))
@pytest.mark.parametrize("plan", ALL_PLANS, ids=_pid(ALL_PLANS))
def test_attention_equals_two_launches(plan, dtype):
    """ragged lengths 1 ... 300 and one empty row at each launch plan; the split-KV plan on its own lengths (2 grid splits: the
    merge launch quantises)"""
    if plan is dc.SPLIT_PLAN:
        key, case = dc.split_window_case(dc.SPLIT_WINDOWS[-1], dtype)
        _check_fp8_attention(key, case)
        key, case = ("fp8-split", dtype), dc.make_case(dc.SPLIT_PLAN, dc.SPLIT_LENS[:2] + [0], dtype, seed=3100)
        _check_fp8_attention(key, case)      # no window, and an empty row under split-KV
    else:
        _check_fp8_attention(*dc.plan_case(plan, dtype))


@pytest.mark.parametrize("dtype", dc.DTYPES, ids=_did(dc.DTYPES))
@pytest.mark.parametrize("W", dc.WINDOWS, ids=[f"W{w}" for w in dc.WINDOWS])
@pytest.mark.parametrize("plan", dc.WINDOW_PLANS, ids=_pid(dc.WINDOW_PLANS))
def test_attention_window_equals_two_launches(plan, W, dtype):
    for key, case in dc.window_cases(plan, W, dtype):
        _check_fp8_attention(key, case)


@pytest.mark.parametrize("dtype", dc.DTYPES, ids=_did(dc.DTYPES))
@pytest.mark.parametrize("W", dc.SPLIT_WINDOWS[:-1], ids=[f"W{w}" for w in dc.SPLIT_WINDOWS[:-1]])
def test_attention_window_under_split_kv_equals_two_launches(W, dtype):
    _check_fp8_attention(*dc.split_window_case(W, dtype))


# ------------------------------------------------------------------------------------------------ graph capture
def test_activation_replays_from_a_graph():
    T, d = 3, 2056
    x = _act_input(T, d, torch.bfloat16, seed=7)
    scale = _f32(0.5)
    ops.act_and_mul_static_fp8_quant(x, scale)                    # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.act_and_mul_static_fp8_quant(x, scale)
    for i in range(2):
        x.copy_(_act_input(T, d, torch.bfloat16, seed=8 + i))
        scale.fill_(0.25 * (i + 1))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(U8), ops.act_and_mul_static_fp8_quant(x, scale).view(U8)), i


GRAPH_PLANS = [dc.PLAN["hpw1_control"], dc.SPLIT_PLAN]


@pytest.mark.parametrize("plan", GRAPH_PLANS, ids=_pid(GRAPH_PLANS))
def test_attention_replays_from_a_graph(plan):
    """one launch (one grid split) and two launches (split-KV), captured on one stream: no parallel branches"""
    dtype = torch.bfloat16
    key, case = dc.split_window_case(dc.SPLIT_WINDOWS[-1], dtype) if plan is dc.SPLIT_PLAN else dc.plan_case(plan, dtype)
    _assert_plan(plan, case["max_kv_len"])
    q, kc, vc, kv, bt = _on_gpu(case)
    W = case["window_left"]
    scale = _f32(2.0 ** -5)
    run = lambda: ops.paged_decode_attention_fp8(q, kc, vc, kv, bt, case["max_kv_len"], case["scale"], scale, window_left=W,
                                                 want_16bit=True)
    run()                                                          # warm-up: the workspace exists before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        q8, o16 = run()
    gen = torch.Generator(device=DEV).manual_seed(5)
    for i in range(2):
        q.copy_(torch.randn(q.shape, device=DEV, generator=gen).to(dtype))
        scale.fill_(2.0 ** -(3 + i))
        g.replay()
        torch.cuda.synchronize()
        e8, e16 = run()
        assert torch.equal(q8.view(U8), e8.view(U8)) and torch.equal(o16.view(torch.int16), e16.view(torch.int16)), i
