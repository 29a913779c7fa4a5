"""CPU-side checks of the e4m3 KV cache operators (xllm_amd/csrc/xllm_mi355_kv_fp8.h):
  * the symbols are declared in the header, exported and bound with the header's argument counts, validation returns its codes
    without a device, and the plan query agrees with a Python restatement of the planning rule on every case of the tables;
  * a float32 restatement of the kernel's arithmetic (folded scales, the kernel's tile order and slot merge, hi + lo P) stays
    within HALF of each bar of the float64 reference on every case -- the room the GPU kernel has under its bars;
  * the reference is sensitive, so a wrong kernel cannot pass: quantisation itself moves the result by more than ten bars,
    halving k_scale or v_scale alone moves every row that can show it past the row bar, and so does moving a window edge or
    kv_len by one key."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import _kv_fp8_cases as kc
from _bars import assert_attn_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "xllm_amd", "csrc", "xllm_mi355_kv_fp8.h")
SYMBOLS = {"xllm_mi355_reshape_paged_cache_kv8": 16, "xllm_mi355_rotary_embedding_and_cache_kv8": 23,
           "xllm_mi355_paged_decode_attention_kv8": 23, "xllm_mi355_paged_decode_kv8_plan": 11}
XM_OK, XM_ERR_INVALID, XM_ERR_UNSUPPORTED = 0, -1, -2


def _built():
    import __graft_entry__ as g
    from xllm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        os.environ["XLLM_MI355_SKIP_SHIM"] = "1"
        g.build()
    return _lib


def _declared():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): len([a for a in m.group(2).split(",") if a.strip()])
            for m in re.finditer(r"XM_API\s+[\w\s\*]+?\b(xllm_mi355_\w+)\s*\(([^)]*)\)", hdr)}


def test_symbols_declared_exported_and_bound():
    _lib = _built()
    assert _declared() == SYMBOLS
    exported = set(re.findall(r"\b(xllm_mi355_\w+)\b", subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()))
    for s, n in SYMBOLS.items():
        assert s in exported and s in _lib.exported_symbols(), s
        assert len(getattr(_lib.lib(), s).argtypes) == n, s
    assert _lib.lib().xllm_mi355_abi_version() == 2
    from xllm_amd import ops
    for w in ("reshape_paged_cache_kv8", "rotary_embedding_and_cache_kv8", "paged_attention_kv8", "paged_decode_kv8_plan"):
        assert callable(getattr(ops, w))


def _addr():
    """a 16-byte aligned host address that is never dereferenced: every case here must return before any device work"""
    buf = (C.c_char * 64)()
    return buf, (C.addressof(buf) + 15) // 16 * 16


def _attn(l, null=(), d=128, nq=28, nkv=4, dtype=1, batch=4, off=None, q_stride=None, max_blocks=8, bs=128):
    buf, a = _addr()
    names = ["q", "k_cache", "v_cache", "k_scale", "v_scale", "out", "kv_lens", "block_table"]
    p = [None if n in null else a + (2 if n == off else 0) for n in names]
    return l.xllm_mi355_paged_decode_attention_kv8(*p, max_blocks, batch, nq, nkv, d, bs, 64, nq * d if q_stride is None else q_stride,
                                                   1024, 0.1, -1, dtype, None, 0, None)


def test_attention_validation_happens_without_a_device():
    l = _built().lib()
    for name in ("q", "k_cache", "v_cache", "k_scale", "v_scale", "out", "kv_lens", "block_table"):
        assert _attn(l, null=(name,)) == XM_ERR_INVALID, name
    assert _attn(l, nq=30) == XM_ERR_INVALID               # n_q_heads % n_kv_heads
    assert _attn(l, batch=-1) == XM_ERR_INVALID
    assert _attn(l, max_blocks=0) == XM_ERR_INVALID
    assert _attn(l, bs=0) == XM_ERR_INVALID
    assert _attn(l, d=96) == XM_ERR_UNSUPPORTED            # head dim other than 64 / 128
    assert _attn(l, d=256) == XM_ERR_UNSUPPORTED
    assert _attn(l, nq=68) == XM_ERR_UNSUPPORTED           # 17 q heads per kv head
    assert _attn(l, dtype=0) == XM_ERR_UNSUPPORTED         # f32
    assert _attn(l, dtype=7) == XM_ERR_UNSUPPORTED
    for name in ("q", "k_cache", "v_cache"):
        assert _attn(l, off=name) == XM_ERR_UNSUPPORTED, name    # misaligned base
    assert _attn(l, q_stride=28 * 128 + 4) == XM_ERR_UNSUPPORTED
    assert _attn(l, batch=0) == XM_OK                      # an empty batch launches nothing


def test_writer_validation_happens_without_a_device():
    l = _built().lib()
    buf, a = _addr()

    def reshape(null=None, n=3, nkv=4, d=128, bs=16, dtype=1):
        p = [None if i == null else a for i in range(7)]   # slot_ids, k, v, k_cache, v_cache, k_scale, v_scale
        return l.xllm_mi355_reshape_paged_cache_kv8(*p, n, nkv, d, bs, 8, nkv * d, nkv * d, dtype, None)

    def rope(null=None, n=3, rot=128, hs=128, bs=16, dtype=1):
        p = [None if i == null else a for i in range(10)]  # positions, q, k, v, cos_sin, slots, k_cache, v_cache, k_scale, v_scale
        return l.xllm_mi355_rotary_embedding_and_cache_kv8(*p, n, 4, 2, hs, rot, 768, 768, 768, bs, 8, 1, dtype, None)

    for i in range(7):
        assert reshape(null=i) == XM_ERR_INVALID, i
    for i in range(10):
        assert rope(null=i) == XM_ERR_INVALID, i
    assert reshape(n=-1) == XM_ERR_INVALID and reshape(bs=0) == XM_ERR_INVALID and reshape(nkv=0) == XM_ERR_INVALID
    assert rope(n=-1) == XM_ERR_INVALID and rope(rot=0) == XM_ERR_INVALID and rope(rot=63) == XM_ERR_INVALID
    assert rope(rot=256) == XM_ERR_INVALID and rope(bs=0) == XM_ERR_INVALID
    assert reshape(dtype=0) == XM_ERR_UNSUPPORTED and rope(dtype=0) == XM_ERR_UNSUPPORTED      # f32 rows
    assert reshape(n=0) == XM_OK and rope(n=0) == XM_OK


def _plan(l, B, nq, nkv, d, bs, max_kv_len, ws):
    v = [C.c_int32(-1) for _ in range(4)]
    rc = l.xllm_mi355_paged_decode_kv8_plan(B, nq, nkv, d, bs, max_kv_len, ws, *[C.byref(x) for x in v])
    return rc, tuple(x.value for x in v)


def test_plan_query_validation():
    l = _built().lib()
    assert _plan(l, 0, 28, 4, 128, 128, 100, 0)[0] == XM_ERR_INVALID
    assert _plan(l, 4, 30, 4, 128, 128, 100, 0)[0] == XM_ERR_INVALID
    assert _plan(l, 4, 28, 4, 128, 0, 100, 0)[0] == XM_ERR_INVALID
    assert _plan(l, 4, 28, 4, 128, 128, -1, 0)[0] == XM_ERR_INVALID
    assert _plan(l, 4, 28, 4, 96, 128, 100, 0)[0] == XM_ERR_UNSUPPORTED
    assert l.xllm_mi355_paged_decode_kv8_plan(4, 28, 4, 128, 128, 100, 0, None, None, None, None) == XM_OK


def test_plan_query_agrees_with_the_planning_rule_on_every_case():
    """every plan of the tables at its own max_kv_len, with the full workspace bound, none, and one that holds 1.5 splits; the named
    expectation of the table (hpw, uniform, nsplit) holds with the full bound"""
    l = _built().lib()
    forced = os.environ.get("XLLM_MI355_DECODE_SPLITS")
    for p, max_len in [(p, max(kc.KV8_LENS)) for p in kc.PLANS] + [(kc.SPLIT_PLAN, max(kc.KV8_SPLIT_LENS))]:
        full = kc.workspace_bound(p.B, p.nq, p.d)
        assert full == l.xllm_mi355_paged_attention_workspace_bytes(p.B, p.nq, p.d, 1, p.B)
        per_split = p.B * p.nq * (p.d + 2) * 4
        for ws in (full, 0, per_split * 3 // 2, per_split * 2, per_split * 2 - 1):
            rc, got = _plan(l, p.B, p.nq, p.nkv, p.d, p.bs, max_len, ws)
            assert rc == XM_OK and got == kc.plan_py(p.B, p.nq, p.nkv, p.d, p.bs, max_len, ws), (p.name, ws, got)
        if forced is None:
            assert _plan(l, p.B, p.nq, p.nkv, p.d, p.bs, max_len, full)[1] == (p.hpw, p.nsplit, p.nsplit, p.uniform), p.name
    if forced is None:   # degradation: the split plan with no / an undersized workspace runs one split, planned stays 2
        p = kc.SPLIT_PLAN
        per_split = p.B * p.nq * (p.d + 2) * 4
        assert _plan(l, p.B, p.nq, p.nkv, p.d, p.bs, 2500, 0)[1] == (1, 2, 1, 1)
        assert _plan(l, p.B, p.nq, p.nkv, p.d, p.bs, 2500, 2 * per_split - 1)[1] == (1, 2, 1, 1)
        assert _plan(l, p.B, p.nq, p.nkv, p.d, p.bs, 2500, 2 * per_split)[1] == (1, 2, 2, 1)
    # a sweep beyond the tables: batches around the hpw thresholds, lengths around the split thresholds
    for B in (1, 3, 47, 48, 95, 96, 191, 192, 256):
        for nkv, nq in ((1, 7), (2, 14), (4, 28), (8, 32)):
            for max_len in (0, 1, 255, 256, 1023, 1024, 4096, 65536):
                for bs in (16, 48, 128):
                    ws = kc.workspace_bound(B, nq, 128)
                    assert _plan(l, B, nq, nkv, 128, bs, max_len, ws)[1] == kc.plan_py(B, nq, nkv, 128, bs, max_len, ws)


# ---------------------------------------------------------------------------------------------- the reference and its room
_CASES = kc.all_cases()


@pytest.mark.parametrize("name,build", _CASES, ids=[n for n, _ in _CASES])
def test_f32_restatement_of_the_kernel_within_half_a_bar(name, build):
    """folded scales, tile order, slot merge and hi + lo P of attention_decode_kv8.hip in float32 against dense_decode_ref64 on
    codes.double() * scale: relative L2 and the element-wise distance both within half of the bar the GPU kernel is held to
    (measured: below 1e-5 relative against bars of 1e-3 for bf16 and 2e-4 for f16)"""
    for key, case in build():
        p = case["plan"]
        ref = kc.reference64(case, key)
        assert torch.isfinite(ref).all() and ref.shape == (p.B, p.nq * p.d)
        got = kc.kernel_restatement_f32(case, p.hpw, p.nsplit)
        assert torch.isfinite(got).all()
        rel, elem = kc.distance(got, ref)
        bar = kc.BAR_REL[case["dtype"]]
        print(f"{name}: f32 restatement vs fp64 rel L2 {rel:.3e} = {rel / bar:.4f} bar, element-wise {elem:.4f} bar")
        assert rel <= 0.5 * bar and elem <= 0.5, (key, rel, elem)
        empty = case["kv_lens"] == 0
        assert empty.any() and not got[empty].any() and not ref[empty].any()


def _row_moved(a, b, dtype):
    """per row: does b miss a under assert_attn_close's bars (relative L2 of the row > bar, or an element beyond 2 bf16 ulp of
    the row maximum)"""
    a, b = a.float(), b.float()
    rel = (a - b).norm(dim=-1) / a.norm(dim=-1).clamp_min(1e-30)
    elem = ((a - b).abs() > 2 * 2.0 ** -8 * a.abs().amax(-1, keepdim=True) + 1e-30).any(-1)
    return (rel > kc.BAR_REL[dtype]) | elem


@pytest.mark.parametrize("dtype", kc.DTYPES, ids=["bf16", "f16"])
def test_reference_is_sensitive_to_the_quantisation_and_to_either_scale(dtype):
    key, case = kc.plan_case(kc.PLAN["hpw4_all_g7"], dtype)
    ref = kc.reference64(case, key)
    lens = case["kv_lens"]
    # (1) the quantisation itself: the float64 result on the original 16-bit cache is more than ten bars away
    ref16 = kc.dense_decode_ref64(case["q"], case["kc16"], case["vc16"], lens, case["block_tables"], case["scale"])
    rel = kc.distance(ref, ref16)[0]
    print(f"dequantised vs original 16-bit cache: rel L2 {rel:.3e} = {rel / kc.BAR_REL[dtype]:.1f} bars")
    assert rel > 10 * kc.BAR_REL[dtype]
    # (2) half the k_scale: every row with more than one visible key moves past the row bar (a row of ONE key is a softmax over one
    #     score -- p = 1 whatever the scale -- and an empty row is zeros: exactly those are excluded)
    half_k = kc.reference64(case, key + ("half_k",), k_scale=case["k_scale"] / 2)
    moved = _row_moved(ref, half_k, dtype)
    can_show = lens > 1
    assert can_show.sum() >= len(lens) - 2 * (len(lens) // len(kc.KV8_LENS) + 1)
    assert moved[can_show].all() and not moved[~can_show].any()
    # (3) half the v_scale: every non-empty row halves
    half_v = kc.reference64(case, key + ("half_v",), v_scale=case["v_scale"] / 2)
    moved = _row_moved(ref, half_v, dtype)
    assert moved[lens > 0].all() and not moved[lens == 0].any()
    with pytest.raises(AssertionError):
        assert_attn_close(half_k.to(dtype), ref.to(dtype), rel=kc.BAR_REL[dtype])


@pytest.mark.parametrize("dtype", kc.DTYPES, ids=["bf16", "f16"])
def test_reference_is_sensitive_to_one_key_at_either_end(dtype):
    """kv_len one key shorter moves every row with L >= 2 (the cases' live rows are clean, so the shortened reference reads only
    live rows); a window edge one key lower (W + 1) moves every row the window binds. The extra key of the W + 1 reference is a
    poisoned row (NaN code), so that row turns non-finite: moved, by any measure."""
    key, case = kc.plan_case(kc.PLAN["hpw4_all_g7"], dtype)
    ref = kc.reference64(case, key)
    lens = case["kv_lens"]
    shorter = kc.reference64(case, key + ("len-1",), kv_lens=(lens - 1).clamp_min(0))
    moved = _row_moved(ref, shorter, dtype)
    assert moved[lens >= 2].all()
    W = 40
    wkey, wcase = kc.window_cases(kc.WINDOW_PLANS[0], W, dtype)[0]
    wref = kc.reference64(wcase, wkey)
    wider = kc.reference64(wcase, wkey + ("W+1",), window_left=W + 1)
    narrower = kc.reference64(wcase, wkey + ("W-1",), window_left=W - 1)
    wl = wcase["kv_lens"]
    bound = wl > W + 1                     # t_lo >= 1: one more key to the left exists (and is poisoned)
    assert bound.any() and (~torch.isfinite(wider[bound])).any(-1).all()
    assert torch.isfinite(wider[~bound]).all() and torch.equal(wider[~bound], wref[~bound])
    moved = _row_moved(wref, narrower, dtype)
    assert moved[wl > W].all()             # rows of at least W + 1 keys lose their oldest visible key


def test_cases_hold_what_they_claim():
    """tile-edge lengths and an empty row in every batch; NaN bytes exactly on the dead rows, in both caches"""
    for t in (1, 2, 3):
        assert {32 * t - 1, 32 * t, 32 * t + 1} <= set(kc.KV8_LENS)
    assert set(kc.LENS) <= set(kc.KV8_LENS)
    for p in kc.PLANS:
        ls = kc.kv8_ragged_lens(p.B)
        assert 0 in ls and len(ls) == p.B
        if p.B >= 16:
            assert set(ls) == set(kc.KV8_LENS) | {0}, p.name
    assert 0 in kc.KV8_SPLIT_LENS and kc.KV8_SPLIT_LENS[:3] == kc.SPLIT_LENS
    assert {p.hpw for p in kc.PLANS} == {1, 2, 4} and {p.uniform for p in kc.PLANS} == {0, 1} and {p.d for p in kc.PLANS} == {64, 128}
    assert {p.nq // p.nkv for p in kc.PLANS} >= {1, 7, 16}
    key, case = kc.window_cases(kc.WINDOW_PLANS[1], 40, torch.bfloat16)[0]
    dead_k, dead_v = ~torch.isfinite(case["kc16"].float()), ~torch.isfinite(case["vc16"].float())
    assert dead_k.any() and torch.equal(dead_k, dead_v)
    assert torch.equal(case["kc"] == 0x7F, dead_k) or ((case["kc"] == 0x7F) & ~dead_k).sum() == 0
    assert (case["kc"][dead_k] == 0x7F).all() and (case["vc"][dead_v] == 0x7F).all()
    assert torch.isnan(case["vc"].view(kc.FP8).float()[dead_v]).all()
