"""GPU: the e4m3 KV cache operators (xllm_amd/csrc/xllm_mi355_kv_fp8.h) -- decode attention over an e4m3 cache with static scales at
every arm its plan query can report, and the two KV writers byte for byte against the operator sequences that define them.

Attention. Every test asserts, through xllm_mi355_paged_decode_kv8_plan, the plan its case is in the table for (heads per
workgroup, page-uniform or gathered tiles, grid splits planned and delivered) before it launches, and holds the result to
dense_decode_ref64 on codes.double() * scale rounded to the tensor dtype under assert_attn_close's bars -- relative L2 <= 1e-3
(bf16) / 2e-4 (f16) and 2 bf16 ulp of the row maximum element-wise: the bars the 16-bit kernel is held to.

  plan (tests/_kv_fp8_cases.py)                          B   nq nkv   d  page  group
  hpw = 4, all kv heads in the workgroup                192  28   4  128  128     7   test_plan, test_window, test_pow2
  hpw = 4, 4 of 16 kv heads, gathered tiles              48  32  16  128   16     2   test_plan, test_window, test_pow2, strided q, graph
  hpw = 2, 2 of 4 kv heads, 2 sub-ranges                 96  28   4  128  128     7   test_plan, test_pow2
  hpw = 2, both kv heads, d = 64                        192  14   2   64   64     7   test_plan, test_pow2
  hpw = 4, d = 64, gathered tiles                       192  16   4   64   16     4   test_plan, test_pow2
  hpw = 1, 4 sub-ranges                                   4  28   4  128  128     7   test_plan, test_pow2
  hpw = 4, group 1                                      192   4   4  128  128     1   test_plan, test_pow2
  hpw = 4, group 16 (1024 epilogue work items)          192  64   4  128  128    16   test_plan, test_pow2
  hpw = 1, 2 grid splits (8 slots), 2500/1000/130/0       4  28   4  128  128     7   test_split, degradation, test_pow2, graph

Lengths: LENS plus one short of, on and one past 32, 64 and 96 (the 32-token tile), an empty row in every batch. The caches are
poisoned with the e4m3 NaN byte 0x7F wherever the kernel may load but must not use (past kv_len, below the window's t_lo, spare
blocks behind table entries of pages wholly below the window), in K and in V.

What these tests catch, each tried on a scratch build of attention_decode_kv8.hip (arithmetic changed, memory accesses not):
  * k_scale not folded into the softmax scale, or q loaded in natural d order under the permuted K fetch: every test_plan,
    test_split, test_pow2, test_workspace_degradation, test_strided_q and graph test fails, and every test_window with W >= 5
    (at W = 0 a row sees ONE key: its softmax is 1 whatever the scores are -- the rows test_kv_fp8_host.py excludes by name);
  * v_scale dropped (kernel epilogue and merge launch), or the rows past kv_len not masked to -inf: every attention test fails;
  * the window's lower bound one key too high (t_lo = kv_len - W): every test_window with a binding W and test_split[W40 / W100
    / W1030] fail;
  * merge launch with weights 1 instead of exp2(m - m*): test_split[W-1, W100, W1030], test_workspace_degradation,
    test_pow2[hpw1_split2] and the split graph test fail (at W = 40 the three live tiles sit in the first grid split, the other
    holds l = 0: nothing to weigh);
  * the workgroup's sub-range merge with weights 1: test_plan and test_pow2 at hpw2_part, hpw2_all_d64 and hpw1, every test_split,
    test_workspace_degradation and the split graph test fail (hpw = 4 has one sub-range: nothing to weigh)."""
import pytest
import torch

import _kv_fp8_cases as kc
from _bars import assert_attn_close

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from xllm_amd import ops
DEV = "cuda"
FP8 = torch.float8_e4m3fn
_NAME = {torch.bfloat16: "bf16", torch.float16: "f16"}
_ids = lambda xs: [x.name if hasattr(x, "name") else _NAME.get(x, f"W{x}") for x in xs]
ALL_PLANS = kc.PLANS + [kc.SPLIT_PLAN]


def _assert_plan(plan, max_kv_len, ws_bytes=None, nsplit=None):
    got = ops.paged_decode_kv8_plan(plan.B, plan.nq, plan.nkv, plan.d, plan.bs, max_kv_len, ws_bytes)
    want = (plan.hpw, plan.nsplit, plan.nsplit if nsplit is None else nsplit, plan.uniform)
    assert got == want, f"{plan.name}: the planner gives (hpw, planned, nsplit, uniform) = {got}, the table says {want}"


def _on_gpu(case):
    s = lambda v: torch.tensor([v], dtype=torch.float32, device=DEV)
    return dict(q=case["q"].to(DEV), kc=case["kc"].to(DEV).view(FP8), vc=case["vc"].to(DEV).view(FP8), ks=s(case["k_scale"]),
                vs=s(case["v_scale"]), kv=case["kv_lens"].to(DEV), bt=case["block_tables"].to(DEV))


def _launch(case, t, **kw):
    return ops.paged_attention_kv8(t["q"], t["kc"], t["vc"], t["ks"], t["vs"], t["kv"], t["bt"], case["max_kv_len"], case["scale"],
                                   window_left=case["window_left"], **kw)


def _assert_meets_reference(out, case, key):
    ref = kc.reference64(case, key).to(case["dtype"])
    bar = kc.BAR_REL[case["dtype"]]
    rel, elem = kc.distance(out, ref)
    print(f"{key}: kernel vs float64 (rel L2 / bar, element-wise / bar) = {rel / bar:.3f}, {elem:.3f}")
    assert_attn_close(out, ref, rel=bar)
    empty = (case["kv_lens"] == 0).to(out.device)
    assert empty.any() and not out[empty].any()


def _run_and_check(key, case):
    _assert_plan(case["plan"], case["max_kv_len"])
    t = _on_gpu(case)
    out = _launch(case, t)
    _assert_meets_reference(out, case, key)
    return out, t


@pytest.mark.parametrize("dtype", kc.DTYPES, ids=_ids(kc.DTYPES))
@pytest.mark.parametrize("plan", kc.PLANS, ids=_ids(kc.PLANS))
def test_plan(plan, dtype):
    """ragged lengths 1 ... 300 with every 32-token tile edge and one empty row at each launch plan, scales that are not powers
    of two, NaN bytes in every dead row of K and V"""
    _run_and_check(*kc.plan_case(plan, dtype))


@pytest.mark.parametrize("dtype", kc.DTYPES, ids=_ids(kc.DTYPES))
@pytest.mark.parametrize("W", kc.WINDOWS, ids=_ids(kc.WINDOWS))
@pytest.mark.parametrize("plan", kc.WINDOW_PLANS, ids=_ids(kc.WINDOW_PLANS))
def test_window(plan, W, dtype):
    """the window lengths of tests/_decode_cases.py (t_lo at 0, 1, on / one short of a tile boundary, on a 16-token page boundary
    inside a tile, rows the window does not bind) on a page-uniform and a gathered plan"""
    for key, case in kc.window_cases(plan, W, dtype):
        _run_and_check(key, case)


@pytest.mark.parametrize("dtype", kc.DTYPES, ids=_ids(kc.DTYPES))
@pytest.mark.parametrize("W", [-1] + kc.SPLIT_WINDOWS, ids=_ids([-1] + kc.SPLIT_WINDOWS))
def test_split(W, dtype):
    """hpw = 1 with 2 grid splits = 8 slots per (sequence, head), the merge launch applying v_scale; under a window the longest
    row keeps 3, 5 or 34 tiles, so slots own no tile and the edge tile is the first live slot's"""
    _run_and_check(*kc.split_case(W, dtype))


@pytest.mark.parametrize("dtype", kc.DTYPES, ids=_ids(kc.DTYPES))
def test_workspace_degradation(dtype):
    """the split plan with a NULL workspace, with one a byte short of two splits and with exactly two splits, a canary behind (and,
    where the launch must not touch it, inside) the workspace"""
    key, case = kc.split_case(-1, dtype)
    p = case["plan"]
    t = _on_gpu(case)
    per_split = p.B * p.nq * (p.d + 2) * 4
    _assert_plan(p, case["max_kv_len"], 0, nsplit=1)
    _assert_meets_reference(_launch(case, t, workspace=None), case, key)
    buf = torch.full((2 * per_split + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    _assert_plan(p, case["max_kv_len"], 2 * per_split - 1, nsplit=1)
    one = _launch(case, t, workspace=buf[:2 * per_split - 1])
    _assert_meets_reference(one, case, key)
    assert (buf == 0xA5).all(), "one grid split writes no partials"
    _assert_plan(p, case["max_kv_len"], 2 * per_split, nsplit=2)
    two = _launch(case, t, workspace=buf[:2 * per_split])
    _assert_meets_reference(two, case, key)
    assert (buf[2 * per_split:] == 0xA5).all() and not (buf[:2 * per_split] == 0xA5).all()


@pytest.mark.parametrize("dtype", kc.DTYPES, ids=_ids(kc.DTYPES))
@pytest.mark.parametrize("plan", ALL_PLANS, ids=_ids(ALL_PLANS))
def test_pow2_scales_against_the_16bit_kernel(plan, dtype):
    """with power-of-two scales codes * scale is exact in bf16 and f16: the same float64 reference binds ops.paged_attention on the
    dequantised 16-bit cache, so the two kernels are within two bars of each other"""
    key, case = kc.pow2_case(plan, dtype)
    out, t = _run_and_check(key, case)
    kd = t["kc"].to(dtype) * case["k_scale"]
    vd = t["vc"].to(dtype) * case["v_scale"]
    live = ~torch.isnan(kd)
    assert torch.equal(kd[live].double().cpu(), kc.dequant64(case["kc"], case["k_scale"])[live.cpu()]), "dequantisation is exact"
    out16 = ops.paged_attention(t["q"], kd, vd, None, t["kv"], t["bt"], 1, case["max_kv_len"], case["scale"],
                                window_left=case["window_left"])
    rel, elem = kc.distance(out, out16)
    bar = kc.BAR_REL[dtype]
    print(f"{key}: kv8 kernel vs 16-bit kernel (rel L2 / bar, element-wise / bar) = {rel / bar:.3f}, {elem:.3f}")
    assert rel <= 2 * bar and elem <= 2.0


@pytest.mark.parametrize("dtype", kc.DTYPES, ids=_ids(kc.DTYPES))
def test_strided_q(dtype):
    """q as the leading columns of packed qkv rows (token stride (nq + 2 nkv) d): the bits of the contiguous call"""
    key, case = kc.plan_case(kc.PLAN["hpw4_part_page16"], dtype)
    p = case["plan"]
    out, t = _run_and_check(key, case)
    qkv = torch.full((p.B, (p.nq + 2 * p.nkv) * p.d), float("nan"), dtype=dtype, device=DEV)
    qkv[:, :p.nq * p.d] = t["q"].reshape(p.B, -1)
    qv = qkv[:, :p.nq * p.d].unflatten(-1, (p.nq, p.d))
    assert qv.stride(0) == (p.nq + 2 * p.nkv) * p.d
    out2 = ops.paged_attention_kv8(qv, t["kc"], t["vc"], t["ks"], t["vs"], t["kv"], t["bt"], case["max_kv_len"], case["scale"])
    assert torch.equal(out.view(torch.int16), out2.view(torch.int16))


@pytest.mark.parametrize("which", ["split", "gathered"])
def test_graph_capture_and_replay_after_in_place_changes(which):
    """captured once; replayed as captured and after kv_lens and the block table changed IN PLACE (the batch rolled by one row: every
    query now reads its neighbour's pages): bit-equal to the eager results"""
    dtype = torch.bfloat16
    key, case = kc.split_case(-1, dtype) if which == "split" else kc.plan_case(kc.PLAN["hpw4_part_page16"], dtype)
    out, t = _run_and_check(key, case)
    kv2, bt2 = torch.roll(t["kv"], 1, 0), torch.roll(t["bt"], 1, 0)
    t2 = dict(t, kv=kv2, bt=bt2)
    want2 = _launch(case, t2).clone()
    assert not torch.equal(out, want2)
    kv, bt = t["kv"].clone(), t["bt"].clone()
    ts = dict(t, kv=kv, bt=bt)
    res = torch.empty_like(out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _launch(case, ts, out=res)
    res.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(res.view(torch.int16), out.view(torch.int16))
    kv.copy_(kv2)
    bt.copy_(bt2)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(res.view(torch.int16), want2.view(torch.int16))


def test_existing_wrappers_refuse_an_e4m3_cache():
    c8 = torch.zeros(2, 16, 2, 128, dtype=FP8, device=DEV)
    q = torch.zeros(1, 4, 128, dtype=torch.bfloat16, device=DEV)
    kv, bt = torch.ones(1, dtype=torch.int32, device=DEV), torch.zeros(1, 1, dtype=torch.int32, device=DEV)
    s = torch.ones(1, device=DEV)
    with pytest.raises(ops.Mi355Error, match="float8_e4m3fn"):
        ops.paged_attention(q, c8, c8, None, kv, bt, 1, 1, 0.1)
    with pytest.raises(ops.Mi355Error, match="float8_e4m3fn"):
        ops.paged_decode_attention_int8(q, c8, c8, kv, bt, 1, 0.1)
    with pytest.raises(ops.Mi355Error, match="float8_e4m3fn"):
        ops.paged_decode_attention_fp8(q, c8, c8, kv, bt, 1, 0.1, s)
    k = torch.zeros(1, 2, 128, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ops.Mi355Error, match="float8_e4m3fn"):
        ops.reshape_paged_cache(kv, k, k, c8, c8)
    qkv = torch.zeros(1, 8 * 128, dtype=torch.bfloat16, device=DEV)
    cs = torch.zeros(8, 128, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ops.Mi355Error, match="float8_e4m3fn"):
        ops.rotary_embedding_and_cache(torch.zeros(1, dtype=torch.int64, device=DEV), qkv[:, :512], qkv[:, 512:768], qkv[:, 768:],
                                       cs, kv, c8, c8, 128)
    with pytest.raises(ops.Mi355Error, match="float8_e4m3fn"):
        ops.paged_attention_shared_prefix(q, c8, c8, kv, bt, torch.tensor([0, 1], dtype=torch.int32, device=DEV),
                                          torch.zeros(1, dtype=torch.int32, device=DEV), 1, 0, 0.1)


# ---------------------------------------------------------------------------------------------------------------- the writers
CANARY = 0xC3


def _writer_inputs(T, nq, nkv, d, bs, dtype, strided, seed):
    """k / v with values beyond +-448 * scale (saturation), exact +-0 and ordinary ones; slots: a permutation with negative and
    out-of-range entries; caches full of a canary byte"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    n_blocks = (T + bs - 1) // bs + 2
    width = (nq + 2 * nkv) * d
    qkv = torch.empty(T, width, dtype=torch.float32, device=DEV).normal_(generator=g)
    qkv[:, nq * d:] *= 3.0
    flat = qkv.view(-1)
    flat[::7] = 0.0
    flat[3::11] = -0.0
    flat[5::13] *= 100.0            # far beyond 448 * scale: saturates to +-448
    qkv = qkv.to(dtype)
    if not strided:
        q, k, v = (x.contiguous() for x in (qkv[:, :nq * d], qkv[:, nq * d:(nq + nkv) * d], qkv[:, (nq + nkv) * d:]))
    else:
        q, k, v = qkv[:, :nq * d], qkv[:, nq * d:(nq + nkv) * d], qkv[:, (nq + nkv) * d:]
    slots = torch.randperm(n_blocks * bs, generator=g, device=DEV)[:T].to(torch.int32)
    if T > 4:
        slots[1] = -1
        slots[2] = n_blocks * bs            # first slot past the cache
        slots[3] = n_blocks * bs + 5 * bs
    mk = lambda: torch.full((n_blocks, bs, nkv, d), CANARY, dtype=torch.uint8, device=DEV)
    ks = torch.tensor([0.037], dtype=torch.float32, device=DEV)
    vs = torch.tensor([0.0219], dtype=torch.float32, device=DEV)
    return q, k, v, slots, mk(), mk(), ks, vs, n_blocks


def _expected_cache(x16, scale, slots, n_blocks, bs, nkv, d):
    """static_scaled_fp8_quant -> torch scatter on a uint8 view"""
    T = x16.size(0)
    q8 = torch.empty(T, nkv * d, dtype=FP8, device=DEV)
    ops.static_scaled_fp8_quant(q8, x16.contiguous(), scale)
    exp = torch.full((n_blocks * bs, nkv * d), CANARY, dtype=torch.uint8, device=DEV)
    ok = (slots >= 0) & (slots < n_blocks * bs)
    exp[slots[ok].long()] = q8.view(torch.uint8)[ok]
    return exp.view(n_blocks, bs, nkv, d), q8.view(torch.uint8)


@pytest.mark.parametrize("dtype", kc.DTYPES, ids=_ids(kc.DTYPES))
@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "packed_qkv"])
@pytest.mark.parametrize("T", [1, 257])
@pytest.mark.parametrize("bs", [16, 128])
@pytest.mark.parametrize("d", [64, 128])
def test_reshape_paged_cache_kv8(d, bs, T, strided, dtype):
    nq, nkv = 4, 2
    q, k, v, slots, kcache, vcache, ks, vs, nb = _writer_inputs(T, nq, nkv, d, bs, dtype, strided, seed=d + bs + T)
    want_k, q8 = _expected_cache(k, ks, slots, nb, bs, nkv, d)
    want_v, _ = _expected_cache(v, vs, slots, nb, bs, nkv, d)
    if T > 1:
        assert (q8 == 0x7E).any() and (q8 == 0xFE).any() and (q8 == 0x00).any() and (q8 == 0x80).any(), "saturation and +-0 present"
    ops.reshape_paged_cache_kv8(slots, k.unflatten(-1, (nkv, d)), v.unflatten(-1, (nkv, d)), kcache.view(FP8), vcache.view(FP8),
                                ks, vs)
    assert torch.equal(kcache, want_k) and torch.equal(vcache, want_v)
    assert (kcache == CANARY).sum() >= (nb * bs - T) * nkv * d, "every byte outside the written slots keeps the canary"


@pytest.mark.parametrize("dtype", kc.DTYPES, ids=_ids(kc.DTYPES))
@pytest.mark.parametrize("neox,rot", [(True, None), (False, None), (True, 64)], ids=["neox", "interleaved", "neox_rot64"])
@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "packed_qkv"])
@pytest.mark.parametrize("T", [1, 257])
@pytest.mark.parametrize("d,bs", [(64, 16), (128, 128), (128, 16)])
def test_rotary_embedding_and_cache_kv8(d, bs, T, strided, neox, rot, dtype):
    """rotate with ops.rotary_embedding, quantise with ops.static_scaled_fp8_quant, scatter with torch: q and k bit-equal, both
    caches byte-equal, canaries kept"""
    nq, nkv = 4, 2
    rot = d if rot is None else rot
    q, k, v, slots, kcache, vcache, ks, vs, nb = _writer_inputs(T, nq, nkv, d, bs, dtype, strided, seed=3 * d + bs + T)
    g = torch.Generator(device=DEV).manual_seed(5)
    ang = torch.empty(512, rot // 2, device=DEV).uniform_(-3.14, 3.14, generator=g)
    cos_sin = torch.cat([ang.cos(), ang.sin()], -1).to(dtype)
    pos = torch.randint(0, 512, (T,), generator=g, device=DEV, dtype=torch.int64)
    q_ref, k_ref = q.clone(), k.clone()
    ops.rotary_embedding(pos, q_ref, k_ref, cos_sin, neox, head_size=d)
    assert not torch.equal(k_ref, k)
    want_k, _ = _expected_cache(k_ref, ks, slots, nb, bs, nkv, d)
    want_v, _ = _expected_cache(v, vs, slots, nb, bs, nkv, d)
    ops.rotary_embedding_and_cache_kv8(pos, q, k, v, cos_sin, slots, kcache.view(FP8), vcache.view(FP8), ks, vs, d, neox)
    i16 = lambda x: x.contiguous().view(torch.int16)
    assert torch.equal(i16(q), i16(q_ref)) and torch.equal(i16(k), i16(k_ref)), "q and k are the bits of rotary_embedding"
    assert torch.equal(kcache, want_k) and torch.equal(vcache, want_v)
