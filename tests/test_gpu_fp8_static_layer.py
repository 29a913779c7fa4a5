"""GPU: the Qwen2 layer in mode "fp8_static" (static activation scales, xllm_amd/layers.py).

The fused layer (RoPE + KV write in one launch, decode attention and activation emitting the next linear's e4m3 operand, the
next layer's add + norm + static quant at the layer's end) is held to the unfused one -- the reference's operator order -- bit
for bit: logits, final hidden states, residual stream and both KV caches, on the same weights and the same calibrated scales.
Both new operators are byte-equal to operator pairs that are already under float64 bars (tests/test_gpu_fp8_static_ops.py), so
the layer needs no bar of its own; the distance between the static-scale logits and the dynamic-scale ones (mode "fp8") is
recorded, not asserted.

Tiny model: 2 layers, hidden 512, 4 / 2 heads of d = 128, intermediate 1024, vocab 1024, pages of 128 -- inside the packed fp8
envelope (N % 16, K % 128, K >= 512). Decode lengths are _decode_cases.ragged_lens(B) with the empty row as one token (a decode
row holds at least its own token); at B = 3 the first row is lengthened to 2860 tokens, where the planner splits the KV range
over the grid (the merge launch quantises), and B = 192 is one grid split with both kv heads in a workgroup (the attention
epilogue quantises). Both plans are asserted. The model is calibrated on the step itself."""
import ctypes as C

import pytest
import torch

import _decode_cases as dc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from xllm_amd import _lib, attention, layers, ops
    from xllm_amd.attention import KVCache
DEV = "cuda"
BS = 128


def _args():
    return layers.ModelArgs(hidden_size=512, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=128, intermediate_size=1024,
                            vocab_size=1024)


_MODELS = {}


def _model(mode, fuse):
    """one model per (mode, fuse) in the process: the same seed, so the same weights in every one of them"""
    if (mode, fuse) not in _MODELS:
        _MODELS[(mode, fuse)] = layers.Qwen2Model(_args(), mode, torch.bfloat16, DEV, seed=41, fuse=fuse)
    return _MODELS[(mode, fuse)]


class Step:
    """the inputs of one model step: cached[b] tokens in the cache, lens[b] after the step, pages dealt from a permutation"""

    def __init__(self, cached, lens, chunked=False, seed=0):
        g = torch.Generator().manual_seed(900 + seed)
        pages = [(L + BS - 1) // BS for L in lens]
        self.nb = sum(pages) + 2
        perm = torch.randperm(self.nb, generator=g).tolist()
        blocks, used = [], 0
        for n in pages:
            blocks.append(perm[used:used + n])
            used += n
        bi = attention.build_batch_input(cached, lens, blocks, BS)
        self.md = attention.build_attention_metadata(bi, False, chunked, DEV)
        T = sum(L - c for c, L in zip(cached, lens))
        self.tokens = torch.randint(0, 1024, (T,), generator=g).to(DEV)
        self.positions = bi.positions.to(torch.int64).to(DEV)
        self.B, self.max_kv_len = len(lens), max(lens)

    def caches(self, model):
        gd = torch.Generator(device=DEV).manual_seed(77)
        mk = lambda: torch.empty(self.nb, BS, 2, 128, dtype=torch.bfloat16, device=DEV).normal_(generator=gd)
        return [KVCache(mk(), mk()) for _ in model.layers]


def _decode_step(B):
    lens = [max(L, 1) for L in dc.ragged_lens(B)]
    if B == 3:
        lens[0] = 2860          # 90 tiles: hpw = 1 (nsub = 4) -> 2 grid splits
    return Step([L - 1 for L in lens], lens, seed=B)


def _plan(B, max_kv_len):
    v = [C.c_int32(-1) for _ in range(4)]
    assert _lib.lib().xllm_mi355_paged_decode_plan(B, 2, BS, max_kv_len, *[C.byref(x) for x in v]) == 0
    return v[0].value, v[1].value      # hpw, nsplit


def _run(model, step, caches):
    """Qwen2Model.forward's loop, returning the residual stream as well: (final hidden states, residual)"""
    x = torch.nn.functional.embedding(step.tokens, model.embed)
    residual, h_in, n = None, None, len(model.layers)
    for i, (layer, kvc) in enumerate(zip(model.layers, caches)):
        last = i + 1 == n
        x, residual, h_in = layer.forward(x, residual, step.positions, step.md, kvc, model.cos_sin, h_in=h_in,
                                          next_norm_w=model.norm_w if last else model.layers[i + 1].input_norm_w,
                                          next_quant=not last,
                                          next_input_scale=None if last else model.layers[i + 1].qkv_proj.input_scale)
        assert last or (h_in is not None) == (layer.fuse_fp8 and not (step.md.is_prefill or step.md.is_chunked_prefill))
    assert h_in is None, "the final norm stays 16-bit"
    ops.fused_add_rms_norm(x, residual, model.norm_w, model.args.rms_norm_eps)
    return x, residual


def _linears(model):
    return [l for layer in model.layers for l in (layer.qkv_proj, layer.o_proj, layer.gate_up_proj, layer.down_proj)]


def _calibrated_pair(step):
    """the fused and the unfused model, both calibrated on this step: the same scales, bit for bit"""
    fused, plain = _model("fp8_static", True), _model("fp8_static", False)
    assert all(l.fuse_fp8 for l in fused.layers) and not any(l.fuse_fp8 for l in plain.layers)
    for m in (fused, plain):
        m.calibrate_fp8_static(step.tokens, step.positions, step.md, step.caches(m))
    for a, b in zip(_linears(fused), _linears(plain)):
        assert torch.equal(a.weight.view(torch.uint8), b.weight.view(torch.uint8))
        assert torch.equal(a.input_scale, b.input_scale)
    return fused, plain


def _assert_steps_equal(step, fused, plain):
    cf, cp = step.caches(fused), step.caches(plain)
    before = [c.k_cache.clone() for c in cf]
    hf, rf = _run(fused, step, cf)
    hp, rp = _run(plain, step, cp)
    i16 = lambda t: t.view(torch.int16)
    assert torch.isfinite(hf.float()).all()
    assert torch.equal(i16(rf), i16(rp)), "residual stream"
    assert torch.equal(i16(hf), i16(hp)), "final hidden states"
    assert torch.equal(i16(fused.logits(hf)), i16(plain.logits(hp))), "logits"
    for a, b, k0 in zip(cf, cp, before):
        assert torch.equal(i16(a.k_cache), i16(b.k_cache)) and torch.equal(i16(a.v_cache), i16(b.v_cache)), "KV caches"
        slots = step.md.slot_mapping.long()
        assert not torch.equal(a.k_cache.view(-1, 2, 128)[slots], k0.view(-1, 2, 128)[slots]), "the step wrote its K rows"
    # and the model's own loop gives what the loop above gives
    assert torch.equal(i16(fused.forward(step.tokens, step.positions, step.md, step.caches(fused))), i16(hf))
    return hf


@pytest.mark.parametrize("B", [3, 192])
def test_fused_decode_step_equals_unfused(B):
    step = _decode_step(B)
    hpw, nsplit = _plan(B, step.max_kv_len)
    assert (hpw, nsplit) == ((1, 2) if B == 3 else (2, 1)), f"B={B}: the planner gives hpw={hpw}, {nsplit} splits"
    fused, plain = _calibrated_pair(step)
    _assert_steps_equal(step, fused, plain)


def test_fused_prefill_chunk_equals_unfused():
    """one chunk of a chunked prefill (a first chunk, a later chunk on cached tokens, a single-token row): the fused form differs
    from the unfused one by the activation kernel and the RoPE + KV write launch only"""
    step = Step([0, 128, 37], [33, 168, 38], chunked=True, seed=7)
    assert step.md.is_chunked_prefill
    fused, plain = _calibrated_pair(step)
    _assert_steps_equal(step, fused, plain)


def test_calibration_sets_every_scale_and_is_deterministic():
    step = _decode_step(3)
    m = _model("fp8_static", True)
    for l in _linears(m):
        assert l.input_scale.dtype == torch.float32 and l.input_scale.shape == (1,) and l.input_scale.is_cuda
        l.input_scale.fill_(1.0)
    h1 = m.calibrate_fp8_static(step.tokens, step.positions, step.md, step.caches(m)).clone()
    first = [l.input_scale.clone() for l in _linears(m)]
    assert len(first) == 8
    for s in first:
        assert torch.isfinite(s).all() and float(s) > 0.0 and float(s) != 1.0
    assert not any(l.calibrating for l in _linears(m))
    h2 = m.calibrate_fp8_static(step.tokens, step.positions, step.md, step.caches(m))
    for l, s in zip(_linears(m), first):
        assert torch.equal(l.input_scale, s)
    assert torch.equal(h1.view(torch.int16), h2.view(torch.int16))
    # a pre-quantised operand is taken as it is; a 16-bit one is quantised with the static scale
    lin = m.layers[0].o_proj
    x = torch.randn(5, 512, device=DEV).bfloat16()
    q, s = ops.fp8_scaled_quantize(x, scale=lin.input_scale)
    assert s is lin.input_scale
    assert torch.equal(lin.forward(x).view(torch.int16), lin.forward(None, pre_quant=(q, lin.input_scale)).view(torch.int16))


@pytest.mark.parametrize("B", [3, 192])
def test_fused_decode_step_replays_from_a_graph(B):
    step = _decode_step(B)
    fused, _ = _calibrated_pair(step)
    want = _run(fused, step, step.caches(fused))[0].clone()
    caches = step.caches(fused)
    start = [(c.k_cache.clone(), c.v_cache.clone()) for c in caches]
    fused.forward(step.tokens, step.positions, step.md, caches)         # warm-up: scratch buffers exist before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        hid = fused.forward(step.tokens, step.positions, step.md, caches)
        logits = fused.logits(hid)
    for i in range(2):
        for c, (k0, v0) in zip(caches, start):
            c.k_cache.copy_(k0)
            c.v_cache.copy_(v0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(hid.view(torch.int16), want.view(torch.int16)), i
        assert torch.equal(logits.view(torch.int16), fused.logits(want).view(torch.int16)), i


def test_static_against_dynamic_scales_is_recorded():
    """per-row relative L2 between the logits of mode "fp8_static" (calibrated on the step) and of mode "fp8" (dynamic per-tensor
    scales) on the same weights; recorded next to the parity records of tests/test_gpu_model_parity.py (its _record;
    profiles/fp8_static_decode.txt keeps a copy), no bar"""
    from test_gpu_model_parity import _record
    for B in (3, 192):
        step = _decode_step(B)
        static, _ = _calibrated_pair(step)
        dyn = _model("fp8", False)
        for a, b in zip(_linears(static), _linears(dyn)):
            assert torch.equal(a.weight.view(torch.uint8), b.weight.view(torch.uint8))
        ls = static.logits(static.forward(step.tokens, step.positions, step.md, step.caches(static))).float()
        ld = dyn.logits(dyn.forward(step.tokens, step.positions, step.md, step.caches(dyn))).float()
        assert torch.isfinite(ls).all() and torch.isfinite(ld).all()
        rel = (ls - ld).norm(dim=1) / ld.norm(dim=1).clamp_min(1e-30)
        print(f"fp8_static vs fp8 (dynamic) logits, tiny model, decode B={B}: per-row rel L2 median {float(rel.median()):.4e} "
              f"max {float(rel.max()):.4e}")
        _record(test="fp8_static_vs_fp8_dynamic_logits", geometry="tiny_2layer_ragged_decode", batch=B,
                rel_l2_median=float(rel.median()), rel_l2_max=float(rel.max()))
