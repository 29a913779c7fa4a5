"""GPU: the Qwen2 layer on an e4m3 KV cache with static scales (xllm_amd/layers.py, xllm_amd/attention.py).

With an e4m3 KVCache the layer skips the fusions that write or read the cache in 16 bits and runs qkv_proj ->
ops.rotary_embedding_and_cache_kv8 -> ops.paged_attention_kv8 -> the mode's own quantiser in front of o_proj. Each step is held,
bit for bit, to a hand-composed sequence of the public operators -- qkv_proj, rotary_embedding, static_scaled_fp8_quant + a torch
scatter, paged_attention_kv8, the mode's quantiser, the rest of the layer: logits, residual stream and both caches' bytes. The
operators themselves are under float64 bars in tests/test_gpu_kv_fp8_ops.py, so the layer needs none of its own; the distance of
the e4m3-cache logits from the 16-bit-cache logits is recorded, not asserted.

Tiny model of tests/test_gpu_fp8_static_layer.py: 2 layers, hidden 512, 4 / 2 heads of d = 128, pages of 128; scales from
Qwen2Model.calibrate_kv_scales on the step. Decode at B = 192 (hpw = 2: both kv heads in a workgroup, one grid split) and at
B = 3 with a row of 2860 tokens (hpw = 1, two grid splits: the merge launch); both plans are asserted."""
import pytest
import torch

import _decode_cases as dc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from xllm_amd import attention, engine, layers, ops
    from xllm_amd.attention import KVCache
DEV = "cuda"
BS = 128
FP8 = torch.float8_e4m3fn
MODES = ["int8", "fp8_static"]


def _args():
    return layers.ModelArgs(hidden_size=512, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=128, intermediate_size=1024,
                            vocab_size=1024)


_MODELS = {}


def _model(mode):
    if mode not in _MODELS:
        _MODELS[mode] = layers.Qwen2Model(_args(), mode, torch.bfloat16, DEV, seed=41, fuse=True)
    return _MODELS[mode]


class Step:
    """the inputs of one model step: cached[b] tokens in the cache, lens[b] after the step, pages dealt from a permutation"""

    def __init__(self, cached, lens, prefill=False, chunked=False, seed=0):
        g = torch.Generator().manual_seed(900 + seed)
        pages = [(L + BS - 1) // BS for L in lens]
        self.nb = sum(pages) + 2
        perm = torch.randperm(self.nb, generator=g).tolist()
        self.blocks, used = [], 0
        for n in pages:
            self.blocks.append(perm[used:used + n])
            used += n
        bi = attention.build_batch_input(cached, lens, self.blocks, BS)
        self.md = attention.build_attention_metadata(bi, prefill, chunked, DEV)
        T = sum(L - c for c, L in zip(cached, lens))
        self.tokens = torch.randint(0, 1024, (T,), generator=g).to(DEV)
        self.positions = bi.positions.to(torch.int64).to(DEV)
        self.B, self.max_kv_len, self.lens = len(lens), max(lens), list(lens)

    def caches16(self, n_layers=2):
        gd = torch.Generator(device=DEV).manual_seed(77)
        mk = lambda: torch.empty(self.nb, BS, 2, 128, dtype=torch.bfloat16, device=DEV).normal_(generator=gd)
        return [KVCache(mk(), mk()) for _ in range(n_layers)]

    def caches8(self, scales, n_layers=2):
        """the 16-bit history quantised with each layer's scales (saturating where the history exceeds 448 * scale)"""
        out = []
        for c, (ks, vs) in zip(self.caches16(n_layers), scales):
            k8, v8 = torch.empty(c.k_cache.shape, dtype=FP8, device=DEV), torch.empty(c.v_cache.shape, dtype=FP8, device=DEV)
            ops.static_scaled_fp8_quant(k8, c.k_cache, ks)
            ops.static_scaled_fp8_quant(v8, c.v_cache, vs)
            out.append(KVCache(k8, v8, ks.clone(), vs.clone()))
        return out


def _decode_step(B):
    lens = [max(L, 1) for L in dc.ragged_lens(B)]
    if B == 3:
        lens[0] = 2860          # 90 tiles: hpw = 1 (nsub = 4) -> 2 grid splits
    return Step([L - 1 for L in lens], lens, seed=B)


def _calibrated_scales(model, step):
    """calibrate_kv_scales on the step, into scratch caches: [(k_scale, v_scale)] per layer"""
    one = lambda: torch.ones(1, dtype=torch.float32, device=DEV)
    scratch = [KVCache(torch.zeros(step.nb, BS, 2, 128, dtype=FP8, device=DEV), torch.zeros(step.nb, BS, 2, 128, dtype=FP8, device=DEV),
                       one(), one()) for _ in model.layers]
    if model.layers[0].mode == "fp8_static":
        model.calibrate_fp8_static(step.tokens, step.positions, step.md, step.caches16())
    model.calibrate_kv_scales(step.tokens, step.positions, step.md, scratch)
    assert not any(getattr(c, "calibrating", False) for c in scratch)
    for c in scratch:
        for s in (c.k_scale, c.v_scale):
            assert s.shape == (1,) and torch.isfinite(s).all() and 0.0 < float(s) < 1.0
    return [(c.k_scale, c.v_scale) for c in scratch]


def _quant_scatter(x, scale, cache, slots):
    """static_scaled_fp8_quant + a torch scatter on the uint8 view"""
    q8 = torch.empty(x.shape, dtype=FP8, device=DEV)
    ops.static_scaled_fp8_quant(q8, x, scale)
    cache.view(torch.uint8).view(-1, x.size(-1))[slots.long()] = q8.view(torch.uint8)


def _hand_layer(layer, x, residual, h_in, step, kvc, cos_sin, next_norm_w, next_quant, next_input_scale):
    """one decode layer as a sequence of public operators around the e4m3 cache"""
    md, static = step.md, layer.mode == "fp8_static"
    if h_in is not None:
        h = h_in
    elif static:
        h, residual = layer._norm_fp8_static(x, residual, layer.input_norm_w, layer.qkv_proj)
    else:
        h, residual = layer._norm(x, residual, layer.input_norm_w)
    qkv = layer.qkv_proj.forward(None, pre_quant=h)
    q, k, v = qkv[:, :layer.q_size], qkv[:, layer.q_size:layer.q_size + layer.kv_size], qkv[:, layer.q_size + layer.kv_size:]
    ops.rotary_embedding(step.positions, q, k, cos_sin, True, head_size=layer.d)
    _quant_scatter(k, kvc.k_scale, kvc.k_cache, md.slot_mapping)
    _quant_scatter(v, kvc.v_scale, kvc.v_cache, md.slot_mapping)
    attn = ops.paged_attention_kv8(q.unflatten(-1, (layer.nq, layer.d)), kvc.k_cache, kvc.v_cache, kvc.k_scale, kvc.v_scale,
                                   md.kv_seq_lens, md.block_table, md.max_seq_len, layer.attn.scale, layer.attn.window_left)
    if not static:
        return layer.post_attention(ops.scaled_quantize(attn), residual, next_norm_w, next_quant)
    s_o, s_d = layer.o_proj.input_scale, layer.down_proj.input_scale
    q8 = torch.empty(attn.shape, dtype=FP8, device=DEV)
    ops.static_scaled_fp8_quant(q8, attn, s_o)
    x = layer.o_proj.forward(None, pre_quant=(q8, s_o))
    h, residual = layer._norm_fp8_static(x, residual, layer.post_norm_w, layer.gate_up_proj)
    gate_up = layer.gate_up_proj.forward(None, pre_quant=h)
    x = layer.down_proj.forward(None, pre_quant=(ops.act_and_mul_static_fp8_quant(gate_up, s_d, "silu"), s_d))
    if next_norm_w is not None and next_input_scale is not None:
        h_next, residual = layer._norm_fp8_static(x, residual, next_norm_w, None, scale=next_input_scale)
        return None, residual, h_next
    return x, residual, None


def _run(model, step, caches, layer_fn=None):
    """Qwen2Model.forward's loop (or the hand-composed layers), returning (final hidden states, residual)"""
    x = torch.nn.functional.embedding(step.tokens, model.embed)
    residual, h_in, n = None, None, len(model.layers)
    for i, (layer, kvc) in enumerate(zip(model.layers, caches)):
        last = i + 1 == n
        nw = model.norm_w if last else model.layers[i + 1].input_norm_w
        ns = None if last else model.layers[i + 1].qkv_proj.input_scale
        if layer_fn is None:
            x, residual, h_in = layer.forward(x, residual, step.positions, step.md, kvc, model.cos_sin, h_in=h_in, next_norm_w=nw,
                                              next_quant=not last, next_input_scale=ns)
        else:
            x, residual, h_in = layer_fn(layer, x, residual, h_in, step, kvc, model.cos_sin, nw, not last, ns)
    if h_in is not None:
        return h_in, residual
    ops.fused_add_rms_norm(x, residual, model.norm_w, model.args.rms_norm_eps)
    return x, residual


_i16 = lambda t: t.contiguous().view(torch.int16)
_u8 = lambda t: t.view(torch.uint8)


@pytest.mark.parametrize("B", [3, 192])
@pytest.mark.parametrize("mode", MODES)
def test_decode_step_equals_the_operator_sequence(mode, B):
    step = _decode_step(B)
    plan = ops.paged_decode_kv8_plan(B, 4, 2, 128, BS, step.max_kv_len)
    assert plan == ((1, 2, 2, 1) if B == 3 else (2, 1, 1, 1)), f"B={B}: (hpw, planned, nsplit, uniform) = {plan}"
    model = _model(mode)
    scales = _calibrated_scales(model, step)
    ca, cb = step.caches8(scales), step.caches8(scales)
    before = [_u8(c.k_cache).clone() for c in ca]
    ha, ra = _run(model, step, ca)
    hb, rb = _run(model, step, cb, _hand_layer)
    assert torch.isfinite(ha.float()).all()
    assert torch.equal(_i16(ra), _i16(rb)), "residual stream"
    assert torch.equal(_i16(ha), _i16(hb)), "final hidden states"
    assert torch.equal(_i16(model.logits(ha)), _i16(model.logits(hb))), "logits"
    slots = step.md.slot_mapping.long()
    for a, b, k0 in zip(ca, cb, before):
        assert torch.equal(_u8(a.k_cache), _u8(b.k_cache)) and torch.equal(_u8(a.v_cache), _u8(b.v_cache)), "cache bytes"
        assert not torch.equal(_u8(a.k_cache).view(-1, 256)[slots], k0.view(-1, 256)[slots]), "the step wrote its K rows"
    # the model's own loop gives what the loop above gives
    assert torch.equal(_i16(model.forward(step.tokens, step.positions, step.md, step.caches8(scales))), _i16(ha))


@pytest.mark.parametrize("mode", MODES)
def test_prefill_writes_the_sequence_bytes_and_reads_no_cache(mode):
    """prefill attention reads the step's 16-bit k / v: logits bit-equal to the 16-bit-cache model's; the e4m3 cache holds
    static_scaled_fp8_quant of the rows the 16-bit model wrote (its cache rows are the rotated k and v), scattered"""
    step = Step([0, 0, 0], [33, 168, 1], prefill=True, seed=11)
    assert step.md.is_prefill
    model = _model(mode)
    scales = _calibrated_scales(model, step)
    c8, c16 = step.caches8(scales), step.caches16()
    canary = [(_u8(c.k_cache).clone(), _u8(c.v_cache).clone()) for c in c8]
    l8 = model.logits(model.forward(step.tokens, step.positions, step.md, c8))
    l16 = model.logits(model.forward(step.tokens, step.positions, step.md, c16))
    assert torch.isfinite(l8.float()).all() and torch.equal(_i16(l8), _i16(l16))
    slots = step.md.slot_mapping.long()
    for a, b, (k0, v0) in zip(c8, c16, canary):
        for got, c16t, scale, start in ((a.k_cache, b.k_cache, a.k_scale, k0), (a.v_cache, b.v_cache, a.v_scale, v0)):
            want = start.clone()
            _quant_scatter(c16t.view(-1, 256)[slots], scale, want, slots)
            assert torch.equal(_u8(got), want)


@pytest.mark.parametrize("mode", MODES)
def test_chunked_prefill_is_refused(mode):
    step = Step([0, 128, 37], [33, 168, 38], chunked=True, seed=7)
    assert step.md.is_chunked_prefill
    model = _model(mode)
    scales = _calibrated_scales(model, _decode_step(3))
    with pytest.raises(NotImplementedError, match="chunked prefill over an e4m3 KV cache"):
        model.forward(step.tokens, step.positions, step.md, step.caches8(scales))
    torch.cuda.synchronize()


def test_existing_wrappers_and_16bit_attention_refuse_an_e4m3_cache():
    step = _decode_step(3)
    c8 = step.caches8([(torch.ones(1, device=DEV), torch.ones(1, device=DEV))] * 2)[0]
    q = torch.zeros(3, 4, 128, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ops.Mi355Error, match="float8_e4m3fn"):
        ops.paged_attention(q, c8.k_cache, c8.v_cache, None, step.md.kv_seq_lens, step.md.block_table, 1, step.max_kv_len, 0.1)
    with pytest.raises(ops.Mi355Error, match="float8_e4m3fn"):
        ops.paged_decode_attention_int8(q, c8.k_cache, c8.v_cache, step.md.kv_seq_lens, step.md.block_table, step.max_kv_len, 0.1)
    with pytest.raises(ValueError):
        KVCache(c8.k_cache, c8.v_cache)                       # an e4m3 cache without scales
    with pytest.raises(ValueError):
        KVCache(c8.k_cache, c8.v_cache, torch.ones(1), torch.ones(1))     # scales on the host


def test_16bit_cache_takes_the_parent_path():
    """a 16-bit KVCache without scales: Qwen2DecoderLayer.forward launches what pre_attention -> attention_kernel -> post_attention
    launch (the dual micro-batch executor's cut of the same decode layer, code this change does not touch): logits, residual and
    caches bit for bit"""
    def parent_layer(layer, x, residual, h_in, step, kvc, cos_sin, nw, nq_, ns):
        q, residual = layer.pre_attention(x, residual, step.positions, step.md, kvc, cos_sin, h_in=h_in)
        return layer.post_attention(layer.attention_kernel(q, step.md, kvc), residual, nw, nq_)

    model = _model("int8")
    for B in (3, 192):
        step = _decode_step(B)
        ca, cb = step.caches16(), step.caches16()
        assert not ca[0].is_fp8 and ca[0].k_scale is None
        ha, ra = _run(model, step, ca)
        hb, rb = _run(model, step, cb, parent_layer)
        assert torch.equal(_i16(ha), _i16(hb)) and torch.equal(_i16(ra), _i16(rb))
        for a, b in zip(ca, cb):
            assert torch.equal(_i16(a.k_cache), _i16(b.k_cache)) and torch.equal(_i16(a.v_cache), _i16(b.v_cache))


@pytest.mark.parametrize("mode", MODES)
def test_engine_graph_replay_equals_eager_steps(mode):
    """three DecodeEngine steps on e4m3 caches: captured graph replays give the tokens and the cache bytes of the eager steps"""
    step = _decode_step(3)
    model = _model(mode)
    scales = _calibrated_scales(model, step)
    seq_lens = [L - 1 for L in step.lens]
    # room for three more tokens per sequence inside the pages dealt above, else one more page each
    nb = step.nb
    blocks = []
    for b, L in zip(step.blocks, step.lens):
        need = (L + 3 + BS - 1) // BS
        blocks.append(list(b) + list(range(nb, nb + need - len(b))))
        nb += need - len(b)

    def caches():
        out = []
        for c in step.caches8(scales):
            grow = lambda t: torch.cat([t.view(torch.uint8), torch.zeros(nb - step.nb, BS, 2, 128, dtype=torch.uint8, device=DEV)]).view(FP8)
            out.append(KVCache(grow(c.k_cache), grow(c.v_cache), c.k_scale, c.v_scale))
        return out

    runs = {}
    for use_graph in (False, True):
        cs = caches()
        eng = engine.DecodeEngine(model, cs, BS, seq_lens, blocks, step.tokens.to(torch.int32), max_seq_len=step.max_kv_len + 3,
                                  use_graph=use_graph)
        toks = [eng.step().clone() for _ in range(3)]
        torch.cuda.synchronize()
        runs[use_graph] = (toks, [(_u8(c.k_cache).clone(), _u8(c.v_cache).clone()) for c in cs])
    for a, b in zip(runs[False][0], runs[True][0]):
        assert torch.equal(a, b), "tokens"
    for (ka, va), (kb, vb) in zip(runs[False][1], runs[True][1]):
        assert torch.equal(ka, kb) and torch.equal(va, vb), "cache bytes"


def test_e4m3_cache_against_16bit_cache_logits_are_recorded():
    """per-row relative L2 between the decode logits on an e4m3 cache (the 16-bit history quantised with the calibrated scales) and
    on the 16-bit cache itself, mode "int8"; recorded next to the parity records of tests/test_gpu_model_parity.py, no bar"""
    from test_gpu_model_parity import _record
    model = _model("int8")
    for B in (3, 192):
        step = _decode_step(B)
        scales = _calibrated_scales(model, step)
        l8 = model.logits(model.forward(step.tokens, step.positions, step.md, step.caches8(scales))).float()
        l16 = model.logits(model.forward(step.tokens, step.positions, step.md, step.caches16())).float()
        assert torch.isfinite(l8).all() and torch.isfinite(l16).all()
        rel = (l8 - l16).norm(dim=1) / l16.norm(dim=1).clamp_min(1e-30)
        print(f"e4m3 KV cache vs 16-bit KV cache logits, tiny model, mode int8, decode B={B}: per-row rel L2 median "
              f"{float(rel.median()):.4e} max {float(rel.max()):.4e}")
        _record(test="kv_fp8_vs_16bit_cache_logits", geometry="tiny_2layer_ragged_decode", batch=B,
                rel_l2_median=float(rel.median()), rel_l2_max=float(rel.max()))
