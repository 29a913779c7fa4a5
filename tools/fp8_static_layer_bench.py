#!/usr/bin/env python3
"""One Qwen2-7B decoder layer at the headline decode shape (B = 256, ctx = 4096, pages of 128 in random placement) in three
variants on the same weights: mode "fp8" (dynamic per-tensor activation scales: the yardstick), mode "fp8_static" unfused (the
reference's operator order on static scales) and mode "fp8_static" fused (the producers emit the next linear's e4m3 operand).
A steady-state layer is timed: two norms each -- the unfused forms run their own input norm and post-attention norm, the fused form
takes its input pre-quantised from its predecessor and ends with its successor's input norm.

Also the two new launches alone against the operator pairs they replace: ops.paged_decode_attention_fp8 against
ops.paged_attention + ops.static_scaled_fp8_quant, and ops.act_and_mul_static_fp8_quant against ops.act_and_mul +
ops.static_scaled_fp8_quant ([256, 2 x 18944]).

Method of tools/shared_prefix_bench.py: every variant is captured in a HIP graph of NC runs that rotate over NC KV-cache copies
(2 GiB each: every run streams its pages from HBM); after a warm-up the graphs of a group alternate in one process, ROUNDS times;
a timing is device events around enough replays for a window of WINDOW seconds. Reported: microseconds per run, median over the
rounds, with the spread (max - min of the rounds). The record is profiles/fp8_static_decode.txt."""
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xllm_amd import attention, layers, ops  # noqa: E402

dev = "cuda"
B, S, bs = int(os.environ.get("FS_BATCH", "256")), int(os.environ.get("FS_CTX", "4096")), 128
NC = int(os.environ.get("FS_COPIES", "2"))
ROUNDS = int(os.environ.get("FS_ROUNDS", "5"))
WINDOW = float(os.environ.get("FS_WINDOW", "0.25"))


def graph_of(fn):
    for i in range(NC):                     # eager once: sizes every scratch buffer outside the capture
        fn(i)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            for i in range(NC):
                fn(i)
    torch.cuda.current_stream().wait_stream(side)
    return g


def time_us(g, replays):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (replays * NC)


def alternate(named_fns):
    """[(name, fn(i))] -> [(name, median us, spread us)], the graphs alternating round by round"""
    graphs = [(n, graph_of(f)) for n, f in named_fns]
    for _, g in graphs:
        time_us(g, 10)
    reps = [max(5, int(WINDOW * 1e6 / (time_us(g, 10) * NC))) for _, g in graphs]
    t = [[] for _ in graphs]
    for _ in range(ROUNDS):
        for k, (_, g) in enumerate(graphs):
            t[k].append(time_us(g, reps[k]))
    return [(n, statistics.median(x), max(x) - min(x)) for (n, _), x in zip(graphs, t)]


def main():
    torch.manual_seed(0)
    args = layers.ModelArgs.qwen2_7b()
    nq, nkv, d, H, I = args.n_heads, args.n_kv_heads, args.head_dim, args.hidden_size, args.intermediate_size
    dtype = torch.bfloat16
    pages = S // bs
    nb = B * pages + 7
    caches = [attention.KVCache(torch.randn(nb, bs, nkv, d, device=dev).to(dtype), torch.randn(nb, bs, nkv, d, device=dev).to(dtype))
              for _ in range(NC)]
    blocks = torch.randperm(nb)[: B * pages].view(B, pages).tolist()
    bi = attention.build_batch_input([S - 1] * B, [S] * B, blocks, bs)
    md = attention.build_attention_metadata(bi, False, False, dev)
    positions = bi.positions.to(torch.int64).to(dev)
    cos_sin = layers.build_cos_sin_cache(args, dtype, dev, 8192)

    def layer(mode, fuse):
        return layers.Qwen2DecoderLayer(args, mode, dtype, dev, torch.Generator(device=dev).manual_seed(3), None, fuse)
    dyn, plain, fused = layer("fp8", False), layer("fp8_static", False), layer("fp8_static", True)
    x = torch.randn(B, H, device=dev).to(dtype)
    xs = [x.clone(), x.clone()]                                             # (the 16-bit norm of mode "fp8" writes its input)
    res = [torch.randn(B, H, device=dev).to(dtype) for _ in range(3)]       # (updated in place by every run: never read back)
    nxt_w = (torch.rand(H, device=dev) + 0.5).to(dtype)
    # static scales: calibrated on this step (every linear quantises dynamically once and keeps its scale)
    for lay in (plain, fused):
        lins = (lay.qkv_proj, lay.o_proj, lay.gate_up_proj, lay.down_proj)
        for l in lins:
            l.calibrating = True
        lay.forward(x.clone(), res[0].clone(), positions, md, caches[0], cos_sin)
        for l in lins:
            l.calibrating = False
    nxt_scale = fused.qkv_proj.input_scale
    h_in, _ = fused._norm_fp8_static(x.clone(), res[0].clone(), fused.input_norm_w, fused.qkv_proj)

    print(f"# fp8 decode layer, Qwen2-7B geometry: B={B} ctx={S} nq={nq} nkv={nkv} d={d} H={H} I={I} page={bs}, {NC} cache copies per "
          f"graph, {ROUNDS} alternating rounds, window {WINDOW} s, {torch.cuda.get_device_name(0)}")
    rows = alternate([
        ("layer, mode fp8 (dynamic scales; the parent's behaviour)", lambda i: dyn.forward(xs[0], res[0], positions, md, caches[i], cos_sin)),
        ("layer, mode fp8_static, fuse=False", lambda i: plain.forward(xs[1], res[1], positions, md, caches[i], cos_sin)),
        ("layer, mode fp8_static, fuse=True", lambda i: fused.forward(None, res[2], positions, md, caches[i], cos_sin, h_in=h_in,
                                                                      next_norm_w=nxt_w, next_input_scale=nxt_scale)),
    ])
    q = torch.randn(B, nq, d, device=dev).to(dtype)
    sc = 1.0 / math.sqrt(d)
    s_o = fused.o_proj.input_scale
    o8 = torch.empty(B, nq * d, dtype=ops.FP8, device=dev)

    def attn_pair(i):
        o = ops.paged_attention(q, caches[i].k_cache, caches[i].v_cache, None, md.kv_seq_lens, md.block_table, 1, S, sc)
        ops.static_scaled_fp8_quant(o8, o, s_o)
    rows += alternate([
        ("attention: paged_attention + static_scaled_fp8_quant", attn_pair),
        ("attention: paged_decode_attention_fp8", lambda i: ops.paged_decode_attention_fp8(
            q, caches[i].k_cache, caches[i].v_cache, md.kv_seq_lens, md.block_table, S, sc, s_o)),
    ])
    gu = torch.randn(B, 2 * I, device=dev).to(dtype)
    s_d = fused.down_proj.input_scale
    a16 = torch.empty(B, I, dtype=dtype, device=dev)
    a8 = torch.empty(B, I, dtype=ops.FP8, device=dev)

    def act_pair(i):
        ops.act_and_mul(a16, gu, "silu")
        ops.static_scaled_fp8_quant(a8, a16, s_d)
    rows += alternate([
        ("activation: act_and_mul + static_scaled_fp8_quant", act_pair),
        ("activation: act_and_mul_static_fp8_quant", lambda i: ops.act_and_mul_static_fp8_quant(gu, s_d, "silu")),
    ])
    print(f"# {'variant':<62} {'us':>9} {'spread':>8}")
    for name, med, spread in rows:
        print(f"  {name:<62} {med:9.1f} {spread:8.1f}", flush=True)


if __name__ == "__main__":
    main()
