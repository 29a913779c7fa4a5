#!/usr/bin/env python3
"""Decode attention on an e4m3 KV cache with static scales (ops.paged_attention_kv8) against ops.paged_attention on a bf16 cache of
the same shape, pages of 128 in random placement, ctx 4096:
  * B = 256, 28 q / 4 kv heads, d = 128 (the headline decode shape);
  * the per-rank shapes B = 64 and B = 32 at 4 kv heads;
  * B = 128 at 1 kv head (7 q heads: a TP-4 rank).
Also the two KV writers against the operator sequences that define them (static_scaled_fp8_quant + a torch scatter, with
ops.rotary_embedding in front for the fused form) at T = 256 (a decode step) and T = 4096 (a prefill chunk), and one Qwen2-7B
decode layer in mode "int8" with a 16-bit and with an e4m3 cache.

Method of tools/fp8_static_layer_bench.py: every variant is captured in a HIP graph of NC runs that rotate over NC cache copies
(every run streams its pages from HBM); after a warm-up the graphs of a group alternate in one process, ROUNDS times; a timing is
device events around enough replays for a window of WINDOW seconds. Reported: microseconds per run, median over the rounds, with
the spread (max - min of the rounds), and for the attention launches the algorithmic bytes B * (S * nkv * d * 2 * e + 2 * nq * d
* 2) (e = cache bytes per element) as GB/s and as a fraction of 8 TB/s. The record is profiles/kv_fp8_decode.txt."""
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xllm_amd import attention, layers, ops  # noqa: E402

dev = "cuda"
S, bs = int(os.environ.get("KV8_CTX", "4096")), 128
NC = int(os.environ.get("KV8_COPIES", "2"))
ROUNDS = int(os.environ.get("KV8_ROUNDS", "5"))
WINDOW = float(os.environ.get("KV8_WINDOW", "0.2"))
FP8 = torch.float8_e4m3fn


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


def scale_t(v):
    return torch.tensor([v], dtype=torch.float32, device=dev)


def make_caches(B, nkv, d):
    """NC bf16 cache pairs and their e4m3 quantisations (scale 0.013: randn does not saturate), one block table"""
    pages = S // bs
    nb = B * pages + 7
    ks, vs = scale_t(0.013), scale_t(0.0135)
    c16, c8 = [], []
    for _ in range(NC):
        k, v = (torch.randn(nb, bs, nkv, d, device=dev).bfloat16() for _ in range(2))
        k8, v8 = torch.empty(k.shape, dtype=FP8, device=dev), torch.empty(v.shape, dtype=FP8, device=dev)
        ops.static_scaled_fp8_quant(k8, k, ks)
        ops.static_scaled_fp8_quant(v8, v, vs)
        c16.append(attention.KVCache(k, v))
        c8.append(attention.KVCache(k8, v8, ks, vs))
    blocks = torch.randperm(nb)[: B * pages].view(B, pages).tolist()
    return c16, c8, blocks


def attention_rows(B, nq, nkv, d=128):
    c16, c8, blocks = make_caches(B, nkv, d)
    bt = torch.tensor(blocks, dtype=torch.int32, device=dev)
    kv = torch.full((B,), S, dtype=torch.int32, device=dev)
    q = torch.randn(B, nq, d, device=dev).bfloat16()
    sc = 1.0 / math.sqrt(d)
    plan16 = ops.paged_decode_kv8_plan(B, nq, nkv, d, bs, S)
    rows = alternate([
        ("paged_attention, bf16 cache", lambda i: ops.paged_attention(q, c16[i].k_cache, c16[i].v_cache, None, kv, bt, 1, S, sc)),
        ("paged_attention_kv8, e4m3 cache", lambda i: ops.paged_attention_kv8(q, c8[i].k_cache, c8[i].v_cache, c8[i].k_scale,
                                                                                c8[i].v_scale, kv, bt, S, sc)),
    ])
    print(f"# attention B={B} ctx={S} nq={nq} nkv={nkv} d={d}: plan (hpw, planned, nsplit, uniform) = {plan16}")
    for (name, med, spread), e in zip(rows, (2, 1)):
        nbytes = B * (S * nkv * d * 2 * e + 2 * nq * d * 2)
        print(f"  {name:<40} {med:9.1f} us  spread {spread:6.1f}  {nbytes:>13d} B  {nbytes / med / 1e3:8.1f} GB/s  "
              f"{nbytes / med / 1e3 / 8000:5.3f} of 8 TB/s", flush=True)
    a, b = rows
    gain = a[1] / b[1]
    verdict = "faster than the 16-bit launch by more than both spreads" if a[1] - b[1] > a[2] + b[2] else \
        "NOT faster than the 16-bit launch by more than both spreads"
    print(f"  -> 16-bit / e4m3 = {gain:.3f} x: {verdict}", flush=True)
    del c16, c8
    torch.cuda.empty_cache()


def writer_rows(T, nq=28, nkv=4, d=128):
    args = layers.ModelArgs.qwen2_7b()
    dtype = torch.bfloat16
    cos_sin = layers.build_cos_sin_cache(args, dtype, dev, 8192)
    nb = (T + bs - 1) // bs + 4
    ks, vs = scale_t(0.05), scale_t(0.05)
    qkv = [torch.randn(T, (nq + 2 * nkv) * d, device=dev).to(dtype) for _ in range(NC)]
    kc, vc = (torch.zeros(nb, bs, nkv, d, dtype=FP8, device=dev) for _ in range(2))
    slots = torch.randperm(nb * bs, device=dev)[:T].to(torch.int32)
    slots64 = slots.long()
    pos = torch.randint(0, 4096, (T,), device=dev, dtype=torch.int64)
    k8, v8 = (torch.empty(T, nkv * d, dtype=FP8, device=dev) for _ in range(2))
    parts = lambda i: (qkv[i][:, :nq * d], qkv[i][:, nq * d:(nq + nkv) * d], qkv[i][:, (nq + nkv) * d:])

    def seq_write(i):
        _, k, v = parts(i)
        ops.static_scaled_fp8_quant(k8, k, ks)
        ops.static_scaled_fp8_quant(v8, v, vs)
        kc.view(torch.uint8).view(-1, nkv * d).index_copy_(0, slots64, k8.view(torch.uint8))
        vc.view(torch.uint8).view(-1, nkv * d).index_copy_(0, slots64, v8.view(torch.uint8))

    def one_write(i):
        _, k, v = parts(i)
        ops.reshape_paged_cache_kv8(slots, k.unflatten(-1, (nkv, d)), v.unflatten(-1, (nkv, d)), kc, vc, ks, vs)

    def seq_rope(i):
        q, k, _ = parts(i)
        ops.rotary_embedding(pos, q, k, cos_sin, True, head_size=d)
        seq_write(i)

    def one_rope(i):
        q, k, v = parts(i)
        ops.rotary_embedding_and_cache_kv8(pos, q, k, v, cos_sin, slots, kc, vc, ks, vs, d, True)

    rows = alternate([(f"T={T}: static_scaled_fp8_quant x 2 + scatter x 2", seq_write), (f"T={T}: reshape_paged_cache_kv8", one_write),
                      (f"T={T}: rotary_embedding + quant x 2 + scatter x 2", seq_rope),
                      (f"T={T}: rotary_embedding_and_cache_kv8", one_rope)])
    for name, med, spread in rows:
        print(f"  {name:<58} {med:9.1f} us  spread {spread:6.1f}", flush=True)


def layer_rows(B=256):
    args = layers.ModelArgs.qwen2_7b()
    nkv, d, H = args.n_kv_heads, args.head_dim, args.hidden_size
    dtype = torch.bfloat16
    c16, c8, blocks = make_caches(B, nkv, d)
    bi = attention.build_batch_input([S - 1] * B, [S] * B, blocks, bs)
    md = attention.build_attention_metadata(bi, False, False, dev)
    positions = bi.positions.to(torch.int64).to(dev)
    cos_sin = layers.build_cos_sin_cache(args, dtype, dev, 8192)
    lay = layers.Qwen2DecoderLayer(args, "int8", dtype, dev, torch.Generator(device=dev).manual_seed(3), None, True)
    x = torch.randn(B, H, device=dev).to(dtype)
    res = [torch.randn(B, H, device=dev).to(dtype) for _ in range(2)]
    nxt_w = (torch.rand(H, device=dev) + 0.5).to(dtype)
    h_in = ops.rms_norm_dynamic_int8_quant(x, lay.input_norm_w, args.rms_norm_eps)
    rows = alternate([
        ("decode layer, mode int8, bf16 KV cache", lambda i: lay.forward(None, res[0], positions, md, c16[i], cos_sin, h_in=h_in,
                                                                       next_norm_w=nxt_w)),
        ("decode layer, mode int8, e4m3 KV cache", lambda i: lay.forward(None, res[1], positions, md, c8[i], cos_sin, h_in=h_in,
                                                                        next_norm_w=nxt_w)),
    ])
    print(f"# one Qwen2-7B decode layer, B={B} ctx={S}, steady state (input pre-quantised by the predecessor, ends with the successor's norm)")
    for name, med, spread in rows:
        print(f"  {name:<58} {med:9.1f} us  spread {spread:6.1f}", flush=True)


def main():
    torch.manual_seed(0)
    print(f"# e4m3 KV cache decode, pages of {bs} in random placement, {NC} cache copies per graph, {ROUNDS} alternating rounds, window "
          f"{WINDOW} s, {torch.cuda.get_device_name(0)}")
    for B, nq, nkv in ((256, 28, 4), (64, 28, 4), (32, 28, 4), (128, 7, 1)):
        attention_rows(B, nq, nkv)
    print("# KV writers, 28 q / 4 kv heads of d = 128, packed qkv rows")
    for T in (256, 4096):
        writer_rows(T)
    layer_rows()


if __name__ == "__main__":
    main()
