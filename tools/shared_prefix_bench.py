#!/usr/bin/env python3
"""ops.paged_attention_shared_prefix against ops.paged_attention on the same tensors, at the headline decode shape (bs 256, ctx
4096, nq 28 / nkv 4 / d 128, pages of 128 in random placement) with shared prefixes of 0, 512, 2048 and 3584 tokens in two
groupings: one group of 256, and 16 groups of 16.

Each operator is captured in a HIP graph of NC launches that rotate over NC KV-cache copies (each far larger than the Infinity
Cache, so every launch streams its private pages from HBM). After a warm-up the two graphs alternate in one process, ROUNDS times;
a timing is device events around enough replays for a window of WINDOW seconds. Per case: microseconds per launch of each
(median over the rounds, with the spread max - min of the rounds), the algorithmic bytes of each (K and V pages that have to be
read once, q and out), and the ratio. The record is profiles/shared_prefix_decode.txt."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xllm_amd import ops  # noqa: E402

dev = "cuda"
B, S, nq, nkv, d, bs = 256, 4096, 28, 4, 128, 128
NC = int(os.environ.get("SP_COPIES", "3"))
ROUNDS = int(os.environ.get("SP_ROUNDS", "5"))
WINDOW = float(os.environ.get("SP_WINDOW", "0.25"))
PREFIXES = [0, 512, 2048, 3584]
GROUPINGS = [("1x256", 256), ("16x16", 16)]
if len(sys.argv) > 1:                       # e.g. "2048" or "512,2048": a subset of the prefixes
    PREFIXES = [int(x) for x in sys.argv[1].split(",")]


def graph_of(fn):
    for i in range(NC):                     # eager once: sizes the workspace outside the capture
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


def main():
    torch.manual_seed(0)
    pages = S // bs
    nb = B * pages + 7
    caches = [(torch.randn(nb, bs, nkv, d, device=dev).bfloat16(), torch.randn(nb, bs, nkv, d, device=dev).bfloat16()) for _ in range(NC)]
    private = torch.randperm(nb, device=dev)[: B * pages].to(torch.int32).view(B, pages)
    kv_lens = torch.full((B,), S, dtype=torch.int32, device=dev)
    q = torch.randn(B, nq, d, device=dev).bfloat16()
    scale = d ** -0.5
    row = nkv * d * 2 * 2                   # K + V bytes of one token
    io = 2 * B * nq * d * 2                 # q + out
    print(f"# shared-prefix decode vs paged_attention: B={B} ctx={S} nq={nq} nkv={nkv} d={d} page={bs}, {NC} cache copies per graph, "
          f"{ROUNDS} alternating rounds, window {WINDOW} s, {torch.cuda.get_device_name(0)}")
    print(f"# {'prefix':>6} {'groups':>6} {'plan (rows, psplit, hpw, nsplit)':>32} | {'plain us':>9} {'spread':>7} {'MB':>7} | "
          f"{'shared us':>9} {'spread':>7} {'MB':>7} | {'ratio':>6} {'bytes ratio':>11} {'max |diff|':>10}")
    for prefix in PREFIXES:
        P = prefix // bs
        for gname, gsize in GROUPINGS:
            table = private.clone()
            for b0 in range(0, B, gsize):
                table[b0:b0 + gsize, :P] = table[b0, :P]
            n_groups = B // gsize
            cu = torch.arange(0, B + 1, gsize, dtype=torch.int32, device=dev)
            pre = torch.full((n_groups,), P, dtype=torch.int32, device=dev)
            plan = ops.shared_prefix_decode_plan(B, nq, nkv, bs, P, S)
            plain = lambda i: ops.paged_attention(q, caches[i][0], caches[i][1], None, kv_lens, table, 1, S, scale)
            shared = lambda i: ops.paged_attention_shared_prefix(q, caches[i][0], caches[i][1], kv_lens, table, cu, pre, S, P, scale)
            diff = float((plain(0).float() - shared(0).float()).abs().max())
            g_plain, g_shared = graph_of(plain), graph_of(shared)
            for g in (g_plain, g_shared):   # warm-up
                time_us(g, 20)
            reps_p = max(5, int(WINDOW * 1e6 / (time_us(g_plain, 10) * NC)))
            reps_s = max(5, int(WINDOW * 1e6 / (time_us(g_shared, 10) * NC)))
            tp, ts = [], []
            for _ in range(ROUNDS):
                tp.append(time_us(g_plain, reps_p))
                ts.append(time_us(g_shared, reps_s))
            mp, ms = statistics.median(tp), statistics.median(ts)
            bytes_plain = B * S * row + io
            bytes_shared = n_groups * P * bs * row + B * (S - P * bs) * row + io
            print(f"  {prefix:>6} {gname:>6} {str(plan):>32} | {mp:9.1f} {max(tp) - min(tp):7.1f} {bytes_plain / 1e6:7.0f} | "
                  f"{ms:9.1f} {max(ts) - min(ts):7.1f} {bytes_shared / 1e6:7.0f} | {ms / mp:6.3f} {bytes_shared / bytes_plain:11.3f} "
                  f"{diff:10.2e}", flush=True)
            del g_plain, g_shared


if __name__ == "__main__":
    main()
