"""Case tables, poisoned inputs and a dense float64 reference for the MLA attention tests
(tests/test_mla_reference.py on the CPU, tests/test_gpu_mla_arms.py on the GPU).

Every case names the launch arm and the split-KV count it is built for (xllm_amd/csrc/attention_mla.hip: mla_plan); the GPU
tests assert them through xllm_mi355_mla_plan before they launch, so a planner change that moves a case elsewhere turns the test
red instead of silently shrinking its coverage.

A call is a list of (q_len, kv_len) entries, one per sequence. Decode is the call whose q_len is 1 everywhere. The latent cache
is [n_blocks, page, 1, 576]; the value of a key is the first 512 dims of its own row."""
import collections
import math
import os

import torch

from oracle import oracle as orc

D, DV, TILE = 576, 512, 64
SCALE = 192 ** -0.5
LOG2E = 1.4426950408889634
DTYPES = [torch.bfloat16, torch.float16]
DTNAME = {torch.bfloat16: "bf16", torch.float16: "f16"}

ARM_STAGED, ARM_DMA, ARM_DMA_NT, ARM_SHARE_P1, ARM_SHARE_HILO = 0, 1, 2, 3, 4

# ragged decode lengths around the 64-key tile and the 16 / 32 / 64 / 128-token pages, an empty row among them; shuffled (fixed
# order) so that the longest row is not the last one
LENS = [0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 300]
LENS_SHUFFLED = [65, 192, 0, 300, 17, 128, 1, 191, 64, 15, 193, 129, 16, 63, 127]
assert sorted(LENS_SHUFFLED) == LENS and LENS_SHUFFLED[-1] != max(LENS)

Plan = collections.namedtuple("Plan", "name H bs arm nsplit")
# nsplit: max_kv_len = 300 is 5 tiles, tiles / 8 = 0 caps the count at 1 whatever the batch
DECODE_PLANS = [
    Plan("dma_nt", 16, 64, ARM_DMA_NT, 1),               # cfg4's arm
    Plan("dma_nt_page128", 16, 128, ARM_DMA_NT, 1),      # second tile of a page: t0 % block_size = 64
    Plan("dma_hb3", 40, 64, ARM_DMA, 1),                 # three head blocks, the last holds 8 live heads
    Plan("staged_page16", 16, 16, ARM_STAGED, 1),        # a tile spans four pages
    Plan("staged_page32_h5", 5, 32, ARM_STAGED, 1),      # 11 dead heads
]

# split-KV at the planner's own count: max_kv_len is passed as a BOUND of 2048 (what the shim passes: table width x page), 32
# tiles. B = 4: resident / (B * hblocks) = 256 / 4 = 64 (DMA), 512 / 4 = 128 (staged), 256 / 12 -> 22 (H = 40); tiles / 8 = 4
# caps all three at 4. At 4 splits the 1100-key row (18 tiles) has slices of 5, 5, 5, 3 tiles; the 300-key row (5 tiles) 2, 2, 1
# and none; the 65-key row (2 tiles) 1, 1 and two empty slices; the empty row only empty slices.
SPLIT_LENS = [1100, 300, 65, 0]
SPLIT_BOUND = 2048
SPLIT_PLANS = [
    Plan("split_dma_nt", 16, 64, ARM_DMA_NT, 4),
    Plan("split_staged_page16", 16, 16, ARM_STAGED, 4),
    Plan("split_dma_hb3", 40, 64, ARM_DMA, 4),           # merge indexing over head blocks
]

# ---- prefill calls
PER_TOKEN_CALL = [(1, 64), (3, 3), (5, 133), (2, 65), (17, 300), (4, 2)]     # (4, 2): two query rows that see no key
# the tile-sharing kernel takes four consecutive query tokens (flat index) per workgroup. Head of every sharing call:
#   (1,64) (1,1) (1,17) (2,65) (1,130)  q_len 1, 1, 2, 1 in a row behind a one-token sequence: group 0 holds FOUR sequences
#   (3,3) (5,133) (2,40)                groups over two and three sequences
#   (66,321)                            a chunk of a long sequence
#   (4,2)                               rows that see no key (kv_len < q_len)
#   (2,9)                               aligns the next chunk: its first token gets a flat index that is a multiple of 4
#   (70,132)                            q_kvlen 63 ... 132: groups at 63/64/65/66 and 127/128/129/130 (waves on both sides of a tile
#                                       edge, kv_w < kv_hi)
_SHARE_HEAD = [(1, 64), (1, 1), (1, 17), (2, 65), (1, 130), (3, 3), (5, 133), (2, 40), (66, 321), (4, 2), (2, 9), (70, 132)]
# H = 128: 8 head blocks; 158 + 8 = 166 tokens, 42 groups (166 % 4 = 2: a dead wave; 42 % 8 = 2: dead workgroups)
SHARE_H128_CALL = _SHARE_HEAD + [(8, 200)]
# H = 20: two head blocks, the second with 4 live heads; 1030 tokens, 258 groups (1030 % 4 = 2, 258 % 8 = 2), 516 live workgroups
SHARE_H20_CALL = _SHARE_HEAD + [(300, 300), (260, 330), (200, 231), (112, 120)]

# seeds: 4200 + index, except where that seed put a rounding flip of the ORACLE on a bf16 element of the top binade of its row (0.5
# ... 1.0 of the element-wise bar): tests/test_mla_reference.py wants the references alone inside half a bar. per_token_page16:
# 4201 gave 0.61; share_h128: the first seed of 4200 ... 4231 that keeps both its causal and its full case under a half (one of 32
# does); share_h20: none of 4200 ... 4231 does (0.60 ... 0.82), it keeps its index seed and is held to the whole bar there.
DECODE_SEED = {"dma_hb3": 4013}        # 4002 gave 0.59
PREFILL_SEED = {"per_token_page64": 4200, "per_token_page16": 4223, "share_h128": 4214, "share_h20": 4203}
PrefillCall = collections.namedtuple("PrefillCall", "name H bs entries arm nsplit")
PREFILL_CALLS = [
    PrefillCall("per_token_page64", 16, 64, PER_TOKEN_CALL, ARM_DMA, 1),      # 8 groups x 1 head block < 128; 5 tiles: 1 split
    PrefillCall("per_token_page16", 16, 16, PER_TOKEN_CALL, ARM_STAGED, 1),
    PrefillCall("share_h128", 128, 64, SHARE_H128_CALL, ARM_SHARE_P1, 1),
    PrefillCall("share_h20", 20, 64, SHARE_H20_CALL, ARM_SHARE_P1, 1),
]

# ---- rescale cases: flat scores (q and K scaled down: the log2-domain scores have a standard deviation of ~0.16) plus a LEVEL
# per key position, in log2 units, carried by one rope dim (SPIKE_DIM >= 512, so no value moves): q[..., SPIKE_DIM] = SPIKE_Q on
# every head, K[t, SPIKE_DIM] = level(t) / (SCALE * LOG2E * SPIKE_Q).
#   jump        one key (133, in the third tile) 10 above the flat scores: the tile maximum exceeds the running one by > 2^8
#   staircase   every key of tile j at 9.5 j: every tile more than 2^8 above the last
#   near_miss   the jump at 7: under 2^8, the lazy kernel never rescales and P reaches ~2^7
# A wrong rescale factor scales the part of the sum that lies in FRONT of the jump, so a row shows it only when it keeps mass
# there: jump / near_miss rows keep >= 0.05 in front of key 133; in the staircase a row of 64 j + 1 keys has one key on the top
# step and 64 one step (2^-9.5) below: ~0.08 in front of ITS last jump. The staircase lengths below give every jump (tiles 1 .. 4)
# such a witness row. tests/test_mla_reference.py checks all of this on the CPU.
SPIKE_DIM, SPIKE_Q, FLAT = 512 + 13, 4.0, 0.25
JUMP_KEY = 133
RESCALE_LEVELS = {
    "jump": lambda t: 10.0 if t == JUMP_KEY else 0.0,
    "staircase": lambda t: 9.5 * (t // TILE),
    "near_miss": lambda t: 7.0 if t == JUMP_KEY else 0.0,
}
RESCALE_DECODE_LENS = {"jump": [300, 134, 40, 192, 133], "near_miss": [300, 134, 40, 192, 133],
                       "staircase": [129, 300, 65, 257, 3, 193, 64]}
# tile-sharing family: H = 128, 80 tokens = 20 groups x 8 head blocks >= 128
RESCALE_SHARE_CALL = {"jump": [(66, 200), (6, 136), (8, 60)], "near_miss": [(66, 200), (6, 136), (8, 60)],
                      "staircase": [(68, 130), (8, 260), (4, 195)]}
RescaleFamily = collections.namedtuple("RescaleFamily", "name kind H bs arm")
RESCALE_FAMILIES = [RescaleFamily("dma_nt", "decode", 16, 64, ARM_DMA_NT),
                    RescaleFamily("staged_page16", "decode", 16, 16, ARM_STAGED),
                    RescaleFamily("share", "prefill", 128, 64, ARM_SHARE_P1)]


# The mask-edge cases (every decode plan, every causal prefill call) scale q by MASK_Q_FLAT: the natural-log scores then have a
# standard deviation of 1.73 / 8 = 0.22 and every key of a row holds between ~1/2 and ~2 times 1 / n of its mass ON EVERY HEAD.
# With unit-size q a key three deviations down holds e^-5 of the average and a mask that is off by that key moves its head's row
# by 3e-5: invisible to any bar. With flat scores a mask edge that is off by one key moves every (query, head) row it touches by
# ~0.5 / sqrt(n) >= 0.028 at n <= 330, past the loosest row bar (tests/test_mla_reference.py asserts it). The split-KV and
# non-causal cases keep unit-size q (score deviation 1.73, a running maximum that moves), the rescale cases have their levels.
MASK_Q_FLAT = 0.125


def n_tokens(entries):
    return sum(q for q, _ in entries)


def q_kvlens(entries, causal=True, causal_shift=0, kv_shift=0):
    """per query token (flat): (sequence, visible key count), bottom-right aligned as mla_expand_queries_kernel writes them"""
    out = []
    for b, (ql, kl) in enumerate(entries):
        kl = max(0, kl + kv_shift)
        for i in range(ql):
            n = kl - (ql - 1 - i) + causal_shift if causal else kl
            out.append((b, min(kl, max(0, n))))
    return out


def group_profile(entries):
    """what the four-token groups of a causal call look like: {distinct sequences per group}, the q_kvlen tuples of the groups"""
    qk = q_kvlens(entries)
    groups = [qk[i:i + 4] for i in range(0, len(qk), 4)]
    return {len({s for s, _ in g}) for g in groups}, [tuple(n for _, n in g) for g in groups if len({s for s, _ in g}) == 1]


def make_case(name, H, bs, entries, dtype, seed, arm, nsplit, causal=True, bound=None, levels=None, poisoned=True, q_flat=1.0):
    """seeded, poisoned inputs of one call (CPU tensors). Pages are dealt from a random permutation of sum(pages) + 3 block ids,
    the last three stay spare. Everything the call may load but must not use is NaN: the rows past kv_len of each last page, the
    spare blocks, and -- through them -- every padding entry of the block table (all table entries stay valid block ids; a row
    with kv_len = 0 gets a table row of spare ids). bound: the max_kv_len the call passes (an upper bound; the table is as wide
    as it takes). q_flat scales q alone (the values keep unit size): see MASK_Q_FLAT."""
    g = torch.Generator().manual_seed(seed)
    kv_lens = [k for _, k in entries]
    B, T = len(entries), n_tokens(entries)
    max_kv = bound if bound is not None else max(kv_lens)
    pages = [(L + bs - 1) // bs for L in kv_lens]
    nb = sum(pages) + 3
    perm = torch.randperm(nb, generator=g).tolist()
    spare = perm[sum(pages):]
    width = max(1, (max_kv + bs - 1) // bs)
    table = torch.tensor([[spare[(b + j) % 3] for j in range(width)] for b in range(B)], dtype=torch.int32)
    used = 0
    for b, n in enumerate(pages):
        table[b, :n] = torch.tensor(perm[used:used + n], dtype=torch.int32)
        used += n
    flat = FLAT if levels is not None else 1.0
    kc = (torch.randn(nb, bs, 1, D, generator=g) * flat).to(dtype)
    q = (torch.randn(T, H, D, generator=g) * flat * q_flat).to(dtype)
    if levels is not None:
        q[..., SPIKE_DIM] = SPIKE_Q
        for b, L in enumerate(kv_lens):
            for t in range(L):
                kc[int(table[b, t // bs]), t % bs, 0, SPIKE_DIM] = levels(t) / (SCALE * LOG2E * SPIKE_Q)
    if poisoned:
        nan = float("nan")
        for s in spare:
            kc[s] = nan
        for b, L in enumerate(kv_lens):
            if L % bs:
                kc[int(table[b, pages[b] - 1]), L % bs:] = nan
    assert int(table.min()) >= 0 and int(table.max()) < nb
    cu_q = torch.tensor([0] + torch.tensor([ql for ql, _ in entries]).cumsum(0).tolist(), dtype=torch.int32)
    return dict(name=name, H=H, bs=bs, entries=list(entries), dtype=dtype, causal=causal, q=q, kc=kc,
                kv_lens=torch.tensor(kv_lens, dtype=torch.int32), cu_q=cu_q, block_tables=table, scale=SCALE,
                max_kv_len=max_kv, arm=arm, nsplit=nsplit, decode=all(ql == 1 for ql, _ in entries), key=(name, causal, dtype))


def scores64(case, b):
    """float64 log2-domain scores [q_len, H, kv_len] and the gathered latent rows [kv_len, 576] of sequence b"""
    ql, L = case["entries"][b]
    bs = case["bs"]
    ids = case["block_tables"][b, :(L + bs - 1) // bs].long()
    k = case["kc"][ids].reshape(-1, D)[:L].double()
    q0 = int(case["cu_q"][b])
    s = torch.einsum("qhd,td->qht", case["q"][q0:q0 + ql].double(), k) * (case["scale"] * LOG2E)
    return s, k


def dense_ref64(case, causal_shift=0, kv_shift=0):
    """MLA attention restated densely in float64: [T, H * 512]. Per sequence: gather the latent rows through the block table;
    query i of q_len sees the keys 0 ... kv_len - (q_len - 1 - i) - 1 under the bottom-right causal mask (all kv_len keys when
    the call is not causal); out = softmax(scale q K^T) @ K[:, :512]. A row with no visible key is exact zero. No tiles, no
    running maximum, nothing shared with oracle/xllm_oracle.c. causal_shift / kv_shift move that edge / kv_len by whole keys
    (the sensitivity test; kv_shift > 0 needs an unpoisoned case)."""
    T, H = case["q"].shape[0], case["H"]
    out = torch.zeros(T, H * DV, dtype=torch.float64)
    vis = q_kvlens(case["entries"], case["causal"], causal_shift, kv_shift)
    bs = case["bs"]
    for b, (ql, L0) in enumerate(case["entries"]):
        L = max(0, L0 + kv_shift)
        if L == 0:
            continue
        assert L <= ((L0 + bs - 1) // bs) * bs
        ids = case["block_tables"][b, :(L + bs - 1) // bs].long()
        k = case["kc"][ids].reshape(-1, D)[:L].double()
        q0 = int(case["cu_q"][b])
        s = torch.einsum("qhd,td->qht", case["q"][q0:q0 + ql].double(), k) * case["scale"]
        n = torch.tensor([vis[q0 + i][1] for i in range(ql)])
        mask = torch.arange(L)[None, :] < n[:, None]                                   # [ql, L]
        s = s.masked_fill(~mask[:, None, :], float("-inf"))
        p = torch.softmax(s, dim=-1)
        p = torch.where(mask[:, None, :], p, torch.zeros_like(p))                      # rows without a key: softmax gave NaN
        o = torch.einsum("qht,tv->qhv", p, k[:, :DV])
        out[q0:q0 + ql] = o.reshape(ql, -1)
    return out


class _Refs(dict):
    """the references of one case, each computed on first use and never modified:
    r64 float64; r64r float64 rounded once to the dtype; fp32 the oracle with fp32 P; p16 / flash the oracle with one 16-bit P per
    score (normalised P rounded / a flash kernel's tile P rounded), for calls that can take the tile-sharing arm"""

    def __init__(self, case):
        super().__init__()
        self.case = case

    def __missing__(self, name):
        c = self.case
        if name == "r64":
            v = dense_ref64(c)
        elif name == "r64r":
            v = self["r64"].to(c["dtype"])
        else:
            mode = {"fp32": False, "p16": True, "flash": "flash"}[name]
            v = orc.paged_attention(c["q"], c["kc"], c["kc"], c["cu_q"], c["kv_lens"], c["block_tables"], c["scale"],
                                    causal=c["causal"] and not c["decode"], dv=DV, p_round=mode)
        self[name] = v
        return v


_REFS = {}


def references(case):
    """the _Refs of a case, one per case key in a process"""
    if case["key"] not in _REFS:
        _REFS[case["key"]] = _Refs(case)
    return _REFS[case["key"]]


def can_share(case):
    return not case["decode"] and case["bs"] % TILE == 0


def seq_slices(case):
    return [slice(int(case["cu_q"][b]), int(case["cu_q"][b + 1])) for b in range(len(case["entries"]))]


def zero_rows(case):
    """bool [T]: query rows that see no key (kv_len = 0, or kv_len < q_len under the causal mask)"""
    return torch.tensor([n == 0 for _, n in q_kvlens(case["entries"], case["causal"])])


# ---- the cases by id; seeds are fixed per id so that the CPU and the GPU file see the same bytes
def _dec(lens):
    return [(1, L) for L in lens]


def decode_case(plan, dtype, poisoned=True):
    seed = DECODE_SEED.get(plan.name, 4000 + DECODE_PLANS.index(plan))
    return make_case(plan.name, plan.H, plan.bs, _dec(LENS_SHUFFLED), dtype, seed, plan.arm, plan.nsplit, poisoned=poisoned, q_flat=MASK_Q_FLAT)


def split_case(plan, dtype):
    return make_case(plan.name, plan.H, plan.bs, _dec(SPLIT_LENS), dtype, 4100 + SPLIT_PLANS.index(plan), plan.arm, plan.nsplit,
                     bound=SPLIT_BOUND)


def prefill_case(call, causal, dtype, poisoned=True):
    return make_case(call.name, call.H, call.bs, call.entries, dtype, PREFILL_SEED[call.name], call.arm, call.nsplit,
                     causal=causal, poisoned=poisoned, q_flat=MASK_Q_FLAT if causal else 1.0)


def last_row_decode_case(call, dtype):
    """the decode call over the cache of a per-token prefill case: the last query row of every sequence"""
    c = prefill_case(call, True, dtype)
    d = dict(c)
    d.update(q=c["q"][c["cu_q"][1:].long() - 1].contiguous(), entries=_dec([k for _, k in c["entries"]]), decode=True,
             cu_q=torch.arange(len(c["entries"]) + 1, dtype=torch.int32), name=c["name"] + "_last_rows",
             arm=ARM_DMA_NT if c["bs"] % TILE == 0 else ARM_STAGED, key=(c["name"] + "_last_rows", True, dtype))
    return c, d


def rescale_case(fam, kind, dtype):
    entries = _dec(RESCALE_DECODE_LENS[kind]) if fam.kind == "decode" else RESCALE_SHARE_CALL[kind]
    # (the decode families' base: 4300 put an oracle rounding flip at 0.53 of the element-wise bar; see PREFILL_SEED)
    # the tile-sharing jump case: 4324 is the one seed of 4320 ... 4331 under a half; for its near_miss and staircase cases none
    # of 52 seeds each is (0.56 ... 0.92): they keep their index seeds and are held to the whole bar
    seed = (4600 if fam.kind == "decode" else 4300) + 10 * RESCALE_FAMILIES.index(fam) + sorted(RESCALE_LEVELS).index(kind)
    seed = 4324 if (fam.name, kind) == ("share", "jump") else seed
    return make_case(f"rescale_{fam.name}_{kind}", fam.H, fam.bs, entries, dtype, seed, fam.arm, 1, levels=RESCALE_LEVELS[kind])


def all_cases():
    """(id, builder) of every case of the tables -- builders, not tensors"""
    out = []
    for dt in DTYPES:
        n = DTNAME[dt]
        for p in DECODE_PLANS:
            out.append((f"decode-{p.name}-{n}", "mask", lambda p=p, dt=dt: decode_case(p, dt)))
        for p in SPLIT_PLANS:
            out.append((f"{p.name}-{n}", "split", lambda p=p, dt=dt: split_case(p, dt)))
        for c in PREFILL_CALLS:
            for causal in (True, False):
                if not causal and c.name == "share_h20":       # one non-causal call per arm: share_h128 is arm 3's (T < 256)
                    continue
                out.append((f"prefill-{c.name}-{'causal' if causal else 'full'}-{n}", "mask" if causal else "full",
                            lambda c=c, causal=causal, dt=dt: prefill_case(c, causal, dt)))
        for f in RESCALE_FAMILIES:
            for k in sorted(RESCALE_LEVELS):
                out.append((f"rescale-{f.name}-{k}-{n}", "rescale", lambda f=f, k=k, dt=dt: rescale_case(f, k, dt)))
    return out


# ---- the plan query (the library loads without a GPU)
def library():
    """the kernel library; raises when it is not built (the CPU tests skip on their own, the GPU tests must not)"""
    from xllm_amd import _lib
    return _lib.lib()


def query_plan(case, ws_bytes):
    """(arm, nsplit) xllm_mi355_mla_plan reports for the call of a case with a workspace of ws_bytes"""
    import ctypes as C
    arm, ns = C.c_int32(-1), C.c_int32(-1)
    T = 0 if case["decode"] else case["q"].shape[0]
    rc = library().xllm_mi355_mla_plan(len(case["entries"]), T, case["H"], case["bs"], case["max_kv_len"], ws_bytes,
                                       C.addressof(arm), C.addressof(ns))
    assert rc == 0, rc
    return arm.value, ns.value


def ops_workspace(case):
    """(bytes, splits it holds) of the workspace ops.mla_decode / ops.mla_prefill pass"""
    T, H = case["q"].shape[0], case["H"]
    if case["decode"]:
        return 32 * per_split_bytes(T, H), 32
    return ((T * 8 + 255) // 256) * 256 + 8 * per_split_bytes(T, H), 8


# ---- the plan a call must take under the switches of the environment
def _switch(name):
    v = os.environ.get(name)
    return None if v is None else int(v)


def natural_nsplit(entries, H, bs, max_kv_len):
    """mla_plan_entries restated: what the planner picks before any override and before the workspace"""
    hblocks, tiles = (H + 15) // 16, (max_kv_len + TILE - 1) // TILE
    resident = 256 if bs % TILE == 0 else 512
    return max(1, min((resident + entries * hblocks - 1) // (entries * hblocks), tiles // 8, 32))


def per_split_bytes(entries, H):
    return entries * H * (DV + 2) * 4


def expected_plan(case, ws_splits):
    """(arm, nsplit) the query must report for a case whose workspace holds ws_splits splits. With no MLA switch in the
    environment that is the TABLE's entry (cut down to the workspace); XLLM_MI355_MLA_SPLITS = n gives min(n, 32, workspace);
    XLLM_MI355_MLA_PREFILL / _PREFILL_P move a prefill call between the tile-sharing arms and the per-token form."""
    splits, share, pmode = _switch("XLLM_MI355_MLA_SPLITS"), _switch("XLLM_MI355_MLA_PREFILL"), _switch("XLLM_MI355_MLA_PREFILL_P")
    T, H, bs = case["q"].shape[0], case["H"], case["bs"]
    arm, nsplit = case["arm"], case["nsplit"]
    if not case["decode"]:
        natural = ((T + 3) // 4) * ((H + 15) // 16) >= 128
        assert natural == (arm in (ARM_SHARE_P1, ARM_SHARE_HILO)) or bs % TILE
        shared = bs % TILE == 0 and share != 0 and (share == 1 or natural)
        if shared:
            return (ARM_SHARE_HILO if pmode == 2 else ARM_SHARE_P1), 1
        if arm in (ARM_SHARE_P1, ARM_SHARE_HILO):         # a sharing call forced onto the per-token form
            arm, nsplit = ARM_DMA, natural_nsplit(T, H, bs, case["max_kv_len"])
    if splits is not None and splits > 0:
        nsplit = min(splits, 32)
    return arm, max(1, min(nsplit, ws_splits))


# ---- distances in the units of the bars
BAR_REL = {torch.bfloat16: 1e-3, torch.float16: 2e-4}     # assert_attn_close's rel, as tests/_decode_cases.py
FLASH_BAR = 1e-3


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def distance(got, ref):
    """(relative L2 over the tensor, largest |got - ref| in units of 2 bf16 ulp of the row maximum): both <= 1 x bar is what
    assert_attn_close(got, ref, rel=bar) asserts"""
    got, ref = got.float().cpu(), ref.float().cpu()
    rel = float((got - ref).norm() / ref.norm().clamp_min(1e-30))
    scale = ref.abs().amax(-1, keepdim=True).clamp_min(1e-30)
    elem = float(((got - ref).abs() / (2 * 2.0 ** -8 * scale + 1e-30)).max())
    return rel, elem


def row_distances(got, ref, H):
    """per (query, head) relative L2 distance [T, H]; NaN where the reference row is zero (checked for exact zeros instead)"""
    T = ref.shape[0]
    g, r = got.double().cpu().reshape(T, H, -1), ref.double().cpu().reshape(T, H, -1)
    n = r.norm(dim=-1)
    return torch.where(n > 0, (g - r).norm(dim=-1) / n.clamp_min(1e-300), torch.full_like(n, float("nan")))


def nanmax(x):
    x = x[~torch.isnan(x)]
    return float(x.max()) if x.numel() else 0.0


# Per (query, head) row: the ORACLE's own largest distance from float64 over every case of the tables, in the mode that has the
# kernel's P form ("hilo": fp32 P, every case; "p16": p_round=True, the calls that can take the tile-sharing arm). The GPU bar is
# twice that. tests/test_mla_reference.py re-measures and fails when a table change moves the oracle past ROW_MEASURED.
ROW_MEASURED = {("hilo", torch.bfloat16): 1.02e-3, ("hilo", torch.float16): 1.75e-4,
                ("p16", torch.bfloat16): 4.86e-3, ("p16", torch.float16): 6.10e-4}
ROW_BAR = {k: 2.0 * v for k, v in ROW_MEASURED.items()}


def check_output(case, out, arm, note=None):
    """every bar of the GPU tests on one output [T, H * 512] (a CPU or GPU tensor of the case's dtype), for the arm the call took.
    note(label, value, case name) collects the distances as fractions of their bars."""
    from _bars import assert_attn_close, assert_p16_attention_close
    c, r, dt, H = case, references(case), case["dtype"], case["H"]
    out = out.cpu().reshape(out.shape[0], -1)
    note = note or (lambda *a: None)
    assert torch.isfinite(out.float()).all(), f"{c['name']}: non-finite output"
    zr = zero_rows(c)
    assert not out[zr].float().abs().any(), f"{c['name']}: a row without a visible key is not exact zero"
    form = "p16" if arm == ARM_SHARE_P1 else "hilo"
    for b, sl in enumerate(seq_slices(c)):
        if bool(zr[sl].all()):
            continue
        if form == "hilo":
            for refname in ("fp32", "r64r"):
                rel, elem = distance(out[sl], r[refname][sl])
                note((form, refname, "rel"), rel / BAR_REL[dt], c["name"])
                note((form, refname, "elem"), elem, c["name"])
                assert_attn_close(out[sl], r[refname][sl], rel=BAR_REL[dt])
        else:
            e_ref = rel_l2(r["p16"][sl], r["r64r"][sl])
            note((form, "r64r", "rel"), rel_l2(out[sl], r["r64r"][sl]) / max(1e-3, 1.25 * e_ref), c["name"])
            note((form, "p16", "rel"), rel_l2(out[sl], r["p16"][sl]) / max(1e-3, 2.0 * e_ref), c["name"])
            note((form, "flash", "rel"), rel_l2(out[sl], r["flash"][sl]) / FLASH_BAR, c["name"])
            assert_p16_attention_close(out[sl], r["r64r"][sl], r["p16"][sl], r["flash"][sl])
    worst = nanmax(row_distances(out, r["r64r"], H))
    note((form, "r64r", "row"), worst / ROW_BAR[(form, dt)], c["name"])
    assert worst <= ROW_BAR[(form, dt)], f"{c['name']}: row distance {worst:.3e} > {ROW_BAR[(form, dt)]:.3e}"


# ---- the mass condition of the rescale cases
def jump_profile(case, thresh=8.0):
    """per (sequence b, query row i): (jump tiles, least softmax mass over the heads in front of the LAST jump's tile, largest
    excess of a tile maximum over the lazy kernel's reference maximum). A tile is a jump when its maximum exceeds the running
    maximum of the tiles before it by more than thresh (log2 domain): the eager kernels rescale there by less than 2^-thresh, the
    lazy one (whose reference maximum never lies above the running one) rescales there too when thresh >= 8. The lazy reference
    maximum follows mla_prefill_dma_kernel's rule: it moves only when a tile exceeds it by more than 8."""
    out = {}
    vis = q_kvlens(case["entries"], case["causal"])
    for b, (ql, L) in enumerate(case["entries"]):
        if L == 0:
            continue
        s, _ = scores64(case, b)
        q0 = int(case["cu_q"][b])
        for i in range(ql):
            n = vis[q0 + i][1]
            if n == 0:
                continue
            si = s[i, :, :n]                                                      # [H, n]
            p = torch.softmax(si * math.log(2.0), dim=-1)
            run = si[:, :TILE].amax(-1)
            lazy = run.clone()
            jumps, front, excess = [], 1.0, 0.0
            for t in range(1, (n + TILE - 1) // TILE):
                tm = si[:, t * TILE:(t + 1) * TILE].amax(-1)
                is_jump = tm > run + thresh
                if bool(is_jump.any()):
                    assert bool(is_jump.all()), "the levels are the same on every head"
                    jumps.append(t)
                    front = float(p[:, :t * TILE].sum(-1).min())
                excess = max(excess, float((tm - lazy).max()))
                lazy = torch.where(tm > lazy + 8.0, tm, lazy)
                run = torch.maximum(run, tm)
            out[(b, i)] = (jumps, front, excess)
    return out
