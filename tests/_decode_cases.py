"""Case tables, poisoned inputs and a dense float64 reference for the paged decode attention tests
(tests/test_decode_reference.py on the CPU, tests/test_gpu_decode_plans.py on the GPU).

Every case names the launch plan it is meant to reach (xllm_amd/csrc/attention_api.hip: decode_heads_per_wg,
decode_num_splits, and the KROWS / UNIFORM template arms launch_paged_decode derives); the GPU tests assert that plan through
xllm_mi355_paged_decode_plan before they launch, so a planner change that moves a case elsewhere turns the test red instead of
silently shrinking its coverage."""
import collections

import torch

from oracle import oracle as orc

# ragged lengths around the 32-token tile and the 16 / 64 / 128-token pages: one key, one short of / on / one past a tile, two
# tiles +- 1, a full page of 128 +- 1, three pages
LENS = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257, 300]

Plan = collections.namedtuple("Plan", "name B nq nkv d bs hpw krows uniform nsplit")
# nsplit: what decode_num_splits gives at max_kv_len <= 300 (10 tiles < 8 * nsub for every hpw, so by_len = 1) without an override
PLANS = [
    Plan("hpw4_headline", 192, 28, 4, 128, 128, hpw=4, krows=0, uniform=1, nsplit=1),      # B*nkv/4 = 192 workgroups
    Plan("hpw4_krows_page16", 48, 32, 16, 128, 16, hpw=4, krows=1, uniform=0, nsplit=1),   # 48*16/4 = 192, 4 of 16 heads per wg
    Plan("hpw2_krows", 96, 28, 4, 128, 128, hpw=2, krows=1, uniform=1, nsplit=1),          # 96*4/4 < 192 <= 96*4/2
    Plan("hpw2_d64", 192, 14, 2, 64, 64, hpw=2, krows=0, uniform=1, nsplit=1),             # nkv = 2: both heads in the wg
    Plan("hpw4_d64_page16", 192, 16, 4, 64, 16, hpw=4, krows=0, uniform=0, nsplit=1),
    Plan("hpw1_control", 4, 28, 4, 128, 128, hpw=1, krows=1, uniform=1, nsplit=1),
]
PLAN = {p.name: p for p in PLANS}
WINDOW_PLANS = [PLANS[0], PLANS[1], PLANS[2], PLANS[-1]]
# split-KV under a window: 79 tiles, hpw = 1 (nsub = 4) -> by_len = 79 / 32 = 2 grid splits = 8 slots per (sequence, head)
SPLIT_PLAN = Plan("hpw1_split2", 3, 28, 4, 128, 128, hpw=1, krows=1, uniform=1, nsplit=2)
SPLIT_LENS = [2500, 1000, 130]
SPLIT_WINDOWS = [40, 100, 1030]      # 3, 5 and 34 live tiles of the longest row: slots without a tile, edge tile in the first live slot
DTYPES = [torch.bfloat16, torch.float16]

# window_left values of the window cases; each call mixes the lengths of window_lens() below. 2**40 is clamped to 0x3fffffff by
# the launcher and binds nowhere.
WINDOWS = [0, 5, 40, 100, 2 ** 40]
# lower bounds t_lo = L - 1 - W the lengths of a window call are built to hit: 0 (W = L - 1), 1 (W = L - 2), a 16-token page
# boundary in the middle of a tile (16, 48) and one past it, one key short of a tile boundary (31, 63, 95, 191), on it (32, 64,
# 96, 160); from 128 on whole pages of 128 lie below the window
T_LOS = [0, 1, 16, 17, 31, 32, 48, 63, 64, 95, 96, 160, 191]


def ragged_lens(B):
    """LENS (longest first, stride 5 so that a batch of 4 already mixes long and short rows) over B - 1 rows plus one empty row"""
    rev = LENS[::-1]
    zero_row = min(5, B - 1)
    return [0 if i == zero_row else rev[(5 * i) % len(rev)] for i in range(B)]


def window_len_list(W):
    """lengths for one window_left: L = 1, every T_LOS bound, two rows the window does not bind (L = W + 1 is t_lo = 0 already;
    L <= W), one empty row"""
    if W >= 2 ** 30:
        return list(LENS) + [0]
    ls = [1] + [W + 1 + t for t in T_LOS if W + 1 + t <= 300] + [max(1, W), max(1, W // 2), 0]
    return ls


def window_batches(plan, W):
    """the kv_lens of each call of a window case: one call when the batch holds the whole list (cycled over the batch), else
    as many batches of plan.B as the list needs (the hpw = 1 control has B = 4)"""
    ls = window_len_list(W)
    if plan.B >= len(ls):
        return [[ls[i % len(ls)] for i in range(plan.B)]]
    out = []
    for i in range(0, len(ls), plan.B):
        chunk = ls[i:i + plan.B]
        out.append(chunk + [ls[0]] * (plan.B - len(chunk)))
    return out


def t_lo_of(L, W):
    return max(0, L - 1 - W) if W >= 0 else 0


def poison(kc, vc, kv_lens, block_tables, spare, window_left):
    """everything the kernel may load but must not use becomes NaN (K) / Inf (V), in place:
      * the rows past kv_len of each sequence's last page;
      * with a binding window, the rows below t_lo = kv_len - 1 - window_left; the block-table entries of pages that lie WHOLLY
        below t_lo are pointed at a spare block (a freed page that was never written: still a valid id);
      * the spare blocks, and through them every padding entry of the table (never read: kv_lens decides)."""
    bs = kc.shape[1]
    nan, inf = float("nan"), float("inf")
    for s in spare:
        kc[s] = nan
        vc[s] = inf
    for b, L in enumerate(kv_lens):
        npg = (L + bs - 1) // bs
        block_tables[b, npg:] = spare[b % len(spare)]
        if L == 0:
            continue
        if L % bs:
            last = int(block_tables[b, npg - 1])
            kc[last, L % bs:] = nan
            vc[last, L % bs:] = inf
        t_lo = t_lo_of(L, window_left)
        for p in range((t_lo + bs - 1) // bs):
            blk = int(block_tables[b, p])
            n = min(bs, t_lo - p * bs)            # rows of this page below the window
            kc[blk, :n] = nan
            vc[blk, :n] = inf
            if n == bs:
                block_tables[b, p] = spare[(b + p) % len(spare)]


def make_case(plan, kv_lens, dtype, seed, window_left=-1):
    """seeded, poisoned inputs of one call (CPU tensors). Pages are shuffled as tests/test_gpu_parity.py::_paged_case does:
    a random permutation of sum(pages) + 3 block ids dealt out in order, the last 3 left spare."""
    B, nq, nkv, d, bs = plan.B, plan.nq, plan.nkv, plan.d, plan.bs
    assert len(kv_lens) == B
    g = torch.Generator().manual_seed(seed)
    pages = [(L + bs - 1) // bs for L in kv_lens]
    nb = sum(pages) + 3
    perm = torch.randperm(nb, generator=g).tolist()
    table = torch.zeros(B, max(1, max(pages)), dtype=torch.int32)
    used = 0
    for b, n in enumerate(pages):
        table[b, :n] = torch.tensor(perm[used:used + n], dtype=torch.int32)
        used += n
    spare = perm[used:]
    assert len(spare) == 3
    kc = torch.randn(nb, bs, nkv, d, generator=g).to(dtype)
    vc = torch.randn(nb, bs, nkv, d, generator=g).to(dtype)
    q = torch.randn(B, nq, d, generator=g).to(dtype)
    poison(kc, vc, kv_lens, table, spare, window_left)
    assert int(table.min()) >= 0 and int(table.max()) < nb
    return dict(plan=plan, q=q, kc=kc, vc=vc, kv_lens=torch.tensor(kv_lens, dtype=torch.int32), block_tables=table,
                cu_q=torch.arange(B + 1, dtype=torch.int32), scale=d ** -0.5, window_left=window_left,
                max_kv_len=max(kv_lens), dtype=dtype)


def dense_decode_ref64(q, kc, vc, kv_lens, block_tables, scale, window_left=-1):
    """Decode attention restated densely in float64: q [B, nq, d], caches [n_blocks, bs, nkv, d] -> [B, nq * d] float64.

    Per sequence: gather its ceil(L / bs) pages through the block table, keep the keys max(0, L - 1 - W) ... L - 1 when
    W = window_left >= 0 (all L keys when W < 0), one softmax over them and one PV product, query head h on kv head
    h // (nq / nkv). A row with L == 0 gives zeros. No tiles, no running maximum, nothing shared with oracle/xllm_oracle.c.

    Window convention: window_left counts the keys visible to the LEFT of the query's own position L - 1, so W = 0 leaves
    the newest key alone and W = L - 1 is the first value that binds nothing. That is what the reference passes down:
    layers/cuda/flashinfer_attention.cpp:97-102 hands FlashInfer `sliding_window - 1` as window_left (a sliding window of S
    tokens = the current one + S - 1 to its left), and layers/dcu/flash_attention.cpp:210,257 hands the flash kernel
    window_size_left (-1 = unbounded) with the same meaning."""
    B, nq, d = q.shape
    bs, nkv = kc.shape[1], kc.shape[2]
    G = nq // nkv
    out = torch.zeros(B, nq * d, dtype=torch.float64)
    for b in range(B):
        L = int(kv_lens[b])
        if L == 0:
            continue
        ids = block_tables[b, :(L + bs - 1) // bs].long()
        lo = t_lo_of(L, window_left)
        k = kc[ids].reshape(-1, nkv, d)[lo:L].double()
        v = vc[ids].reshape(-1, nkv, d)[lo:L].double()
        s = torch.einsum("hgd,thd->hgt", q[b].double().view(nkv, G, d), k) * scale
        p = torch.softmax(s, dim=-1)
        out[b] = torch.einsum("hgt,thd->hgd", p, v).reshape(-1)
    return out


_REFS = {}


def references(case, key):
    """(oracle output, float64 reference rounded to the case's dtype), computed once per key in a process and never modified"""
    if key not in _REFS:
        c = case
        o = orc.paged_attention(c["q"], c["kc"], c["vc"], c["cu_q"], c["kv_lens"], c["block_tables"], c["scale"],
                                window_left=c["window_left"])
        r = dense_decode_ref64(c["q"], c["kc"], c["vc"], c["kv_lens"], c["block_tables"], c["scale"],
                               c["window_left"]).to(c["dtype"])
        _REFS[key] = (o, r)
    return _REFS[key]


# ---- the cases, by id; seeds are fixed per id so that the CPU and the GPU file see the same bytes
def plan_case(plan, dtype):
    key = ("plan", plan.name, dtype)
    return key, make_case(plan, ragged_lens(plan.B), dtype, seed=1000 + PLANS.index(plan))


def window_cases(plan, W, dtype):
    out = []
    for i, lens in enumerate(window_batches(plan, W)):
        key = ("window", plan.name, W, i, dtype)
        out.append((key, make_case(plan, lens, dtype, seed=2000 + 10 * WINDOW_PLANS.index(plan) + i, window_left=W)))
    return out


def split_window_case(W, dtype):
    key = ("split", W, dtype)
    return key, make_case(SPLIT_PLAN, SPLIT_LENS, dtype, seed=3000, window_left=W)


INT8_WINDOWS = [-1, 40]


def int8_case(W, dtype):
    """headline plan; without a window the ragged lengths, with one the lengths of the W = 40 window case"""
    plan = PLANS[0]
    if W < 0:
        return plan_case(plan, dtype)
    return window_cases(plan, W, dtype)[0]


def all_cases():
    """(id, builder) of every case of the tables -- builders, not tensors: a case is up to 80 MB of cache"""
    out = []
    for dt in DTYPES:
        n = str(dt).split(".")[-1]
        for p in PLANS:
            out.append((f"plan-{p.name}-{n}", lambda p=p, dt=dt: [plan_case(p, dt)]))
        for p in WINDOW_PLANS:
            for W in WINDOWS:
                out.append((f"window-{p.name}-W{W}-{n}", lambda p=p, W=W, dt=dt: window_cases(p, W, dt)))
        for W in SPLIT_WINDOWS:
            out.append((f"split-W{W}-{n}", lambda W=W, dt=dt: [split_window_case(W, dt)]))
    return out


# ---- distances in the units of the bars of tests/test_gpu_parity.py::assert_attn_close
BAR_REL = {torch.bfloat16: 1e-3, torch.float16: 2e-4}


def distance(got, ref):
    """(relative L2 over the tensor, largest |got - ref| in units of 2 bf16 ulp of the row maximum): both <= 1 x bar is what
    assert_attn_close(got, ref, rel=bar) asserts"""
    got, ref = got.float().cpu(), ref.float().cpu()
    rel = float((got - ref).norm() / ref.norm().clamp_min(1e-30))
    scale = ref.abs().amax(-1, keepdim=True).clamp_min(1e-30)
    elem = float(((got - ref).abs() / (2 * 2.0 ** -8 * scale + 1e-30)).max())
    return rel, elem
