"""Case tables, poisoned inputs and a dense float64 reference for the prefill / chunked-prefill attention tests
(tests/test_prefill_reference.py on the CPU, tests/test_gpu_prefill_masks.py on the GPU).

Every case names the kernel arm it is built for. The arm is restated here from the dispatch in
xllm_amd/csrc/attention_prefill.hip::launch_flash_prefill (see arm_of below); the GPU tests check it by numerics: an arm with
ONE 16-bit P per score is held to the oracle's "flash" cast-point mode, an arm with P = hi + lo to the fp32-P oracle, and on
bf16 rows of a hundred keys the two are ~2.5e-3 apart, so a case that the dispatcher moved to another arm goes red.

Geometry the tables are built around: K tiles are 64 keys on the m32 (LDS-DMA) kernel and 32 keys on the register-staged
kernel; a wave owns 32 queries, a workgroup (q block) 128; pf_block_coords maps blocks to (head, sequence, q block) in three
forms by P = sequences x kv heads (P >= 8, P dividing 8, neither)."""
import collections
import os

import torch

from oracle import oracle as orc

Arm = collections.namedtuple("Arm", "name d paged bs")
# launch_flash_prefill: D = 128 goes to flash_prefill_m32_kernel when the K/V rows are unpaged or the page size is a multiple
# of the 64-key tile, and 64 row pitches fit a 32-bit buffer offset (pitch < 2^24 elements); everything else -- D = 64, pages of
# 16 tokens, pitches from 2^24 elements on -- goes to the register-staged flash_prefill_kernel<T, D, PAGED>
ARMS = [
    Arm("m32_unpaged", 128, False, 0),
    Arm("m32_paged", 128, True, 64),
    Arm("staged_paged_d128", 128, True, 16),
    Arm("staged_d64_unpaged", 64, False, 0),
    Arm("staged_d64_paged", 64, True, 16),
]
ARM = {a.name: a for a in ARMS}
WIDE_ARM = Arm("staged_wide_pitch", 128, False, 0)
M32_ARMS = [ARMS[0], ARMS[1]]
STAGED_CONTROL = ARMS[2]
WIDE_PITCH = 1 << 24
DTYPES = [torch.bfloat16, torch.float16]
DTNAME = {torch.bfloat16: "bf16", torch.float16: "f16"}


def arm_of(d, paged, bs, pitch):
    """the arm launch_flash_prefill picks (pitch: K / V row pitch in elements; paged caches have pitch nkv * d)"""
    if d == 128 and (not paged or bs % 64 == 0) and pitch * 2 * 64 < (1 << 31):
        return "m32_paged" if paged else "m32_unpaged"
    if d == 128:
        return "staged_paged_d128" if paged else "staged_wide_pitch"
    return "staged_d64_paged" if paged else "staged_d64_unpaged"


def p_form(arm):
    """"p16": one RNE-rounded 16-bit P per score in front of PV (the m32 arms by default); "hilo": P = hi + lo, fp32-P accuracy
    (the register-staged kernel always, the m32 arms under XLLM_MI355_PREFILL_P=2)"""
    if arm.name.startswith("m32") and os.environ.get("XLLM_MI355_PREFILL_P") != "2":
        return "p16"
    return "hilo"


# ---- the mask-edge tables ------------------------------------------------------------------------------------------------
# window_left values; 2**40 is clamped to 0x3fffffff by the launcher and binds nowhere, -1 is "no window"
WINDOWS = [-1, 0, 1, 31, 32, 63, 64, 65, 100, 2 ** 40]
# (causal, W) of the calls of one arm: every W under the causal mask, three without it (the window then also shows the future)
MASKS = [(1, W) for W in WINDOWS] + [(0, -1), (0, 32), (0, 65)]
# nq, nkv: G = nq / nkv in {2, 1, 7}, cycled over the calls of an arm
HEADS = [(4, 2), (2, 2), (7, 1)]
# (q_len, kv_len) of every mask-edge call. q_len: 1, 31, 32, 33, 64, 65, 127, 128, 129, 257 (one short of / on / one past a
# wave, a q block, two q blocks) and one EMPTY sequence in the middle; kvoff = kv_len - q_len: 63, 0, 31, 1, 64, 64, 0, 0, 200,
# 65; kv_len on and either side of a tile edge (63 / 64 / 65, 127 / 128 / 129 -- 64 and 128 are page edges of the 16- and
# 64-token pages as well)
SEQS = [(1, 64), (31, 31), (32, 63), (64, 65), (33, 97), (0, 40), (65, 129), (127, 127), (128, 128), (129, 329), (257, 322)]
# unpaged arms only: kv_len < q_len (the first q_len - kv_len rows see nothing under the causal mask and are zeros), by 10 and
# by 1, next to a plain sequence
SEQS_SHORT_KV = [(40, 30), (70, 70), (20, 19)]
PAD_MAX_Q = 257 + 200        # one call per arm passes this max_q_len: padding q blocks behind the longest sequence

# pf_block_coords forms on the m32 arms, together with a window: (sequences, nq, nkv) -> P = 1, 2, 3, 4, 8, 10
PFORMS = [(1, 7, 1), (1, 4, 2), (3, 2, 1), (2, 4, 2), (4, 4, 2), (5, 4, 2)]
PFORM_SEQS = [(257, 322), (129, 329), (65, 129), (33, 97), (128, 128)]
PFORM_W = 63

# ---- poison table: (q_len, kv_len) per call and W. kv_len - q_len - W is the lowest window bound of a sequence; with 16-token
# pages and the 32-key tile of the staged kernel (bound mod 32) >= 16 puts a poisoned spare page into the edge tile:
# 300 - 44 - 100 = 156 = 4 * 32 + 28, 329 - 129 - 100 = 100 = 3 * 32 + 4 (control: the edge tile starts on a live page),
# 257 - 33 - 100 = 124 = 3 * 32 + 28, 130 - 5 - 100 = 25 (no whole page of 64 below, one of 16)
POISON_SEQS = [(44, 300), (129, 329), (33, 257), (5, 130), (0, 77), (64, 65)]
POISON_MASKS = [(1, 100), (1, -1), (0, 31)]

# ---- rescale table: q[..., 0] = A for every query, chosen keys are B * e_0, so their scaled score is A * B * scale exactly and
# every other key's stays ~N(0, 0.15): the size of a jump of the running maximum is set in log2 units
RESCALE_A = 1.0
RESCALE_SEQS = [(330, 330), (100, 260)]      # second sequence: kvoff = 160, key 208 is seen from query 48 on (middle of wave 1)
RESCALE = {
    # key index -> level in log2 units above the flat keys. 208 = tile 3 of the m32 kernel (two tiles accumulated before it),
    # in the middle of the wave that owns queries 192 ... 223
    "jump": {208: 11.0},
    "near_miss": {208: 7.2},                  # below the 2^8 threshold: no rescale on m32, P up to ~2^7
    # tiles 2, 3, 4 of the m32 kernel: three successive rescales of 9.4 / 9.2 / 9.2 units. Forty keys on each of the first two
    # levels, one on the third: under the causal mask the row AT a level's first key sees none of that level's other keys, and
    # the forty keys of the level below keep 40 / (40 + 2^9.2) = 0.064 of its mass in front of the jump
    "staircase": {**{j: 10.4 for j in range(144, 184)}, **{j: 19.6 for j in range(208, 248)}, 272: 28.8},
}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _paged_layout(arm, seqs, nkv, g, poison_window, W):
    """shuffled pages + 3 spare ones; returns (n_blocks, table, spare, dead): dead = the pages no live token maps to any more.
    Table entries past ceil(kv_len / bs) and -- with
    poison_window -- of pages wholly below max(0, kv_len - q_len - W) point at a spare page (valid id, poisoned content)"""
    bs = arm.bs
    pages = [(kv + bs - 1) // bs for _, kv in seqs]
    nb = sum(pages) + 3
    perm = torch.randperm(nb, generator=g).tolist()
    table = torch.zeros(len(seqs), max(pages) + 1, dtype=torch.int32)
    spare = perm[sum(pages):]
    used = 0
    dead = []                                  # pages no live token maps to
    for b, ((ql, kv), n) in enumerate(zip(seqs, pages)):
        table[b, :n] = torch.tensor(perm[used:used + n], dtype=torch.int32)
        table[b, n:] = spare[b % 3]
        if poison_window and W >= 0:
            lo = max(0, kv - ql - W)
            for p in range(lo // bs):
                dead.append(int(table[b, p]))
                table[b, p] = spare[(b + p) % 3]
        used += n
    return nb, table, spare, dead


def build_case(arm, dtype, seqs, causal, W, nq, nkv, seed, poison_window=False, max_q_len=None, spikes=None, neighbour=False,
               layout="packed"):
    """seeded inputs of one call (CPU tensors, compact). Flat inputs: q = randn / 8, k and v randn, so that every visible key
    carries comparable weight. Always poisoned (K = NaN, V = Inf): the rows past kv_len of a sequence's last page, spare pages,
    padding table entries; unpaged, 64 rows behind cu_k[-1]. poison_window adds the pages wholly below the sequence's lowest
    window bound; neighbour makes the whole second sequence's K / V poison (only the first one is asserted)."""
    d = arm.d
    g = _gen(seed)
    nan, inf = float("nan"), float("inf")
    Tq = sum(ql for ql, _ in seqs)
    q = torch.randn(Tq, nq, d, generator=g) / 8
    cu_q = torch.tensor([0] + torch.tensor([ql for ql, _ in seqs]).cumsum(0).tolist(), dtype=torch.int32)
    kv_lens = torch.tensor([kv for _, kv in seqs], dtype=torch.int32)
    c = dict(arm=arm, dtype=dtype, seqs=list(seqs), causal=int(causal), window_left=W, nq=nq, nkv=nkv, scale=d ** -0.5,
             cu_q=cu_q, kv_lens=kv_lens, max_q_len=max_q_len or max(ql for ql, _ in seqs), max_kv_len=max(kv for _, kv in seqs),
             layout=layout, assert_seqs=[b for b, (ql, _) in enumerate(seqs) if ql > 0])
    if spikes:
        q[:, :, 0] = RESCALE_A
    if arm.paged:
        bs = arm.bs
        nb, table, spare, dead = _paged_layout(arm, seqs, nkv, g, poison_window, W)
        kc = torch.randn(nb, bs, nkv, d, generator=g)
        vc = torch.randn(nb, bs, nkv, d, generator=g)
        for b, (_, kv) in enumerate(seqs):
            for j, level in (spikes or {}).items():
                if j < kv:
                    kc[int(table[b, j // bs]), j % bs] = 0.0
                    kc[int(table[b, j // bs]), j % bs, :, 0] = level / (RESCALE_A * c["scale"] * 1.4426950408889634)
            if kv % bs:
                last = int(table[b, (kv - 1) // bs])
                kc[last, kv % bs:] = nan
                vc[last, kv % bs:] = inf
        for s in spare + dead:
            kc[s] = nan
            vc[s] = inf
        assert int(table.min()) >= 0 and int(table.max()) < nb
        c.update(kc=kc.to(dtype), vc=vc.to(dtype), block_tables=table)
    else:
        Tk = sum(kv for _, kv in seqs)
        cu_k = torch.tensor([0] + torch.tensor([kv for _, kv in seqs]).cumsum(0).tolist(), dtype=torch.int32)
        k = torch.randn(Tk + 64, nkv, d, generator=g)
        v = torch.randn(Tk + 64, nkv, d, generator=g)
        for b, (_, kv) in enumerate(seqs):
            for j, level in (spikes or {}).items():
                if j < kv:
                    k[int(cu_k[b]) + j] = 0.0
                    k[int(cu_k[b]) + j, :, 0] = level / (RESCALE_A * c["scale"] * 1.4426950408889634)
        k[Tk:] = nan
        v[Tk:] = inf
        if neighbour:
            k[int(cu_k[1]):int(cu_k[2])] = nan
            v[int(cu_k[1]):int(cu_k[2])] = inf
            c["assert_seqs"] = [0]
        c.update(k=k.to(dtype), v=v.to(dtype), cu_k=cu_k)
    c["q"] = q.to(dtype)
    return c


# ---- the dense float64 reference ------------------------------------------------------------------------------------------
def visibility(q_len, kv_len, causal, W, causal_shift=0, window_shift=0, kv_shift=0):
    """bool [q_len, kv_len]: query i sits at pos = kv_len - q_len + i; key j is visible iff j < kv_len, (not causal or
    j <= pos) and (W < 0 or j >= pos - W). The shifts move ONE edge by whole keys (sensitivity check only)."""
    pos = (kv_len - q_len + torch.arange(q_len)).view(-1, 1)
    j = torch.arange(kv_len).view(1, -1)
    vis = j < kv_len + kv_shift
    if causal:
        vis = vis & (j <= pos + causal_shift)
    if W >= 0:
        vis = vis & (j >= pos - W + window_shift)
    return vis.expand(q_len, kv_len)


def gather_keys(case, b):
    """K and V rows 0 ... kv_len - 1 of sequence b, [kv_len, nkv, d], through the block table for a paged case"""
    kv = int(case["kv_lens"][b])
    if case["arm"].paged:
        bs = case["arm"].bs
        ids = case["block_tables"][b, :(kv + bs - 1) // bs].long()
        sh = (-1, case["nkv"], case["arm"].d)
        return case["kc"][ids].reshape(sh)[:kv], case["vc"][ids].reshape(sh)[:kv]
    k0 = int(case["cu_k"][b])
    return case["k"][k0:k0 + kv], case["v"][k0:k0 + kv]


def dense_prefill_ref64(case, causal_shift=0, window_shift=0, kv_shift=0):
    """Prefill attention restated densely in float64 -> [Tq, nq * d] float64. Per sequence: gather the kv_len keys, one
    visibility mask (see visibility), one softmax and one PV product per row, query head h on kv head h // (nq / nkv); a row
    with no visible key gives zeros. No tiles, no running maximum, nothing shared with oracle/xllm_oracle.c. The window
    convention (window_left = keys visible to the LEFT of the query's own position) is the one documented in
    tests/_decode_cases.py::dense_decode_ref64."""
    nq, nkv, d = case["nq"], case["nkv"], case["arm"].d
    G = nq // nkv
    out = torch.zeros(int(case["cu_q"][-1]), nq * d, dtype=torch.float64)
    for b, (ql, kv) in enumerate(case["seqs"]):
        if ql == 0 or kv == 0:
            continue
        q0 = int(case["cu_q"][b])
        vis = visibility(ql, kv, case["causal"], case["window_left"], causal_shift, window_shift, kv_shift)
        k, v = gather_keys(case, b)
        k, v = k.double(), v.double().clone()
        seen = vis.any(0)
        k[~seen] = 0.0                         # a key no row sees may be poison: it must not reach the arithmetic
        v[~seen] = 0.0
        s = torch.einsum("ihgd,jhd->hgij", case["q"][q0:q0 + ql].double().view(ql, nkv, G, d), k) * case["scale"]
        s = s.masked_fill(~vis, float("-inf"))
        p = torch.softmax(s, dim=-1)
        p = torch.where(vis.any(1).view(1, 1, ql, 1), p, torch.zeros_like(p))
        out[q0:q0 + ql] = torch.einsum("hgij,jhd->ihgd", p, v).reshape(ql, nq * d)
    return out


_REFS = {}


def references(case, key):
    """dict(fp32 = oracle with fp32 P, p16 = oracle p_round=True, flash = oracle "flash" mode, r64 = the float64 reference,
    r64r = the same rounded to the case's dtype), computed once per key in a process and never modified"""
    if key not in _REFS:
        c = case
        r = {}
        for name, mode in (("fp32", False), ("p16", True), ("flash", "flash")):
            if c["arm"].paged:
                r[name] = orc.paged_attention(c["q"], c["kc"], c["vc"], c["cu_q"], c["kv_lens"], c["block_tables"], c["scale"],
                                              causal=c["causal"], window_left=c["window_left"], p_round=mode)
            else:
                r[name] = orc.attention_varlen(c["q"], c["k"], c["v"], c["cu_q"], c["cu_k"], c["scale"], causal=c["causal"],
                                               window_left=c["window_left"], p_round=mode)
        r["r64"] = dense_prefill_ref64(c)
        r["r64r"] = r["r64"].to(c["dtype"])
        _REFS[key] = r
    return _REFS[key]


# ---- the tables, by id; seeds are fixed per id so that the CPU and the GPU file see the same bytes
def mask_case(arm, mi, dtype):
    causal, W = MASKS[mi]
    nq, nkv = HEADS[mi % 3]
    seqs = SEQS + (SEQS_SHORT_KV if not arm.paged else [])
    key = ("mask", arm.name, mi, dtype)
    return key, build_case(arm, dtype, seqs, causal, W, nq, nkv, seed=100 * ARMS.index(arm) + mi,
                           max_q_len=PAD_MAX_Q if W == 1 else None)


def pform_case(arm, pi, dtype):
    n, nq, nkv = PFORMS[pi]
    key = ("pform", arm.name, pi, dtype)
    return key, build_case(arm, dtype, PFORM_SEQS[:n], 1, PFORM_W, nq, nkv, seed=1000 + 10 * ARMS.index(arm) + pi)


def poison_case(arm, pi, dtype):
    causal, W = POISON_MASKS[pi]
    key = ("poison", arm.name, pi, dtype)
    return key, build_case(arm, dtype, POISON_SEQS, causal, W, 4, 2, seed=2000 + 10 * ARMS.index(arm) + pi, poison_window=True)


def neighbour_case(arm, dtype):
    """unpaged: the second sequence's K is NaN and its V Inf, 28 of its rows share the first sequence's last 64-key tile (100 =
    64 + 36) and 4 its last 32-key tile; only the first sequence is asserted"""
    key = ("neighbour", arm.name, dtype)
    return key, build_case(arm, dtype, [(70, 100), (50, 90)], 1, -1, 4, 2, seed=2500 + ARMS.index(arm), neighbour=True)


def rescale_case(arm, kind, dtype):
    key = ("rescale", arm.name, kind, dtype)
    seqs = RESCALE_SEQS if kind != "staircase" else RESCALE_SEQS[:1]
    return key, build_case(arm, dtype, seqs, 1, -1, 4, 2, seed=3000 + 10 * ARMS.index(arm) + list(RESCALE).index(kind),
                           spikes=RESCALE[kind])


def split_pitch_case(arm, dtype):
    """k from a buffer of row pitch nkv * d + 64, v contiguous (the GPU test builds the layouts; the CPU side is compact)"""
    key = ("split_pitch", arm.name, dtype)
    return key, build_case(arm, dtype, [(129, 329), (33, 97), (64, 65)], 1, 64, 4, 2, seed=4000 + ARMS.index(arm),
                           layout="split_pitch")


def wide_pitch_case():
    """two sequences, nq = 2, nkv = 1, bf16; on the GPU k and v are column slices of one [40, 1 << 24] buffer"""
    key = ("wide_pitch",)
    return key, build_case(WIDE_ARM, torch.bfloat16, [(12, 12), (5, 20)], 1, 3, 2, 1, seed=5000, layout="wide_pitch")


def all_cases():
    """(id, kind, builder) of every case of the tables -- builders, not tensors"""
    out = []
    for dt in DTYPES:
        n = DTNAME[dt]
        for a in ARMS:
            for mi in range(len(MASKS)):
                out.append((f"mask-{a.name}-c{MASKS[mi][0]}W{MASKS[mi][1]}-{n}", "mask", lambda a=a, mi=mi, dt=dt: mask_case(a, mi, dt)))
            for pi in range(len(POISON_MASKS)):
                out.append((f"poison-{a.name}-c{POISON_MASKS[pi][0]}W{POISON_MASKS[pi][1]}-{n}", "poison",
                            lambda a=a, pi=pi, dt=dt: poison_case(a, pi, dt)))
            if not a.paged:
                out.append((f"neighbour-{a.name}-{n}", "poison", lambda a=a, dt=dt: neighbour_case(a, dt)))
                out.append((f"split_pitch-{a.name}-{n}", "layout", lambda a=a, dt=dt: split_pitch_case(a, dt)))
        for a in M32_ARMS + [STAGED_CONTROL]:
            for kind in RESCALE:
                out.append((f"rescale-{a.name}-{kind}-{n}", "rescale", lambda a=a, kind=kind, dt=dt: rescale_case(a, kind, dt)))
    for ai, a in enumerate(M32_ARMS):
        for pi in range(len(PFORMS)):
            dt = DTYPES[(pi + ai) % 2]
            out.append((f"pform-{a.name}-P{PFORMS[pi][0] * PFORMS[pi][2]}-{DTNAME[dt]}", "pform",
                        lambda a=a, pi=pi, dt=dt: pform_case(a, pi, dt)))
    out.append(("wide_pitch-bf16", "layout", wide_pitch_case))
    return out


# ---- bars ----------------------------------------------------------------------------------------------------------------
# whole tensor, per sequence: tests/_bars.py::assert_p16_attention_close on the one-16-bit-P arms, assert_attn_close at these
# relative bars on the hi + lo arms
BAR_REL = {torch.bfloat16: 1e-3, torch.float16: 2e-4}
# per (query, head) row: the largest relative L2 distance of the ORACLE in the matching mode (p_round=True for one 16-bit P,
# fp32 P for hi + lo) from float64 rounded to the dtype, measured on the CPU over every case of all_cases()
# (MEASURED_ON, N_CASES); the bar is twice that -- the kernel rounds the un-normalised P, the oracle the normalised one.
# tests/test_prefill_reference.py re-measures and fails when a table change moves the oracle past ROW_MEASURED.
MEASURED_ON, N_CASES = "2026-10-19", 199
ROW_MEASURED = {("p16", torch.bfloat16): 5.02e-3, ("p16", torch.float16): 6.19e-4,      # p_round=True oracle, the m32-arm cases
                ("hilo", torch.bfloat16): 2.52e-3, ("hilo", torch.float16): 3.13e-4}    # fp32-P oracle, every case
ROW_BAR = {k: 2.0 * v for k, v in ROW_MEASURED.items()}
ORACLE_MODE = {"p16": "p16", "hilo": "fp32"}


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def distance(got, ref):
    """(relative L2 over the tensor, largest |got - ref| in units of 2 bf16 ulp of the token's maximum): both <= 1 x bar is
    what tests/test_gpu_parity.py::assert_attn_close(got, ref, rel=bar) asserts"""
    got, ref = got.float().cpu(), ref.float().cpu()
    rel = float((got - ref).norm() / ref.norm().clamp_min(1e-30))
    scale = ref.abs().amax(-1, keepdim=True).clamp_min(1e-30)
    elem = float(((got - ref).abs() / (2 * 2.0 ** -8 * scale + 1e-30)).max())
    return rel, elem


def row_distances(got, ref, nq):
    """per (query, head) relative L2 distance, [T, nq]; NaN where the reference row is zero (those rows are checked for
    exact zeros instead)"""
    T = ref.shape[0]
    g, r = got.double().cpu().view(T, nq, -1), ref.double().cpu().view(T, nq, -1)
    n = r.norm(dim=-1)
    return torch.where(n > 0, (g - r).norm(dim=-1) / n.clamp_min(1e-300), torch.full_like(n, float("nan")))


def asserted_rows(case):
    """bool [Tq]: the query rows of the sequences a case asserts"""
    m = torch.zeros(int(case["cu_q"][-1]), dtype=torch.bool)
    for b in case["assert_seqs"]:
        m[int(case["cu_q"][b]):int(case["cu_q"][b + 1])] = True
    return m


def check_output(out, case, key, form=None):
    """every bar the GPU test holds a kernel output to (out: [Tq, nq * d], any device), applied per sequence; returns the
    largest distances seen (for the records). form: the P form of the arm the case ran on."""
    from _bars import FLASH_BAR, assert_attn_close, assert_p16_attention_close
    out = out.cpu()
    form = form or p_form(case["arm"])
    r = references(case, key)
    dt, nq = case["dtype"], case["nq"]
    rows = asserted_rows(case)
    assert torch.isfinite(out[rows].float()).all(), f"{key}: non-finite output rows {(~torch.isfinite(out.float()).all(-1) & rows).nonzero().flatten()[:8].tolist()}"
    worst = dict(rel=0.0, elem=0.0, flash=0.0, row=0.0)
    for b in case["assert_seqs"]:
        sl = slice(int(case["cu_q"][b]), int(case["cu_q"][b + 1]))
        o = out[sl]
        if form == "p16":
            assert_p16_attention_close(o, r["r64r"][sl], r["p16"][sl], r["flash"][sl])
            worst["flash"] = max(worst["flash"], rel_l2(o, r["flash"][sl]))
            worst["rel"] = max(worst["rel"], rel_l2(o, r["r64r"][sl]))
        else:
            assert_attn_close(o, r["fp32"][sl], rel=BAR_REL[dt])
            assert_attn_close(o, r["r64r"][sl], rel=BAR_REL[dt])
            for ref in (r["fp32"][sl], r["r64r"][sl]):
                rel, elem = distance(o, ref)
                worst["rel"], worst["elem"] = max(worst["rel"], rel), max(worst["elem"], elem)
    rd = row_distances(out, r["r64r"], nq)
    blind = torch.isnan(rd) & rows.view(-1, 1)
    assert not out.view(out.shape[0], nq, -1)[blind].any(), f"{key}: a row that sees no key is not exactly zero"
    rd = rd[rows]
    rd = rd[~torch.isnan(rd)]
    worst["row"] = float(rd.max()) if rd.numel() else 0.0
    print(f"{key} [{form}]: rel L2 {worst['rel']:.3e}, vs flash {worst['flash']:.3e}, element-wise {worst['elem']:.3f} bar, "
          f"row {worst['row']:.3e} (bar {ROW_BAR[(form, dt)]:.3e})")
    assert worst["row"] <= ROW_BAR[(form, dt)], f"{key}: row distance {worst['row']:.3e} > {ROW_BAR[(form, dt)]:.3e}"
    if form == "p16":
        assert worst["flash"] <= FLASH_BAR
    return worst
