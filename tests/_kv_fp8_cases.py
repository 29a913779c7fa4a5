"""Case tables for decode attention over an e4m3 KV cache with static scales (xllm_amd/csrc/xllm_mi355_kv_fp8.h), shared by
tests/test_kv_fp8_host.py (CPU) and tests/test_gpu_kv_fp8_ops.py (GPU). Built on tests/_decode_cases.py: the seeded, poisoned
16-bit case of make_case is quantised with static_scaled_fp8_quant's rule -- e4m3fn(clamp(x * (1 / scale), +-448)) -- under scales
that are NOT powers of two, the dead rows (NaN in K, Inf in V there) are re-poisoned with the e4m3 NaN byte 0x7F in BOTH caches
(e4m3fn has no Inf), and the reference is dense_decode_ref64 on codes.double() * scale.

Every case names the launch plan it is meant to reach (kv8_plan, attention_decode_kv8.hip): heads per workgroup, page-uniform or
gathered tiles, the grid split count the planner asks for and the one left after degradation to the workspace given. plan_py()
restates the planning rule; the host test holds xllm_mi355_paged_decode_kv8_plan to it on every case, the GPU tests assert the
plan before they launch."""
import collections
import os

import torch

import _decode_cases as dc
from _decode_cases import BAR_REL, LENS, SPLIT_LENS, SPLIT_WINDOWS, T_LOS, WINDOWS, dense_decode_ref64, distance, make_case, poison, ragged_lens  # noqa: F401

FP8 = torch.float8_e4m3fn
TILE = 32                      # kTile8 of attention_decode_kv8.hip
K_SCALE, V_SCALE = 0.013, 0.0135    # not powers of two; |randn| < 5.8 keeps |x / scale| < 448 (asserted per case)
K_SCALE_P2, V_SCALE_P2 = 2.0 ** -6, 2.0 ** -6   # powers of two: codes * scale is exact in bf16 and f16 (|x / scale| < 448 asserted)
DTYPES = dc.DTYPES

# LENS plus one short of, on and one past every multiple of the 32-token tile up to three tiles (31 ... 65 are in LENS already)
KV8_LENS = sorted(set(LENS + [t * TILE + e for t in (1, 2, 3) for e in (-1, 0, 1)]))

Plan = collections.namedtuple("Plan", "name B nq nkv d bs hpw uniform nsplit")
# nsplit: planned == delivered at max_kv_len <= 300 (10 tiles < 8 * nsub for every hpw) with the full workspace
PLANS = [
    Plan("hpw4_all_g7", 192, 28, 4, 128, 128, hpw=4, uniform=1, nsplit=1),         # all 4 kv heads in the workgroup, group 7
    Plan("hpw4_part_page16", 48, 32, 16, 128, 16, hpw=4, uniform=0, nsplit=1),     # 4 of 16 kv heads per workgroup, gathered
    Plan("hpw2_part", 96, 28, 4, 128, 128, hpw=2, uniform=1, nsplit=1),            # 2 of 4 kv heads, 2 sub-ranges per head
    Plan("hpw2_all_d64", 192, 14, 2, 64, 64, hpw=2, uniform=1, nsplit=1),          # both kv heads in the workgroup, d = 64
    Plan("hpw4_d64_page16", 192, 16, 4, 64, 16, hpw=4, uniform=0, nsplit=1),       # d = 64 gathered
    Plan("hpw1", 4, 28, 4, 128, 128, hpw=1, uniform=1, nsplit=1),                  # 4 sub-ranges of one head per workgroup
    Plan("hpw4_g1", 192, 4, 4, 128, 128, hpw=4, uniform=1, nsplit=1),              # group size 1 (MHA)
    Plan("hpw4_g16", 192, 64, 4, 128, 128, hpw=4, uniform=1, nsplit=1),            # group size 16: all 1024 epilogue work items
]
PLAN = {p.name: p for p in PLANS}
WINDOW_PLANS = [PLANS[0], PLANS[1]]           # page-uniform and gathered
# split-KV: SPLIT_PLAN's 3 x 2500 / 1000 / 130 tokens plus an empty row; 79 tiles, hpw = 1 (nsub = 4) -> 79 / 32 = 2 grid splits
SPLIT_PLAN = Plan("hpw1_split2", 4, 28, 4, 128, 128, hpw=1, uniform=1, nsplit=2)
KV8_SPLIT_LENS = SPLIT_LENS + [0]


def kv8_ragged_lens(B):
    """KV8_LENS (longest first; stride 4 is coprime with their number, so 15 rows already hold them all) over B - 1 rows plus one
    empty row, as dc.ragged_lens deals LENS"""
    rev = KV8_LENS[::-1]
    zero_row = min(5, B - 1)
    return [0 if i == zero_row else rev[(4 * i) % len(rev)] for i in range(B)]


# ---- the planning rule, restated (attention_api.hip: decode_heads_per_wg, decode_num_splits; attention_decode_kv8.hip: kv8_plan)
def workspace_bound(B, nq, d):
    return B * nq * 32 * (d + 2) * 4       # xllm_mi355_paged_attention_workspace_bytes, decode form


def plan_py(B, nq, nkv, d, bs, max_kv_len, ws_bytes):
    """(hpw, nsplit_planned, nsplit, uniform)"""
    hpw = 1
    for h in (4, 2):
        if nkv % h == 0 and B * (nkv // h) >= 192:
            hpw = h
            break
    nsub = 4 // hpw
    base = B * (nkv // hpw)
    by_len = max(1, ((max_kv_len + 31) // 32) // (8 * nsub))
    forced = int(os.environ.get("XLLM_MI355_DECODE_SPLITS", "-1"))
    n = forced if forced > 0 else min((256 + base - 1) // base, by_len)
    planned = max(1, min(32, n))
    per_split = B * nq * (d + 2) * 4
    n = planned
    if n * per_split > ws_bytes:
        n = ws_bytes // per_split
    return hpw, planned, max(1, n), 1 if bs % TILE == 0 else 0


# ---- quantisation of a 16-bit case
def quantise(x, scale):
    """static_scaled_fp8_quant's rule on the CPU: e4m3fn(clamp(x * (1 / scale), +-448)) with the f32 reciprocal the kernels form;
    non-finite inputs (the poison) become the NaN byte 0x7F. Returns uint8 codes."""
    sinv = torch.tensor(scale, dtype=torch.float32).reciprocal()
    y = (x.float() * sinv).clamp(-448.0, 448.0)
    codes = y.to(FP8).view(torch.uint8).clone()
    codes[~torch.isfinite(x.float())] = 0x7F
    return codes


def dequant64(codes, scale):
    """codes.double() * scale, scale being the f32 value the kernel reads"""
    return codes.view(FP8).to(torch.float64) * float(torch.tensor(scale, dtype=torch.float32))


def make_kv8_case(plan, kv_lens, dtype, seed, window_left=-1, k_scale=K_SCALE, v_scale=V_SCALE):
    c = make_case(plan, kv_lens, dtype, seed, window_left)
    live_k, live_v = torch.isfinite(c["kc"].float()), torch.isfinite(c["vc"].float())
    assert float(c["kc"].float()[live_k].abs().max()) / k_scale < 448 and float(c["vc"].float()[live_v].abs().max()) / v_scale < 448, \
        "a live value saturates: choose larger scales"
    c["kc16"], c["vc16"] = c["kc"], c["vc"]            # the poisoned 16-bit caches (sensitivity checks)
    c["kc"], c["vc"] = quantise(c["kc16"], k_scale), quantise(c["vc16"], v_scale)
    assert (c["kc"][~live_k] == 0x7F).all() and (c["vc"][~live_v] == 0x7F).all()
    c["k_scale"], c["v_scale"] = k_scale, v_scale
    return c


_REFS = {}


def reference64(case, key, k_scale=None, v_scale=None, kv_lens=None, window_left=None):
    """dense_decode_ref64 on the dequantised cache (float64, [B, nq * d]); computed once per key and never modified. The keyword
    arguments are the mutations of the sensitivity checks (their key names them)."""
    if key not in _REFS:
        c = case
        ks = c["k_scale"] if k_scale is None else k_scale
        vs = c["v_scale"] if v_scale is None else v_scale
        _REFS[key] = dense_decode_ref64(c["q"], dequant64(c["kc"], ks), dequant64(c["vc"], vs),
                                        c["kv_lens"] if kv_lens is None else kv_lens, c["block_tables"], c["scale"],
                                        c["window_left"] if window_left is None else window_left)
    return _REFS[key]


# ---- the cases, by id; seeds are fixed per id so that the CPU and the GPU file see the same bytes
def plan_case(plan, dtype):
    return ("kv8-plan", plan.name, dtype), make_kv8_case(plan, kv8_ragged_lens(plan.B), dtype, seed=5000 + PLANS.index(plan))


def pow2_case(plan, dtype):
    """power-of-two scales: the dequantised cache is exact in the 16-bit dtype, so ops.paged_attention can run on it"""
    lens = KV8_SPLIT_LENS if plan is SPLIT_PLAN else kv8_ragged_lens(plan.B)
    seed = 5500 + (len(PLANS) if plan is SPLIT_PLAN else PLANS.index(plan))
    return ("kv8-pow2", plan.name, dtype), make_kv8_case(plan, lens, dtype, seed=seed, k_scale=K_SCALE_P2, v_scale=V_SCALE_P2)


def window_cases(plan, W, dtype):
    out = []
    for i, lens in enumerate(dc.window_batches(plan, W)):
        out.append((("kv8-window", plan.name, W, i, dtype),
                    make_kv8_case(plan, lens, dtype, seed=6000 + 10 * WINDOW_PLANS.index(plan) + i, window_left=W)))
    return out


def split_case(W, dtype):
    """W = -1: no window"""
    return ("kv8-split", W, dtype), make_kv8_case(SPLIT_PLAN, KV8_SPLIT_LENS, dtype, seed=7000, window_left=W)


def all_cases():
    """(id, builder) of every case of the tables -- builders, not tensors"""
    out = []
    for dt in DTYPES:
        n = str(dt).split(".")[-1]
        for p in PLANS:
            out.append((f"plan-{p.name}-{n}", lambda p=p, dt=dt: [plan_case(p, dt)]))
        for p in WINDOW_PLANS:
            for W in WINDOWS:
                out.append((f"window-{p.name}-W{W}-{n}", lambda p=p, W=W, dt=dt: window_cases(p, W, dt)))
        for W in [-1] + SPLIT_WINDOWS:
            out.append((f"split-W{W}-{n}", lambda W=W, dt=dt: [split_case(W, dt)]))
    return out


# ---- a float32 restatement of the kernel's arithmetic (attention_decode_kv8.hip): k_scale folded into the log2-domain softmax
# scale, every (sequence, head, slot) walks its 32-token tiles in order with a running maximum, P = hi + lo in the 16-bit dtype,
# slots merged first inside the workgroup (sub-ranges) and then over the grid splits, v_scale applied once to the quotient
def kernel_restatement_f32(case, hpw, nsplit):
    c = case
    q, dtype = c["q"].float(), c["dtype"]
    B, nq, d = q.shape
    bs, nkv = c["kc"].shape[1], c["kc"].shape[2]
    G = nq // nkv
    f32 = torch.float32
    ks, vs = torch.tensor(c["k_scale"], dtype=f32), torch.tensor(c["v_scale"], dtype=f32)
    sl2 = torch.tensor(c["scale"], dtype=f32) * torch.tensor(1.4426950408889634, dtype=f32) * ks
    nsub = 4 // hpw
    nslots = nsplit * nsub
    W = c["window_left"]
    W = -1 if W < 0 else min(W, 0x3fffffff)
    out = torch.zeros(B, nq * d, dtype=f32)
    NEG = torch.tensor(-1e30, dtype=f32)
    for b in range(B):
        L = int(c["kv_lens"][b])
        if L == 0:
            continue
        ids = c["block_tables"][b, :(L + bs - 1) // bs].long()
        kf = c["kc"][ids].view(FP8).float().reshape(-1, nkv, d)     # NaN codes in dead rows stay NaN: masked below like the kernel
        vf = c["vc"][ids].view(FP8).float().reshape(-1, nkv, d)
        t_lo = max(0, L - 1 - W) if W >= 0 else 0
        tile_lo, tile_hi = t_lo // TILE, (L + TILE - 1) // TILE
        per = (tile_hi - tile_lo + nslots - 1) // nslots
        qb = q[b].view(nkv, G, d)
        m = NEG.repeat(nslots, nkv, G)
        l = torch.zeros(nslots, nkv, G, dtype=f32)
        o = torch.zeros(nslots, nkv, G, d, dtype=f32)
        for slot in range(nslots):
            for tile in range(tile_lo + slot * per, min(tile_lo + (slot + 1) * per, tile_hi)):
                r0, r1 = tile * TILE, min((tile + 1) * TILE, kf.shape[0])
                live = torch.tensor([t_lo <= t < L for t in range(r0, r1)])
                kt = torch.where(live[:, None, None], kf[r0:r1], torch.zeros((), dtype=f32))
                vt = torch.where(live[:, None, None], vf[r0:r1], torch.zeros((), dtype=f32))   # V rows zeroed on both sides
                s = torch.einsum("hgd,thd->hgt", qb, kt) * sl2
                s = torch.where(live[None, None, :], s, torch.tensor(float("-inf")))
                m_new = torch.maximum(m[slot], s.amax(-1))
                alpha = torch.exp2(m[slot] - m_new)
                p = torch.exp2(s - m_new[..., None])
                hi = p.to(dtype).float()
                lo = (p - hi).to(dtype).float()
                l[slot] = l[slot] * alpha + p.sum(-1)
                o[slot] = o[slot] * alpha[..., None] + torch.einsum("hgt,thd->hgd", hi, vt) + torch.einsum("hgt,thd->hgd", lo, vt)
                m[slot] = m_new
        # workgroup merge over the sub-ranges of each grid split, then the merge launch over the splits
        m, l, o = m.view(nsplit, nsub, nkv, G), l.view(nsplit, nsub, nkv, G), o.view(nsplit, nsub, nkv, G, d)
        mw = m.amax(1)
        f = torch.exp2(m - mw[:, None])
        lw, ow = (f * l).sum(1), (f[..., None] * o).sum(1)
        ms = mw.amax(0)
        f = torch.exp2(mw - ms[None])
        lt, ot = (f * lw).sum(0), (f[..., None] * ow).sum(0)
        out[b] = torch.where(lt[..., None] > 0, ot / lt[..., None] * vs, torch.zeros((), dtype=f32)).reshape(-1)
    return out
