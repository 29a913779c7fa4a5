"""Case tables and dense float64 references for the MoE routing tests (tests/test_moe_reference.py on the CPU,
tests/test_gpu_moe_routing.py on the GPU). Nothing here touches a GPU, and nothing here reads oracle/xllm_oracle.c.

References (float64 torch, one expression per sentence of the operator's definition):
  gate64          softmax | sigmoid scores; choice = score + bias; stable descending sort (ties: lower index); weight = the
                  UNBIASED score; renormalise by the selected sum
  grouped_gate64  group value = max choice (no bias) | sum of the two largest (bias); the topk_group best groups stay (ties: lower
                  group); experts by choice among them; weight = unbiased score * routed_scaling_factor (/ selected sum)
  index_ref       valid = 0 <= id < E; sizes = bincount(valid ids); position = rank in a stable sort by expert; -1 for the rest;
                  dst_src on [0, n_valid) only
  combine64       weighted sum over the PRESENT rows (index >= 0 and < nv) and sum_k |w x| per element, for the bar

Gate inputs are PLACED, not drawn from a continuous law. Logits are multiples of 1/16 in [-6, 6] (exact in bf16, f16 and f32),
biases multiples of 1/512 in [-1/8, 1/8]. Equal logits under equal bias give bit-equal fp32 scores on any implementation, so
every tie is exact and index decides it; values that differ must differ CLEARLY: the builders check, in float64, the topk + 1 best
choice scores of every row and the group values on both sides of the group cut -- each adjacent gap is exactly 0 (and then the
logits and biases behind the two values are the same), or at least MIN_REL_GAP = 1e-5 relative (about a hundred fp32 roundings of
a score of order 1). A row that fails is drawn again from a bumped seed; no row is left out. gaps_ok / grouped_gaps_ok are the
same checks the CPU test re-asserts over every case.

The all-negative mode ("sigmoid_bias_neg": bias - 2, E % 64 != 0) draws its logits from [0, 6]. Its weight is (s + b - 2) - (b - 2)
in fp32 on every implementation (the reference's own expression); the rounding of the inner sum is half an ulp of the choice score:
2^-25 below 1, 2^-24 in [1, 2), 2^-23 = 1.19e-7 from 2 on. With s >= 1/2 the choice score stays inside (-1.63, -0.87), so the
cancellation error is <= 6e-8 and the project's gate bar (rtol 3e-6, atol 1e-7) is a statement about the kernel; at s < 1/8 it
would be a coin toss about the format."""
import collections
import functools
import math

import torch

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
HALF = [torch.bfloat16, torch.float16]
NAME = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
MANT = {torch.float32: 23, torch.bfloat16: 7, torch.float16: 10}          # stored mantissa bits
EMIN = {torch.float32: -126, torch.bfloat16: -126, torch.float16: -14}    # exponent of the smallest normal
MIN_REL_GAP = 1e-5
GATE_RTOL, GATE_ATOL = 3e-6, 1e-7          # the project's gate bar (tests/test_gpu_parity.py::test_moe_fused_topk)
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


# ============================================================================================================ references
def scores64(x, scoring):
    x = x.double()
    return torch.softmax(x, -1) if scoring == "softmax" else torch.sigmoid(x)


def gate64(x, topk, renorm, bias, scoring):
    """x [T, E] -> (weights float64 [T, topk], ids int32 [T, topk])"""
    s = scores64(x, scoring)
    c = s if bias is None else s + bias.double()
    ids = torch.sort(c, dim=-1, descending=True, stable=True).indices[:, :topk]
    w = s.gather(1, ids)
    if renorm:
        w = w / w.sum(-1, keepdim=True)
    return w, ids.to(torch.int32)


def group_values64(c, G, biased):
    T, E = c.shape
    cg = c.view(T, G, E // G)
    if not biased:
        return cg.max(-1).values
    return torch.sort(cg, dim=-1, descending=True, stable=True).values[..., :2].sum(-1)


def kept_groups64(c, G, topk_group, biased):
    """bool [T, G]: the topk_group best groups by value, ties to the lower group"""
    gv = group_values64(c, G, biased)
    order = torch.sort(gv, dim=-1, descending=True, stable=True).indices[:, :topk_group]
    kept = torch.zeros(gv.shape, dtype=torch.bool)
    kept.scatter_(1, order, True)
    return kept


def grouped_gate64(x, topk, G, topk_group, renorm, bias, scoring, scale):
    """-> (weights float64 [T, topk], ids int32 [T, topk], kept bool [T, G])"""
    T, E = x.shape
    s = scores64(x, scoring)
    c = s if bias is None else s + bias.double()
    kept = kept_groups64(c, G, topk_group, bias is not None)
    c = torch.where(kept.repeat_interleave(E // G, dim=1), c, torch.full_like(c, -math.inf))
    ids = torch.sort(c, dim=-1, descending=True, stable=True).indices[:, :topk]
    w = s.gather(1, ids)
    w = w * scale / w.sum(-1, keepdim=True) if renorm else w * scale
    return w, ids.to(torch.int32), kept


Index = collections.namedtuple("Index", "src_dst dst_src sizes n_valid")


def index_ref(ids, E):
    """ids: int32 [n] (any values). dst_src has n_valid entries."""
    ids = ids.flatten().long()
    valid = (ids >= 0) & (ids < E)
    rows = valid.nonzero().flatten()
    sizes = torch.bincount(ids[rows], minlength=E).to(torch.int32)
    order = torch.sort(ids[rows], stable=True).indices
    dst_src = rows[order].to(torch.int32)
    src_dst = torch.full((ids.numel(),), -1, dtype=torch.int32)
    src_dst[dst_src.long()] = torch.arange(rows.numel(), dtype=torch.int32)
    return Index(src_dst, dst_src, sizes, int(rows.numel()))


def combine64(rows, w, src_dst=None, nv=None):
    """rows [N, H] (the expanded rows t * topk + k when src_dst is None, the sorted rows otherwise), w [T, topk] ->
    (sum float64 [T, H], sum_k |w x| float64 [T, H]) over the present rows"""
    T, topk = w.shape
    idx = torch.arange(T * topk) if src_dst is None else src_dst.flatten().long()
    present = idx >= 0
    if nv is not None:
        present &= idx < nv
    x = rows.double()[idx.clamp(0, rows.size(0) - 1)]
    x = torch.where(present[:, None], x, torch.zeros_like(x))        # an absent row may hold NaN: it is not multiplied
    terms = x.view(T, topk, -1) * w.double()[..., None]
    return terms.sum(1), terms.abs().sum(1)


def ulp(v, dtype):
    """spacing of `dtype` at |v| (float64 tensor), the subnormal spacing below the smallest normal"""
    v = v.abs().double()
    e = torch.frexp(v).exponent - 1                                  # |v| in [2^e, 2^(e+1))
    e = torch.where(v > 0, e, torch.full_like(e, EMIN[dtype])).clamp(min=EMIN[dtype]).double()
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - MANT[dtype])


def combine_bar(got, ref, abs_sum, topk, dtype):
    """0.5 ulp_T(max(|got|, |ref|)) -- one rounding to the output type -- plus topk * 2^-23 * sum_k |w x| -- the fp32 accumulate,
    with or without FMA (a rounding per product and per addition, each <= 2^-24 of a partial sum that is <= sum_k |w x|)"""
    return 0.5 * ulp(torch.maximum(got.double().abs(), ref.abs()), dtype) + topk * 2.0 ** -23 * abs_sum


def assert_combine(got, ref, abs_sum, topk, dtype, tag):
    """every element inside the bar; returns the largest |got - ref| / bar"""
    g = got.double().cpu()
    assert bool(torch.isfinite(g).all()), (tag, "non-finite output")
    assert bool(torch.isfinite(ref).all()) and g.shape == ref.shape, (tag, "the reference itself is not finite")
    bar = combine_bar(g, ref, abs_sum, topk, dtype)
    err = (g - ref).abs()
    bad = err > bar
    assert not bool(bad.any()), (tag, int(bad.sum()), float(err[bad].max()), float(bar[bad].min()))
    frac = torch.where(bar > 0, err / bar, torch.zeros_like(err))
    return float(frac.max()) if frac.numel() else 0.0


def assert_gate_weights(got, ref, rtol, atol, tag):
    """|got - ref| <= atol + rtol |ref| everywhere; returns (largest relative offset, largest offset / bar)"""
    g, r = got.double().cpu(), ref.double()
    err = (g - r).abs()
    bar = atol + rtol * r.abs()
    assert bool((err <= bar).all()), (tag, float((err / bar).max()), float(err.max()))
    return float((err / r.abs().clamp(min=1e-300)).max()), float((err / bar).max())


# ============================================================================================================ placed inputs
def grid_logits(g, shape, lo=-6.0, hi=6.0):
    return torch.randint(int(lo * 16), int(hi * 16) + 1, shape, generator=g).float() / 16


def grid_bias(g, E):
    return torch.randint(-64, 65, (E,), generator=g).float() / 512


def _adjacent_ok(vals, same):
    """vals [T, n] float64 sorted descending, same [T, n - 1]: the inputs behind neighbours j, j + 1 are equal -> bool [T]"""
    if vals.size(1) < 2:
        return torch.ones(vals.size(0), dtype=torch.bool)
    a, b = vals[:, :-1], vals[:, 1:]
    gap = a - b
    scale = torch.maximum(a.abs(), b.abs())
    both_inf = torch.isinf(a) & torch.isinf(b)                       # two dropped / absent candidates: nothing to order
    clear = gap >= MIN_REL_GAP * scale
    return (((gap == 0) & same) | (clear & (gap > 0)) | both_inf).all(1)


def gaps_ok(x, bias, scoring, n_top):
    """the plain gate's condition per row: bool [T]"""
    s = scores64(x, scoring)
    c = s if bias is None else s + bias.double()
    n = min(n_top, x.size(1))
    srt = torch.sort(c, dim=-1, descending=True, stable=True)
    idx, vals = srt.indices[:, :n], srt.values[:, :n]
    lx = x.gather(1, idx)
    same = lx[:, :-1] == lx[:, 1:]
    if bias is not None:
        lb = bias[idx]
        same &= lb[:, :-1] == lb[:, 1:]
    return _adjacent_ok(vals, same)


def grouped_gaps_ok(x, bias, scoring, G, topk_group, n_top):
    """the grouped gate's condition per row: the two group values at the cut, then the n_top best choices among the kept groups"""
    T, E = x.shape
    EG = E // G
    s = scores64(x, scoring)
    c = s if bias is None else s + bias.double()
    ok = torch.ones(T, dtype=torch.bool)
    if topk_group < G:
        gv = group_values64(c, G, bias is not None)
        srt = torch.sort(gv, dim=-1, descending=True, stable=True)
        pair = srt.indices[:, topk_group - 1:topk_group + 1]                                  # the groups on both sides of the cut
        vals = srt.values[:, topk_group - 1:topk_group + 1]
        m = 2 if bias is not None else 1
        top = torch.sort(c.view(T, G, EG), dim=-1, descending=True, stable=True).indices[..., :m]   # what a group value is made of
        eidx = top + (torch.arange(G) * EG)[None, :, None]
        lx = x.gather(1, eidx.view(T, -1)).view(T, G, m)
        same = (lx.gather(1, pair[:, :1, None].expand(T, 1, m)) == lx.gather(1, pair[:, 1:, None].expand(T, 1, m))).all(-1)
        if bias is not None:
            lb = bias[eidx]
            same &= (lb.gather(1, pair[:, :1, None].expand(T, 1, m)) == lb.gather(1, pair[:, 1:, None].expand(T, 1, m))).all(-1)
        ok &= _adjacent_ok(vals, same)
    kept = kept_groups64(c, G, topk_group, bias is not None)
    cm = torch.where(kept.repeat_interleave(EG, dim=1), c, torch.full_like(c, -math.inf))
    n = min(n_top, topk_group * EG)
    srt = torch.sort(cm, dim=-1, descending=True, stable=True)
    idx, vals = srt.indices[:, :n], srt.values[:, :n]
    lx = x.gather(1, idx)
    same = lx[:, :-1] == lx[:, 1:]
    if bias is not None:
        lb = bias[idx]
        same &= lb[:, :-1] == lb[:, 1:]
    return ok & _adjacent_ok(vals, same)


def place_rows(make_row, T, seed, check):
    """make_row(generator, t) -> [E]; check([T, E]) -> bool [T]. Row t is drawn from seed + 1000003 t and drawn again from a seed
    bumped by 7919 until it passes: deterministic, and every row ends up in the table."""
    seeds = [seed + 1000003 * t for t in range(T)]
    rows = [make_row(torch.Generator().manual_seed(s), t) for t, s in enumerate(seeds)]
    for _ in range(400):
        x = torch.stack(rows)
        bad = (~check(x)).nonzero().flatten().tolist()
        if not bad:
            return x
        for t in bad:
            seeds[t] += 7919
            rows[t] = make_row(torch.Generator().manual_seed(seeds[t]), t)
    raise AssertionError("a row could not be placed")


# ---------------------------------------------------------------------------------------------------------- the plain gate
GATE_E = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512]      # every PL arm (1, 2, 4, 8) on both sides of each switch
GATE_T = [1, 2, 3, 4, 5, 37]                                             # 4 tokens per workgroup: every remainder, and 10 workgroups
GATE_MODES = ["softmax", "sigmoid", "sigmoid_bias", "sigmoid_bias_neg"]
SCORING = {"softmax": "softmax", "sigmoid": "sigmoid", "sigmoid_bias": "sigmoid", "sigmoid_bias_neg": "sigmoid"}


def gate_modes(E):
    return [m for m in GATE_MODES if m != "sigmoid_bias_neg" or E % 64 != 0]


def gate_topks(E):
    return sorted({k for k in (1, 8, min(E, 64)) if k <= E})


def _mode_bias(mode, E, seed):
    if mode not in ("sigmoid_bias", "sigmoid_bias_neg"):
        return None
    b = grid_bias(torch.Generator().manual_seed(seed), E)
    return b - 2.0 if mode == "sigmoid_bias_neg" else b


@functools.lru_cache(maxsize=None)
def gate_case(E, T, mode):
    """(x f32 [T, E], bias f32 [E] | None): grid rows that meet the gap condition for every topk of gate_topks(E)"""
    seed = 100000 * GATE_E.index(E) + 1000 * GATE_T.index(T) + GATE_MODES.index(mode)
    bias = _mode_bias(mode, E, seed + 500)
    lo = 0.0 if mode == "sigmoid_bias_neg" else -6.0
    n_top = min(E, 64) + 1
    x = place_rows(lambda g, t: grid_logits(g, (E,), lo), T, seed, lambda x: gaps_ok(x, bias, SCORING[mode], n_top))
    return x, bias


def gate_cases():
    return [(E, T, mode) for E in GATE_E for T in GATE_T for mode in gate_modes(E)]


TIE_MODES = ["softmax", "sigmoid", "sigmoid_bias"]
TieRows = collections.namedtuple("TieRows", "x bias names groups left")


def _tie_specs(E, topk):
    """(name, group, places left at the cut): the group's members are equal, `left` of them are selected (the lowest indices)"""
    out = []
    if E >= 65:
        out.append(("63|64", [63, 64], 1))                                          # neighbours in different lanes AND slots
    if E >= 129:
        out += [("0|64|128", [0, 64, 128], 1), ("0|64|128", [0, 64, 128], 2)]        # one lane, three slots
    if E >= 8:
        grp = sorted({1, E // 4, E // 2, E // 2 + 1, E - 2})
        out += [("spread", grp, 1), ("spread", grp, len(grp) - 1)]                   # r = 1 and r = m - 1
    if E >= 4:
        out += [("last", [E - 3, E - 2, E - 1], 1), ("last", [E - 3, E - 2, E - 1], 2)]   # the group ends on the last real expert
    return [(n, g, r) for n, g, r in out if r <= topk and topk - r <= E - len(g)]


def tie_special(E):
    return sorted({e for e in (0, 63, 64, 128, 1, E // 4, E // 2, E // 2 + 1, E - 3, E - 2, E - 1) if 0 <= e < E})


@functools.lru_cache(maxsize=None)
def gate_tie_rows(E, topk, mode):
    """rows in three classes that no bias can mix: topk - left experts with logits in [3, 6] (sigmoid >= 0.95), the tie group at
    0 (sigmoid 1/2), the rest in [-6, -3] (sigmoid <= 0.05); the bias is one value on every position a group may take. The last
    row is all-equal logits (under a bias: ordered by bias, ties by index)."""
    seed = 7000000 + 1000 * GATE_E.index(E) + 10 * topk + TIE_MODES.index(mode)
    bias = _mode_bias(mode, E, seed + 500)
    if bias is not None:
        bias[tie_special(E)] = 3.0 / 512
    specs = _tie_specs(E, topk)

    def make_row(g, t):
        if t == len(specs):
            return torch.full((E,), 0.5)
        _, grp, left = specs[t]
        x = grid_logits(g, (E,), -6.0, -3.0)
        others = torch.tensor([e for e in range(E) if e not in grp], dtype=torch.long)
        above = others[torch.randperm(others.numel(), generator=g)[:topk - left]]
        x[above] = grid_logits(g, (above.numel(),), 3.0, 6.0)
        x[grp] = 0.0
        return x
    x = place_rows(make_row, len(specs) + 1, seed, lambda x: gaps_ok(x, bias, SCORING[mode], topk + 1))
    # the cut is where the builder put it
    _, ids = gate64(x, topk, False, bias, SCORING[mode])
    s = scores64(x, SCORING[mode])
    c = s if bias is None else s + bias.double()
    for t, (name, grp, left) in enumerate(specs):
        assert ids[t, topk - left:].tolist() == grp[:left], (E, topk, mode, name)
        assert len(set(c[t, grp].tolist())) == 1 and not set(ids[t, :topk - left].tolist()) & set(grp)
    if bias is None:
        assert ids[-1].tolist() == list(range(topk))
    return TieRows(x, bias, [n for n, _, _ in specs] + ["all_equal"], [g for _, g, _ in specs], [r for _, _, r in specs])


@functools.lru_cache(maxsize=None)
def gate_inf_case(E, mode):
    """-inf logits on about a third of the experts (lane 0's slot 0, the seam and the last expert among them); more than 64 + 1
    (or E // 2) finite ones remain"""
    seed = 8000000 + 10 * GATE_E.index(E) + GATE_MODES.index(mode)
    bias = _mode_bias(mode, E, seed + 500)
    T = 5

    def make_row(g, t):
        x = grid_logits(g, (E,))
        dead = torch.randperm(E, generator=g)[:E // 3]
        x[dead] = -math.inf
        for e in (0, 63, 64, E - 1):
            if e < E and t % 2 == 0:
                x[e] = -math.inf
        return x
    x = place_rows(make_row, T, seed, lambda x: gaps_ok(x, bias, SCORING[mode], min(E // 2, 64) + 1))
    assert int(torch.isfinite(x).sum(1).min()) > min(E // 2, 64)
    return x, bias


def saturated_case(E):
    """logits at +-30: sigmoid(30) is exactly 1 in fp32 (a tie) and below 1 in float64 -- the documented departure, held to the
    fp32 oracle only. Every logit is +30 or -30: equal inputs give equal scores on any implementation."""
    g = torch.Generator().manual_seed(9000000 + E)
    x = torch.where(torch.rand(7, E, generator=g) < 0.5, torch.tensor(30.0), torch.tensor(-30.0))
    x[0] = 30.0
    x[1] = -30.0
    return x


# -------------------------------------------------------------------------------------------------------- the grouped gate
GROUPED_EG = [(64, 64), (128, 64), (96, 3), (160, 8), (256, 8), (512, 64), (512, 2)]
GROUPED_T = [3, 37]
GROUPED_MODES = ["softmax", "sigmoid", "sigmoid_bias"]


def grouped_modes(E, G):
    if (E, G) == (64, 64):
        return ["softmax", "sigmoid"]                      # one expert per group: the biased group value needs two
    if (E, G) == (128, 64):
        return ["sigmoid_bias"]                            # EG = 2 with bias: the group value is the sum of the whole group
    return GROUPED_MODES


def grouped_topk_groups(G):
    return sorted({1, (G + 1) // 2 if G > 2 else 1, G})


def grouped_topks(E, G, kg):
    cap = min(kg * (E // G), 64)
    return sorted({k for k in (1, 8, cap) if k <= cap})


@functools.lru_cache(maxsize=None)
def grouped_case(E, G, kg, mode, T):
    seed = 20000000 + 100000 * GROUPED_EG.index((E, G)) + 1000 * kg + 10 * GROUPED_MODES.index(mode) + GROUPED_T.index(T)
    bias = _mode_bias(mode, E, seed + 500)
    n_top = max(grouped_topks(E, G, kg)) + 1
    x = place_rows(lambda g, t: grid_logits(g, (E,)), T, seed,
                   lambda x: grouped_gaps_ok(x, bias, SCORING[mode], G, kg, n_top))
    return x, bias


def grouped_cases():
    return [(E, G, kg, mode, T) for E, G in GROUPED_EG for kg in grouped_topk_groups(G) for mode in grouped_modes(E, G)
            for T in GROUPED_T]


Placed = collections.namedtuple("Placed", "name x bias")


@functools.lru_cache(maxsize=None)
def grouped_placed(E, G, kg, mode, topk):
    """the placed rows of the grouped gate, one launch each (a row pins the bias it needs); every property is asserted here, in
    float64, before anything else sees the row.
      twin_groups    (kg < G) kg - 1 groups with logits in [3, 6], two groups of IDENTICAL logits (and bias) in [0, 1/2], the
                     rest in [-6, -4]: the twins are ranks kg - 1 and kg, the lower one stays
      best_loses     (bias, kg < G) group A holds the row's best expert (logit 6, bias + 1/8) and nothing else above -6;
                     group B holds two experts at 4: B wins the top-2 sum, A would win the max
      choice_vs_weight (bias) expert p: logit 3, bias - 1/8 (choice 0.83); expert q: logit 2, bias + 1/8 (choice 1.01): q is
                     selected first with the smaller weight
      all_equal      one logit (and one bias) everywhere: groups 0 .. kg - 1, then the lowest experts"""
    EG = E // G
    biased = mode == "sigmoid_bias"
    scoring = SCORING[mode]
    seed = 30000000 + 100000 * GROUPED_EG.index((E, G)) + 1000 * kg + 10 * GROUPED_MODES.index(mode) + topk
    gen = torch.Generator().manual_seed(seed + 1)
    out = []

    def place(name, make_row, bias):
        x = place_rows(make_row, 1, seed + len(out), lambda x: grouped_gaps_ok(x, bias, scoring, G, kg, topk + 1))
        s = scores64(x, scoring)
        c = s if bias is None else s + bias.double()
        out.append(Placed(name, x, bias))
        w, ids, kept = grouped_gate64(x, topk, G, kg, False, bias, scoring, 1.0)
        return s[0], c[0], kept[0], w[0], ids[0]

    if kg < G:
        perm = torch.randperm(G, generator=gen).tolist()
        tops, (ga, gb) = perm[:kg - 1], sorted(perm[kg - 1:kg + 1])
        bias = _mode_bias(mode, E, seed + 500)
        if biased:
            bias[gb * EG:(gb + 1) * EG] = bias[ga * EG:(ga + 1) * EG]

        def twin(g, t):
            x = grid_logits(g, (E,), -6.0, -4.0)
            for grp in tops:
                x[grp * EG:(grp + 1) * EG] = grid_logits(g, (EG,), 3.0, 6.0)
            x[ga * EG:(ga + 1) * EG] = grid_logits(g, (EG,), 0.0, 0.5)
            x[gb * EG:(gb + 1) * EG] = x[ga * EG:(ga + 1) * EG]
            return x
        s, c, kept, w, ids = place("twin_groups", twin, bias)
        gv = group_values64(c[None], G, biased)[0]
        assert float(gv[ga]) == float(gv[gb]) and int((gv > gv[ga]).sum()) == kg - 1, (E, G, kg, mode)
        assert bool(kept[ga]) and not bool(kept[gb])
    if biased and kg == 1 and G >= 2:
        A, B = G - 1, 0
        bias = _mode_bias(mode, E, seed + 501)
        bias[A * EG] = 0.125

        def loses(g, t):
            x = torch.full((E,), -6.0)
            x[A * EG] = 6.0
            x[B * EG + torch.randperm(EG, generator=g)[:2]] = 4.0
            return x
        s, c, kept, w, ids = place("best_loses", loses, bias)
        assert int(c.argmax()) // EG == A and not bool(kept[A]) and bool(kept[B]), (E, G, kg, mode)
        assert bool(kept_groups64(c[None], G, kg, False)[0, A])                           # ... and A would stay under the max rule
        assert not (ids // EG == A).any()
    if biased:
        p, q = E - 1, E - 2                                                               # one group (EG >= 2 under a bias)
        bias = _mode_bias(mode, E, seed + 502)
        bias[p], bias[q] = -0.125, 0.125

        def cvw(g, t):
            x = grid_logits(g, (E,), -6.0, -3.0)
            x[p], x[q] = 3.0, 2.0
            return x
        s, c, kept, w, ids = place("choice_vs_weight", cvw, bias)
        assert float(c[q]) > float(c[p]) and float(s[q]) < float(s[p]) and bool(kept[G - 1])
        assert int(ids[0]) == q and int(s.argmax()) == p                                  # by weight, p would have been first
        if topk >= 2:
            assert ids[:2].tolist() == [q, p] and float(w[0]) < float(w[1])
    bias = torch.full((E,), 3.0 / 512) if biased else None     # (a drawn bias would put sums of two biases a rounding apart)
    s, c, kept, w, ids = place("all_equal", lambda g, t: torch.full((E,), 0.25), bias)
    assert ids.tolist() == list(range(topk)) and kept.tolist() == [g < kg for g in range(G)]
    return out


def grouped_placed_keys():
    out = []
    for E, G in GROUPED_EG:
        for kg in grouped_topk_groups(G):
            for mode in grouped_modes(E, G):
                out.append((E, G, kg, mode))
    return out


# -------------------------------------------------------------------------------------------------------- the index build
CHUNK = 1024            # kMoeChunk: expanded rows per workgroup of the placement pass; n <= CHUNK is the single-launch form
INDEX_N = [1, 63, 64, 65, 1023, 1024, 1025, 2047, 2049, 5121, 9217]
INDEX_E = [1, 2, 3, 64, 65, 300, 512, 513, 1024]
# (n, E). The last two rows are outside INDEX_N on purpose: 5 and 9 chunks, where E = 512 (2 parts) and E = 65 (8 parts) leave the
# last part of moe_scan_kernel short (5121 and 9217 rows are 6 and 10 chunks).
INDEX_PAIRS = [(1, 1), (1, 1024), (63, 3), (64, 64), (65, 65), (65, 513), (1023, 1), (1023, 300), (1024, 2), (1024, 512),
               (1024, 1024),
               (1025, 1), (1025, 2), (1025, 3), (1025, 64), (1025, 512), (1025, 1024), (2047, 65), (2047, 513), (2049, 300),
               (2049, 512), (2049, 1024), (5121, 3), (5121, 65), (5121, 512), (5121, 1024), (9217, 1), (9217, 64), (9217, 65),
               (9217, 512), (9217, 513), (9217, 1024), (5120, 512), (9216, 65)]
INVALID = [-1, None, INT32_MAX, INT32_MIN]      # None: E itself


def scan_geometry(n, E):
    """moe_scan_kernel's (parts, nchunks, per): 1024 threads = (expert padded to a power of two) x parts; a part takes `per`
    consecutive chunks"""
    epad = 1
    while epad < E:
        epad *= 2
    parts = 1024 // epad
    nchunks = (n + CHUNK - 1) // CHUNK
    return parts, nchunks, (nchunks + parts - 1) // parts


@functools.lru_cache(maxsize=None)
def index_inputs(n, E):
    """[(name, ids int32 [n])]: the distributions of one (n, E) pair"""
    g = torch.Generator().manual_seed(40000000 + 2048 * n + E)
    nchunks = (n + CHUNK - 1) // CHUNK
    uniform = torch.randint(0, E, (n,), generator=g, dtype=torch.int32)
    out = [("uniform", uniform), ("all_first", torch.zeros(n, dtype=torch.int32)),
           ("all_last", torch.full((n,), E - 1, dtype=torch.int32))]
    if E >= 2:                                                  # an expert that only the final (partial) chunk holds
        x = torch.randint(0, E - 1, (n,), generator=g, dtype=torch.int32)
        x[(nchunks - 1) * CHUNK + torch.arange(n - (nchunks - 1) * CHUNK)[::3]] = E - 1
        out.append(("last_chunk_only", x))
    if n >= 64:
        w0 = 64 * ((n // 64 - 1) // 2)                          # a whole wave in the middle of the rows
        if E >= 64:
            x = uniform.clone()
            x[w0:w0 + 64] = (torch.randperm(E, generator=g)[:64]).to(torch.int32)
            out.append(("wave_64_distinct", x))
        x = uniform.clone()
        x[w0:w0 + 64] = E // 2
        out.append(("wave_one_expert", x))
    x = uniform.clone()                                         # invalid ids in every chunk, lane 0 of a wave among them
    bad = [E if v is None else v for v in INVALID]
    for c in range(nchunks):
        base, size = c * CHUNK, min(CHUNK, n - c * CHUNK)
        pos = sorted({p for p in (0, 64 if c % 2 else 128, 5, 63, 200, 777, size - 1) if 0 <= p < size})
        for j, p in enumerate(pos):
            x[base + p] = bad[(j + c) % 4]
    out.append(("invalid_everywhere", x))
    x = uniform.clone()                                         # one chunk entirely invalid (the single chunk: see all_invalid)
    if nchunks >= 2:
        c = nchunks // 2
        size = min(CHUNK, n - c * CHUNK)
        x[c * CHUNK:c * CHUNK + size] = torch.tensor(bad, dtype=torch.int64).repeat(size // 4 + 1)[:size].to(torch.int32)
        out.append(("one_chunk_invalid", x))
    out.append(("all_invalid", torch.tensor(bad, dtype=torch.int64).repeat(n // 4 + 1)[:n].to(torch.int32)))
    return out


# ------------------------------------------------------------------------------------------------------------ the combines
PLAIN_H, PLAIN_TOPK, PLAIN_T = [1, 7, 255, 256, 257, 1000], [1, 3, 8], [1, 5]
SORTED_H = [8, 248, 2040, 2048, 2056, 4104]        # one sweep is 256 threads x 8 = 2048: part of one, one, one and a bit, two and a bit
SORTED_TOPK = [1, 2, 7, 8, 9, 16]                  # 8: the HOIST8 instantiation
LOCAL_N = [1, 255, 256, 257, 600]                  # 256 threads sum the local sizes: one stride, one and a bit, two and a bit


def combine_inputs(T, topk, H, dtype, seed):
    """rows [T * topk, H] in `dtype`, weights f32 [T, topk] with negatives and exact zeros"""
    g = torch.Generator().manual_seed(seed)
    rows = (torch.randn(T * topk, H, generator=g) * 2).to(dtype)
    w = torch.randn(T, topk, generator=g)
    w[torch.rand(T, topk, generator=g) < 0.15] = 0.0
    w[0, 0] = -0.75
    if T > 1:
        w[1, topk - 1] = 0.0
    return rows, w


def sorted_inputs(T, topk, H, dtype, seed, skips=True):
    """the same rows scattered to a sorted order: sorted[src_dst[i]] = rows[i]. skips: token 1 loses k = 0, token 2 loses
    k = topk - 1, token 3 loses every row (src_dst = -1; the sorted row they would have had is filled with NaN)"""
    rows, w = combine_inputs(T, topk, H, dtype, seed)
    g = torch.Generator().manual_seed(seed + 1)
    N = T * topk
    src_dst = torch.randperm(N, generator=g).to(torch.int32)
    srt = torch.empty_like(rows)
    srt[src_dst.long()] = rows
    if skips:
        gone = []
        if T > 1:
            gone.append(1 * topk)
        if T > 2:
            gone.append(2 * topk + topk - 1)
        if T > 3:
            gone += list(range(3 * topk, 4 * topk))
        for i in gone:
            srt[int(src_dst[i])] = math.nan
            src_dst[i] = -1
    return srt, src_dst, w


def local_sizes(n_local, nv, seed):
    """int32 [n_local] that sums to nv (zeros allowed: n_local may exceed nv)"""
    g = torch.Generator().manual_seed(seed)
    sizes = torch.bincount(torch.randint(0, n_local, (nv,), generator=g), minlength=n_local).to(torch.int32)
    assert int(sizes.sum()) == nv and sizes.numel() == n_local
    return sizes


def poison(srt, nv):
    """rows at or past nv are what the real layer leaves uninitialised: NaN and +-Inf"""
    out = srt.clone()
    n = out.size(0) - nv
    if n > 0:
        fill = torch.tensor([math.nan, math.inf, -math.inf]).repeat(n * out.size(1) // 3 + 1)[:n * out.size(1)]
        out[nv:] = fill.view(n, out.size(1)).to(out.dtype)
    return out
