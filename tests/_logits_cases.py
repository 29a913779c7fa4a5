"""Case tables and a dense float64 reference for the top-k / top-p tests (tests/test_logits_reference.py on the CPU,
tests/test_gpu_logits_processors.py on the GPU).

top_k_top_p_kernel (xllm_amd/csrc/logits_processors.hip) picks its code path from (dtype, V, row base address, pitch) alone:
a row takes the VECTOR final pass and a sweep without head / tail loops when it starts on a 16-byte boundary and holds a whole
number of 16-byte vectors, and the SCALAR final pass (one column per lane) otherwise. arm() restates the two conditions; every
case names the arm it is in the table for and the GPU tests assert it from the tensor's real address before they launch.

ref64() is the operation itself in float64: stable descending sort (ties by column index), top-k, exp(x - max), one cumulative
sum, the rule's prefix against p * Z. It sees the values the kernel sees (scaled(): x / t in fp32, rounded to the tensor dtype).

Where p sits decides the bar. A "clear" row has p on the midpoint of two adjacent float64 prefixes that are >= MIN_GAP apart
(asserted here, when the case is built), or at a value no prefix can be near (p <= 0, 1e-30, p >= 1): the surviving set must EQUAL
float64's. A "step" row has p on the fp32 value nearest a float64 prefix, or one of its two fp32 neighbours: the surviving set
must be a prefix of the stable sorted order, and every rank on which it disagrees with float64 must have its prefix within BAND
of p (the band of tests/test_gpu_parity.py::_mask_mismatch_is_a_boundary_case, held for EVERY disagreeing rank here).

One row kind is outside the fp32 oracle's reach: p < 0 under the one-of-them rule. The reference's expression
(cumsum - probs > p) masks rank 0 as well and leaves a row without a finite logit; the kernel keeps rank 0 (the row stays
sampleable), and so does ref64. Those rows carry quirk = True: the kernel is held to ref64, the oracle to what it does.
And p = 1.0 is "clear" for the kernel only (`p >= 1` keeps the top-k set by construction); for the oracle it sits on the last
prefix, which an fp32 cumsum can overshoot, so check_rows(oracle=True) holds those rows to the "step" bar."""
import collections
import functools

import numpy as np
import torch

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
NAME = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
SIZE = {torch.float32: 4, torch.bfloat16: 2, torch.float16: 2}
WAVES = 16           # kLpWaves
BAND = 2e-5          # |prefix - p| a disagreeing rank may have on a "step" row
MIN_GAP = 1e-4       # smallest distance of the two prefixes a "clear" p sits between
SENTINEL = 7.0       # pad columns of a pitched tensor

Ref = collections.namedtuple("Ref", "keep prefix order kk n")
Layout = collections.namedtuple("Layout", "off pitch")            # first column of the view inside the wide tensor, row pitch
Launch = collections.namedtuple("Launch", "name rows temps k p kinds quirk scaled refs")
Case = collections.namedtuple("Case", "mech dtype V layout expect launches")


# --------------------------------------------------------------------------------------------------- the kernel's arms
def arm(dtype, V, first_row_byte_offset, pitch, rows=1):
    """'vector' / 'scalar' per row: the kernel's `v_head == 0 && v_n * VEC == V` (v_head: columns before the first 16-byte
    boundary; v_n: whole vectors after it). first_row_byte_offset: address of row 0 modulo 16; pitch in elements."""
    size = SIZE[dtype]
    vec = 16 // size
    out = []
    for b in range(rows):
        addr = first_row_byte_offset + b * pitch * size
        v_head = min(((16 - addr % 16) % 16) // size, V)
        v_n = (V - v_head) // vec
        out.append("vector" if v_head == 0 and v_n * vec == V else "scalar")
    return out


def segment(dtype, V, arm_):
    """(seg, step): columns per wave and per step of the final pass, as the kernel computes them"""
    step = 64 * (16 // SIZE[dtype]) if arm_ == "vector" else 64
    per_wave = (V + WAVES - 1) // WAVES
    return (per_wave + step - 1) // step * step, step


def seams(dtype, V, arm_):
    """[(name, c)]: column pairs (c, c + 1) across which a tie's rank is assembled from different terms. All in or next to wave 1,
    so that every rank also carries wave 0's count."""
    seg, step = segment(dtype, V, arm_)
    out = []
    if arm_ == "vector":
        vec = 16 // SIZE[dtype]
        out += [("in_lane", seg + 5 * vec + 1), ("lane", seg + 21 * vec - 1)]     # inside lane 5's vector; lane 20 | lane 21
    else:
        out += [("lane", seg + 20), ("wave2", 2 * seg - 1)]
    out.append(("wave", seg - 1))                                                    # wave 0's last column | wave 1's first
    if seg > step:
        out.append(("step", seg + step - 1))                                         # lane 63 of a step | lane 0 of the next
    assert all(3 < c - 1 and c + 2 < V - 2 for _, c in out)
    return out


# ------------------------------------------------------------------------------------------------ the float64 reference
def rule_of(k, p):
    return "both" if k is not None and p is not None else "one"


def scaled(rows, temps):
    """what the kernel ranks and writes back: x / t in fp32 (t = 0 means 1), rounded to the tensor dtype"""
    if temps is None:
        return rows.clone()
    t = torch.where(temps == 0, torch.ones_like(temps), temps).float()
    return (rows.float() / t[:, None]).to(rows.dtype)


def ref64(row, k, p, rule):
    """row: 1-D tensor of the values as the kernel sees them. k, p: numbers or None. rule: 'one' (exclusive prefix E_i <= p * Z)
    or 'both' (rank 0, and rank i > 0 iff E_i + m_i <= p * Z). Returns the keep-mask by column, the rule's normalised prefix by
    rank (inf past the top-k set), the stable descending order, the size of the top-k set and the number of survivors."""
    x = row.detach().double().numpy()
    V = x.size
    order = np.argsort(-x, kind="stable")
    kk = V if (k is None or k <= 0 or k > V) else int(k)
    xs = x[order]
    m = np.exp(xs - xs[0])
    m[kk:] = 0.0
    cum = np.cumsum(m)
    Z = cum[kk - 1]
    pref = cum - m if rule == "one" else cum
    keep_r = np.zeros(V, dtype=bool)
    if p is None:
        keep_r[:kk] = True
    else:
        keep_r[:kk] = pref[:kk] <= float(np.float32(p)) * Z
        keep_r[0] = True
    n = int(keep_r.sum())
    assert keep_r[:n].all()                                  # (the prefix is monotone: the survivors are a prefix of the order)
    keep = np.zeros(V, dtype=bool)
    keep[order[:n]] = True
    prefix = pref / Z
    prefix[kk:] = np.inf
    return Ref(torch.from_numpy(keep), prefix, order, kk, n)


def clear_p(row, k, rule, last_kept, walk=False):
    """p on the midpoint of the prefixes of ranks last_kept and last_kept + 1 (the survivors are ranks 0 .. last_kept); the two
    must be MIN_GAP apart. walk: step towards rank 0 until they are (random rows: the masses grow that way)."""
    pre = ref64(row, k, None, rule).prefix
    c = last_kept
    while walk and c > 0 and not pre[c + 1] - pre[c] >= MIN_GAP:
        c -= 1
    assert pre[c + 1] - pre[c] >= MIN_GAP, (c, pre[c], pre[c + 1])
    return float(np.float32((pre[c] + pre[c + 1]) / 2)), c


def step_ps(row, k, rule, rank):
    """the fp32 value nearest the rule's prefix of `rank`, and its two fp32 neighbours"""
    p0 = np.float32(ref64(row, k, None, rule).prefix[rank])
    return [float(np.nextafter(p0, np.float32(0))), float(p0), float(np.nextafter(p0, np.float32(2)))]


def check_rows(got, launch, who, oracle=False):
    """got: [B, V] in the launch's dtype. Holds every row to its bar against float64; returns the largest |prefix - p| seen on a
    disagreeing rank of a 'step' row (0.0 when there was none). oracle: `got` is the fp32 oracle's output, whose quirk rows
    (module docstring) are held to what the reference's expression does: every column masked."""
    worst = 0.0
    masked = torch.isinf(got) & (got < 0)
    assert torch.equal(got[~masked], launch.scaled[~masked]), f"{who} {launch.name}: a surviving value changed"
    for b, (kind, ref) in enumerate(zip(launch.kinds, launch.refs)):
        keep = ~masked[b]
        n_got = int(keep.sum())
        tag = (who, launch.name, b, n_got, ref.n)
        if oracle and launch.quirk[b]:
            assert n_got == 0, tag
            continue
        if oracle and launch.p is not None and float(launch.p[b]) == 1.0:
            kind = "step"           # the last prefix IS 1: an fp32 cumsum may end above it; the kernel's `p >= 1` cannot
        assert n_got >= 1 and bool(keep[ref.order[0]]), tag                       # rank 0 always survives
        if kind == "clear":
            assert torch.equal(keep, ref.keep), tag
            continue
        assert bool(keep[torch.from_numpy(ref.order[:n_got].copy())].all()) and n_got <= ref.kk, tag   # a prefix of the order
        if n_got != ref.n:
            lo, hi = min(n_got, ref.n), max(n_got, ref.n)
            off = float(np.abs(ref.prefix[lo:hi] - float(launch.p[b])).max())
            worst = max(worst, off)
            assert off <= BAND, tag + (off,)
    return worst


# ------------------------------------------------------------------------------------------------------------ the rows
TEMPS = [1.0, 0.7, 0.0, 1.3, 2.0, 0.5, 0.9, 1.1]
EDGE_P = [0.0, 1e-30, 1.0, 1.5, -0.5]


def edge_k(V):
    return [1, 2, V - 1, V, V + 5, 0, -1]


def _launch(name, rows, temps, k, p, kinds=None):
    B = rows.size(0)
    temps = None if temps is None else torch.tensor(temps, dtype=torch.float32)
    k = None if k is None else torch.tensor(k, dtype=torch.int64)
    p = None if p is None else torch.tensor(p, dtype=torch.float32)
    sc = scaled(rows, temps)
    rule = rule_of(k, p)
    refs = [ref64(sc[b], None if k is None else int(k[b]), None if p is None else float(p[b]), rule) for b in range(B)]
    kinds = kinds or ["clear"] * B
    quirk = [rule == "one" and p is not None and float(p[b]) < 0 for b in range(B)]
    assert len(kinds) == B and all(x is None or x.numel() == B for x in (temps, k, p))
    return Launch(name, rows, temps, k, p, kinds, quirk, sc, refs)


def _random_rows(g, B, V, dtype, mean=0.0):
    return (torch.randn(B, V, generator=g) * 2.5 + mean).to(dtype)


def _clear_launches(g, V, dtype):
    """random rows under a temperature; k in {none, 1, 17, 300, V}, p between the prefixes of ranks 1, 5, 40, 250"""
    ranks = [1, 5, 40, 250]
    out = []
    rows = _random_rows(g, 4, V, dtype)
    out.append(_launch("clear/k", rows, TEMPS[:4], [1, 17, 300, V], None))
    rows = _random_rows(g, 4, V, dtype)
    sc = scaled(rows, torch.tensor(TEMPS[4:8]))
    out.append(_launch("clear/p", rows, TEMPS[4:8], None, [clear_p(sc[i], None, "one", r, walk=True)[0] for i, r in enumerate(ranks)]))
    ks, cs = [1], [0]
    for k in (17, 300, V):
        for r in ranks:
            if r + 1 < k:
                ks.append(k)
                cs.append(r)
    rows = _random_rows(g, len(ks), V, dtype)
    temps = [TEMPS[i % 8] for i in range(len(ks))]
    sc = scaled(rows, torch.tensor(temps))
    ps = [0.5] + [clear_p(sc[i], ks[i], "both", cs[i], walk=True)[0] for i in range(1, len(ks))]      # k = 1: one rank, any p
    out.append(_launch("clear/both", rows, temps, ks, ps))
    return out


def _tie_value(V):
    return 2.5 if V < 20000 else 4.0       # exp(t) / Z >= MIN_GAP over a row of V standard normals (asserted by clear_p)


def _tie_row(g, V, dtype, cols, t):
    x = torch.randn(V, generator=g).to(dtype)
    x[x == t] = t - 1.0                     # the group is the only place the value occurs
    x[cols] = t
    return x, int((x > t).sum())


def _tie_launches(g, V, dtype, arms, n_rows=8):
    """the boundary value is shared by a group of columns that straddles a seam of the final pass; the cut leaves exactly the
    columns up to the seam (even rows), then one more (odd rows); as the top-k boundary, as the top-p boundary, as both"""
    t = _tie_value(V)
    rows, ks, ps, kb, pb = [], [], [], [], []
    for b in range(n_rows):
        sm = seams(dtype, V, arms[b % len(arms)])
        _, c = sm[(b // 2) % len(sm)]
        cols = sorted({3, c - 1, c, c + 1, c + 2, V - 2})
        assert len(cols) >= 6
        x, G = _tie_row(g, V, dtype, cols, t)
        r = cols.index(c) + 1 + (b & 1)     # ties that survive
        rows.append(x)
        ks.append(G + r)
        ps.append(clear_p(x, None, "one", G + r - 1)[0])
        kb.append(G + r + 1)                # top-k keeps one tie more than top-p then does
        pb.append(clear_p(x, G + r + 1, "both", G + r - 1)[0])
    rows = torch.stack(rows)
    out = [_launch("tie/k", rows, None, ks, None), _launch("tie/p", rows, None, None, ps), _launch("tie/both", rows, None, kb, pb)]
    for L, keep in zip(out, (ks, ks, ks)):
        assert [ref.n for ref in L.refs] == keep                                   # the cut is where the builder put it
        for b, ref in enumerate(L.refs):
            assert float(rows[b][ref.order[ref.n - 1]]) == t and float(rows[b][ref.order[ref.n]]) == t
    return out


def _negative_launches(g, V, dtype):
    """boundary keys of negative values: every value negative (top-k), a tail of negative values that p = 0.999 cuts into"""
    rows = _random_rows(g, 3, V, dtype, mean=-6.0).clamp(max=-0.25)
    k = [5, 17, 300]
    out = [_launch("neg/k", rows, None, k, None)]
    head = torch.tensor([3.0, 2.75, 2.5, 3.25, 2.25])
    tail = -0.5 - torch.rand(200, generator=g)                                      # (-1.5, -0.5]
    x = -30.0 + 0.25 * torch.randn(2, V, generator=g)                               # the rest: no mass in 2^-40 fixed point
    perm = torch.randperm(V, generator=g)
    x[:, perm[:5]] = head
    x[:, perm[5:205]] = tail
    x = x.to(dtype)
    cut = int(np.searchsorted(ref64(x[0], None, None, "one").prefix, 0.999)) - 1    # last rank whose exclusive prefix is < 0.999
    out.append(_launch("neg/p", x[:1], None, None, [clear_p(x[0], None, "one", cut, walk=True)[0]]))
    cutb = int(np.searchsorted(ref64(x[1], 150, None, "both").prefix, 0.999)) - 1
    out.append(_launch("neg/both", x[1:], None, [150], [clear_p(x[1], 150, "both", cutb, walk=True)[0]]))
    for L in out:
        for b, ref in enumerate(L.refs):
            assert float(L.scaled[b][ref.order[ref.n - 1]]) < 0 and float(L.scaled[b][ref.order[min(ref.kk, V) - 1]]) < 0
    return out


def _edge_launches(g, V, dtype):
    """k in {1, 2, V - 1, V, V + 5, 0, -1} x p in {0, 1e-30, 1, 1.5, -0.5}; the last rows of each launch have their second-largest
    logit about 40 below the maximum (its mass in 2^-40 fixed point is 0)"""
    ks = edge_k(V)

    def rows_for(n, far):
        rows = _random_rows(g, n + far, V, dtype)
        rows[n:] = torch.randn(far, V, generator=g).to(dtype)
        rows[n:, V // 3] = 45.0
        return rows
    out = [_launch("edge/k", rows_for(len(ks), 1), None, ks + [3], None)]
    out.append(_launch("edge/p", rows_for(len(EDGE_P), 2), None, None, EDGE_P + [0.5, 1.0]))
    kk, pp = [k for k in ks for _ in EDGE_P], [p for _ in ks for p in EDGE_P]
    out.append(_launch("edge/both", rows_for(len(kk), 3), None, kk + [5, 5, -1], pp + [0.5, 1.0, 0.5]))
    for L in out[1:]:
        for b, ref in enumerate(L.refs):
            p = float(L.p[b])
            if p >= 1.0:
                assert ref.n == ref.kk
            if p <= 1e-30:
                assert ref.n == 1 and int(ref.order[0]) == int(L.scaled[b].float().argmax())
    return out


def _step_launches(g, V, dtype):
    """p on a float64 prefix (the fp32 value nearest to it) and on its two fp32 neighbours"""
    ranks = [1, 5, 40]
    rows = _random_rows(g, 3, V, dtype).repeat_interleave(3, 0)
    temps = [TEMPS[i // 3] for i in range(9)]
    sc = scaled(rows, torch.tensor(temps))
    ps = [step_ps(sc[3 * i], None, "one", r)[j] for i, r in enumerate(ranks) for j in range(3)]
    out = [_launch("step/p", rows, temps, None, ps, ["step"] * 9)]
    rows = _random_rows(g, 3, V, dtype).repeat_interleave(3, 0)
    ks = [17] * 3 + [300] * 6
    ps = [step_ps(rows[3 * i], ks[3 * i], "both", r)[j] for i, r in enumerate(ranks) for j in range(3)]
    out.append(_launch("step/both", rows, None, ks, ps, ["step"] * 9))
    return out


def _model_vocab_launches(g, V, dtype):
    """8 rows at the model's vocabulary (19 sweep iterations, 19 steps per wave): a tie group on the step seam and on the wave seam,
    a negative k-th key, clear and on-the-step cuts"""
    t = _tie_value(V)
    sm = dict(seams(dtype, V, "vector"))
    out = []
    rows, ks = [], []
    for name in ("step", "wave"):
        c = sm[name]
        cols = sorted({3, c - 1, c, c + 1, c + 2, V - 2})
        x, G = _tie_row(g, V, dtype, cols, t)
        rows.append(x)
        ks.append(G + cols.index(c) + 1)
    neg = _random_rows(g, 1, V, dtype, mean=-12.0).clamp(max=-0.25)[0]
    out.append(_launch("vocab/k", torch.stack(rows + [neg]), None, ks + [300], None))
    assert float(neg[out[-1].refs[2].order[299]]) < 0
    r = _random_rows(g, 2, V, dtype)
    out.append(_launch("vocab/p", torch.stack([rows[1], r[0], r[1]]), None, None,
                       [clear_p(rows[1], None, "one", ks[1] - 1)[0], clear_p(r[0], None, "one", 40, walk=True)[0],
                        step_ps(r[1], None, "one", 5)[1]], ["clear", "clear", "step"]))
    out.append(_launch("vocab/both", torch.stack([rows[0], r[0]]), None, [ks[0] + 1, 300],
                       [clear_p(rows[0], ks[0] + 1, "both", ks[0] - 1)[0], clear_p(r[0], 300, "both", 40, walk=True)[0]]))
    assert sum(L.rows.size(0) for L in out) == 8
    return out


# ------------------------------------------------------------------------------------------------------------ the table
def mechanisms(dtype):
    """(name, V, layout, arm): the smallest shapes at which each mechanism of the kernel runs"""
    wide = SIZE[dtype] == 4
    multi = 8448 if wide else 16896                       # > 16 waves x STEP columns: 3 steps per wave, 3 sweep iterations
    out = [("vector_one_step", 1000, Layout(0, 1000), "vector"),
           ("vector_multi_step", multi, Layout(0, multi), "vector"),
           ("scalar_tail", 1003, Layout(0, 1003), "scalar"),                        # V is not a whole number of vectors
           ("scalar_multi_step", 4099, Layout(0, 4099), "scalar"),                  # ... with 5 steps per wave
           ("scalar_head", 1000, Layout(1, 1008), "scalar"),                        # wide[:, 1:1001]: every row starts off a boundary
           ("mixed_pitch", 1000, Layout(0, 1003 if wide else 1004), "mixed"),       # rows 0, 4, 8 / the even rows stay aligned
           ("pitched_vector", 1000, Layout(0, 1004 if wide else 1008), "vector")]
    if dtype == torch.bfloat16:
        out.append(("model_vocab", 152064, Layout(0, 152064), "vector"))
    return out


CASE_KEYS = [(m[0], dt) for dt in DTYPES for m in mechanisms(dt)]
CASE_IDS = [f"{m}-{NAME[dt]}" for m, dt in CASE_KEYS]


@functools.lru_cache(maxsize=None)
def case(mech, dtype):
    name, V, layout, expect = next(m for m in mechanisms(dtype) if m[0] == mech)
    g = torch.Generator().manual_seed(1000 * DTYPES.index(dtype) + [m[0] for m in mechanisms(torch.bfloat16)].index(mech))
    if mech == "model_vocab":
        return Case(mech, dtype, V, layout, expect, _model_vocab_launches(g, V, dtype))
    arms = arm(dtype, V, layout.off * SIZE[dtype], layout.pitch, rows=8)
    launches = (_clear_launches(g, V, dtype) + _tie_launches(g, V, dtype, arms) + _negative_launches(g, V, dtype)
                + _edge_launches(g, V, dtype) + _step_launches(g, V, dtype))
    return Case(mech, dtype, V, layout, expect, launches)


def expected_arms(c, rows):
    return arm(c.dtype, c.V, c.layout.off * SIZE[c.dtype], c.layout.pitch, rows)


def arms_match(arms, expect):
    return set(arms) == ({"vector", "scalar"} if expect == "mixed" else {expect})
