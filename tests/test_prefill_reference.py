"""CPU: the oracle's prefill / chunked-prefill attention against a dense float64 restatement, on the inputs of every case that
tests/test_gpu_prefill_masks.py runs on the GPU (tests/_prefill_cases.py), and the properties of those inputs the GPU tests
rely on.

  * The oracle (attention_varlen / paged_attention) in its three modes -- fp32 P, p_round=True, "flash" -- is finite on every
    asserted row although K is NaN and V Inf wherever a call is not entitled to read, gives exact zeros on rows that see no
    key, and agrees with an implementation that shares no code with it:
      - fp32 P vs float64 rounded to the dtype: relative L2 per sequence within HALF of the hi + lo bar (1e-3 bf16, 2e-4 f16);
        element-wise within half a bar for f16 and within ONE bar for bf16 -- the element-wise bar is 2^-7 of the token's
        maximum, which is exactly one bf16 ulp of an element just above a power of two, so two correctly rounded references may
        sit a whole bar apart on one element and no test can ask for less;
      - per (query, head) row, the oracle in the mode that matches the kernel's P form stays within ROW_MEASURED = half of the
        row bar the GPU test asserts (the constants are re-measured here: a table change that moves them fails this test);
      - the "flash" mode, put in the kernel's place, passes assert_p16_attention_close against (float64, p_round=True). Its
        bars are multiples of e_ref, the distance between those two references, so "half a bar" has no meaning for them: the
        flash mode uses 0.86 of the float64 bar and 0.72 of the p_round bar at most (bf16; f16: 0.36, 0.47).
  * Sensitivity: on every mask-edge case, moving ONE edge by ONE key (causal +- 1, window +- 1, kv_len - 1) moves every row the
    edge touches by more than twice the loosest row bar. That is what makes the row bar a test of the masks.
  * The rescale cases do what they claim: jump sizes in their ranges, and >= 0.05 of the probability mass in front of the jump
    and of each of the staircase's three jumps, so that a wrong rescale factor shows.
  * The tables reach every arm, every window (each binding at least one row), every length edge and every block-coordinate form."""
import collections

import pytest
import torch

import _prefill_cases as pc
from _bars import assert_p16_attention_close

CASES = pc.all_cases()
_MAX = collections.defaultdict(float)


def _note(k, v, name):
    if v > _MAX[k]:
        _MAX[k] = v
        _MAX[k + ("at",)] = name


_SEEN = set()


@pytest.mark.parametrize("name,kind,build", CASES, ids=[c[0] for c in CASES])
def test_oracle_prefill_equals_dense_float64(name, kind, build):
    _check_case(name, build)


def _check_case(name, build):
    _SEEN.add(name)
    key, c = build()
    r = pc.references(c, key)
    dt, nq, d = c["dtype"], c["nq"], c["arm"].d
    rows = pc.asserted_rows(c)
    assert r["r64r"].shape == (int(c["cu_q"][-1]), nq * d) and torch.isfinite(r["r64"][rows]).all()
    blind = torch.isnan(pc.row_distances(r["r64r"], r["r64r"], nq)) & rows.view(-1, 1)
    for mode in ("fp32", "p16", "flash"):
        assert r[mode].shape == r["r64r"].shape and torch.isfinite(r[mode][rows].float()).all(), (key, mode)
        assert not r[mode].view(-1, nq, d)[blind].any(), (key, mode)            # rows that see no key: exact zeros
        rd = pc.row_distances(r[mode], r["r64r"], nq)
        rd = rd[rows.view(-1, 1) & ~torch.isnan(rd)]
        if mode != "p16" or c["arm"].name.startswith("m32"):                  # one 16-bit P only ever runs on the m32 arms
            _note((pc.DTNAME[dt], mode, "row"), float(rd.max()), name)
        if mode == "fp32":
            assert float(rd.max()) <= pc.ROW_MEASURED[("hilo", dt)], (key, float(rd.max()))
        if mode == "p16" and c["arm"].name.startswith("m32"):
            assert float(rd.max()) <= pc.ROW_MEASURED[("p16", dt)], (key, float(rd.max()))
    for b in c["assert_seqs"]:
        sl = slice(int(c["cu_q"][b]), int(c["cu_q"][b + 1]))
        rel, elem = pc.distance(r["fp32"][sl], r["r64r"][sl])
        _note((pc.DTNAME[dt], "fp32", "rel"), rel, name)
        _note((pc.DTNAME[dt], "fp32", "elem"), elem, name)
        assert rel <= 0.5 * pc.BAR_REL[dt], (key, b, rel)
        assert elem <= (1.0 if dt == torch.bfloat16 else 0.5), (key, b, elem)
        if c["arm"].name.startswith("m32"):
            assert_p16_attention_close(r["flash"][sl], r["r64r"][sl], r["p16"][sl])
            e = pc.rel_l2(r["p16"][sl], r["r64r"][sl])
            _note((pc.DTNAME[dt], "flash", "of the float64 bar"), pc.rel_l2(r["flash"][sl], r["r64r"][sl]) / max(1e-3, 1.25 * e), name)
            _note((pc.DTNAME[dt], "flash", "of the p_round bar"), pc.rel_l2(r["flash"][sl], r["p16"][sl]) / max(1e-3, 2 * e), name)


def test_row_bars_are_twice_the_measured_oracle_distance():
    """prints the largest distances per dtype and mode and holds the constants of _prefill_cases.py to them: no smaller
    (asserted per case above) and no more than 2 % larger. (After the parametrised test above, in file order, every reference
    is already cached; alone it computes them.)"""
    for name, _, build in CASES:
        if name not in _SEEN:
            _check_case(name, build)
    for k in sorted(k for k in _MAX if k[-1] != "at"):
        print(f"{k}: {_MAX[k]:.4e} at {_MAX[k + ('at',)]}")
    assert pc.N_CASES == len(CASES)
    for form, mode in pc.ORACLE_MODE.items():
        for dt in pc.DTYPES:
            got = _MAX[(pc.DTNAME[dt], mode, "row")]
            assert got <= pc.ROW_MEASURED[(form, dt)] <= 1.02 * got, (form, dt, got)
            assert pc.ROW_BAR[(form, dt)] == 2.0 * pc.ROW_MEASURED[(form, dt)]


MASK_CASES = [c for c in CASES if c[1] == "mask"]


@pytest.mark.parametrize("name,kind,build", MASK_CASES, ids=[c[0] for c in MASK_CASES])
def test_one_key_moves_every_touched_row_beyond_the_row_bar(name, kind, build):
    key, c = build()
    r64 = pc.references(c, key)["r64"]
    need = 2.0 * max(v for (form, dt), v in pc.ROW_BAR.items() if dt == c["dtype"])
    nq = c["nq"]
    touched_any = 0
    for shift in (dict(causal_shift=1), dict(causal_shift=-1), dict(window_shift=1), dict(window_shift=-1), dict(kv_shift=-1)):
        if ("causal_shift" in shift and not c["causal"]) or ("window_shift" in shift and c["window_left"] < 0):
            continue
        moved = pc.dense_prefill_ref64(c, **shift)
        for b, (ql, kv) in enumerate(c["seqs"]):
            if ql == 0 or kv == 0:
                continue
            sl = slice(int(c["cu_q"][b]), int(c["cu_q"][b + 1]))
            touched = (pc.visibility(ql, kv, c["causal"], c["window_left"]) !=
                       pc.visibility(ql, kv, c["causal"], c["window_left"], **shift)).any(1)
            if not touched.any():
                continue
            a, m = r64[sl].view(ql, nq, -1)[touched], moved[sl].view(ql, nq, -1)[touched]
            base = torch.maximum(a.norm(dim=-1), m.norm(dim=-1))            # (one of the two may be a zero row)
            dist = (a - m).norm(dim=-1) / base
            touched_any += int(touched.sum())
            _note((pc.DTNAME[c["dtype"]], "smallest one-key shift", "inv"), 1.0 / float(dist.min()), name)
            assert float(dist.min()) > need, (key, shift, b, float(dist.min()), need)
    assert touched_any > 0


def test_smallest_one_key_shift():
    for dt in pc.DTYPES:
        k = (pc.DTNAME[dt], "smallest one-key shift", "inv")
        if k in _MAX:
            print(f"{pc.DTNAME[dt]}: smallest shift of a touched row {1.0 / _MAX[k]:.3e} at {_MAX[k + ('at',)]}")


def _scores_log2(c, b, h):
    """float64 scaled scores of (sequence b, q head h) in log2 units, [q_len, kv_len], and the visibility mask"""
    ql, kv = c["seqs"][b]
    k, _ = pc.gather_keys(c, b)
    q0 = int(c["cu_q"][b])
    s = c["q"][q0:q0 + ql, h].double() @ k[:, h // (c["nq"] // c["nkv"])].double().T * c["scale"] * 1.4426950408889634
    return s, pc.visibility(ql, kv, c["causal"], c["window_left"])


@pytest.mark.parametrize("dtype", pc.DTYPES, ids=list(pc.DTNAME.values()))
@pytest.mark.parametrize("arm", pc.M32_ARMS + [pc.STAGED_CONTROL], ids=lambda a: a.name)
def test_rescale_cases_do_what_they_claim(arm, dtype):
    """from float64 scores. jump: the key at 208 (>= 128: two m32 tiles accumulated; middle of the wave of queries 192 ... 223
    resp. 32 ... 63, so under the causal mask half of that wave's lanes rescale and half keep alpha == 1) exceeds every earlier
    key of every row that sees it by 9 ... 14 log2 units, and the keys before it keep >= 0.05 of the mass of every such row.
    near_miss: 6 ... 7.5 units, below the 2^8 threshold. staircase: three levels in three successive 64-key tiles, each 9 ... 14
    above everything before it, forty keys on each of the first two; the row AT a level's first key (under the causal mask it
    sees none of that level's other keys) keeps >= 0.05 of its mass in front of that key, at all three jumps -- so a wrong
    alpha at the second or third successive rescale moves that row by a multiple of the row bar."""
    lo_hi = {"jump": (9.0, 14.0), "near_miss": (6.0, 7.5), "staircase": (9.0, 14.0)}
    for kind, spikes in pc.RESCALE.items():
        key, c = pc.rescale_case(arm, kind, dtype)
        levels = sorted(set(spikes.values()))
        first = {lv: min(j for j, v in spikes.items() if v == lv) for lv in levels}
        assert min(spikes) >= 128 and len({j // 64 for j in first.values()}) == len(levels)
        assert all(j % 32 == 16 for j in first.values())
        for b, (ql, kv) in enumerate(c["seqs"]):
            for h in range(c["nq"]):
                s, vis = _scores_log2(c, b, h)
                p = torch.softmax(s.masked_fill(~vis, float("-inf")) * 0.6931471805599453, -1)      # s is in log2 units
                for li, lv in enumerate(levels):
                    j = first[lv]
                    sees = vis[:, j]
                    assert sees.any() and not sees.all()
                    jump = s[sees, j] - s[sees, :j].masked_fill(~vis[sees, :j], float("-inf")).amax(-1)
                    assert lo_hi[kind][0] <= float(jump.min()) and float(jump.max()) <= lo_hi[kind][1], (key, b, h, lv, jump.min(), jump.max())
                    if kind == "near_miss":
                        continue
                    if kind == "staircase":              # the row whose newest key is the level's first one
                        at = torch.zeros_like(sees)
                        at[j - (kv - ql)] = True
                        assert sees[j - (kv - ql)] and (j + 1 >= kv or not vis[j - (kv - ql), j + 1])
                    else:
                        at = sees
                    before = p[at, :j].sum(-1)
                    assert float(before.min()) >= 0.05, (key, b, h, lv, float(before.min()))


def test_tables_reach_every_arm_window_and_length():
    seen_arms = set()
    for a in pc.ARMS:
        pitch = 2 * a.d if a.paged else (4 + 2 * 2) * a.d
        assert pc.arm_of(a.d, a.paged, a.bs, pitch) == a.name
        seen_arms.add(a.name)
    assert pc.arm_of(128, False, 0, pc.WIDE_PITCH) == "staged_wide_pitch" and pc.arm_of(128, False, 0, pc.WIDE_PITCH - 8) == "m32_unpaged"
    assert pc.arm_of(128, True, 128, 256) == "m32_paged"
    assert len(seen_arms) == 5
    assert {W for _, W in pc.MASKS} == set(pc.WINDOWS) and {c for c, _ in pc.MASKS} == {0, 1}
    qls, offs, kvs = {q for q, _ in pc.SEQS}, {kv - q for q, kv in pc.SEQS if q}, {kv for _, kv in pc.SEQS}
    assert {0, 1, 31, 32, 33, 64, 65, 127, 128, 129, 257} <= qls
    assert {0, 1, 31, 63, 64, 65, 200} <= offs
    assert {63, 64, 65, 127, 128, 129} <= kvs and max(kvs) <= 330
    assert pc.SEQS[len(pc.SEQS) // 2][0] == 0                                  # the empty sequence sits in the middle
    assert {kv - q for q, kv in pc.SEQS_SHORT_KV} == {-10, 0, -1}
    # every binding W hides at least one key from at least one row, under the causal mask (lower edge) on every arm's lengths
    for causal, W in pc.MASKS:
        if 0 <= W < 2 ** 30:
            bound = sum(int((pc.visibility(q, kv, causal, W) != pc.visibility(q, kv, causal, -1)).any(1).sum()) for q, kv in pc.SEQS if q)
            assert bound > 0, (causal, W)
    assert {n * nkv for n, _, nkv in pc.PFORMS} == {1, 2, 3, 4, 8, 10}
    assert {nq // nkv for nq, nkv in pc.HEADS} == {1, 2, 7}
    # poison table: a poisoned page inside the edge tile of the 32-key kernel, and a control without
    lows = [kv - q - 100 for q, kv in pc.POISON_SEQS if q]
    assert any(lo > 0 and lo % 32 >= 16 for lo in lows) and any(lo > 0 and lo % 32 < 16 for lo in lows)
    ids = [c[0] for c in CASES]
    assert len(ids) == len(set(ids)) and len(ids) <= 210


def test_the_poison_is_where_the_docstring_says():
    for arm in (pc.ARM["staged_paged_d128"], pc.ARM["m32_paged"]):
        key, c = pc.poison_case(arm, 0, torch.bfloat16)
        bs, W = arm.bs, c["window_left"]
        whole = 0
        for b, (ql, kv) in enumerate(c["seqs"]):
            npg = (kv + bs - 1) // bs
            assert torch.isnan(c["kc"][c["block_tables"][b, npg:].long()]).all()           # padding entries -> spare pages
            k, v = pc.gather_keys(c, b)
            lo = max(0, kv - ql - W) // bs * bs                                            # pages wholly below the lowest bound
            assert torch.isnan(k[:lo]).all() and torch.isinf(v[:lo]).all()
            assert torch.isfinite(k[lo:].float()).all() and torch.isfinite(v[lo:].float()).all()
            if kv % bs:
                last = int(c["block_tables"][b, npg - 1])
                assert torch.isnan(c["kc"][last, kv % bs:]).all() and torch.isinf(c["vc"][last, kv % bs:]).all()
            whole += lo // bs
        assert whole > 0
        live = set(int(x) for b, (_, kv) in enumerate(c["seqs"]) for x in c["block_tables"][b, :(kv + bs - 1) // bs])
        spare_or_dead = [i for i in range(c["kc"].shape[0]) if torch.isnan(c["kc"][i]).all()]
        assert len(spare_or_dead) >= 3 + whole
        assert 0 <= int(c["block_tables"].min()) and int(c["block_tables"].max()) < c["kc"].shape[0]
        assert live
    key, c = pc.neighbour_case(pc.ARM["m32_unpaged"], torch.float16)
    assert torch.isnan(c["k"][100:]).all() and torch.isinf(c["v"][100:]).all() and torch.isfinite(c["k"][:100].float()).all()
    assert c["assert_seqs"] == [0] and c["k"].shape[0] == 190 + 64
