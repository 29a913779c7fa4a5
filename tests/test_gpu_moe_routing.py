"""GPU: every arm and seam of xllm_amd/csrc/moe.hip -- the softmax / sigmoid gate, the grouped (DeepSeek) gate, the three-pass and
single-launch index build, the plain combine and the sorted / expert-parallel combine -- against the dense float64 restatements
of tests/_moe_cases.py (whose room to the fp32 C oracle tests/test_moe_reference.py measures on the CPU).

GATE (moe_fused_topk_kernel<T, PL>, PL = 1, 2, 4, 8; f32, bf16, f16). E in {1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511,
512} (both sides of every PL switch; 513 raises), T in {1, 2, 3, 4, 5, 37} (every remainder of the 4-token workgroup), topk in
{1, 8, min(E, 64)} (65 and topk > E raise), softmax | sigmoid | sigmoid + bias | sigmoid + (bias - 2) with E % 64 != 0 (every choice
score negative: only the -inf padding lanes are below them), renormalisation on and off. Inputs are placed on a grid
(_moe_cases: logits k / 16, biases k / 512), so every tie is exact; tie groups are placed across 63 | 64 (different lanes), on
0 | 64 | 128 (one lane, three slots), as a group of m with 1 and m - 1 places left at the k-th cut, on the last real expert, and as an
all-equal row; one case has -inf logits on a third of the experts. ids EQUAL float64's in order; weights are within (6e-6, 2e-7)
of float64 -- the project's GPU-vs-oracle bar (3e-6, 1e-7) plus the same allowance for the oracle -- and within (3e-6, 1e-7) of
the oracle. Logits at +-30 (sigmoid saturates to a tie in fp32, not in float64) are held to the oracle's ids only. Rows with fewer
than topk finite choice scores are out of scope: the oracle and the kernel both repeat an id there.

GROUPED GATE. (E, G) in {(64, 64) EG = 1 no bias, (128, 64) EG = 2 bias, (96, 3), (160, 8), (256, 8), (512, 64), (512, 2)},
topk_group in {1, middle, G}, topk in {1, 8, min(topk_group EG, 64)}, both scorings, bias with sigmoid, renormalisation on / off,
scale in {1, 2.5}, T in {3, 37}; placed rows (each property asserted in float64 by the builder): twin groups across the group cut,
the best expert's group losing on the top-2 sum, choice order != weight order, all-equal. Same bars; no id from a dropped group.

INDEX BUILD. Exact equality with index_ref over 34 (n, E) pairs x 9 distributions, through the C entry point with src_dst,
dst_src (64 guard entries behind it) and expert_sizes pre-filled with a sentinel: dst_src[n_valid:] and the guard keep it.
moe_scan_kernel's geometries: parts = 1024 / epad in {1, 2, 8, 16, 256, 512, 1024}, nchunks <, =, > parts, a short last part
((n, E) = (2049, 512), (2049, 300), (5120, 512), (9216, 65)). n = 1023 | 1024 | 1025 is the single-launch | three-launch seam.
E = 1025 raises. E = 1024 (64 KiB dynamic + 4 KiB static LDS in the single-launch form, no function attribute set): the launch
is ACCEPTED on gfx950 (a workgroup may take the CU's whole 160 KiB) and the result is exact -- the declared limit stands.

COMBINE. Bar per element: |got - ref64| <= 0.5 ulp_T(max(|got|, |ref64|)) + topk 2^-23 sum_k |w x|. Plain: f32 / bf16 / f16, H in
{1, 7, 255, 256, 257, 1000}, topk in {1, 3, 8}, T in {1, 5}. Sorted: bf16 / f16, H in {8, 248, 2040, 2048, 2056, 4104} (the
2048-element sweep ends early, exactly, loops), topk in {1, 2, 7, 8, 9, 16} (8 = HOIST8), src_dst = -1 at k = 0, at k = topk - 1
and for a whole token (output exactly 0) with NaN in the rows nobody points to, bit-equal to index_copy_ + moe_combine_result and
from run to run; topk = 17, H = 12 and f32 raise. Local form: n_local in {1, 255, 256, 257, 600}, rows nv - 1 (kept) and nv
(skipped), nv = 0, every row at or past nv NaN / Inf. Rank sum for ep in {2, 4}: ids rotated as layers.FusedMoE does, index built on
the GPU, rows past each rank's nv poisoned: the float64 sum of the ranks' outputs is within the sum of the per-rank bars of the
un-partitioned float64 combine.

Largest offsets from float64 observed (printed by the tests; identical for f32, bf16 and f16 logits, which hold the same values):
gate weights 1.43e-06 relative (E = 63, softmax, topk = 63, renormalised) and 0.066 of the (6e-6, 2e-7) bar; placed ties 6.3e-07 /
0.054; -inf rows 8.7e-07 / 0.045; grouped gate 8.6e-07 / 0.11 (E = 160, G = 8, softmax, topk = 64). The oracle's own figures are
1.47e-06 and 2.49e-06 (tests/test_moe_reference.py). Combines, as a fraction of the bar: plain f32 0.33; 16-bit outputs reach 1.00
(a sum next to the midpoint of two 16-bit values: the bar's half ulp). The whole file: 169 tests in 6 s on an MI355X, the slowest 0.23 s.

What these tests catch, each tried on a scratch build of moe.hip (169 tests; the count that fails, and which):
  * plain gate, in-lane tie rule `v[j] == best && e < best_e` turned into "the later slot wins" (`>=`): 58 -- test_gate and
    test_gate_placed_ties for every E >= 127 (two or more slots per lane), test_gate_placed_ties[65-*], the -inf and saturated
    rows; E <= 64 passes (one slot). (Dropping the clause alone changes nothing: the slots are walked in ascending order.)
  * plain gate, butterfly tie rule `ob == best && oe < best_e` dropped: 79 -- every gate test with E >= 2;
  * plain gate, padding: the sigmoid branch's `e < E` and the arg-max loop's `e < E` guard EACH OTHER -- with either one removed
    (padding lanes score sigmoid(-inf) = 0 but cannot be picked / stay -inf) all 169 pass; with both removed 30 fail: every
    test_gate with E % 64 != 0 (the all-negative mode picks a padding lane first) and the saturated rows;
  * grouped gate, `rank < topk_group` -> `<=` (one group too many): 18 -- test_grouped_gate for every (E, G) but (64, 64), where
    one expert per group makes the group limit a no-op for topk <= topk_group;
  * grouped gate, tie between groups to the HIGHER group: all 21 test_grouped_gate; group value always the max: 18 (all with a
    bias); weight = the biased choice score: 18 (the same);
  * moe_scan_kernel, `before` dropped from `run`: 17 -- test_index_build for every multi-chunk pair whose chunks spread over more
    than one part ((1025, 1) ... (9216, 65)); the pairs with parts = 1 (E = 513, 1024) and the single-launch pairs pass;
  * moe_place_kernel, `live` replaced by clamping the id into [0, E) (the guard itself cannot be dropped without an LDS index out
    of range, which was not run): all 34 test_index_build;
  * moe_combine_sorted_kernel, plain form, `rows[k] >= nv` dropped (rows at or past nv are read): 12 -- every test_local_combine
    and both test_expert_parallel_ranks_sum_to_the_whole; HOIST8 form, the skip test reduced to `rows[k] < nv` with the index
    clamped to row 0 (a negative index was not run): all 12 test_sorted_combine. `rows[k] < nv` in the HOIST8 form cannot fail
    today: that instantiation is launched without local sizes only, where nv is INT_MAX."""
import functools

import pytest
import torch

import _moe_cases as mc
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from xllm_amd import _lib, ops
DEV = "cuda"
_dt_ids = [mc.NAME[d] for d in mc.DTYPES]
SENTINEL = -12345
GUARD = 64


def _dev(t, dtype=None):
    if t is None:
        return None
    if dtype is not None:
        c = t.to(dtype)
        assert torch.equal(c.float(), t), "a placed logit is not exact in the tensor type"
        t = c
    return t.to(DEV)


# ------------------------------------------------------------------------------------------------------------- references
@functools.lru_cache(maxsize=None)
def _gate_refs(key, topk, renorm):
    """(float64 weights, float64 ids, oracle weights, oracle ids) of one launch; computed once, shared by the three dtypes"""
    x, bias, scoring = _gate_launch(key)
    w64, id64 = mc.gate64(x, topk, renorm, bias, scoring)
    wo, ido = orc.moe_fused_topk(x, topk, renorm, None if bias is None else bias.clone(), scoring)
    return w64, id64, wo, ido


def _gate_launch(key):
    kind = key[0]
    if kind == "table":
        _, E, T, mode = key
        x, bias = mc.gate_case(E, T, mode)
    elif kind == "tie":
        _, E, topk, mode = key
        tr = mc.gate_tie_rows(E, topk, mode)
        x, bias = tr.x, tr.bias
    else:
        _, E, mode = key
        x, bias = mc.gate_inf_case(E, mode)
    return x, bias, mc.SCORING[mode]


class _Worst:
    def __init__(self):
        self.rel, self.frac, self.where = 0.0, 0.0, None

    def note(self, rel_frac, where):
        if rel_frac[1] > self.frac:
            self.frac, self.where = rel_frac[1], where
        self.rel = max(self.rel, rel_frac[0])


def _check_gate(key, topk, renorm, dtype, worst):
    x, bias, scoring = _gate_launch(key)
    w64, id64, wo, ido = _gate_refs(key, topk, renorm)
    w, ids = ops.moe_fused_topk(_dev(x, dtype), topk, renorm, _dev(bias), scoring)
    tag = (key, topk, renorm, mc.NAME[dtype])
    assert torch.equal(ids.cpu(), id64), tag
    worst.note(mc.assert_gate_weights(w, w64, 2 * mc.GATE_RTOL, 2 * mc.GATE_ATOL, tag), tag)
    assert torch.equal(ids.cpu(), ido), tag
    mc.assert_gate_weights(w, wo, mc.GATE_RTOL, mc.GATE_ATOL, tag + ("oracle",))


# ------------------------------------------------------------------------------------------------------------------ gate
@pytest.mark.parametrize("dtype", mc.DTYPES, ids=_dt_ids)
@pytest.mark.parametrize("E", mc.GATE_E)
def test_gate(E, dtype):
    worst = _Worst()
    for T in mc.GATE_T:
        for mode in mc.gate_modes(E):
            for topk in mc.gate_topks(E):
                for renorm in (False, True):
                    _check_gate(("table", E, T, mode), topk, renorm, dtype, worst)
    print(f"gate E = {E} {mc.NAME[dtype]}: largest weight offset from float64 {worst.rel:.3g} relative, {worst.frac:.3g} of the "
          f"(6e-6, 2e-7) bar at {worst.where}")


@pytest.mark.parametrize("dtype", mc.DTYPES, ids=_dt_ids)
@pytest.mark.parametrize("E", mc.GATE_E)
def test_gate_placed_ties(E, dtype):
    worst, names = _Worst(), set()
    for topk in mc.gate_topks(E):
        for mode in mc.TIE_MODES:
            names |= set(mc.gate_tie_rows(E, topk, mode).names)
            for renorm in (False, True):
                _check_gate(("tie", E, topk, mode), topk, renorm, dtype, worst)
    want = {"all_equal"} | ({"63|64"} if E >= 65 else set()) | ({"0|64|128"} if E >= 129 else set()) \
        | ({"spread", "last"} if E >= 8 else set())
    assert names == want, (names, want)
    print(f"gate ties E = {E} {mc.NAME[dtype]}: {worst.rel:.3g} relative, {worst.frac:.3g} of the bar")


@pytest.mark.parametrize("dtype", mc.DTYPES, ids=_dt_ids)
def test_gate_minus_inf_logits(dtype):
    worst = _Worst()
    for E in [e for e in mc.GATE_E if e >= 16]:
        for mode in ("softmax", "sigmoid", "sigmoid_bias"):
            for topk in [k for k in mc.gate_topks(E) if k <= min(E // 2, 64)]:
                for renorm in (False, True):
                    _check_gate(("inf", E, mode), topk, renorm, dtype, worst)
    print(f"gate -inf {mc.NAME[dtype]}: {worst.rel:.3g} relative, {worst.frac:.3g} of the bar")


@pytest.mark.parametrize("dtype", mc.DTYPES, ids=_dt_ids)
def test_gate_saturated_sigmoid_follows_the_oracle(dtype):
    """the documented departure from float64: at +-30 the fp32 sigmoid is 1 (a tie); ids are held to the fp32 oracle's only"""
    for E in (65, 257):
        x = mc.saturated_case(E)
        g = torch.Generator().manual_seed(E)
        for bias in (None, mc.grid_bias(g, E)):
            for topk in (1, 8, 64):
                _, ido = orc.moe_fused_topk(x, topk, False, None if bias is None else bias.clone(), "sigmoid")
                _, ids = ops.moe_fused_topk(_dev(x, dtype), topk, False, _dev(bias), "sigmoid")
                assert torch.equal(ids.cpu(), ido), (E, bias is not None, topk)


def test_gate_declines_what_it_cannot_do():
    x = torch.zeros(3, 513, device=DEV)
    with pytest.raises(ops.Mi355Error):
        ops.moe_fused_topk(x, 8, True, None, "softmax")                       # E = 513: more than 8 experts per lane
    with pytest.raises(ops.Mi355Error):
        ops.moe_fused_topk(x[:, :128].contiguous(), 65, True, None, "softmax")   # topk = 65: one selected weight per lane
    with pytest.raises(ops.Mi355Error):
        ops.moe_fused_topk(x[:, :2].contiguous(), 3, True, None, "sigmoid")   # topk > E
    w, ids = ops.moe_fused_topk(x[:, :512].contiguous(), 64, True, None, "softmax")
    assert ids.cpu().tolist() == [list(range(64))] * 3


# ---------------------------------------------------------------------------------------------------------- grouped gate
@functools.lru_cache(maxsize=None)
def _grouped_refs(E, G, kg, mode, topk, which, renorm, scale):
    x, bias = _grouped_launch(E, G, kg, mode, topk, which)
    scoring = mc.SCORING[mode]
    w64, id64, kept = mc.grouped_gate64(x, topk, G, kg, renorm, bias, scoring, scale)
    wo, ido = orc.moe_grouped_topk(x, topk, G, kg, renorm, None if bias is None else bias.clone(), scoring, scale)
    return w64, id64, kept, wo, ido


def _grouped_launch(E, G, kg, mode, topk, which):
    if which[0] == "table":
        return mc.grouped_case(E, G, kg, mode, which[1])
    p = next(p for p in mc.grouped_placed(E, G, kg, mode, topk) if p.name == which[1])
    return p.x, p.bias


@pytest.mark.parametrize("dtype", mc.DTYPES, ids=_dt_ids)
@pytest.mark.parametrize("E,G", mc.GROUPED_EG)
def test_grouped_gate(E, G, dtype):
    worst, seen = _Worst(), set()
    for kg in mc.grouped_topk_groups(G):
        for mode in mc.grouped_modes(E, G):
            for topk in mc.grouped_topks(E, G, kg):
                placed = [p.name for p in mc.grouped_placed(E, G, kg, mode, topk)]      # (asserts every placed property)
                seen |= set(placed)
                for which in [("table", T) for T in mc.GROUPED_T] + [("placed", n) for n in placed]:
                    x, bias = _grouped_launch(E, G, kg, mode, topk, which)
                    xd, bd = _dev(x, dtype), _dev(bias)
                    for renorm in (False, True):
                        for scale in (1.0, 2.5):
                            w64, id64, kept, wo, ido = _grouped_refs(E, G, kg, mode, topk, which, renorm, scale)
                            w, ids = ops.moe_grouped_topk(xd, topk, G, kg, renorm, bd, mc.SCORING[mode], scale)
                            tag = (E, G, kg, mode, topk, which, renorm, scale, mc.NAME[dtype])
                            idc = ids.cpu()
                            assert torch.equal(idc, id64), tag
                            assert bool(kept.gather(1, (idc // (E // G)).long()).all()), tag     # no id from a dropped group
                            worst.note(mc.assert_gate_weights(w, w64, 2 * mc.GATE_RTOL, 2 * mc.GATE_ATOL, tag), tag)
                            assert torch.equal(idc, ido), tag
                            mc.assert_gate_weights(w, wo, mc.GATE_RTOL, mc.GATE_ATOL, tag + ("oracle",))
    assert "all_equal" in seen and "twin_groups" in seen
    assert (E, G) == (64, 64) or {"best_loses", "choice_vs_weight"} <= seen
    print(f"grouped gate E = {E} G = {G} {mc.NAME[dtype]}: largest weight offset from float64 {worst.rel:.3g} relative, "
          f"{worst.frac:.3g} of the (6e-6, 2e-7) bar at {worst.where}")


# ----------------------------------------------------------------------------------------------------------- index build
def _build_index(ids, E):
    """the C entry point as ops.moe_compute_index calls it (which first sizes the workspace), on sentinel-filled outputs"""
    n = ids.numel()
    d = ids.to(DEV)
    first = ops.moe_compute_index(d.view(n, 1), E)
    src_dst = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)
    dst_src = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    sizes = torch.full((E + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().xllm_mi355_moe_compute_index(d.data_ptr(), n, 1, E, src_dst.data_ptr(), dst_src.data_ptr(),
                                                     sizes.data_ptr(), torch.cuda.current_stream().cuda_stream),
              "moe_compute_index")
    return src_dst.cpu(), dst_src.cpu(), sizes.cpu(), [t.cpu() for t in first]


@pytest.mark.parametrize("n,E", mc.INDEX_PAIRS)
def test_index_build(n, E):
    for name, ids in mc.index_inputs(n, E):
        ref = mc.index_ref(ids, E)
        src_dst, dst_src, sizes, first = _build_index(ids, E)
        tag = (n, E, name, mc.scan_geometry(n, E))
        assert torch.equal(sizes[:E], ref.sizes), tag
        assert torch.equal(src_dst, ref.src_dst), tag
        assert torch.equal(dst_src[:ref.n_valid], ref.dst_src), tag
        assert bool((dst_src[ref.n_valid:] == SENTINEL).all()) and bool((sizes[E:] == SENTINEL).all()), tag   # nothing else written
        assert torch.equal(first[0], ref.src_dst) and torch.equal(first[1][:ref.n_valid], ref.dst_src) \
            and torch.equal(first[2], ref.sizes), tag


def test_index_build_limits():
    ids = torch.zeros(5, 2, dtype=torch.int32, device=DEV)
    with pytest.raises(ops.Mi355Error):
        ops.moe_compute_index(ids, 1025)
    src_dst, _, sizes = ops.moe_compute_index(ids, 1024)                 # the declared limit itself: accepted
    assert src_dst.cpu().tolist() == list(range(10)) and sizes.cpu().tolist() == [10] + [0] * 1023


# --------------------------------------------------------------------------------------------------------------- combine
@pytest.mark.parametrize("dtype", mc.DTYPES, ids=_dt_ids)
def test_plain_combine(dtype):
    worst = 0.0
    for H in mc.PLAIN_H:
        for topk in mc.PLAIN_TOPK:
            for T in mc.PLAIN_T:
                rows, w = mc.combine_inputs(T, topk, H, dtype, 1000 * H + 10 * topk + T)
                ref, a = mc.combine64(rows, w)
                got = ops.moe_combine_result(rows.to(DEV), w.to(DEV), T, topk)
                worst = max(worst, mc.assert_combine(got, ref, a, topk, dtype, (H, topk, T)))
    print(f"plain combine {mc.NAME[dtype]}: largest offset {worst:.4f} of the bar")


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("dtype", mc.HALF, ids=[mc.NAME[d] for d in mc.HALF])
@pytest.mark.parametrize("H", mc.SORTED_H)
def test_sorted_combine(H, dtype):
    worst, T = 0.0, 5
    for topk in mc.SORTED_TOPK:
        for skips in (False, True):
            srt, src_dst, w = mc.sorted_inputs(T, topk, H, dtype, 100 * H + topk, skips)
            ref, a = mc.combine64(srt, w, src_dst)
            d_srt, d_sd, d_w = srt.to(DEV), src_dst.to(DEV), w.to(DEV)
            got = ops.moe_combine_sorted(d_srt, d_sd, d_w, T, topk)
            tag = (H, topk, skips, mc.NAME[dtype])
            worst = max(worst, mc.assert_combine(got, ref, a, topk, dtype, tag))
            if skips:
                assert bool((_bits(got[3]) == 0).all()), tag                                  # a token without a row: exactly +0
            again = ops.moe_combine_sorted(d_srt, d_sd, d_w, T, topk)
            assert torch.equal(_bits(got), _bits(again)), tag                                 # run to run: the same bits
            # the two operators it fuses: zero rows, index_copy_ of the present rows, the plain combine
            full = torch.zeros_like(d_srt)
            live = (src_dst >= 0).nonzero().flatten().to(DEV)
            full.index_copy_(0, live, d_srt[d_sd[live].long()])
            two = ops.moe_combine_result(full, d_w, T, topk)
            assert torch.equal(_bits(got), _bits(two)), tag
    print(f"sorted combine H = {H} {mc.NAME[dtype]}: largest offset {worst:.4f} of the bar")


def test_sorted_combine_declines_what_it_cannot_do():
    def call(T, topk, H, dtype):
        rows = torch.zeros(T * topk, H, dtype=dtype, device=DEV)
        sd = torch.arange(T * topk, dtype=torch.int32, device=DEV)
        return ops.moe_combine_sorted(rows, sd, torch.ones(T, topk, device=DEV), T, topk)
    for bad in ((2, 17, 64, torch.bfloat16), (2, 4, 12, torch.float16), (2, 4, 64, torch.float32)):
        with pytest.raises(ops.Mi355Error):
            call(*bad)
    assert call(2, 16, 8, torch.bfloat16).shape == (2, 8)


@pytest.mark.parametrize("dtype", mc.HALF, ids=[mc.NAME[d] for d in mc.HALF])
@pytest.mark.parametrize("n_local", mc.LOCAL_N)
def test_local_combine(n_local, dtype):
    """the expert-parallel form: nv = sum(local sizes) is summed by 256 threads with atomicAdd; rows at or past nv are absent"""
    worst, T = 0.0, 6
    for topk, H in ((2, 8), (8, 2056), (7, 248)):
        N = T * topk
        for nv in (0, 1, N // 2, N - 1, N):
            srt, src_dst, w = mc.sorted_inputs(T, topk, H, dtype, 7 * n_local + topk + nv, skips=False)
            if 0 < nv < N:
                assert bool((src_dst == nv - 1).any()) and bool((src_dst == nv).any())       # the last kept row, the first skipped
            if nv == N // 2:
                src_dst[(src_dst == 0).nonzero().flatten()] = -1                             # ... and one row without a position
            sizes = mc.local_sizes(n_local, nv, n_local + nv)
            bad = mc.poison(srt, nv)
            ref, a = mc.combine64(bad, w, src_dst, nv)
            got = ops.moe_combine_sorted(bad.to(DEV), src_dst.to(DEV), w.to(DEV), T, topk, sizes.to(DEV))
            tag = (n_local, topk, H, nv, mc.NAME[dtype])
            worst = max(worst, mc.assert_combine(got, ref, a, topk, dtype, tag))
            if nv == 0:
                assert bool((_bits(got) == 0).all()), tag
    print(f"local combine n_local = {n_local} {mc.NAME[dtype]}: largest offset {worst:.4f} of the bar")


@pytest.mark.parametrize("ep", [2, 4])
def test_expert_parallel_ranks_sum_to_the_whole(ep):
    T, topk, E, H, dtype = 33, 4, 16, 264, torch.bfloat16
    g = torch.Generator().manual_seed(50 + ep)
    ids = torch.stack([torch.randperm(E, generator=g)[:topk] for _ in range(T)]).to(torch.int32)
    rows, w = mc.combine_inputs(T, topk, H, dtype, 60 + ep)               # rows[i]: what expert ids[i] made of token i // topk
    whole, _ = mc.combine64(rows, w)
    E_local = E // ep
    total, bar = torch.zeros_like(whole), torch.zeros_like(whole)
    nvs = []
    for r in range(ep):
        rot = torch.remainder(ids - r * E_local, E).to(torch.int32)       # layers.FusedMoE: the rank's experts sort to the front
        src_dst, dst_src, sizes = ops.moe_compute_index(rot.to(DEV), E)
        ref_i = mc.index_ref(rot, E)
        assert torch.equal(src_dst.cpu(), ref_i.src_dst) and torch.equal(sizes.cpu(), ref_i.sizes)
        local = sizes[:E_local]
        nv = int(ref_i.sizes[:E_local].sum())
        nvs.append(nv)
        srt = torch.empty_like(rows)
        srt[ref_i.src_dst.long()] = rows
        bad = mc.poison(srt, nv)
        got = ops.moe_combine_sorted(bad.to(DEV), src_dst, w.to(DEV), T, topk, local)
        ref, a = mc.combine64(bad, w, ref_i.src_dst, nv)
        mc.assert_combine(got, ref, a, topk, dtype, (ep, r))
        total += got.double().cpu()
        bar += mc.combine_bar(got.double().cpu(), ref, a, topk, dtype)
    assert sum(nvs) == T * topk and min(nvs) > 0
    err = (total - whole).abs()
    assert bool((err <= bar).all()), (ep, float((err / bar.clamp(min=1e-300)).max()))
