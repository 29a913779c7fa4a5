"""CPU: the room between the two references of the MoE routing tests -- the fp32 C oracle (oracle/xllm_oracle.c) and the float64
restatements of tests/_moe_cases.py -- over every case the GPU tests run (tests/test_gpu_moe_routing.py).

  * every gate and grouped-gate case: the oracle's ids EQUAL float64's, in order; its weights are inside the project's gate bar
    (rtol 3e-6, atol 1e-7: tests/test_gpu_parity.py::test_moe_fused_topk); the gap condition of _moe_cases (adjacent choice
    scores, and the group values at the group cut, exactly equal or >= 1e-5 relative apart) holds for every row of every case;
  * orc.moe_compute_index equals index_ref on the distributions without an invalid id (the oracle indexes
    expert_sizes[expert_id[i]] unguarded: it cannot serve for the others);
  * orc.moe_combine is inside the combine bar (0.5 ulp_T + topk 2^-23 sum |w x|) of combine64.

Largest offsets of the oracle from float64 (printed by the tests):
  plain gate     1.47e-06 relative; 0.33 of the (3e-6, 1e-7) bar (E = 511 / 512, where the softmax sum runs over 512 fp32 terms)
  grouped gate   2.49e-06 relative; 0.24 of the bar (E = 512, G = 2)
  combine        f32 0.3333 of the bar (the accumulate term is all of it); bf16 1.0000 and f16 0.9998: a sum that falls next to the
                 midpoint of two 16-bit values is rounded by half an ulp, which is the bar's first term
The kernels' own figures are in the docstring of tests/test_gpu_moe_routing.py."""
import pytest
import torch

import _moe_cases as mc
from oracle import oracle as orc


def _bias_arg(bias):
    return None if bias is None else bias.clone()


def test_references_on_hand_computed_rows():
    x = torch.tensor([[0.0, 1.0, 1.0, -1.0]])
    w, ids = mc.gate64(x, 3, False, None, "sigmoid")
    assert ids.tolist() == [[1, 2, 0]]                                                     # of two ties, the lower index first
    assert torch.allclose(w, torch.tensor([[0.7310585786300049, 0.7310585786300049, 0.5]], dtype=torch.float64), rtol=1e-15, atol=0)
    w, ids = mc.gate64(x, 2, True, torch.tensor([0.0, 0.0, 0.0, 1.0]), "sigmoid")          # the bias selects, the weight ignores it
    assert ids.tolist() == [[3, 1]]
    s3, s1 = 0.2689414213699951, 0.7310585786300049
    assert torch.allclose(w, torch.tensor([[s3 / (s3 + s1), s1 / (s3 + s1)]], dtype=torch.float64), rtol=1e-15, atol=0)
    w, ids = mc.gate64(torch.tensor([[0.0, 0.0]]), 2, False, None, "softmax")
    assert ids.tolist() == [[0, 1]] and w.tolist() == [[0.5, 0.5]]
    # grouped: 3 groups of 2. max rule: group 1 (2.0) and group 0 (1.0, tie with group 2: the lower group) stay
    x = torch.tensor([[1.0, -1.0, 2.0, -3.0, 1.0, 0.5]])
    w, ids, kept = mc.grouped_gate64(x, 3, 3, 2, False, None, "sigmoid", 2.0)
    assert kept.tolist() == [[True, True, False]] and ids.tolist() == [[2, 0, 1]]
    assert abs(float(w[0, 0]) - 2.0 * 0.8807970779778823) < 1e-15
    # top-2 sum rule (zero bias): group 2 (0.731 + 0.622) beats group 1 (0.881 + 0.047) and group 0 (0.731 + 0.269)
    _, ids, kept = mc.grouped_gate64(x, 2, 3, 1, False, torch.zeros(6), "sigmoid", 1.0)
    assert kept.tolist() == [[False, False, True]] and ids.tolist() == [[4, 5]]
    r = mc.index_ref(torch.tensor([2, 0, 7, 2, -1, 0], dtype=torch.int32), 3)
    assert r.sizes.tolist() == [2, 0, 2] and r.src_dst.tolist() == [2, 0, -1, 3, -1, 1] and r.dst_src.tolist() == [1, 5, 0, 3]
    rows = torch.tensor([[1.0], [2.0], [float("nan")], [4.0]])
    s, a = mc.combine64(rows, torch.tensor([[1.0, -1.0], [0.5, 2.0]]), torch.tensor([3, 0, 2, 1]), 2)
    assert s.tolist() == [[-1.0], [4.0]] and a.tolist() == [[1.0], [4.0]]                   # rows 3 and 2 are past nv = 2
    assert mc.ulp(torch.tensor([1.0, 1.5, 2.0, 0.0, 3e-5], dtype=torch.float64), torch.float16).tolist() == \
        [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -24, 2.0 ** -24]
    assert float(mc.ulp(torch.tensor([1.0], dtype=torch.float64), torch.bfloat16)) == 2.0 ** -7
    for n, E, want in ((2049, 1024, (1, 3, 3)), (2049, 512, (2, 3, 2)), (9216, 65, (8, 9, 2)), (9217, 1, (1024, 10, 1)),
                       (5120, 512, (2, 5, 3)), (1025, 3, (256, 2, 1))):
        assert mc.scan_geometry(n, E) == want


def test_index_table_reaches_every_scan_geometry():
    geo = [mc.scan_geometry(n, E) for n, E in mc.INDEX_PAIRS if n > mc.CHUNK]
    assert {1, 2, 8, 256, 1024} <= {p for p, _, _ in geo}
    assert any(c < p for p, c, _ in geo) and any(c == p for p, c, _ in geo) and any(c > p for p, c, _ in geo)
    assert any(c % per for p, c, per in geo if p > 1)                                     # the last used part is short
    assert {n for n, _ in mc.INDEX_PAIRS} >= set(mc.INDEX_N) and {E for _, E in mc.INDEX_PAIRS} == set(mc.INDEX_E)
    names = {name for n, E in mc.INDEX_PAIRS for name, _ in mc.index_inputs(n, E)}
    assert names == {"uniform", "all_first", "all_last", "last_chunk_only", "wave_64_distinct", "wave_one_expert",
                     "invalid_everywhere", "one_chunk_invalid", "all_invalid"}


_worst = {"gate": (0.0, 0.0), "grouped": (0.0, 0.0), "combine": 0.0}


def _note(kind, rel, frac):
    _worst[kind] = (max(_worst[kind][0], rel), max(_worst[kind][1], frac))


@pytest.mark.parametrize("E", mc.GATE_E)
def test_gate_oracle_against_float64(E):
    n_top = min(E, 64) + 1
    for T in mc.GATE_T:
        for mode in mc.gate_modes(E):
            x, bias = mc.gate_case(E, T, mode)
            scoring = mc.SCORING[mode]
            assert bool(mc.gaps_ok(x, bias, scoring, n_top).all()), (E, T, mode)
            assert float(x.min()) >= -6 and float(x.max()) <= 6 and torch.equal(x * 16, (x * 16).round())
            if bias is not None:
                b0 = bias + 2.0 if mode == "sigmoid_bias_neg" else bias
                assert float(b0.abs().max()) <= 0.125 and torch.equal(b0 * 512, (b0 * 512).round())
                if mode == "sigmoid_bias_neg":
                    assert float((mc.scores64(x, scoring) + bias.double()).max()) < 0      # every choice score is negative
            for topk in mc.gate_topks(E):
                for renorm in (False, True):
                    w64, id64 = mc.gate64(x, topk, renorm, bias, scoring)
                    w, ids = orc.moe_fused_topk(x, topk, renorm, _bias_arg(bias), scoring)
                    assert torch.equal(ids, id64), (E, T, mode, topk, renorm)
                    _note("gate", *mc.assert_gate_weights(w, w64, mc.GATE_RTOL, mc.GATE_ATOL, (E, T, mode, topk, renorm)))
    for topk in mc.gate_topks(E):
        for mode in mc.TIE_MODES:
            tr = mc.gate_tie_rows(E, topk, mode)
            assert bool(mc.gaps_ok(tr.x, tr.bias, mc.SCORING[mode], topk + 1).all())
            for renorm in (False, True):
                w64, id64 = mc.gate64(tr.x, topk, renorm, tr.bias, mc.SCORING[mode])
                w, ids = orc.moe_fused_topk(tr.x, topk, renorm, _bias_arg(tr.bias), mc.SCORING[mode])
                assert torch.equal(ids, id64), (E, mode, topk, tr.names)
                _note("gate", *mc.assert_gate_weights(w, w64, mc.GATE_RTOL, mc.GATE_ATOL, (E, "tie", mode, topk)))
    if E >= 16:
        for mode in ("softmax", "sigmoid", "sigmoid_bias"):
            x, bias = mc.gate_inf_case(E, mode)
            for topk in [k for k in mc.gate_topks(E) if k <= min(E // 2, 64)]:
                w64, id64 = mc.gate64(x, topk, True, bias, mc.SCORING[mode])
                w, ids = orc.moe_fused_topk(x, topk, True, _bias_arg(bias), mc.SCORING[mode])
                assert torch.equal(ids, id64), (E, "inf", mode, topk)
                _note("gate", *mc.assert_gate_weights(w, w64, mc.GATE_RTOL, mc.GATE_ATOL, (E, "inf", mode, topk)))
    print(f"E = {E}: oracle vs float64, largest relative weight offset so far {_worst['gate'][0]:.3g} "
          f"({_worst['gate'][1]:.3g} of the bar)")


def test_saturated_sigmoid_is_a_tie_in_fp32_only():
    """the documented departure: at +-30 the fp32 sigmoid is a tie that index decides; float64 still tells the values apart only
    through the bias -- without one it agrees, with one it need not, so such rows are held to the oracle alone"""
    x = mc.saturated_case(65)
    _, ids = orc.moe_fused_topk(x, 8, False, None, "sigmoid")
    assert ids[0].tolist() == list(range(8)) and ids[1].tolist() == list(range(8))
    assert float(torch.sigmoid(torch.tensor(30.0))) == 1.0 and float(torch.sigmoid(torch.tensor(30.0, dtype=torch.float64))) < 1.0


@pytest.mark.parametrize("E,G", mc.GROUPED_EG)
def test_grouped_gate_oracle_against_float64(E, G):
    seen = set()
    for kg in mc.grouped_topk_groups(G):
        topks = mc.grouped_topks(E, G, kg)
        for mode in mc.grouped_modes(E, G):
            scoring = mc.SCORING[mode]
            launches = [(x, bias, "table") for T in mc.GROUPED_T for x, bias in [mc.grouped_case(E, G, kg, mode, T)]]
            assert all(bool(mc.grouped_gaps_ok(x, b, scoring, G, kg, max(topks) + 1).all()) for x, b, _ in launches)
            for topk in topks:
                placed = mc.grouped_placed(E, G, kg, mode, topk)
                seen |= {p.name for p in placed}
                for x, bias, name in launches + [(p.x, p.bias, p.name) for p in placed]:
                    if name != "table":
                        assert bool(mc.grouped_gaps_ok(x, bias, scoring, G, kg, topk + 1).all()), (E, G, kg, mode, name)
                    for renorm, scale in ((False, 1.0), (True, 2.5), (True, 1.0), (False, 2.5)):
                        w64, id64, kept = mc.grouped_gate64(x, topk, G, kg, renorm, bias, scoring, scale)
                        w, ids = orc.moe_grouped_topk(x, topk, G, kg, renorm, _bias_arg(bias), scoring, scale)
                        tag = (E, G, kg, mode, topk, name, renorm, scale)
                        assert torch.equal(ids, id64), tag
                        assert bool(kept.gather(1, (id64 // (E // G)).long()).all()), tag
                        _note("grouped", *mc.assert_gate_weights(w, w64, mc.GATE_RTOL, mc.GATE_ATOL, tag))
    assert "all_equal" in seen and (G == 1 or "twin_groups" in seen)
    if (E, G) != (64, 64):
        assert {"best_loses", "choice_vs_weight"} <= seen
    print(f"E = {E}, G = {G}: oracle vs float64, largest relative weight offset so far {_worst['grouped'][0]:.3g} "
          f"({_worst['grouped'][1]:.3g} of the bar)")


def test_index_oracle_equals_index_ref():
    for n, E in mc.INDEX_PAIRS:
        for name, ids in mc.index_inputs(n, E):
            ref = mc.index_ref(ids, E)
            if ref.n_valid != n:
                continue                                   # an invalid id: outside the oracle's domain (module docstring)
            src_dst, dst_src, sizes = orc.moe_compute_index(ids.view(n, 1), E)
            assert torch.equal(src_dst, ref.src_dst) and torch.equal(dst_src, ref.dst_src) and torch.equal(sizes, ref.sizes), \
                (n, E, name)


@pytest.mark.parametrize("dtype", mc.DTYPES, ids=[mc.NAME[d] for d in mc.DTYPES])
def test_combine_oracle_against_float64(dtype):
    worst = 0.0
    for H in mc.PLAIN_H:
        for topk in mc.PLAIN_TOPK + [16]:
            for T in mc.PLAIN_T:
                rows, w = mc.combine_inputs(T, topk, H, dtype, 1000 * H + 10 * topk + T)
                ref, a = mc.combine64(rows, w)
                got = orc.moe_combine(rows, w, T, topk)
                worst = max(worst, mc.assert_combine(got, ref, a, topk, dtype, (H, topk, T)))
    print(f"{mc.NAME[dtype]}: oracle combine vs float64, largest offset {worst:.4f} of the bar")
