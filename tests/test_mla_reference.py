"""CPU checks of the MLA attention cases (tests/_mla_cases.py) that tests/test_gpu_mla_arms.py runs on the GPU.

  * Every case's arm and split-KV count hold through the read-only plan query xllm_mi355_mla_plan (the library loads without a
    GPU): the table's in a plain environment, what _mla_cases.expected_plan derives from the MLA switches when one is set.
  * The two references agree: the oracle (orc.paged_attention, dv = 512, the cache aliased as V) stays within HALF of every bar the
    GPU test asserts against the dense float64 reference, over every case and both dtypes: relative L2, the element-wise bar
    (2 bf16 ulp of the row maximum), the one-P bars for the calls that can take the tile-sharing arm. The element-wise bar: ONE
    rounding flip of a bf16 element in the top binade of its row is 0.5 ... 1.0 of it whatever caused the flip, so seeds are
    picked per call (_mla_cases.PREFILL_SEED, the rescale seeds) until the oracle alone stays under a half. WHOLE_ELEM_BAR names
    the bf16 calls for which no seed of the scan did: they are held to the whole bar, as tests/test_prefill_reference.py does.
    The oracle's largest per-row distance is what _mla_cases.ROW_MEASURED records (the GPU row bar is twice that), re-measured
    here. Measured fractions: see the docstring of tests/test_gpu_mla_arms.py.
  * Sensitivity: on every mask-edge case, moving kv_len by +-1 or the causal edge by +-1 moves EVERY touched (query, head) row of
    the float64 reference by more than the loosest row bar of its dtype (_mla_cases.MASK_Q_FLAT is what makes that possible).
  * The mass condition of the rescale cases holds (every jump has a witness row that keeps >= 0.05 of its mass in front of it).
  * Poison never meets a visible key: the reference is finite everywhere, rows without a key are exact zeros.
  * The tile-sharing calls contain the group shapes they are built for."""
import ctypes as C
import os

import pytest
import torch

import _mla_cases as mc

CASES = mc.all_cases()
_WORST = {}
# bf16 cases whose oracle no seed of the scan kept under half of the element-wise bar: held to the whole bar
WHOLE_ELEM_BAR = {"prefill-share_h20-causal-bf16", "rescale-share-near_miss-bf16", "rescale-share-staircase-bf16"}


def _note(label, value, name):
    if value > _WORST.get(label, (-1.0, None))[0]:
        _WORST[label] = (value, name)


def _lib():
    from xllm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip(f"{_lib.LIB_PATH} is not built")
    return mc.library()


@pytest.mark.parametrize("name,kind,build", CASES, ids=[c[0] for c in CASES])
def test_case_takes_the_arm_and_split_count_of_its_table(name, kind, build):
    _lib()
    c = build()
    ws, cap = mc.ops_workspace(c)
    assert mc.query_plan(c, ws) == mc.expected_plan(c, cap)
    if not any(v in os.environ for v in ("XLLM_MI355_MLA_SPLITS", "XLLM_MI355_MLA_PREFILL", "XLLM_MI355_MLA_PREFILL_P")):
        assert mc.query_plan(c, ws) == (c["arm"], c["nsplit"])          # the table's literal entry
    if kind == "split":                       # the workspace cases: room for exactly two splits, one byte less, and none
        per = mc.per_split_bytes(len(c["entries"]), c["H"])
        want = mc.expected_plan(c, 32)[1]
        assert mc.query_plan(c, 2 * per) == (c["arm"], min(2, want)) == mc.expected_plan(c, 2)
        assert mc.query_plan(c, 2 * per - 1) == (c["arm"], 1)
        assert mc.query_plan(c, 0) == (c["arm"], 1)


def test_plan_query_validates():
    l = _lib()
    a = C.c_int32(-1)
    assert l.xllm_mi355_mla_plan(0, 0, 16, 64, 300, 0, C.addressof(a), None) == -1
    assert l.xllm_mi355_mla_plan(4, 0, 0, 64, 300, 0, C.addressof(a), None) == -1
    assert l.xllm_mi355_mla_plan(4, 0, 16, 64, 300, 0, None, None) == 0
    assert l.xllm_mi355_mla_plan(4, 32, 16, 64, 300, 255, C.addressof(a), None) != 0      # below the index arrays
    assert l.xllm_mi355_mla_plan(4, 32, 16, 16, 300, 256, C.addressof(a), None) == 0 and a.value == mc.ARM_STAGED


def _measure(name, build):
    """the oracle's distances from float64 on one case, asserted against half (or, for WHOLE_ELEM_BAR, the whole) of the bars"""
    c = build()
    r, dt, H = mc.references(c), c["dtype"], c["H"]
    assert torch.isfinite(r["r64"]).all(), "poison met a visible key"
    zr = mc.zero_rows(c)
    assert not r["r64"][zr].abs().any() and not r["fp32"][zr].float().abs().any()
    assert bool((r["r64"][~zr].abs().amax(-1) > 0).all())
    elem_bar = 1.0 if name in WHOLE_ELEM_BAR else 0.5
    for sl in mc.seq_slices(c):
        if bool(zr[sl].all()):
            continue
        rel, elem = mc.distance(r["fp32"][sl], r["r64r"][sl])
        _note((mc.DTNAME[dt], "fp32", "rel"), rel / mc.BAR_REL[dt], name)
        _note((mc.DTNAME[dt], "fp32", "elem"), elem, name)
        assert rel <= 0.5 * mc.BAR_REL[dt], (name, rel)
        assert elem <= elem_bar, (name, elem)
        if mc.can_share(c):     # the flash mode, put in the kernel's place, passes the one-P bars against (float64, p_round=True)
            from _bars import assert_p16_attention_close
            assert torch.isfinite(r["p16"].float()).all() and torch.isfinite(r["flash"].float()).all()
            assert_p16_attention_close(r["flash"][sl], r["r64r"][sl], r["p16"][sl])
            _note((mc.DTNAME[dt], "flash", "rel"), mc.rel_l2(r["flash"][sl], r["r64r"][sl]) /
                  max(1e-3, 1.25 * mc.rel_l2(r["p16"][sl], r["r64r"][sl])), name)
    row = mc.nanmax(mc.row_distances(r["fp32"], r["r64r"], H))
    _note((mc.DTNAME[dt], "hilo", "row"), row, name)
    assert row <= mc.ROW_MEASURED[("hilo", dt)], (name, row)
    if mc.can_share(c):
        row = mc.nanmax(mc.row_distances(r["p16"], r["r64r"], H))
        _note((mc.DTNAME[dt], "p16", "row"), row, name)
        assert row <= mc.ROW_MEASURED[("p16", dt)], (name, row)


_MEASURED = set()


@pytest.mark.parametrize("name,kind,build", CASES, ids=[c[0] for c in CASES])
def test_oracle_within_half_of_every_bar_of_float64(name, kind, build):
    _MEASURED.add(name)
    _measure(name, build)


def test_zz_row_bars_are_the_measured_ones():
    """after the parametrised test above (file order); measures whatever of it did not run in this process. Prints the largest
    distances and holds ROW_MEASURED to them"""
    for name, _, build in CASES:
        if name not in _MEASURED:
            _MEASURED.add(name)
            _measure(name, build)
    for k in sorted(_WORST, key=str):
        print(k, "%.3e" % _WORST[k][0], _WORST[k][1])
    for dt in mc.DTYPES:
        for form in ("hilo", "p16"):
            got = _WORST[(mc.DTNAME[dt], form, "row")][0]
            assert got <= mc.ROW_MEASURED[(form, dt)] <= 1.02 * got, (form, dt, got)
            assert mc.ROW_BAR[(form, dt)] == 2.0 * mc.ROW_MEASURED[(form, dt)]


def _mask_case(name, dtype, poisoned):
    """the mask-edge case of an id, with or without its poison (the same bytes elsewhere)"""
    for p in mc.DECODE_PLANS:
        if name == f"decode-{p.name}-{mc.DTNAME[dtype]}":
            return mc.decode_case(p, dtype, poisoned=poisoned)
    for call in mc.PREFILL_CALLS:
        if name == f"prefill-{call.name}-causal-{mc.DTNAME[dtype]}":
            return mc.prefill_case(call, True, dtype, poisoned=poisoned)
    raise KeyError(name)


MASK_CASES = [c for c in CASES if c[1] == "mask"]


@pytest.mark.parametrize("name,kind,build", MASK_CASES, ids=[c[0] for c in MASK_CASES])
def test_moving_an_edge_by_one_key_moves_every_touched_row_past_the_row_bar(name, kind, build):
    c = build()
    dt = c["dtype"]
    need = max(v for (form, d), v in mc.ROW_BAR.items() if d == dt)        # the loosest row bar of the dtype
    base = mc.references(c)["r64"]
    vis = mc.q_kvlens(c["entries"], c["causal"])
    was_zero = torch.tensor([n == 0 for _, n in vis])
    plain = _mask_case(name, dt, poisoned=False)     # the key behind kv_len is poison in the case itself
    live = ~torch.isnan(c["kc"])
    assert torch.equal(plain["kc"][live], c["kc"][live]) and torch.equal(plain["q"], c["q"])
    least, n_touched = float("inf"), 0
    for kv_shift, causal_shift in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        if causal_shift and c["decode"]:
            continue
        # a key behind kv_len exists only where the last page has room for it
        ent = [(ql, L + (kv_shift if kv_shift < 0 or L % c["bs"] else 0)) for ql, L in c["entries"]]
        moved_case = dict(plain if kv_shift > 0 else c, entries=ent)
        moved = mc.dense_ref64(moved_case, causal_shift=causal_shift)
        vis2 = mc.q_kvlens(ent, c["causal"], causal_shift)
        touched = torch.tensor([a[1] != b[1] for a, b in zip(vis, vis2)])
        if not bool(touched.any()):
            continue
        n_touched += int(touched.sum())
        assert torch.isfinite(moved).all()
        rd = mc.row_distances(moved, base, c["H"])                      # [T, H]
        t = touched & ~was_zero
        least = min(least, float(rd[t].min()))
        assert bool((rd[t] > need).all()), (name, kv_shift, causal_shift, float(rd[t].min()), need)
        assert bool((moved[touched & was_zero].reshape(-1, c["H"], mc.DV).abs().amax(-1) > 0).all())   # now sees a key
        assert torch.equal(moved[~touched], base[~touched])
    assert n_touched > 0
    print("least moved (query, head) row / bar: %.2f" % (least / need), name)


RESCALE = [c for c in CASES if c[1] == "rescale"]


@pytest.mark.parametrize("name,kind,build", RESCALE, ids=[c[0] for c in RESCALE])
def test_rescale_cases_keep_mass_in_front_of_their_jumps(name, kind, build):
    c = build()
    prof = mc.jump_profile(c)
    if "near_miss" in name:
        # no tile exceeds the lazy kernel's reference maximum by 2^8 (it never rescales), one comes within 2^1.5 of that, and P
        # there is ~2^7 against keys that hold >= 0.05 of the mass in front of it
        assert all(not j for j, _, _ in prof.values())
        assert max(e for _, _, e in prof.values()) > 6.5 and all(e <= 8.0 for _, _, e in prof.values())
        near = mc.jump_profile(c, thresh=5.5)
        rows = [k for k, (j, _, _) in near.items() if j]
        assert rows and all(near[k][1] >= 0.05 for k in rows), min(near[k][1] for k in rows)
        return
    witnessed = set()
    for (b, i), (jumps, front, _) in prof.items():
        if jumps and front >= 0.05:
            witnessed.add(jumps[-1])
    if "staircase" in name:
        assert witnessed == {1, 2, 3, 4}, witnessed
        assert max(len(j) for j, _, _ in prof.values()) == 4                 # a row that climbs every step
    else:
        assert witnessed == {mc.JUMP_KEY // mc.TILE}
        assert all(front >= 0.05 for jumps, front, _ in prof.values() if jumps)   # EVERY row behind the jump is a witness
        assert sum(1 for j, _, _ in prof.values() if j) >= 3 and sum(1 for j, _, _ in prof.values() if not j) >= 1


def test_sharing_calls_contain_the_groups_they_are_built_for():
    for call in (mc.SHARE_H128_CALL, mc.SHARE_H20_CALL):
        T = mc.n_tokens(call)
        distinct, one_seq = mc.group_profile(call)
        assert {1, 2, 3, 4} <= distinct
        assert (63, 64, 65, 66) in one_seq and (127, 128, 129, 130) in one_seq
        assert (66, 321) in call and (4, 2) in call
        assert T % 4 != 0 and ((T + 3) // 4) % 8 != 0
    assert mc.n_tokens(mc.SHARE_H20_CALL) == 1030 and ((1030 + 3) // 4) * 2 >= 128
    assert ((mc.n_tokens(mc.SHARE_H128_CALL) + 3) // 4) * 8 >= 128
    assert mc.n_tokens(mc.PER_TOKEN_CALL) < 256
