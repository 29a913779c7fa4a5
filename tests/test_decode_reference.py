"""CPU: the oracle's paged decode attention against a dense float64 restatement, on the poisoned inputs of every case that
tests/test_gpu_decode_plans.py runs on the GPU (tests/_decode_cases.py).

Two things follow from a pass: the oracle's window and tail semantics (which keys a row sees, that nothing outside them is
read) agree with an implementation that shares no code with it; and the two references the GPU file compares the kernel with
are no further apart than HALF of that file's bars on any case, so a kernel that meets one cannot miss the other for lack of
room between them."""
import pytest
import torch

import _decode_cases as dc


@pytest.mark.parametrize("name,build", dc.all_cases(), ids=[n for n, _ in dc.all_cases()])
def test_oracle_paged_decode_equals_dense_float64(name, build):
    for key, case in build():
        orc_out, ref = dc.references(case, key)
        assert torch.isfinite(orc_out.float()).all() and torch.isfinite(ref.float()).all(), key
        assert orc_out.shape == ref.shape == (case["plan"].B, case["plan"].nq * case["plan"].d)
        rel, elem = dc.distance(orc_out, ref)
        print(f"{name}: oracle vs fp64 rel L2 {rel:.3e} = {rel / dc.BAR_REL[case['dtype']]:.3f} bar, element-wise {elem:.3f} bar")
        assert rel <= 0.5 * dc.BAR_REL[case["dtype"]], (key, rel)
        assert elem <= 0.5, (key, elem)
        # rows of length 0 are zeros in both (the padded-row contract of the decode kernel)
        empty = case["kv_lens"] == 0
        assert not orc_out[empty].any() and not ref[empty].any()


def test_the_poison_is_where_the_docstring_says():
    """the inputs really hold what the GPU tests claim to survive: NaN / Inf past kv_len, below t_lo, in the spare blocks and
    behind every entry of a page wholly below the window -- and none inside the visible range"""
    plan = dc.PLAN["hpw4_krows_page16"]
    W = 40
    key, case = dc.window_cases(plan, W, torch.bfloat16)[0]
    kc, vc, bt, bs = case["kc"], case["vc"], case["block_tables"], plan.bs
    seen_whole_page = seen_edge = seen_tail = False
    for b, L in enumerate(case["kv_lens"].tolist()):
        npg = (L + bs - 1) // bs
        assert torch.isnan(kc[bt[b, npg:].long()]).all()                      # padding entries -> spare blocks
        if L == 0:
            continue
        rows_k = kc[bt[b, :npg].long()].reshape(-1, plan.nkv, plan.d)
        rows_v = vc[bt[b, :npg].long()].reshape(-1, plan.nkv, plan.d)
        lo = dc.t_lo_of(L, W)
        assert torch.isfinite(rows_k[lo:L].float()).all() and torch.isfinite(rows_v[lo:L].float()).all()
        assert torch.isnan(rows_k[:lo]).all() and torch.isinf(rows_v[:lo]).all()
        assert torch.isnan(rows_k[L:]).all() and torch.isinf(rows_v[L:]).all()
        seen_whole_page |= lo >= bs
        seen_edge |= lo % 32 != 0
        seen_tail |= L % bs != 0
    assert seen_whole_page and seen_edge and seen_tail


def test_window_lengths_hit_every_edge():
    """each binding window_left meets t_lo = 0, 1, a tile boundary, one key short of it and a 16-token page boundary inside a
    tile, next to rows it does not bind, L = 1 and L = 0"""
    for W in dc.WINDOWS[:-1]:
        ls = dc.window_len_list(W)
        lo = {dc.t_lo_of(L, W) for L in ls if L > W + 1}
        assert {1, 16, 17, 31, 32, 63, 64} <= lo, (W, sorted(lo))
        assert W + 1 in ls and 1 in ls and 0 in ls and max(ls) <= 300
        for plan in dc.WINDOW_PLANS:
            flat = [L for batch in dc.window_batches(plan, W) for L in batch]
            assert set(ls) <= set(flat) and all(len(b) == plan.B for b in dc.window_batches(plan, W))
    assert 0 in dc.ragged_lens(4) and set(dc.LENS) | {0} == set(dc.ragged_lens(192))
    # split-KV under a window: the live tiles of the longest row, against its 2 x 4 slots
    live = [(2500 + 31) // 32 - dc.t_lo_of(2500, W) // 32 for W in dc.SPLIT_WINDOWS]
    assert live == [3, 5, 34]          # of 8 slots: 5 and 3 own nothing, then one
