"""GPU: every arm of the logits processors (xllm_amd/csrc/logits_processors.hip) against the dense float64 restatement of
tests/_logits_cases.py, for f32, bf16 and f16 logits.

top_k_top_p_kernel chooses its code from (dtype, V, row address, pitch): every test first asserts, from the tensor's real
address, the arm its case is in the table for.

  mechanism (tests/_logits_cases.py::mechanisms)          V               layout                      arm
  vector_one_step     one step per wave                   1000            contiguous                  vector
  vector_multi_step   3 steps per wave, 3 sweep rounds    16896 / 8448    contiguous                  vector
  scalar_tail         V is no whole number of vectors     1003            contiguous                  scalar
  scalar_multi_step   ... 5 steps of 64 columns per wave  4099            contiguous                  scalar
  scalar_head         every row starts off a boundary     1000            wide[:, 1:1001]             scalar
  mixed_pitch         aligned and unaligned rows          1000            pitch 1004 (f32: 1003)      both in one launch
  pitched_vector      pitch > V, rows stay aligned        1000            pitch 1008 (f32: 1004)      vector
  model_vocab         19 sweep rounds (bf16, 8 rows)      152064          contiguous                  vector

Every case runs the same launches: clear/* (random rows under a temperature, p on the midpoint of two float64 prefixes >= 1e-4
apart), tie/* (a group of equal values across a seam of the final pass -- inside one lane's vector, lane | lane, step | step,
wave | wave -- as the top-k boundary, as the top-p boundary, and as both with top-p cutting inside what top-k kept; the cut
leaves exactly the columns up to the seam, then one more), neg/* (negative boundary keys), edge/* (k in {1, 2, V - 1, V, V + 5,
0, -1} x p in {0, 1e-30, 1, 1.5, -0.5}, rows whose second-largest logit has no mass in 2^-40 fixed point) and step/* (p on a
float64 prefix and on its fp32 neighbours).

Bars: on clear, tie, neg and edge rows the surviving set EQUALS float64's; on step rows it is a prefix of the stable sorted
order and every rank it disagrees on has its prefix within 2e-5 of p. Survivors are bit-equal to the temperature-scaled,
dtype-rounded input, dropped columns are -inf, the pad columns of a pitched tensor and a guard row behind it keep their bits,
two runs give the same bits.

Largest |prefix - p| at a rank on which the kernel and float64 disagree (step rows only; printed by every test_top_k_top_p):
1.31e-08 (f32, vector_multi_step, step/p), 1.16e-08 for f16 (vector_multi_step and scalar_multi_step, step/p) and 5.41e-09 for bf16
(mixed_pitch, step/p): 0.0007 of the band. The fp32 oracle's own largest is 1.22e-06 (tests/test_logits_reference.py).

What these tests catch, each tried on a scratch build of logits_processors.hip:
  * lp_low returns `prefix` for a negative key (the low bits stay zero): every bf16 and f16 test_top_k_top_p fails, first in
    neg/k (model_vocab: vocab/k); f32 has no low bits to complete and passes;
  * `ex_k += r_k; ex_p += r_p` dropped (a tie forgets the earlier waves and steps): every vector-arm and mixed test_top_k_top_p
    (tie/k first), test_rows_are_independent and the vector and mixed cases of test_fused_sampler fail; the scalar arm passes;
  * `r_k += tot_k; r_p += tot_p` dropped (no carry from step to step): test_top_k_top_p[vector_multi_step-*] and [model_vocab-bf16]
    fail (tie/k: the step | step seam) and nothing else does -- at one step per wave the carry is never read;
  * the sweep's head loop dropped: every scalar_head and mixed_pitch case fails, and so do scalar_tail / scalar_multi_step, whose
    rows 1 .. 7 start off a boundary as well (clear/k first: wrong histograms); the sweep's tail loop dropped: the same cases.
    (`v_head` forced to 0 instead was NOT tried: the sweep would then issue 16-byte loads at unaligned addresses, whose
    outcome is a property of the device's memory mode, not of this code.)
  * f16 kLowShift = 16 (two digits, as for bf16): every f16 test_top_k_top_p (clear/k, clear/p) and every f16
    test_fused_sampler case fail; f32 and bf16 pass;
  * `sh.cnt[bb] += kth_live` on the first digit only: every test_top_k_top_p fails in tie/both (vocab/both), and the fused
    sampler's tie/both launch with it -- the launches where ONE key is both boundaries."""
import pytest
import torch

import _logits_cases as lc
from oracle import sampling as osm

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from xllm_amd import _lib, ops
DEV = "cuda"
_dt_ids = [lc.NAME[d] for d in lc.DTYPES]


def _place(rows, layout):
    """rows [B, V] as a view of a sentinel-filled [B + 1, pitch] device tensor (the last row is a guard); returns (wide, view)"""
    B, V = rows.shape
    wide = torch.full((B + 1, layout.pitch), lc.SENTINEL, dtype=rows.dtype, device=DEV)
    assert wide.data_ptr() % 16 == 0
    view = wide[:B, layout.off:layout.off + V]
    view.copy_(rows)
    return wide, view


def _arms(view, dtype):
    return lc.arm(dtype, view.size(1), view.data_ptr() % 16, view.stride(0), view.size(0))


def _assert_outside_untouched(wide, layout, B, V):
    outside = torch.ones(wide.shape, dtype=torch.bool)
    outside[:B, layout.off:layout.off + V] = False
    w = wide.cpu()
    assert torch.equal(w[outside], torch.full_like(w[outside], lc.SENTINEL)), "a pad column or the guard row was written"


def _dev(t):
    return None if t is None else t.to(DEV)


@pytest.mark.parametrize("key", lc.CASE_KEYS, ids=lc.CASE_IDS)
def test_top_k_top_p(key):
    c = lc.case(*key)
    assert lc.arms_match(lc.expected_arms(c, 8), c.expect), (key, lc.expected_arms(c, 8))
    worst, where = 0.0, None
    for L in c.launches:
        B = L.rows.size(0)
        wide, view = _place(L.rows, c.layout)
        assert _arms(view, c.dtype) == lc.expected_arms(c, B), (L.name, _arms(view, c.dtype))
        ops.apply_top_k_top_p(view, _dev(L.temps), _dev(L.k), _dev(L.p))
        wide2, view2 = _place(L.rows, c.layout)
        ops.apply_top_k_top_p(view2, _dev(L.temps), _dev(L.k), _dev(L.p))
        assert torch.equal(wide.view(torch.uint8), wide2.view(torch.uint8)), L.name            # run to run: the same bits
        _assert_outside_untouched(wide, c.layout, B, c.V)
        got = view.cpu()
        off = lc.check_rows(got, L, "kernel")
        if off > worst:
            worst, where = off, L.name
        # against the fp32 oracle too where it is defined and p is clear of every step
        if all(k == "clear" for k in L.kinds) and not any(L.quirk) and (L.p is None or not bool((L.p == 1.0).any())):
            ref = osm.apply_top_k_top_p(L.scaled.float(), None, L.k, L.p).to(c.dtype)
            assert torch.equal(got, ref), L.name
    print(f"{lc.CASE_IDS[lc.CASE_KEYS.index(key)]}: largest |prefix - p| at a disagreeing rank = {worst:.3g} ({where})")


@pytest.mark.parametrize("dtype", lc.DTYPES, ids=_dt_ids)
def test_rows_are_independent(dtype):
    """one launch over the mixed-arm pitched layout, every row with its own (temperature, k, p): each row equals the same row run
    alone in a contiguous [1, V] tensor"""
    V = 1000
    layout = next(m[2] for m in lc.mechanisms(dtype) if m[0] == "mixed_pitch")
    g = torch.Generator().manual_seed(5)
    rows = (torch.randn(8, V, generator=g) * 2.5).to(dtype)
    rows[6] = rows[6].float().round().to(dtype)                                      # ties everywhere
    temps = torch.tensor([1.0, 0.0, 0.7, 1.3, 2.0, 0.5, 1.0, 0.9])
    top_k = torch.tensor([50, -1, 2, 300, V, 17, 5, 0], dtype=torch.int64)
    top_p = torch.tensor([0.9, 0.5, 1.0, 0.999, 0.3, 1.0, 0.6, 0.75])
    for k, p in ((top_k, None), (None, top_p), (top_k, top_p)):
        wide, view = _place(rows, layout)
        assert set(_arms(view, dtype)) == {"vector", "scalar"}
        ops.apply_top_k_top_p(view, temps.to(DEV), _dev(k), _dev(p))
        _assert_outside_untouched(wide, layout, 8, V)
        for b in range(8):
            alone = rows[b:b + 1].clone().to(DEV)
            assert _arms(alone, dtype) == ["vector"]
            ops.apply_top_k_top_p(alone, temps[b:b + 1].to(DEV), None if k is None else k[b:b + 1].to(DEV),
                                  None if p is None else p[b:b + 1].to(DEV))
            assert torch.equal(view[b].cpu(), alone[0].cpu()), (b, k is not None, p is not None)


def _place_u(L):
    """u per row on the midpoint of two adjacent float64 CDF steps >= MIN_GAP apart of the surviving set (CDF in column order, as
    the sampler inverts it); returns (u, the column float64 inversion gives)"""
    us, toks = [], []
    for b, ref in enumerate(L.refs):
        x = L.scaled[b].double()
        m = torch.where(ref.keep, torch.exp(x - x.max()), torch.zeros_like(x))
        prob = m / m.sum()
        cdf = prob.cumsum(0)
        cand = torch.nonzero(prob >= lc.MIN_GAP).flatten()
        j = int(cand[len(cand) // 2])
        us.append(float(cdf[j] - prob[j] / 2))
        toks.append(j)
    return torch.tensor(us, dtype=torch.float32), torch.tensor(toks, dtype=torch.int32)


_FUSED = [(m, d) for d in lc.DTYPES for m in ("vector_one_step", "scalar_tail", "scalar_head", "mixed_pitch", "pitched_vector")
          if m != "vector_one_step" or d == torch.float16]


@pytest.mark.parametrize("key", _FUSED, ids=[f"{m}-{lc.NAME[d]}" for m, d in _FUSED])
def test_fused_sampler_on_the_same_layouts(key):
    """ops.sample_top_k_top_p on the f16, scalar-arm and pitched cases: processed logits bit-equal to apply_top_k_top_p alone,
    and with u clear of every CDF step the token EQUALS float64 CDF inversion over the float64 surviving set"""
    c = lc.case(*key)
    assert lc.arms_match(lc.expected_arms(c, 8), c.expect)
    for L in c.launches:
        if L.name not in ("clear/k", "clear/p", "clear/both", "tie/both"):
            continue
        B = L.rows.size(0)
        wide, view = _place(L.rows, c.layout)
        assert _arms(view, c.dtype) == lc.expected_arms(c, B)
        ops.apply_top_k_top_p(view, _dev(L.temps), _dev(L.k), _dev(L.p))
        u, want = _place_u(L)
        wide2, view2 = _place(L.rows, c.layout)
        tok = ops.sample_top_k_top_p(view2, _dev(L.temps), _dev(L.k), _dev(L.p), uniform=u.to(DEV)).cpu()
        assert torch.equal(wide.view(torch.uint8), wide2.view(torch.uint8)), L.name
        _assert_outside_untouched(wide2, c.layout, B, c.V)
        assert torch.equal(tok, want), (L.name, tok.tolist(), want.tolist())


_PEN_LAYOUTS = {"contiguous": lambda d: lc.Layout(0, 1000), "scalar_head": lambda d: lc.Layout(1, 1008),
                "mixed_pitch": lambda d: lc.Layout(0, 1003 if d == torch.float32 else 1004)}


@pytest.mark.parametrize("dtype", lc.DTYPES, ids=_dt_ids)
@pytest.mark.parametrize("lay", list(_PEN_LAYOUTS))
def test_penalties_and_temperatures_layouts(lay, dtype):
    """apply_penalties / apply_temperatures in every dtype, contiguous and pitched: bit-equal to the expressions of
    logits_utils.cpp:24-64 with the in-place operators' cast points written out (fp32 arithmetic, rounded to the logits dtype
    after each of sub_, sub_, where); ids outside [0, V) are skipped and nothing is written outside the rows; a live id listed
    twice with the same count gives the single-copy result (both copies are computed from the row as it was before the call)"""
    layout = _PEN_LAYOUTS[lay](dtype)
    B, V, U = 5, 1000, 12
    g = torch.Generator().manual_seed(11)
    rows = (torch.randn(B, V, generator=g) * 3).to(dtype)
    ids = torch.stack([torch.randperm(V - 1, generator=g)[:U] + 1 for _ in range(B)])      # live ids in [1, V): 0 is the padding id
    cnt = torch.randint(1, 6, (B, U), generator=g, dtype=torch.int32)
    ids[:, 4], ids[:, 9] = -1, V + 3                                                       # outside [0, V): skipped
    ids[:, 7], cnt[:, 7] = ids[:, 2], cnt[:, 2]                                            # one live id twice, the same count
    ids[1, 10:], cnt[1, 10:] = 0, 0                                                        # padding: id 0, count 0
    freq, pres = torch.rand(B, generator=g) * 2 - 0.5, torch.rand(B, generator=g) * 2 - 0.5
    rep = torch.rand(B, generator=g) * 1.5 + 0.5
    rt = lambda t: t.to(dtype).float()
    valid = (ids >= 0) & (ids < V)
    for use_fp, use_rep in ((True, True), (True, False), (False, True)):
        sc = rows.float().gather(1, ids.clamp(0, V - 1))
        if use_fp:
            sc = rt(sc - cnt * freq.unsqueeze(1))
            sc = rt(sc - (cnt > 0) * pres.unsqueeze(1))
        if use_rep:
            sc = rt(torch.where(sc < 0, sc * rep.unsqueeze(1), sc / rep.unsqueeze(1)))
        want = rows.float().clone()
        for b in range(B):
            for u in range(U):
                if valid[b, u]:
                    want[b, ids[b, u]] = sc[b, u]
        wide, view = _place(rows, layout)
        ops.apply_penalties(view, ids.to(DEV), cnt.to(DEV), _dev(freq) if use_fp else None, _dev(pres) if use_fp else None,
                            _dev(rep) if use_rep else None)
        assert torch.equal(view.float().cpu(), want), (use_fp, use_rep)
        _assert_outside_untouched(wide, layout, B, V)
        keep = [u for u in range(U) if u != 7]
        wide1, view1 = _place(rows, layout)
        ops.apply_penalties(view1, ids[:, keep].to(DEV), cnt[:, keep].to(DEV), _dev(freq) if use_fp else None,
                            _dev(pres) if use_fp else None, _dev(rep) if use_rep else None)
        assert torch.equal(view1.float().cpu(), want)                                      # the single-copy result
    # U = 0 and B = 0: nothing to do, nothing written
    wide, view = _place(rows, layout)
    ops.apply_penalties(view, ids[:, :0].to(DEV), cnt[:, :0].to(DEV), _dev(freq), _dev(pres), _dev(rep))
    # (a [0, V] tensor has no address: batch = 0 goes straight through the C ABI, with every other argument live)
    d_ids, d_cnt, d_f, ws = ids.to(DEV), cnt.to(DEV), freq.to(DEV), torch.empty(B * U, dtype=torch.float32, device=DEV)
    stream, dt = torch.cuda.current_stream().cuda_stream, ops._DT[dtype]
    lib = _lib.lib()
    assert lib.xllm_mi355_apply_penalties(view.data_ptr(), 0, V, view.stride(0), dt, d_ids.data_ptr(), d_cnt.data_ptr(), U,
                                          d_f.data_ptr(), d_f.data_ptr(), d_f.data_ptr(), ws.data_ptr(), ws.numel() * 4, stream) == 0
    assert lib.xllm_mi355_apply_temperatures(view.data_ptr(), 0, V, view.stride(0), dt, d_f.data_ptr(), stream) == 0
    assert lib.xllm_mi355_apply_top_k_top_p(view.data_ptr(), 0, V, view.stride(0), dt, d_f.data_ptr(), 0, d_f.data_ptr(), stream) == 0
    assert torch.equal(view.cpu(), rows)
    _assert_outside_untouched(wide, layout, B, V)
    temps = torch.tensor([0.0, 1.0, 0.7, 1.3, 2.0])
    ops.apply_temperatures(view, temps.to(DEV))
    assert torch.equal(view.cpu(), lc.scaled(rows, temps))
    _assert_outside_untouched(wide, layout, B, V)
