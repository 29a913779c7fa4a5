"""GPU: the prefill / chunked-prefill flash kernels (xllm_amd/csrc/attention_prefill.hip) on every arm, mask edge and rescale
path against TWO references -- the CPU oracle and the dense float64 restatement of tests/_prefill_cases.py rounded to the tensor
dtype. Every case goes through ops.prefill_attention (unpaged) or ops.paged_attention with max_q_len > 1 (paged).

  arm (tests/_prefill_cases.py::ARMS)   kernel                                   d   K / V            P form   covered by
  m32_unpaged                           flash_prefill_m32_kernel<T, false, P1>  128  packed rows      one P    every test
  m32_paged                             flash_prefill_m32_kernel<T, true, P1>   128  pages of 64      one P    every test but layouts
  staged_paged_d128                     flash_prefill_kernel<T, 128, true>      128  pages of 16      hi + lo  masks, poison, rescale (control)
  staged_d64_unpaged                    flash_prefill_kernel<T, 64, false>       64  packed rows      hi + lo  masks, poison, layouts
  staged_d64_paged                      flash_prefill_kernel<T, 64, true>        64  pages of 16      hi + lo  masks, poison
  staged_wide_pitch                     flash_prefill_kernel<T, 128, false>     128  pitch 2^24       hi + lo  test_layouts[wide_pitch]
Under XLLM_MI355_PREFILL_P=2 (tests/test_zz_gpu_variants.py re-runs this file with it) the m32 arms are hi + lo arms too.

The arm is checked by numerics, not by a query function. A one-P case is held to tests/_bars.py::assert_p16_attention_close
(float64, p_round=True oracle, "flash" oracle within FLASH_BAR = 1e-3), a hi + lo case to assert_attn_close at 1e-3 (bf16) /
2e-4 (f16) against the fp32-P oracle and against float64; on bf16 rows of a hundred keys the two forms are ~2.5e-3 apart, so a
case the dispatcher moved to another arm fails. All whole-tensor bars are applied PER SEQUENCE. On top of them: no non-finite
element (the caller's out= is pre-filled with NaN, so a (head, sequence, q block) that no workgroup served shows), exact zeros
on rows that see no key, and a per-(query, head)-row bar of twice the oracle's own largest row distance from float64
(_prefill_cases.ROW_BAR; tests/test_prefill_reference.py shows on the CPU that moving any mask edge by one key moves every
touched row by more than twice that bar).

Every input is poisoned (K = NaN, V = Inf) where the call is not entitled to read: rows past kv_len in the last page, spare
pages, padding table entries, 64 rows behind cu_k[-1]; test_poison adds the table entries of pages wholly below the lowest
window bound of a sequence (a spare page with a valid id) and a neighbouring sequence that is all NaN / Inf. Rows of a LIVE
page below a query's window are finite (they hold earlier tokens in service; 0 x finite = 0): that is the contract.

What these tests catch, each tried on a scratch build of attention_prefill.hip (run of this file alone):
  1. `tok <= qpos` -> `tok < qpos`. In flash_prefill_kernel: every causal test_mask_edges, every test_poison, all six
     test_rescale and the test_layouts cases of the three staged arms plus test_layouts[wide_pitch] fail (83), no m32 test; in
     pf32_step: the same tests of the two m32 arms and all twelve test_block_coordinate_forms_under_a_window (76), no staged
     test. The non-causal mask cases pass, as they must.
  2. `tok >= qpos - window_left` -> `>`. In flash_prefill_kernel: test_mask_edges at W = 0, 1, 31, 32, 63, 64, 65, 100 causal and
     W = 32, 65 non-causal, test_poison, test_layouts[split_pitch] and [wide_pitch] on the staged arms (75); in pf32_step: the same
     on the m32 arms plus test_block_coordinate_forms_under_a_window (62). W = -1 and W = 2^40 pass, as they must.
  3. the window_left term of need_mask removed from the m32 kernel: the same 62 tests as 2. on the m32 arms.
  4. `acc_o[db] *= alpha` of pf32_step made a multiplication by 1: test_rescale[jump] and [staircase] on both m32 arms, bf16
     and f16 (8). near_miss passes (it never rescales), and so does every mask test: with flat inputs alpha != 1 only meets
     accumulators that are still zero -- the gap this file closes.
  5. the 2^8 threshold of pf32_step raised to 2^1000 (the maximum never moves after a row's first tile): test_rescale[staircase]
     on both m32 arms and both dtypes, test_rescale[jump] in bf16 (6). [jump] in f16 passes and cannot fail: without the move the
     row is the same softmax on another reference exponent, and an f16 P of 2^11 is as exact as one of 2^0.
  6. the zeroing of the V rows below lo_tok in flash_prefill_kernel::write_lds removed (the kernel as it was before this file):
     test_poison at (causal, W = 100) and (non-causal, W = 31) on staged_paged_d128 and staged_d64_paged, bf16 and f16 (8):
     non-finite rows. The m32 arms pass: a 64-key tile lies inside one page, so the window's edge tile is a live page.
  7. `acc_o[db] *= alpha` given twice the right factor wherever 0 < alpha < 1 (a subtly wrong rescale; the row sum keeps the right
     one): test_rescale[jump] and [staircase] on both m32 arms, bf16 and f16 (8), through the row bar -- the rows at the
     staircase's level edges and behind the jump keep >= 0.05 of their mass in front of it.
Largest distances seen on the default build (bf16 / f16). Relative L2 per sequence from float64: m32_unpaged 2.74e-3 / 3.37e-4,
m32_paged 2.94e-3 / 3.64e-4 (one 16-bit P: the p_round oracle itself is up to 3.4e-3 / 4.1e-4 away), from the "flash" oracle
1.15e-4 / 5.8e-5 (0.12 of FLASH_BAR); hi + lo arms, from either reference: staged_paged_d128 3.46e-4 / 3.1e-5,
staged_d64_unpaged 2.32e-4 / 6.0e-5, staged_d64_paged 2.51e-4 / 3.1e-5, wide pitch 2.13e-4, element-wise 0.93 of the bar (bf16,
one rounding flip) / 0.12. Per row, as a fraction of ROW_BAR: 0.33 ... 0.50 on every arm. 199 tests, 8 s."""
import pytest
import torch

import _prefill_cases as pc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from xllm_amd import ops
DEV = "cuda"
CASES = pc.all_cases()


def _of(kind):
    sel = [c for c in CASES if c[1] == kind]
    return pytest.mark.parametrize("name,kind,build", sel, ids=[c[0] for c in sel])


def _unpaged_layout(c):
    """q, k, v on the device in the case's layout, from ONE host-to-device copy per tensor"""
    nq, nkv, d, dt = c["nq"], c["nkv"], c["arm"].d, c["dtype"]
    q, k, v = c["q"].to(DEV), c["k"].to(DEV), c["v"].to(DEV)
    Tq, Tk = q.shape[0], k.shape[0]
    if c["layout"] == "packed":           # slices of one packed qkv row (Tq != Tk: the buffer has max(Tq, Tk) rows)
        buf = torch.full((max(Tq, Tk), (nq + 2 * nkv) * d), float("nan"), dtype=dt, device=DEV)
        buf[:Tq, :nq * d] = q.flatten(1)
        buf[:Tk, nq * d:(nq + nkv) * d] = k.flatten(1)
        buf[:Tk, (nq + nkv) * d:] = v.flatten(1)
        return (buf[:Tq, :nq * d].unflatten(-1, (nq, d)), buf[:Tk, nq * d:(nq + nkv) * d].unflatten(-1, (nkv, d)),
                buf[:Tk, (nq + nkv) * d:].unflatten(-1, (nkv, d)))
    if c["layout"] == "split_pitch":      # k pitch nkv * d + 64, v contiguous
        kb = torch.full((Tk, nkv * d + 64), float("nan"), dtype=dt, device=DEV)
        kb[:, :nkv * d] = k.flatten(1)
        kk = kb[:, :nkv * d].unflatten(-1, (nkv, d))
        assert kk.stride(0) != v.stride(0)
        return q, kk, v
    assert c["layout"] == "wide_pitch"    # column slices of one uninitialised [40, 1 << 24] buffer: row pitch 2^24 elements
    buf = torch.empty(40, pc.WIDE_PITCH, dtype=dt, device=DEV)
    buf[:, :nkv * d] = k[:40].flatten(1)
    buf[:, nkv * d:2 * nkv * d] = v[:40].flatten(1)
    kk, vv = buf[:, :nkv * d].unflatten(-1, (nkv, d)), buf[:, nkv * d:2 * nkv * d].unflatten(-1, (nkv, d))
    assert kk.stride(0) == pc.WIDE_PITCH and int(c["cu_k"][-1]) <= 40
    return q, kk, vv


def _run_and_check(name, build):
    key, c = build()
    arm = c["arm"]
    Tq = int(c["cu_q"][-1])
    out = torch.full((Tq, c["nq"] * arm.d), float("nan"), dtype=c["dtype"], device=DEV)
    if arm.paged:
        assert pc.arm_of(arm.d, True, arm.bs, c["nkv"] * arm.d) == arm.name and c["max_q_len"] > 1
        ops.paged_attention(c["q"].to(DEV), c["kc"].to(DEV), c["vc"].to(DEV), c["cu_q"].to(DEV), c["kv_lens"].to(DEV),
                            c["block_tables"].to(DEV), c["max_q_len"], c["max_kv_len"], c["scale"], is_causal=bool(c["causal"]),
                            window_left=c["window_left"], out=out)
    else:
        q, k, v = _unpaged_layout(c)
        assert pc.arm_of(arm.d, False, 0, max(k.stride(0), v.stride(0))) == arm.name
        ops.prefill_attention(q, k, v, c["cu_q"].to(DEV), c["cu_k"].to(DEV), c["max_q_len"], c["scale"],
                              is_causal=bool(c["causal"]), window_left=c["window_left"], out=out)
    return pc.check_output(out, c, key)


@_of("mask")
def test_mask_edges(name, kind, build):
    """flat inputs (q = randn / 8), one (causal, window_left) per call, eleven sequences per call: q_len 1 ... 257 on and either
    side of a wave, a q block and two q blocks, kv_len on and either side of the 64- and 128-key edges, kv_len - q_len from 0 to
    200, an empty sequence in the middle; unpaged, kv_len < q_len by 10 and by 1 as well. The W = 1 call passes a max_q_len 200
    past the longest sequence (padding q blocks)."""
    _run_and_check(name, build)


@_of("pform")
def test_block_coordinate_forms_under_a_window(name, kind, build):
    """pf_block_coords on the m32 arms at P = sequences x kv heads = 1, 2, 4, 8 (dealt over the XCDs), 10 (P >= 8) and 3 (the
    plain order), causal with window_left = 63, sequences of more than one q block"""
    _run_and_check(name, build)


@_of("poison")
def test_poison(name, kind, build):
    """paged: the table entries of pages wholly below max(0, kv_len - q_len - W) point at a poisoned spare page; the lengths
    put such a page into the first HALF of the window's edge tile of the 32-key kernel ((kv_len - q_len - W) mod 32 >= 16 at
    16-token pages: 300 / 44 / 100) and leave a control. Unpaged (neighbour): the sequence behind the asserted one is all NaN /
    Inf and shares its last tile."""
    _run_and_check(name, build)


@_of("rescale")
def test_rescale(name, kind, build):
    """the lazy rescale of pf32_step on non-zero accumulators: one key at index 208 whose score is 11 log2 units above every
    earlier one (jump: alpha = 2^-11 for half of a wave's lanes, 1 for the other half), 7.2 units (near_miss: below the 2^8
    threshold, no rescale, P up to 2^7 in front of the 16-bit conversion), three levels ~9.2 units apart in three successive
    tiles with forty keys on each of the first two (staircase: the row at each level's first key keeps >= 0.05 of its mass in
    front of the jump); staged_paged_d128 is the control on which every rise of the maximum rescales"""
    _run_and_check(name, build)


@_of("layout")
def test_layouts(name, kind, build):
    """k and v from two buffers of different row pitch (voff_k / voff_v of the m32 kernel, k_stride / v_stride of the staged
    one), and the single wide-pitch case that reaches flash_prefill_kernel<T, 128, false>"""
    _run_and_check(name, build)
