"""CPU: the room between the two references of the top-k / top-p tests, and the arm table.

oracle/sampling.py::apply_top_k_top_p (the reference's torch expressions: stable sort, fp32 softmax, fp32 cumsum) is run over
every launch of tests/_logits_cases.py and held to the float64 restatement ref64 under the bars the GPU test holds the kernel
to: the same surviving set on every "clear" row, a prefix of the sorted order that leaves float64's cut only across ranks whose
prefix is within 2e-5 of p on the "step" rows. That the fp32 oracle meets the "clear" bar is what makes the bar a fair one for a
kernel that accumulates in 2^-40 fixed point; it also proves the builders' MIN_GAP assertion for the reference alone.

Largest |prefix - p| at a rank on which the oracle and float64 disagree (printed per case; all on "step" rows): 1.22e-06 (bf16,
vector_multi_step, V = 16896: the fp32 cumsum's rounding over 17k terms); at V <= 4099 it stays below 2.3e-07. The kernel's own
figure is in the docstring of tests/test_gpu_logits_processors.py."""
import pytest
import torch

import _logits_cases as lc
from oracle import sampling as osm

# the model vocabulary adds nothing here that V = 16896 does not show, and costs the most
KEYS = [k for k in lc.CASE_KEYS if k[0] != "model_vocab"]


def test_arm_on_hand_computed_rows():
    f32, bf16, f16 = lc.DTYPES
    assert lc.arm(bf16, 1000, 0, 1000, 3) == ["vector"] * 3                # 2000 bytes per row: every row on a boundary
    assert lc.arm(f32, 1000, 0, 1000, 2) == ["vector"] * 2
    assert lc.arm(bf16, 1003, 0, 1003, 9) == ["scalar"] * 9                # 1003 columns are no whole number of 8-column vectors,
    assert lc.arm(f32, 4099, 0, 4099, 5) == ["scalar"] * 5                 # ... aligned (row 0, row 8 of bf16) or not
    assert lc.arm(f16, 1000, 2, 1008, 4) == ["scalar"] * 4                 # wide[:, 1:1001]: v_head = 7 on every row
    assert lc.arm(f32, 1000, 4, 1008, 4) == ["scalar"] * 4                 # v_head = 3
    # f32, pitch 1003: row b starts at 4012 b = 12 b (mod 16): aligned when b is a multiple of 4
    assert lc.arm(f32, 1000, 0, 1003, 9) == ["vector", "scalar", "scalar", "scalar"] * 2 + ["vector"]
    # 16 bit, pitch 1004: 2008 b = 8 b (mod 16): the even rows
    assert lc.arm(bf16, 1000, 0, 1004, 4) == ["vector", "scalar"] * 2
    assert lc.arm(f16, 1000, 0, 1008, 3) == ["vector"] * 3 and lc.arm(f32, 1000, 0, 1004, 3) == ["vector"] * 3
    assert lc.arm(f16, 5, 14, 5, 1) == ["scalar"]                          # v_head = 1, no whole vector
    assert lc.arm(f32, 2, 8, 2, 1) == ["scalar"]                           # v_head = V: the head loop is the whole row
    # segments: ceil(V / 16) columns per wave, rounded up to a step of 64 lanes x one vector (one column in the scalar form)
    assert lc.segment(bf16, 1000, "vector") == (512, 512) and lc.segment(f32, 1000, "vector") == (256, 256)
    assert lc.segment(bf16, 16896, "vector") == (1536, 512) and lc.segment(f32, 8448, "vector") == (768, 256)
    assert lc.segment(f16, 1003, "scalar") == (64, 64) and lc.segment(f16, 4099, "scalar") == (320, 64)
    assert lc.segment(bf16, 152064, "vector") == (9728, 512)


def test_every_table_row_is_in_its_arm():
    for mech, dtype in lc.CASE_KEYS:
        name, V, layout, expect = next(m for m in lc.mechanisms(dtype) if m[0] == mech)
        arms = lc.arm(dtype, V, layout.off * lc.SIZE[dtype], layout.pitch, 8)
        assert lc.arms_match(arms, expect), (mech, dtype, arms)
        assert layout.off + V <= layout.pitch or layout.off == 0


def test_ref64_on_hand_computed_rows():
    row = torch.tensor([0.0, 2.0, 1.0, 2.0, -1.0])                         # sorted: columns 1, 3, 2, 0, 4
    r = lc.ref64(row, 3, None, "one")
    assert r.keep.tolist() == [False, True, True, True, False] and list(r.order) == [1, 3, 2, 0, 4]
    assert lc.ref64(row, 1, None, "one").keep.tolist() == [False, True, False, False, False]      # of two ties, the lower column
    for k in (0, -1, 5, 9):
        assert lc.ref64(row, k, None, "one").n == 5
    e = torch.tensor([1.0, 1.0, torch.e ** -1, torch.e ** -2, torch.e ** -3]).double()
    z = float(e.sum())
    # exclusive prefixes 0, 1/z, 2/z, ...: p just above 2/z keeps three ranks, just below it two
    assert lc.ref64(row, None, 2 / z + 1e-3, "one").n == 3 and lc.ref64(row, None, 2 / z - 1e-3, "one").n == 2
    # inclusive prefixes 1/z, 2/z, ...: the same p keeps two ranks / one
    assert lc.ref64(row, 5, 2 / z + 1e-3, "both").n == 2 and lc.ref64(row, 5, 2 / z - 1e-3, "both").n == 1
    for rule in ("one", "both"):
        for p in (0.0, -0.5, 1e-30):
            assert lc.ref64(row, None if rule == "one" else 4, p, rule).keep.tolist() == [False, True, False, False, False]
        assert lc.ref64(row, None if rule == "one" else 4, 1.0, rule).n == (5 if rule == "one" else 4)
    # top-k renormalises: with k = 2 the inclusive prefixes are 1/2 and 1
    assert lc.ref64(row, 2, 0.75, "both").n == 1 and lc.ref64(row, 2, 1.0, "both").n == 2


@pytest.mark.parametrize("key", KEYS, ids=[i for i, k in zip(lc.CASE_IDS, lc.CASE_KEYS) if k in KEYS])
def test_fp32_oracle_against_float64(key):
    c = lc.case(*key)
    worst, kinds = 0.0, set()
    for L in c.launches:
        out = osm.apply_top_k_top_p(L.scaled.float(), None, L.k, L.p).to(c.dtype)
        worst = max(worst, lc.check_rows(out, L, "oracle", oracle=True))
        kinds |= {L.name.split("/")[0]}
    print(f"{lc.CASE_IDS[lc.CASE_KEYS.index(key)]}: largest |prefix - p| at a disagreeing rank = {worst:.3g}")
    assert kinds == {"clear", "tie", "neg", "edge", "step"}
