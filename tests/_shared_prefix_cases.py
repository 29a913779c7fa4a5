"""Case tables and seeded, poisoned inputs of the shared-prefix decode tests (tests/test_shared_prefix_host.py builds every case
on the CPU and checks the promise the operator's contract makes; tests/test_gpu_shared_prefix.py runs them).

A case is a list of groups (members, P shared pages, suffix length of every member). Shared pages are written ONCE and every
member's block-table row names them; the other conventions are those of tests/_decode_cases.py: pages dealt from a random
permutation with 3 spare blocks, NaN in K / Inf in V on every row past kv_len and on the spare blocks, table padding pointing at
spare blocks. Every case names the plan it is meant to reach -- rows per tile and token splits of the shared stage, heads per
workgroup and grid splits of the suffix stage (xllm_mi355_shared_prefix_decode_plan) -- worked out from the planner's rules:

  shared stage   rows_per_tile = 32; splits = max(1, min(1024 // (ceil(B * G / 32) * nkv), tiles // 4, 8)), tiles of 32 tokens
                 over the longest prefix
  suffix stage   decode_heads_per_wg / decode_num_splits of xllm_amd/csrc/attention_api.hip at max_kv_len (see _decode_cases.py)"""
import collections

import torch

import _decode_cases as dc

SUFFIXES = [130, 0, 1, 31, 32, 33]      # cycled inside each group: the leader gets 130 (more than a page of 16 / 64 / 128)

Shape = collections.namedtuple("Shape", "nq nkv d bs")
G7 = Shape(28, 4, 128, 128)
G2 = Shape(32, 16, 128, 16)
D64 = Shape(14, 2, 64, 64)

# name -> (shape, groups [(members, P, suffix lengths or None = SUFFIXES cycled)], plan (rows_per_tile, prefix_splits, hpw, suffix_nsplit),
#          index pairs (group, member) whose row agrees with the leader's for one page more than P)
Case = collections.namedtuple("Case", "name shape groups plan agree")


def _cyc(n, start=0):
    return [SUFFIXES[(start + i) % len(SUFFIXES)] for i in range(n)]


CASES = [
    # G = 7, B = 24: 1 (no prefix), 2, 3, 5, 13 sequences = 7, 14, 21, 35, 91 rows: below one N block, one N block + a part, a
    # tile + a part, two tiles with a tail. 24 waves -> splits = min(42, 12 // 4) = 3. Suffix: hpw 1, 17 tiles < 32 -> 1 split
    Case("g7", G7, [(1, 0, [33]), (2, 1, None), (3, 2, None), (5, 3, None), (13, 1, None)], (32, 3, 1, 1), [(4, 6)]),
    # G = 2, B = 40, pages of 16: 18, 16, 2 and 44 rows; 16, 32, 48 and 336 shared tokens. 48 waves, 11 tiles -> 2 splits.
    # Suffix: 40 * 16 / 2 = 320 workgroups -> hpw 2, 1 split
    Case("g2_page16", G2, [(9, 1, None), (8, 2, None), (1, 3, [130]), (22, 21, None)], (32, 2, 2, 1), []),
    # d = 64, B = 12: 6 waves, 10 tiles -> 2 splits. Suffix: nkv = 2, 12 workgroups -> hpw 1, 15 tiles -> 1 split
    Case("d64", D64, [(4, 1, None), (8, 5, None)], (32, 2, 1, 1), []),
    # the suffix stage under its own split-KV (_decode_cases.SPLIT_PLAN: hpw 1, 87 tiles / 32 = 2 grid splits); shared stage: 4
    # waves, 8 tiles -> 2 splits
    Case("suffix_split2", G7, [(3, 2, dc.SPLIT_LENS)], (32, 2, 1, 2), []),
    # the headline suffix plan: B = 192 -> hpw 4, 1 split; 168 waves, 4 tiles -> 1 split
    Case("b192_hpw4", G7, [(16, 1, None)] * 12, (32, 1, 4, 1), []),
    # degenerate groupings on the g7 lengths: every sequence alone without a prefix (and one empty row) ...
    Case("singletons", G7, [(1, 0, [L]) for L in [300, 0, 129, 1, 517, 33, 128, 64]], (32, 1, 1, 1), []),
    # ... one group of the whole batch with nothing but the prefix ...
    Case("all_prefix", G7, [(24, 2, [0] * 24)], (32, 2, 1, 1), []),
    # ... and padding rows (kv_len 0, singletons without a prefix) between and behind the groups
    Case("padding_rows", G7, [(3, 1, None), (1, 0, [0]), (4, 2, None), (1, 0, [0])], (32, 2, 1, 1), []),
]
CASE = {c.name: c for c in CASES}
# the second grouping of the graph-capture test: the batch size and the group count of "g7", other members and prefixes
G7_REGROUPED = Case("g7_regrouped", G7, [(13, 2, None), (5, 1, None), (3, 3, None), (2, 0, [5, 200]), (1, 1, [7])], (32, 3, 1, 1), [])
DTYPES = dc.DTYPES


def make_case(case, dtype, seed):
    """CPU tensors of one call: q [B, nq, d], caches, kv_lens, block table, group_cu, group_prefix_blocks, and the scalars"""
    nq, nkv, d, bs = case.shape
    g = torch.Generator().manual_seed(seed)
    lens, rows, cu, pre = [], [], [0], []           # rows: per sequence, the list of page SLOTS (indices into the permutation)
    n_slots = 0
    for gi, (n, P, suf) in enumerate(case.groups):
        suf = _cyc(n) if suf is None else list(suf)
        assert len(suf) == n
        shared = list(range(n_slots, n_slots + P))
        n_slots += P
        first = len(rows)
        for m in range(n):
            L = P * bs + suf[m]
            own = (L + bs - 1) // bs - P
            row = shared + list(range(n_slots, n_slots + own))
            n_slots += own
            if (gi, m) in case.agree:               # one more page in common with the leader than the group declares
                assert suf[m] >= bs and suf[0] >= bs
                row[P] = rows[first][P]
            rows.append(row)
            lens.append(L)
        cu.append(len(rows))
        pre.append(P)
    B = len(rows)
    nb = n_slots + 3
    perm = torch.randperm(nb, generator=g).tolist()
    spare = perm[n_slots:]
    table = torch.zeros(B, max(1, max(len(r) for r in rows)), dtype=torch.int32)
    for b, r in enumerate(rows):
        table[b, :len(r)] = torch.tensor([perm[s] for s in r], dtype=torch.int32)
    kc = torch.randn(nb, bs, nkv, d, generator=g).to(dtype)
    vc = torch.randn(nb, bs, nkv, d, generator=g).to(dtype)
    q = torch.randn(B, nq, d, generator=g).to(dtype)
    dc.poison(kc, vc, lens, table, spare, -1)
    return dict(case=case, q=q, kc=kc, vc=vc, kv_lens=torch.tensor(lens, dtype=torch.int32), block_tables=table,
                group_cu=torch.tensor(cu, dtype=torch.int32), group_prefix_blocks=torch.tensor(pre, dtype=torch.int32),
                scale=d ** -0.5, max_kv_len=max(lens), max_prefix_blocks=max(pre), dtype=dtype, B=B)


def check_promise(c):
    """what the operator's contract lets it assume: group_cu ascending from 0 to B, and for every member of a group with P
    pages the first P table entries are the leader's and kv_len >= P * block_size"""
    cu, pre, bt, lens = c["group_cu"].tolist(), c["group_prefix_blocks"].tolist(), c["block_tables"], c["kv_lens"].tolist()
    bs = c["kc"].shape[1]
    assert cu[0] == 0 and cu[-1] == c["B"] and all(a < b for a, b in zip(cu, cu[1:])) and len(pre) == len(cu) - 1
    assert c["max_prefix_blocks"] <= bt.shape[1]
    for gi, P in enumerate(pre):
        for b in range(cu[gi], cu[gi + 1]):
            assert torch.equal(bt[b, :P], bt[cu[gi], :P]) and lens[b] >= P * bs, (c["case"].name, gi, b)


_REFS = {}


def reference(c, key):
    """dense float64 decode attention on the case's tensors, rounded to its dtype; once per key, never modified"""
    if key not in _REFS:
        _REFS[key] = dc.dense_decode_ref64(c["q"], c["kc"], c["vc"], c["kv_lens"], c["block_tables"], c["scale"]).to(c["dtype"])
    return _REFS[key]


def seeded(case, dtype):
    key = (case.name, dtype)
    names = [x.name for x in CASES] + [G7_REGROUPED.name]
    return key, make_case(case, dtype, seed=7000 + names.index(case.name))
