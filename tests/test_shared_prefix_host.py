"""CPU-side checks of shared-prefix decode (xllm_mi355_paged_decode_attention_shared_prefix and its companions): the symbols,
the validation that happens before any device work, the host grouping rule against a restatement in Python, the same helper
under AddressSanitizer + UBSan in a stand-alone program, and the GPU file's case builders (every case keeps the promise the
operator's contract lets it rely on, and the float64 reference runs on it)."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import _shared_prefix_cases as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["xllm_mi355_shared_prefix_decode_workspace_bytes", "xllm_mi355_shared_prefix_decode_plan",
           "xllm_mi355_paged_decode_attention_shared_prefix", "xllm_mi355_host_shared_prefix_groups"]
XM_ERR_INVALID, XM_ERR_UNSUPPORTED, XM_ERR_WORKSPACE = -1, -2, -4
# the operator's C declarations: a header of its own next to the kernels (include/ is pinned by tests/test_host_abi.py)
HEADER = os.path.join(ROOT, "xllm_amd", "csrc", "xllm_mi355_shared_prefix.h")


def _built():
    import __graft_entry__ as g
    from xllm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        os.environ["XLLM_MI355_SKIP_SHIM"] = "1"
        g.build()
    return _lib


def test_symbols_declared_exported_and_bound():
    _lib = _built()
    hdr = open(HEADER).read()
    declared = set(re.findall(r"XM_API\s+[\w\s\*]+?\b(xllm_mi355_\w+)\s*\(", hdr))
    exported = set(re.findall(r"\b(xllm_mi355_\w+)\b", subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()))
    for s in SYMBOLS:
        assert s in declared and s in exported and s in _lib.exported_symbols(), s
        assert getattr(_lib.lib(), s).argtypes is not None
    assert _lib.lib().xllm_mi355_abi_version() == 2


def _call(l, ws_bytes, d=128, nq=28, nkv=4, null=False, dtype=1, n_groups=1, max_prefix_blocks=2, max_blocks=8):
    """the entry point with host addresses that are never dereferenced: every case here must return before any device work"""
    buf = (C.c_char * 64)()
    a = 0 if null else (C.addressof(buf) + 15) // 16 * 16
    return l.xllm_mi355_paged_decode_attention_shared_prefix(a, a, a, a, a, a, max_blocks, a, a, n_groups, 4, nq, nkv, d, 128, 64,
                                                             nq * d, 1024, max_prefix_blocks, 0.1, 0, dtype, a, ws_bytes, None)


def test_validation_happens_without_a_device():
    l = _built().lib()
    need = l.xllm_mi355_shared_prefix_decode_workspace_bytes(4, 28, 128, 8, 1024, 4)
    assert need > 0
    assert _call(l, need, null=True) == XM_ERR_INVALID
    assert _call(l, need, n_groups=0) == XM_ERR_INVALID
    assert _call(l, need, max_prefix_blocks=9) == XM_ERR_INVALID          # more than max_blocks
    assert _call(l, need, d=96) == XM_ERR_UNSUPPORTED
    assert _call(l, need, nq=68) == XM_ERR_UNSUPPORTED                    # 17 q heads per kv head
    assert _call(l, need, dtype=0) == XM_ERR_UNSUPPORTED                  # f32
    assert _call(l, need - 1) == XM_ERR_WORKSPACE
    assert l.xllm_mi355_shared_prefix_decode_plan(0, 28, 4, 128, 1, 128, None, None, None, None) == XM_ERR_INVALID


def test_workspace_bytes_is_monotone():
    l = _built().lib()
    f = l.xllm_mi355_shared_prefix_decode_workspace_bytes
    prev = 0
    for B in (1, 2, 3, 20, 32, 64, 192, 256):                             # batch (the suffix planner's split count falls with it)
        cur = f(B, 28, 128, 32, 4096, 4)
        assert cur > prev
        prev = cur
    prev = 0
    for L in (32, 1024, 4096, 32768, 1 << 20):                            # length: more grid splits in both stages
        cur = f(8, 28, 128, max(1, L // 128), L, 4)
        assert cur >= prev > -1
        prev = cur
    # room for the split counts both planners return at these shapes: their (o, m, l) rows and the metadata
    for B, L in ((1, 1 << 20), (8, 4096), (256, 4096)):
        v = [C.c_int32(0) for _ in range(4)]
        assert l.xllm_mi355_shared_prefix_decode_plan(B, 28, 4, 128, L // 128, L, *[C.addressof(x) for x in v]) == 0
        rows, psplit, hpw, nsplit = [x.value for x in v]
        assert rows == 32 and 1 <= psplit <= 8 and 1 <= nsplit <= 32 and hpw in (1, 2, 4)
        assert f(B, 28, 128, L // 128, L, 4) >= B * 28 * (nsplit + psplit) * 130 * 4 + (2 * B + B * (L // 128)) * 4


# ---- the grouping rule, restated
def _groups_py(table, lens, bs, min_group, min_prefix):
    B, cu, pre, i = len(lens), [0], [], 0
    while i < B:
        j, c = i + 1, min(lens[i] // bs, len(table[i]))
        while lens[i] > 0 and j < B and lens[j] > 0:
            common = next((k for k, (x, y) in enumerate(zip(table[i], table[j])) if x != y), len(table[i]))
            c2 = min(c, common, lens[j] // bs)
            if c2 < min_prefix:
                break
            c, j = c2, j + 1
        whole = lens[i] > 0 and j - i >= min_group and c >= min_prefix
        for end, p in ([(j, c)] if whole else [(b + 1, 0) for b in range(i, j)]):
            cu.append(end)
            pre.append(p)
        i = j
    return cu, pre


def _groups_c(table, lens, bs, min_group, min_prefix):
    from xllm_amd import attention
    cu, pre = attention.shared_prefix_groups(torch.tensor(table, dtype=torch.int32).reshape(len(lens), -1), lens, bs, min_group, min_prefix)
    return cu.tolist(), pre.tolist()


def _tables():
    """(name, table, kv_lens, block_size, min_group, min_prefix_blocks, expected or None)"""
    eq = [[5, 6, 7, 8]] * 4
    out = [
        ("all rows equal", eq, [512] * 4, 128, 2, 1, ([0, 4], [4])),
        ("no two rows equal", [[1, 2], [3, 4], [5, 6]], [256] * 3, 128, 2, 1, ([0, 1, 2, 3], [0, 0, 0])),
        ("prefix shrinks as members join", [[1, 2, 3, 4], [1, 2, 3, 9], [1, 2, 8, 9], [1, 7, 8, 9]], [512] * 4, 128, 2, 1, ([0, 4], [1])),
        ("shrinks until min_prefix cuts", [[1, 2, 3, 4], [1, 2, 3, 9], [1, 2, 8, 9], [1, 7, 8, 9]], [512] * 4, 128, 2, 2, ([0, 3, 4], [2, 0])),
        ("cut by a first entry", [[1, 2], [1, 2], [9, 2], [9, 2], [9, 3]], [256] * 5, 128, 2, 1, ([0, 2, 5], [2, 1])),
        ("runs shorter than min_group", [[1, 2], [1, 2], [3, 4], [3, 4], [3, 4]], [256] * 5, 128, 3, 1, ([0, 1, 2, 5], [0, 0, 2])),
        ("kv_len caps the prefix at full pages", eq, [512, 300, 511, 129], 128, 2, 1, ([0, 4], [1])),
        ("kv_len below one page leaves no prefix", eq, [512, 100, 512, 512], 128, 2, 1, ([0, 1, 2, 4], [0, 0, 4])),
        ("kv_len = 0 inside a run", eq, [512, 512, 0, 512], 128, 2, 1, ([0, 2, 3, 4], [4, 0, 0])),
        ("batch 1", [[4, 5]], [256], 128, 1, 1, ([0, 1], [2])),
        ("batch 1, min_group 2", [[4, 5]], [256], 128, 2, 1, ([0, 1], [0])),
    ]
    g = torch.Generator().manual_seed(11)
    r = lambda hi, n=1: torch.randint(0, hi, (n,), generator=g).tolist()
    for i in range(200):                                              # few distinct ids and lengths: long and short runs, zeros
        B, W, bs = r(9)[0] + 1, r(4)[0] + 1, (16, 128)[i % 2]
        table = [r(2, W) for _ in range(B)]
        lens = [0 if x == 0 else x * bs // 2 - r(3)[0] for x in r(2 * W + 2, B)]
        lens = [max(0, L) for L in lens]
        out.append((f"random {i}", table, lens, bs, r(3)[0] + 1, r(3)[0], None))
    return out


def test_host_groups_follow_the_rule():
    _built()
    for name, table, lens, bs, mg, mp, expected in _tables():
        got = _groups_c(table, lens, bs, mg, mp)
        assert got == _groups_py(table, lens, bs, mg, mp), name
        if expected is not None:
            assert got == expected, name
        cu, pre = got                                                 # and what the operator is promised holds
        assert cu[0] == 0 and cu[-1] == len(lens) and all(a < b for a, b in zip(cu, cu[1:]))
        for gi, P in enumerate(pre):
            for b in range(cu[gi], cu[gi + 1]):
                assert table[b][:P] == table[cu[gi]][:P] and lens[b] >= P * bs, name


_MAIN = r"""
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "xllm_mi355_shared_prefix.h"
// input: n_cases, then per case B W bs min_group min_prefix, B*W table entries, B lens; output: per case cu... | pre...
int main() {
  int n;
  if (scanf("%d", &n) != 1) return 2;
  for (int c = 0; c < n; ++c) {
    long B, W, bs, mg, mp;
    if (scanf("%ld %ld %ld %ld %ld", &B, &W, &bs, &mg, &mp) != 5) return 2;
    std::vector<int32_t> table(B * W), lens(B), cu(B + 1), pre(B);
    for (auto& x : table) if (scanf("%d", &x) != 1) return 2;
    for (auto& x : lens) if (scanf("%d", &x) != 1) return 2;
    int32_t ng = -1;
    const int rc = xllm_mi355_host_shared_prefix_groups(table.data(), W, lens.data(), B, bs, mg, mp, cu.data(), pre.data(), &ng);
    if (rc != 0) return 3;
    for (int i = 0; i <= ng; ++i) printf("%d ", cu[i]);
    printf("|");
    for (int i = 0; i < ng; ++i) printf(" %d", pre[i]);
    printf("\n");
  }
  return 0;
}
"""


def test_host_groups_under_address_and_ub_sanitizers(tmp_path):
    """host_batch.hip and a small program of its own, built with -fsanitize=address,undefined and run as a child process on the
    tables above: exact-size vectors, so one entry read or written past a row, the table or an output array aborts the run"""
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    main = tmp_path / "groups_main.cpp"
    main.write_text(_MAIN)
    exe = tmp_path / "groups_main"
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", *san, "-I", os.path.dirname(HEADER),
                           "-x", "hip", os.path.join(ROOT, "xllm_amd", "csrc", "host_batch.hip"), str(main), "-o", str(exe)])
    cases = _tables()
    text = [str(len(cases))]
    for _, table, lens, bs, mg, mp, _ in cases:
        text.append(f"{len(lens)} {len(table[0])} {bs} {mg} {mp}")
        text.append(" ".join(str(x) for row in table for x in row))
        text.append(" ".join(str(x) for x in lens))
    r = subprocess.run([str(exe)], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(cases)
    for line, (name, table, lens, bs, mg, mp, _) in zip(lines, cases):
        cu, pre = (list(map(int, part.split())) for part in line.split("|"))
        assert (cu, pre) == _groups_py(table, lens, bs, mg, mp), name


@pytest.mark.parametrize("case", sp.CASES + [sp.G7_REGROUPED], ids=lambda c: c.name)
def test_gpu_cases_keep_the_promise_and_have_a_reference(case):
    """the inputs of tests/test_gpu_shared_prefix.py, built here on the CPU: the table equality and the length bound the contract
    promises hold, the poison is where the kernels may load but must not use, and the float64 reference is finite on them"""
    key, c = sp.seeded(case, torch.bfloat16)
    sp.check_promise(c)
    assert c["B"] == sum(n for n, _, _ in case.groups) and c["block_tables"].min() >= 0
    assert torch.isnan(c["kc"].float()).any() and torch.isinf(c["vc"].float()).any()
    if case.agree:
        (gi, m), = case.agree
        b0 = int(c["group_cu"][gi])
        P = int(c["group_prefix_blocks"][gi])
        assert torch.equal(c["block_tables"][b0 + m, :P + 1], c["block_tables"][b0, :P + 1])
    if c["B"] <= 48:
        ref = sp.reference(c, key)
        assert torch.isfinite(ref.float()).all() and not ref[c["kv_lens"] == 0].any()
