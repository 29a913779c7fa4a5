"""The product switches (forced kernels / fallbacks / fusion switches that stay in the library) are
parity-green: the parity tests of the operator are re-run in subprocesses with each selector (read once per process).
The file is named test_zz_* so that it is collected LAST: under the driver's `pytest -x` a broken opt-in arm must not hide
the shim, fixture and property tests (round-3 review). Arms whose A/B verdict is recorded as lost are no longer in the
product library at all (round 4: -DXM_TUNING flavour only)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELECT = ("scaled_matmul_int32_exact or splitk_workspace or w8a8_dynamic or matmul_16bit or gemm_add_norm or group_gemm "
          "or matmul_weight_stream or qkv_gemm_rope or gate_up_silu or packed_gemm_qwen2")


@pytest.mark.parametrize("env", [
    {"XLLM_MI355_P8": "1"},                                  # 8-phase kernels forced on every legal shape (+ split-K)
    {"XLLM_MI355_P8": "0", "XLLM_MI355_SKINNY_DISABLE": "1"},  # 128x128 kernel only
    {"XLLM_MI355_WSB": "0"},                                  # 16-bit decode linears / few-row experts on the tiled kernels
    {"XLLM_MI355_WSB": "2"},                                  # ... on every M <= 64 (default policy: M <= 32)
    {"XLLM_MI355_PACKED": "1"},                               # packed kernels (int8, fp8, 16-bit) everywhere legal
    {"XLLM_MI355_PACKED": "0"},                               # ... nowhere: the row-major kernels serve the decode shapes
], ids=["p8_forced", "general_only", "wsb_off", "wsb_to_64", "packed_everywhere", "packed_nowhere"])
def test_gemm_parity_under_kernel_selector(env):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_parity.py"), "-q", "-x",
                        "-k", SELECT, "-p", "no:cacheprovider"], cwd=ROOT, env=e, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("env", [
    {"XLLM_MI355_MLA_SPLITS": "3"},                          # LDS-DMA kernel with a forced split-KV (uneven slices)
    {"XLLM_MI355_MLA_SPLITS": "1"},
    {"XLLM_MI355_MLA_PREFILL": "0"},                         # prefill: one decode-kernel entry per query token
    {"XLLM_MI355_MLA_PREFILL": "1"},                         # prefill: the tile-sharing kernel on every batch size
    {"XLLM_MI355_MLA_PREFILL": "1", "XLLM_MI355_MLA_PREFILL_P": "2"},   # ... with P = hi + lo (fp32-P accuracy)
    {"XLLM_MI355_MLA_SPLITS": "7"},                          # the uneven merge above four splits
    {"XLLM_MI355_MLA_SPLITS": "32"},                         # the largest count the workspace is sized for
], ids=["mla_dma_split3", "mla_dma_nosplit", "mla_prefill_per_token",
        "mla_prefill_shared_forced", "mla_prefill_shared_p_hi_lo", "mla_dma_split7", "mla_dma_split32"])
def test_mla_parity_under_kernel_selector(env):
    """The MLA tests of test_gpu_parity.py and every arm, length edge and rescale case of tests/test_gpu_mla_arms.py (`-k mla`
    selects that whole file) under each MLA selector. The latter asserts through xllm_mi355_mla_plan what each switch dictates: min(n, 32, what the workspace holds) splits, the tile-sharing
    arm for the small per-token calls under XLLM_MI355_MLA_PREFILL=1"""
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_parity.py"),
                        os.path.join(ROOT, "tests", "test_gpu_mla_arms.py"), "-q", "-x",
                        "-k", "mla", "-p", "no:cacheprovider"], cwd=ROOT, env=e, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("env", [
    {"XLLM_MI355_PREFILL_P": "2"},                           # P = hi + lo on the default kernel (fp32-P accuracy, 1e-3 bar)
], ids=["prefill_p_hi_lo"])
def test_prefill_parity_under_kernel_selector(env):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_parity.py"),
                        os.path.join(ROOT, "tests", "test_gpu_fullsize.py"),
                        os.path.join(ROOT, "tests", "test_gpu_prefill_masks.py"), "-q", "-x", "-k",
                        "prefill or chunked or model", "-p", "no:cacheprovider"], cwd=ROOT, env=e, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_group_gemm_parity_on_the_fallback_kernel():
    e = dict(os.environ)
    e["XLLM_MI355_GROUP_P8"] = "0"                          # 128x128 kernel with the per-workgroup expert walk
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_parity.py"), "-q", "-x",
                        "-k", "moe", "-p", "no:cacheprovider"], cwd=ROOT, env=e, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("env", [
    {"XLLM_MI355_ATTN_FINISH": "0"},                         # split-KV partials: merge launch + scaled_quantize instead of ONE finishing launch
    {"XLLM_MI355_QKV_ROPE": "0"},                            # qkv projection, RoPE and KV write as separate operators
], ids=["attn_finish_off", "qkv_rope_unfused"])
def test_decode_fusion_switches(env):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_parity.py"), "-q", "-x",
                        "-k", "fusion or model_step or engine or dual_micro", "-p", "no:cacheprovider"], cwd=ROOT, env=e,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("splits", ["3", "7", "32"])
def test_decode_parity_under_forced_split_counts(splits):
    """XLLM_MI355_DECODE_SPLITS: uneven slices (3), the generic finish / merge arm above 4 splits (7) and the largest count the
    workspace is sized for (32), on every plan and window case of tests/test_gpu_decode_plans.py and the decode tests of
    test_gpu_parity.py (not the must_fuse ones: a forced count changes which calls decline)"""
    e = dict(os.environ)
    e["XLLM_MI355_DECODE_SPLITS"] = splits
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_decode_plans.py"),
                        os.path.join(ROOT, "tests", "test_gpu_parity.py"), "-q", "-x", "-k",
                        "test_gpu_decode_plans or paged_decode_attention or split_kv_and_garbage or decode_window or "
                        "rescale_branch", "-p", "no:cacheprovider"], cwd=ROOT, env=e, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("env", [{}, {"XLLM_MI355_P8": "1"}, {"XLLM_MI355_P8": "0"}, {"XLLM_MI355_PACKED": "0"},
                                 {"XLLM_MI355_P8": "0", "XLLM_MI355_SKINNY_DISABLE": "1"}],
                         ids=["default", "p8_forced", "p8_off", "packed_off", "general_only"])
def test_gate_up_act_row_major_only_is_never_silently_empty(env):
    """round-3 red test, pinned: xllm_mi355_scaled_matmul_gate_up_act with ROW-MAJOR weights only (no packed copy), M in
    {1, 256, 8192}, under every GEMM selector: non-zero and bit-equal to the unfused operators (or a clean decline)"""
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_parity.py"), "-q", "-x",
                        "-k", "gate_up_act_row_major_only", "-p", "no:cacheprovider"], cwd=ROOT, env=e, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
