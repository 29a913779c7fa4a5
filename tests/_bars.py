"""Shared accuracy bars of the GPU tests."""
import torch


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def assert_attn_close(got, ref, rel=1e-3):
    """attention with fp32-P accuracy: relative L2 over the tensor <= rel, and element-wise within 2 bf16 ulp of the row maximum"""
    got, ref = got.float().cpu(), ref.float().cpu()
    assert torch.isfinite(got).all()
    err = (got - ref).norm() / ref.norm().clamp_min(1e-30)
    assert err <= rel, f"relative L2 error {err:.3e} > {rel}"
    scale = ref.abs().amax(-1, keepdim=True).clamp_min(1e-30)
    assert ((got - ref).abs() <= 2 * 2.0 ** -8 * scale + 1e-30).all(), f"max abs {(got - ref).abs().max()}"


FLASH_BAR = 1e-3   # north_star's bf16 tolerance, held ABSOLUTELY against the oracle mode that has the kernel's cast point


def assert_p16_attention_close(out, ref_fp32_p, ref_p16, ref_flash=None):
    """prefill / chunked prefill with ONE 16-bit P per score in front of PV, as the reference computes it
    (flashinfer_attention.cpp:84-90; oracle p_round=True). That rounding alone moves the result by e_ref from the fp32-P
    result (2.5e-3 on long rows, up to ~4e-3 on rows of a handful of keys where nothing averages out), so the bars are
    relative to it: no further from the fp32-P result than the reference's own arithmetic (x 1.25), and within 2 e_ref of the
    p_round oracle (the kernel rounds the un-normalised P, the oracle the normalised one). Never looser than that and never
    tighter than the 1e-3 the hi+lo form holds."""
    e_ref = rel_l2(ref_p16, ref_fp32_p)
    assert torch.isfinite(out.float()).all()
    assert rel_l2(out, ref_fp32_p) <= max(1e-3, 1.25 * e_ref), (rel_l2(out, ref_fp32_p), e_ref)
    assert rel_l2(out, ref_p16) <= max(1e-3, 2.0 * e_ref), (rel_l2(out, ref_p16), e_ref)
    import os
    # the oracle's flash mode restates the DEFAULT kernel (64-key tiles, one 16-bit P): the A/B arms -- register-staged tiles, P = hi + lo
    # (which lands on the fp32-P result instead) -- stay under the bars above
    default_arm = (os.environ.get("XLLM_MI355_PREFILL_DMA") != "0" and os.environ.get("XLLM_MI355_PREFILL_P") != "2"
                   and os.environ.get("XLLM_MI355_MLA_PREFILL_P") != "2")
    if ref_flash is not None and default_arm:
        assert rel_l2(out, ref_flash) <= FLASH_BAR, rel_l2(out, ref_flash)
