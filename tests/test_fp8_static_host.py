"""CPU-side checks of the static-scale fp8 producers (xllm_mi355_act_and_mul_static_fp8_quant and
xllm_mi355_paged_decode_attention_fp8, xllm_amd/csrc/xllm_mi355_fp8_static.h): the symbols are declared, exported and bound with the
header's argument counts, and the validation that happens before any device work returns its codes without a device."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["xllm_mi355_act_and_mul_static_fp8_quant", "xllm_mi355_paged_decode_attention_fp8"]
XM_OK, XM_ERR_INVALID, XM_ERR_UNSUPPORTED = 0, -1, -2
# the operators' C declarations: a header of its own next to the kernels (include/ is pinned by tests/test_host_abi.py)
HEADER = os.path.join(ROOT, "xllm_amd", "csrc", "xllm_mi355_fp8_static.h")


def _built():
    import __graft_entry__ as g
    from xllm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        os.environ["XLLM_MI355_SKIP_SHIM"] = "1"
        g.build()
    return _lib


def _declared():
    """name -> number of parameters, from the header's text"""
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): len([a for a in m.group(2).split(",") if a.strip()])
            for m in re.finditer(r"XM_API\s+[\w\s\*]+?\b(xllm_mi355_\w+)\s*\(([^)]*)\)", hdr)}


def test_symbols_declared_exported_and_bound():
    _lib = _built()
    declared = _declared()
    exported = set(re.findall(r"\b(xllm_mi355_\w+)\b", subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()))
    assert sorted(declared) == sorted(SYMBOLS)
    assert declared == {SYMBOLS[0]: 8, SYMBOLS[1]: 23}
    for s in SYMBOLS:
        assert s in exported and s in _lib.exported_symbols(), s
        assert len(getattr(_lib.lib(), s).argtypes) == declared[s], s
    assert _lib.lib().xllm_mi355_abi_version() == 2


def _addr():
    """a 16-byte aligned host address that is never dereferenced: every case here must return before any device work"""
    buf = (C.c_char * 64)()
    return buf, (C.addressof(buf) + 15) // 16 * 16


def _act(l, out=True, inp=True, scale=True, n=3, d=64, mode=0, dtype=1):
    buf, a = _addr()
    return l.xllm_mi355_act_and_mul_static_fp8_quant(a if out else None, a if inp else None, a if scale else None, n, d, mode,
                                                     dtype, None)


def test_activation_validation_happens_without_a_device():
    l = _built().lib()
    assert _act(l, out=False) == XM_ERR_INVALID
    assert _act(l, inp=False) == XM_ERR_INVALID
    assert _act(l, scale=False) == XM_ERR_INVALID
    assert _act(l, n=-1) == XM_ERR_INVALID
    assert _act(l, d=0) == XM_ERR_INVALID
    assert _act(l, dtype=0) == XM_ERR_UNSUPPORTED          # f32: the input is 16-bit
    assert _act(l, dtype=7) == XM_ERR_UNSUPPORTED
    assert _act(l, mode=3) == XM_ERR_UNSUPPORTED           # act modes of xllm_mi355_act_and_mul: silu, gelu, gelu_tanh
    assert _act(l, n=0) == XM_OK                           # nothing to do, nothing launched


def _attn(l, null=(), d=128, nq=28, nkv=4, dtype=1, batch=4, q_off=0, q_stride=None, max_blocks=8, bs=128):
    buf, a = _addr()
    names = ["q", "k_cache", "v_cache", "out", "out_q", "out_scale", "kv_lens", "block_table"]
    p = [None if n in null else a for n in names]
    if p[0] is not None:
        p[0] += q_off
    return l.xllm_mi355_paged_decode_attention_fp8(*p, max_blocks, batch, nq, nkv, d, bs, 64, nq * d if q_stride is None else q_stride,
                                                   1024, 0.1, -1, dtype, None, 0, None)


def test_attention_validation_happens_without_a_device():
    l = _built().lib()
    for name in ("q", "k_cache", "v_cache", "out_q", "out_scale", "kv_lens", "block_table"):
        assert _attn(l, null=(name,)) == XM_ERR_INVALID, name
    assert _attn(l, nq=30) == XM_ERR_INVALID               # n_q_heads % n_kv_heads
    assert _attn(l, batch=-1) == XM_ERR_INVALID
    assert _attn(l, max_blocks=0) == XM_ERR_INVALID
    assert _attn(l, bs=0) == XM_ERR_INVALID
    assert _attn(l, d=96) == XM_ERR_UNSUPPORTED            # head dim other than 64 / 128
    assert _attn(l, d=256) == XM_ERR_UNSUPPORTED
    assert _attn(l, nq=68) == XM_ERR_UNSUPPORTED           # 17 q heads per kv head
    assert _attn(l, dtype=0) == XM_ERR_UNSUPPORTED         # f32
    assert _attn(l, q_off=2) == XM_ERR_UNSUPPORTED         # q not 16-byte aligned
    assert _attn(l, q_stride=28 * 128 + 4) == XM_ERR_UNSUPPORTED
    assert _attn(l, null=("out",), batch=0) == XM_OK       # the 16-bit output is optional; an empty batch launches nothing
