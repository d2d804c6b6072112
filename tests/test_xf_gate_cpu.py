"""The gate of TMAC_XF_GLU / TMAC_XF_GLU_NORM without a GPU: the three constants are in the public header next to an unchanged ABI version, the
ggml glue declares and defines its gated segment call, the wrapper resolves the gate out of the kind string without a change of signature,
and without a device a gated call answers like every compute entry point."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_constants_are_in_the_header():
    hdr = read("include", "tmac_hip.h")
    assert re.search(r"#define\s+TMAC_XF_GATE_SILU\s+0x000\b", hdr)
    assert re.search(r"#define\s+TMAC_XF_GATE_RELU2\s+0x100\b", hdr)
    assert re.search(r"#define\s+TMAC_XF_GATE_GELU\s+0x200\b", hdr)
    assert re.search(r"#define\s+TMAC_HIP_ABI_VERSION\s+1\b", hdr), "the struct and the ABI version do not change"
    assert re.search(r"#define\s+TMAC_XF_GLU_NORM\s+4\b", hdr) and re.search(r"#define\s+TMAC_XF_GLU\s+2\b", hdr)


def test_binding_has_the_constants():
    import tmac_amd
    b = tmac_amd.binding
    assert (b.XF_GATE_SILU, b.XF_GATE_RELU2, b.XF_GATE_GELU) == (0, 0x100, 0x200)
    assert (b.XF_NONE, b.XF_NORM, b.XF_GLU, b.XF_GLU_NORM) == (0, 1, 2, 4)


def test_glue_declares_and_defines_the_gated_segment_call():
    sig = (r"int\s+ggml_tmac_hip_segment_glu_gate\s*\(\s*const\s+void\s*\*\s*in2_f16\s*,\s*int\s+gate\s*(/\*.*?\*/\s*)?,\s*const\s+float\s*\*\s*norm_weight\s*"
           r"(/\*.*?\*/\s*)?,\s*float\s+eps\s*\)")
    assert re.search(sig + r"\s*;", read("include", "ggml-tmac-hip.h"))
    src = read("src", "ggml_tmac_hip.cc")
    assert re.search(sig + r"\s*\{", src)
    # the two earlier calls keep their signatures and go through the gated one with silu
    assert len(re.findall(r"ggml_tmac_hip_segment_glu_gate\s*\(\s*in2_f16\s*,\s*TMAC_XF_GATE_SILU\b", src)) == 2


def test_wrapper_resolves_the_gate_and_keeps_its_kinds():
    import tmac_amd
    W = tmac_amd.TMACGeMMWrapper
    assert W._XF_KINDS == {None: 0, "norm": 1, "glu": 2, "glu_norm": 4}
    assert W._XF_GATES == {"silu": 0, "relu2": 0x100, "gelu": 0x200}
    assert W._xf_kind("glu_norm:relu2") == 0x104
    assert W._xf_kind("glu:gelu") == 0x202
    assert W._xf_kind("glu:relu2") == 0x102 and W._xf_kind("glu_norm:gelu") == 0x204
    assert W._xf_kind("glu:silu") == W._xf_kind("glu") == 2 and W._xf_kind("glu_norm:silu") == W._xf_kind("glu_norm") == 4
    assert W._xf_kind("norm") == 1 and W._xf_kind(None) == 0
    # all four methods go through the one resolver: the struct the row forms build carries the gate
    assert W._xform("glu_norm:relu2", None, None, None, 1e-5, None, False, True).kind == 0x104
    assert W._xform("glu:gelu", None, None, None, 1e-5, None, False, True).kind == 0x202


@pytest.mark.parametrize("kind", ["glu:tanh", "glu_norm:", "glu:RELU2"])
def test_an_unknown_gate_name_raises(kind):
    import tmac_amd
    W = tmac_amd.TMACGeMMWrapper
    with pytest.raises(ValueError):
        W._xf_kind(kind)
    with pytest.raises(ValueError):
        W._xform(kind, None, None, None, 1e-5, None, False, True)


def test_no_device_is_reported():
    import tmac_amd
    L = tmac_amd.lib()
    if L.tmac_hip_device_count() > 0:
        return      # (a machine with a GPU: tests/test_gpu_xf_gate.py covers the entry points)
    xf = tmac_amd.binding.XForm()
    xf.kind = 0x104
    assert L.tmac_hip_qgemm_fused_xf_dev(None, 1, None, tmac_amd.F16, C.byref(xf), None, tmac_amd.F16, None) == -2      # TMAC_HIP_E_NODEVICE
    assert b"no HIP device" in L.tmac_hip_last_error()
    assert L.tmac_hip_qgemm_fused_xf_rows_dev(None, 1, None, tmac_amd.F16, C.byref(xf), None, tmac_amd.F16, 2, None) == -2
    assert L.tmac_hip_debug_xf_rows(None, tmac_amd.F16, C.byref(xf), 64, 2, None, None) == -2
