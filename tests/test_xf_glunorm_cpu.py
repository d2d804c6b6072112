"""TMAC_XF_GLU_NORM without a GPU: the constant is in the public header, the ggml glue declares and defines its segment call, the wrapper
maps "glu_norm" without a change of signature, and without a device a kind-4 call answers like every compute entry point."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_constant_is_in_the_header():
    hdr = read("include", "tmac_hip.h")
    assert re.search(r"#define\s+TMAC_XF_GLU_NORM\s+4\b", hdr)
    assert re.search(r"#define\s+TMAC_XF_GLU\s+2\b", hdr) and re.search(r"#define\s+TMAC_XF_NORM\s+1\b", hdr)
    assert re.search(r"#define\s+TMAC_HIP_ABI_VERSION\s+1\b", hdr), "the struct and the ABI version do not change"
    assert "kind outside 0..2" not in hdr


def test_glue_declares_and_defines_the_segment_call():
    sig = r"int\s+ggml_tmac_hip_segment_glu_norm\s*\(\s*const\s+void\s*\*\s*in2_f16\s*,\s*const\s+float\s*\*\s*norm_weight\s*,\s*float\s+eps\s*\)"
    assert re.search(sig + r"\s*;", read("include", "ggml-tmac-hip.h"))
    src = read("src", "ggml_tmac_hip.cc")
    assert re.search(sig + r"\s*\{", src)
    assert "TMAC_XF_GLU_NORM" in src


def test_wrapper_maps_glu_norm_and_keeps_its_signatures():
    import tmac_amd
    W = tmac_amd.TMACGeMMWrapper
    assert W._XF_KINDS == {None: 0, "norm": 1, "glu": 2, "glu_norm": 4}
    xf = W._xform("glu_norm", None, None, None, 1e-5, None, False, True)
    assert xf.kind == 4
    par = lambda f: list(inspect.signature(f).parameters)[1:]
    assert par(W.chain_xform) == ["kind", "in2", "residual", "gamma", "eps", "residual_out", "keep"]
    assert par(W.fused_xf) == ["weights_list", "B_dev", "C_list", "kind", "in2", "residual", "gamma", "eps", "residual_out", "act_dtype", "out_dtype",
                               "stream"]
    assert par(W.fused_xf_rows) == ["weights_list", "B_dev", "C_list", "kind", "N", "in2", "residual", "gamma", "eps", "residual_out", "act_dtype",
                                    "out_dtype", "stream"]
    assert par(W.xf_rows_tap) == ["B_dev", "x_out", "kind", "K", "N", "in2", "residual", "gamma", "eps", "residual_out", "act_dtype", "stream"]


def test_no_device_is_reported():
    import tmac_amd
    L = tmac_amd.lib()
    if L.tmac_hip_device_count() > 0:
        return      # (a machine with a GPU: tests/test_gpu_xf_glunorm.py covers the entry points)
    xf = tmac_amd.binding.XForm()
    xf.kind = 4
    assert L.tmac_hip_qgemm_fused_xf_dev(None, 1, None, tmac_amd.F16, C.byref(xf), None, tmac_amd.F16, None) == -2      # TMAC_HIP_E_NODEVICE
    assert b"no HIP device" in L.tmac_hip_last_error()
    assert L.tmac_hip_qgemm_fused_xf_rows_dev(None, 1, None, tmac_amd.F16, C.byref(xf), None, tmac_amd.F16, 2, None) == -2
    assert L.tmac_hip_debug_xf_rows(None, tmac_amd.F16, C.byref(xf), 64, 2, None, None) == -2
