"""tmac_hip_qgemm_fused_xf_dev without a GPU: the symbol is exported and declared, the wrapper has its method, and without a device the
entry point answers like every compute entry point."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_exported_and_declared():
    import tmac_amd
    L = tmac_amd.lib()
    fn = L.tmac_hip_qgemm_fused_xf_dev
    assert fn.restype is C.c_int32 and len(fn.argtypes) == 8
    hdr = open(os.path.join(ROOT, "include", "tmac_hip.h")).read()
    assert re.search(r"int32_t\s+tmac_hip_qgemm_fused_xf_dev\s*\(", hdr)
    assert "no stand-alone counterpart" not in hdr
    ggml = open(os.path.join(ROOT, "include", "ggml-tmac-hip.h")).read()
    assert re.search(r"int\s+ggml_tmac_hip_mul_mat_dev_xf\s*\(", ggml)


def test_wrapper_method_exists():
    import inspect
    import tmac_amd
    sig = inspect.signature(tmac_amd.TMACGeMMWrapper.fused_xf)
    assert list(sig.parameters)[1:] == ["weights_list", "B_dev", "C_list", "kind", "in2", "residual", "gamma", "eps", "residual_out",
                                        "act_dtype", "out_dtype", "stream"]
    assert sig.parameters["eps"].default == 1e-5


def test_no_device_is_reported():
    import tmac_amd
    L = tmac_amd.lib()
    if L.tmac_hip_device_count() > 0:
        return      # (a machine with a GPU: tests/test_gpu_xf.py covers the entry point)
    xf = tmac_amd.binding.XForm()
    xf.kind = 1
    for pxf in (None, C.byref(xf)):
        assert L.tmac_hip_qgemm_fused_xf_dev(None, 1, None, tmac_amd.F16, pxf, None, tmac_amd.F16, None) == -2      # TMAC_HIP_E_NODEVICE
        assert b"no HIP device" in L.tmac_hip_last_error()
