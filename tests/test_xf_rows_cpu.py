"""tmac_hip_qgemm_fused_xf_rows_dev and tmac_hip_debug_xf_rows without a GPU: the symbols are exported and declared, the wrapper has its
methods, and without a device the entry points say so."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_exported_and_declared():
    import tmac_amd
    L = tmac_amd.lib()
    hdr = open(os.path.join(ROOT, "include", "tmac_hip.h")).read()
    for name, arity in (("tmac_hip_qgemm_fused_xf_rows_dev", 9), ("tmac_hip_debug_xf_rows", 7), ("tmac_hip_debug_xf_rows_plan", 6)):
        fn = getattr(L, name)
        assert len(fn.argtypes) == arity, name
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == arity, name
    ghdr = open(os.path.join(ROOT, "include", "ggml-tmac-hip.h")).read()
    m = re.search(r"int\s+ggml_tmac_hip_mul_mat_dev_xf_rows\s*\(([^;]*)\)\s*;", ghdr)
    assert m and "n_rows" in m.group(1)
    assert "ggml_tmac_hip_mul_mat_dev_xf_rows" in open(os.path.join(ROOT, "src", "ggml_tmac_hip.cc")).read()


def test_wrapper_methods():
    import tmac_amd
    sig = inspect.signature(tmac_amd.TMACGeMMWrapper.fused_xf_rows)
    assert list(sig.parameters) == ["self", "weights_list", "B_dev", "C_list", "kind", "N", "in2", "residual", "gamma", "eps", "residual_out",
                                    "act_dtype", "out_dtype", "stream"]
    assert sig.parameters["eps"].default == 1e-5 and sig.parameters["in2"].default is None
    tap = inspect.signature(tmac_amd.TMACGeMMWrapper.xf_rows_tap)
    assert list(tap.parameters)[:6] == ["self", "B_dev", "x_out", "kind", "K", "N"]
    # fused_xf keeps its signature
    old = inspect.signature(tmac_amd.TMACGeMMWrapper.fused_xf)
    assert list(old.parameters) == ["self", "weights_list", "B_dev", "C_list", "kind", "in2", "residual", "gamma", "eps", "residual_out",
                                    "act_dtype", "out_dtype", "stream"]


def test_no_device():
    import ctypes as C
    import tmac_amd
    try:
        import torch
        if torch.cuda.is_available():
            return                       # (with a device the GPU tests speak)
    except Exception:
        pass
    L = tmac_amd.lib()
    xf = tmac_amd.binding.XForm()
    xf.kind = 1
    assert L.tmac_hip_qgemm_fused_xf_rows_dev(None, 1, None, tmac_amd.F16, C.byref(xf), None, tmac_amd.F16, 2, None) == -2     # TMAC_HIP_E_NODEVICE
    assert L.tmac_hip_debug_xf_rows(None, tmac_amd.F16, C.byref(xf), 64, 2, None, None) == -2
