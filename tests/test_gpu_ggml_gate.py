"""BitNet b1.58 2B-4T's FFN, ffn_sub_norm(relu(gate)^2 * up), through the ggml glue (include/ggml-tmac-hip.h): tests/cpp/ggml_gate_main.cc runs one
layer of that shape (H = 640, F = 1728, unified scales, one act group per row) twice -- as one recorded segment with
ggml_tmac_hip_segment_glu_gate(up, TMAC_XF_GATE_RELU2, w, eps), and call by call with ggml_tmac_hip_mul_mat_dev_xf(kind 0x104) -- checks that a gate
of 0x300 is refused by both, and dumps every tensor into the test's temporary directory.  Each mpGEMM is recomputed here with the oracle from
the vector the call saw (2e-3 of max |C|; relu(gate)^2 * up rounded to fp16 first where the segment hands it over), the residual stream with
fp32 adds (bit for bit)."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc
from test_gpu_ggml_xf import ROOT, gxx

pytestmark = pytest.mark.gpu


def test_ggml_glue_bitnet_2b4t_layer_segment_and_call_by_call(tmp_path):
    import torch
    from tmac_amd import convert
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    H, F, bits, bm, mg, eps = 640, 1728, 2, 128, 1, 1e-5
    d = str(tmp_path)
    rng = np.random.default_rng(41)
    names = ["q", "k", "v", "o", "gate", "up", "down"]
    shape = {"q": (H, H), "k": (H, H), "v": (H, H), "o": (H, H), "gate": (F, H), "up": (F, H), "down": (H, F)}
    mats = {}
    for n in names:
        Mw, K = shape[n]
        case = orc.make_case(3100 + names.index(n), Mw, K, bits=bits, ags=K, m_groups=mg, zero_point=False)
        S = (case["sc"] * (1.0 / np.sqrt(2.5 * K))).astype(np.float32)
        A = orc.preprocess_weights(case["w"], bits, bm, 16)
        np.concatenate([A.reshape(-1), S.view(np.uint8).reshape(-1)]).tofile(os.path.join(d, f"blob_{n}.bin"))
        mats[n] = (A, S, Mw, K)
    convert.write_kcfg(os.path.join(d, "kcfg.ini"), [[bits, H, H, 1, mg], [bits, F, H, 1, mg], [bits, H, F, 1, mg]], act_group_size=-1, zero_point=False,
                       bm={(bits, H, H): bm, (bits, F, H): bm, (bits, H, F): bm})
    h0 = rng.standard_normal(H).astype(np.float32)
    h0.tofile(os.path.join(d, "h0.bin"))
    attn = rng.standard_normal(H).astype(np.float16)
    attn.tofile(os.path.join(d, "attn.bin"))
    g = [(1.0 + 0.1 * rng.standard_normal(n)).astype(np.float32) for n in (H, H, F)]
    for i, gi in enumerate(g):
        gi.tofile(os.path.join(d, f"g{i + 1}.bin"))
    exe = os.path.join(d, "ggml_gate_main")
    gxx(exe, os.path.join(ROOT, "tests", "cpp", "ggml_gate_main.cc"), os.path.join(ROOT, "src", "ggml_tmac_hip.cc"),
        extra=("-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"))
    env = dict(os.environ); env.pop("TMAC_KCFG_FILE", None); env.pop("TMAC_CHAIN_GLU_EPILOGUE", None)
    r = subprocess.run([exe, d, str(H), str(F), str(bits)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr

    def oracle(n, x):
        A, S, Mw, K = mats[n]
        q, ls, lb = orc.preprocessor(x[None, :].astype(np.float32), K)
        return orc.qgemm_scale_final(A, q, S, ls[:, 0], lb[:, 0], Mw, K, 1, bits, bm, 16, mg)[0][0]

    def np_norm(t, gam):
        rs = np.float32(1.0) / np.sqrt(np.float32((t.astype(np.float64) ** 2).mean()) + np.float32(eps))
        return (t * rs).astype(np.float32) * gam

    def np_glu(a, b):
        return (np.maximum(a, 0) ** 2 * b).astype(np.float32)

    def rel(a, b):
        return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))

    a = attn.astype(np.float32)
    for tag, f16_handover in (("seg", True), ("cbc", False)):
        def out(name, dt=np.float16):
            return np.fromfile(os.path.join(d, f"{tag}_{name}.bin"), dtype=dt).astype(np.float32)
        o = out("o")
        assert rel(o, oracle("o", a)) <= 2e-3, tag
        t2 = o + h0
        x2 = np_norm(t2, g[1])
        gt, up = out("gate"), out("up")
        assert rel(gt, oracle("gate", x2)) <= 2e-3 and rel(up, oracle("up", x2)) <= 2e-3, tag
        gl = np_glu(gt, up)
        if f16_handover:
            gl = gl.astype(np.float16).astype(np.float32)
        dn = out("down")
        e = rel(dn, oracle("down", np_norm(gl, g[2])))
        print(f"{tag}: down behind relu^2 and the sub-layer norm, rel err vs oracle {e:.2e}")
        assert e <= 2e-3, (tag, e)
        t3 = dn + t2
        assert np.array_equal(out("t3", np.float32), t3), f"{tag}: residual stream"
        x3 = np_norm(t3, g[0])
        for n in ("q", "k", "v"):
            assert rel(out(n), oracle(n, x3)) <= 2e-3, (tag, n)
