"""The ggml glue's call-by-call form of a decoder layer (include/ggml-tmac-hip.h: ggml_tmac_hip_mul_mat_dev_xf): tests/cpp/ggml_xf_main.cc
runs one llama-shaped layer (H = 1024, F = 2816) with the element-wise operators inside the mat-mul kernels and the residual stream in
two alternating buffers, and dumps every tensor into the test's temporary directory; each mpGEMM is recomputed here with the oracle
from the vector the call saw (2e-3 of max |C|), the residual stream with fp32 adds (bit for bit)."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "tmac_amd", "lib")


def gxx(out, *srcs, extra=()):
    subprocess.run(["g++", "-O2", "-std=c++17", "-w", "-I" + os.path.join(ROOT, "include"), *srcs, "-o", out, "-L" + LIBDIR, "-ltmac_hip",
                    "-Wl,-rpath," + LIBDIR, "-ldl", "-lpthread", *extra], check=True, capture_output=True, timeout=300)


def test_ggml_glue_layer_call_by_call(tmp_path):
    import torch
    from tmac_amd import convert
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    H, F, bits, bm, eps = 1024, 2816, 2, 128, 1e-5
    d = str(tmp_path)
    rng = np.random.default_rng(31)
    names = ["q", "k", "v", "o", "gate", "up", "down"]
    shape = {"q": (H, H), "k": (H, H), "v": (H, H), "o": (H, H), "gate": (F, H), "up": (F, H), "down": (H, F)}
    mats = {}
    for n in names:
        Mw, K = shape[n]
        case = orc.make_case(2000 + names.index(n), Mw, K, bits=bits, fp16_values=True)
        c = 1.0 / np.sqrt(2.5 * K)
        sc = (case["sc"] * c).astype(np.float16).astype(np.float32)
        zr = (case["zr"] * c + ((2 ** bits - 1) / 2.0 - 2 ** (bits - 1)) * sc).astype(np.float16).astype(np.float32)
        A = orc.preprocess_weights(case["w"], bits, bm, 16)
        S = orc.preprocess_scales(sc, zr, bits, bm)
        np.concatenate([A.reshape(-1), S.astype(np.float32).view(np.uint8).reshape(-1)]).tofile(os.path.join(d, f"blob_{n}.bin"))
        mats[n] = (A, S, Mw, K)
    convert.write_kcfg(os.path.join(d, "kcfg.ini"), [[bits, H, H, 1, -1], [bits, F, H, 1, -1], [bits, H, F, 1, -1]],
                       bm={(bits, H, H): bm, (bits, F, H): bm, (bits, H, F): bm})
    h0 = rng.standard_normal(H).astype(np.float32)
    h0.tofile(os.path.join(d, "h0.bin"))
    g = [(1.0 + 0.1 * rng.standard_normal(H)).astype(np.float32) for _ in range(3)]
    for i, gi in enumerate(g):
        gi.tofile(os.path.join(d, f"g{i + 1}.bin"))
    exe = os.path.join(d, "ggml_xf_main")
    gxx(exe, os.path.join(ROOT, "tests", "cpp", "ggml_xf_main.cc"), os.path.join(ROOT, "src", "ggml_tmac_hip.cc"),
        extra=("-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"))
    env = dict(os.environ); env.pop("TMAC_KCFG_FILE", None)
    r = subprocess.run([exe, d, str(H), str(F), str(bits)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr

    def out(name, dt=np.float16):
        return np.fromfile(os.path.join(d, f"out_{name}.bin"), dtype=dt).astype(np.float32)

    def oracle(n, x):
        A, S, Mw, K = mats[n]
        q, ls, lb = orc.preprocessor(x[None, :].astype(np.float32), 64)
        return orc.qgemm_float(A, q, S, ls, lb, Mw, K, 1, bits, bm, 16, 128, 64, True)[0]

    def np_norm(t, gam):
        rs = np.float32(1.0) / np.sqrt(np.float32((t.astype(np.float64) ** 2).mean()) + np.float32(eps))
        return (t * rs).astype(np.float32) * gam

    def np_glu(a, b):
        return (a / (np.float32(1.0) + np.exp(-a))).astype(np.float32) * b

    def rel(a, b):
        return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))

    x1 = np_norm(h0, g[0])
    for n in ("q", "k", "v"):
        assert rel(out(n), oracle(n, x1)) <= 2e-3, n
    a = out("attn")
    assert np.array_equal(a, out("q"))                                 # the outside operator ran between the calls
    o = out("o")
    assert rel(o, oracle("o", a)) <= 2e-3
    t2 = o + h0
    assert np.array_equal(out("t2", np.float32), t2), "residual stream (attention half)"
    x2 = np_norm(t2, g[1])
    gt, up = out("gate"), out("up")
    assert rel(gt, oracle("gate", x2)) <= 2e-3 and rel(up, oracle("up", x2)) <= 2e-3
    dn = out("down")
    assert rel(dn, oracle("down", np_glu(gt, up))) <= 2e-3
    t3 = dn + t2
    assert np.array_equal(out("t3", np.float32), t3), "residual stream"
    x3 = np_norm(t3, g[2])
    for n in ("q", "k", "v"):
        assert rel(out(f"next_{n}", np.float32), oracle(n, x3)) <= 2e-3, n
