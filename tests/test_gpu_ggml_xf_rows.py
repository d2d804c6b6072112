"""The ggml glue's transformed mat-muls for several rows (include/ggml-tmac-hip.h: ggml_tmac_hip_mul_mat_dev_xf_rows):
tests/cpp/ggml_xf_rows_main.cc runs the MLP half of a llama-shaped layer (H = 256, F = 512) for N = 3 rows -- gate/up behind [+ residual,
RMSNorm], then down behind [silu(gate) * up] -- and dumps every tensor into the test's temporary directory; each mpGEMM is recomputed here
with the oracle from the rows the call saw (2e-3 of max |C|), the residual stream with fp32 adds (bit for bit)."""
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


def test_ggml_glue_mlp_rows(tmp_path):
    import torch
    from tmac_amd import convert
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    H, F, N, bits, bm, eps = 256, 512, 3, 2, 128, 1e-5
    d = str(tmp_path)
    rng = np.random.default_rng(33)
    names = ["gate", "up", "down"]
    shape = {"gate": (F, H), "up": (F, H), "down": (H, F)}
    mats = {}
    for n in names:
        Mw, K = shape[n]
        case = orc.make_case(3000 + names.index(n), Mw, K, bits=bits, fp16_values=True)
        c = 1.0 / np.sqrt(2.5 * K)
        sc = (case["sc"] * c).astype(np.float16).astype(np.float32)
        zr = (case["zr"] * c + ((2 ** bits - 1) / 2.0 - 2 ** (bits - 1)) * sc).astype(np.float16).astype(np.float32)
        A = orc.preprocess_weights(case["w"], bits, bm, 16)
        S = orc.preprocess_scales(sc, zr, bits, bm)
        np.concatenate([A.reshape(-1), S.astype(np.float32).view(np.uint8).reshape(-1)]).tofile(os.path.join(d, f"blob_{n}.bin"))
        mats[n] = (A, S, Mw, K)
    convert.write_kcfg(os.path.join(d, "kcfg.ini"), [[bits, F, H, 1, -1], [bits, H, F, 1, -1]], bm={(bits, F, H): bm, (bits, H, F): bm})
    x = rng.standard_normal((N, H)).astype(np.float16)
    h = rng.standard_normal((N, H)).astype(np.float32)
    g = (1.0 + 0.1 * rng.standard_normal(H)).astype(np.float32)
    x.tofile(os.path.join(d, "x.bin")); h.tofile(os.path.join(d, "h.bin")); g.tofile(os.path.join(d, "g.bin"))
    exe = os.path.join(d, "ggml_xf_rows_main")
    gxx(exe, os.path.join(ROOT, "tests", "cpp", "ggml_xf_rows_main.cc"), os.path.join(ROOT, "src", "ggml_tmac_hip.cc"),
        extra=("-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"))
    env = dict(os.environ); env.pop("TMAC_KCFG_FILE", None)
    r = subprocess.run([exe, d, str(H), str(F), str(bits), str(N)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr

    def out(name, cols, dt=np.float16):
        return np.fromfile(os.path.join(d, f"out_{name}.bin"), dtype=dt).astype(np.float32).reshape(N, cols)

    def oracle(n, X):
        A, S, Mw, K = mats[n]
        q, ls, lb = orc.preprocessor(np.ascontiguousarray(X, np.float32), 64)
        return orc.qgemm_float(A, q, S, ls, lb, Mw, K, N, bits, bm, 16, 128, 64, True)

    def np_norm(t, gam):
        rs = np.float32(1.0) / np.sqrt((t.astype(np.float64) ** 2).mean(axis=1).astype(np.float32) + np.float32(eps))
        return (t * rs[:, None]).astype(np.float32) * gam[None, :]

    def np_glu(a, b):
        return (a / (np.float32(1.0) + np.exp(-a))).astype(np.float32) * b

    def rel(a, b):
        return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))

    t = x.astype(np.float32) + h
    assert np.array_equal(out("t", H, np.float32), t), "residual stream"
    xn = np_norm(t, g)
    gt, up = out("gate", F), out("up", F)
    assert rel(gt, oracle("gate", xn)) <= 2e-3 and rel(up, oracle("up", xn)) <= 2e-3
    assert rel(out("down", H, np.float32), oracle("down", np_glu(gt, up))) <= 2e-3
