"""Child process of tests/test_gpu_hostptr_purity.py (A5): the host-pointer layer under a mode that is an environment variable read
once per process.  usage: hostptr_purity_child.py <zero_copy_off | small_cache> <scratch dir>; prints CHILD OK and exits 0, or fails
with the assertion that did not hold."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402,F401  (first: libtmac_hip.so binds to the HIP runtime torch brings)
import tmac_amd  # noqa: E402
from hostptr_common import Cfg, Lut, Matrix, acts, check, load_kcfg  # noqa: E402

FWD, REV, SUB = [0, 1, 2, 3], [2, 0, 3, 1], [2, 1]


def modes(L):
    L.tmac_hip_debug_host_runs.argtypes = [C.c_int]
    for runs in (1, 0):
        assert L.tmac_hip_debug_host_runs(runs) == 0
        assert L.tmac_hip_cache_clear() == 0
        yield runs
    assert L.tmac_hip_debug_host_runs(1) == 0
    assert L.tmac_hip_cache_clear() == 0


def zero_copy_off(L, d):
    """copy commands and a stream synchronisation instead of kernels that write host memory: the first configuration of A1 (W4, bm 256,
    zero points; a fresh LUT per GEMV) and the realistic flow of A2 (W2; three vectors into one set of LUT buffers, then the first again)"""
    assert os.environ.get("TMAC_HIP_HOST_ZERO_COPY") == "0"
    K = 1024
    w4, w2 = Cfg(256, K, 4, 256), Cfg(256, K, 2, 128)
    load_kcfg(L, os.path.join(d, "kcfg.ini"), [w4, w2])
    for runs in modes(L):
        mat, lut = Matrix(w4, 9400), Lut(K, 64)
        for i, order in enumerate((FWD, FWD, REV, SUB, FWD)):
            lut.preprocess(L, acts(9410 + i, K), w4.Mw * w4.bits, w4.bits)
            check(L, mat, lut, order, 1, ("w4", runs, i))
        mat, lut = Matrix(w2, 9420), Lut(K, 64)
        for i, seed in enumerate((1, 2, 3, 1)):
            lut.preprocess(L, acts(9430 + seed, K), w2.Mw * w2.bits, w2.bits)
            check(L, mat, lut, FWD, 1, ("w2 flow", runs, i))
        lut.write(acts(9440, K))
        check(L, mat, lut, REV, 1, ("w2 caller-built", runs))


def small_cache(L, d):
    """a 1 MB cap on the device copies of host-pointer weights and three matrices of 16 tiles (512 KB of weights and 128 KB of scales each)
    whose runs cannot all fit: the values stay right while runs are evicted and learnt again"""
    assert os.environ.get("TMAC_HIP_HOST_CACHE_MB") == "1"
    cfg = Cfg(1024, 2048, 2, 128)
    load_kcfg(L, os.path.join(d, "kcfg.ini"), [cfg])
    order = list(range(cfg.ntile))
    for runs in modes(L):
        mats = [Matrix(cfg, 9500 + i) for i in range(3)]
        lut = Lut(cfg.K, 64)
        for step in range(4):
            lut.preprocess(L, acts(9510 + step, cfg.K), cfg.Mw * cfg.bits, cfg.bits)
            for i, mat in enumerate(mats):
                check(L, mat, lut, order if step % 2 == 0 else order[::-1], 1, ("cache", runs, step, i))
        for i, mat in enumerate(mats):          # one matrix at a time: each learns its run again although the others' are evicted for it
            for step in range(3):
                lut.write(acts(9520 + 3 * i + step, cfg.K))
                check(L, mat, lut, order, 1, ("cache, one by one", runs, i, step))


if __name__ == "__main__":
    mode, scratch = sys.argv[1], sys.argv[2]
    assert torch.cuda.is_available(), "needs a GPU"
    lib = tmac_amd.lib()
    {"zero_copy_off": zero_copy_off, "small_cache": small_cache}[mode](lib, scratch)
    print("CHILD OK", mode)
