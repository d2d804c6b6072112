"""Where the kernels touch memory: no store outside an output, no store into an input, no value from outside an input reaching a result.

The other GPU files pass exactly sized torch tensors, which the caching allocator rounds up to 512 bytes and packs side by side: a
store of a whole pair, quad or padded tile where a tail belongs, or a LUT build that walks an act group too far, passes all of them.
Here every caller-owned buffer of a call is carved out of a guard-band arena (tests/footprint.py; its own proof is
tests/test_footprint_cpu.py), and every case makes the same assertion (footprint.check_footprint):

  1. the call on ordinary tensors, held to the oracle at the bar the kernel's own file uses (integers array_equal, floats by
     rel_err or by bits), finite everywhere: `want`;
  2. the same call on arena views, at a 256-byte placement and at ggml's (32 bytes and not 64), each with guards of 0x00 and of 0x7B:
     nothing outside the outputs changed, every output element written, every output equal to `want` BIT FOR BIT.

Shapes are the smallest of the other files at which a tail exists.  Out of scope: a read past an extent whose value is discarded
(visible only as a fault), and library-owned buffers (LUT workspace, weight and hand-off arenas).
The last tests pin the alignment contract of include/tmac_hip.h: a pointer below it is refused, nothing launched, queued or recorded.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import footprint as fp
from oracle import oracle as orc
from test_gpu_chain import BITS_BM, Model, tm, _short_spin, rel_err      # noqa: F401  (fixtures)
from test_gpu_chain_xform import Layer
from test_gpu_gemm_planes import mrow
from test_gpu_parity import GOLD, REL_TOL, check_bits, oracle_case
from xf_common import Mat, np_glu, np_norm

pytestmark = pytest.mark.gpu

DTYPES = [(False, False), (True, True), (False, True), (True, False)]      # (activations fp16, outputs fp16)
DTYPE_IDS = ["a32-o32", "a16-o16", "a32-o16", "a16-o32"]


def npdt(f16):
    return np.float16 if f16 else np.float32


# -------------------------------------------------------------------------------------------------
# split path, N = 1: tmac_hip_preprocessor_dev (B) + tmac_hip_qgemm_dev (C), every variant

SPLIT_CFGS = [  # Mw, K, bits, bm, kf, gs, ags, zp, m_groups
    (256, 1024, 2, 128, 16, 128, 64, True, -1), (256, 1024, 4, 256, 16, 64, 64, False, -1), (256, 1024, 1, 128, 16, 128, 64, True, -1),
    (256, 1024, 3, 192, 16, 128, 64, False, -1), (256, 1024, 2, 128, 8, 128, 32, True, -1),
    (320, 3200, 2, 320, 16, 128, 3200, False, 1), (160, 640, 2, 320, 16, 128, 640, False, 1),
]


@pytest.mark.parametrize("act_f16,out_f16", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("Mw,K,bits,bm,kf,gs,ags,zp,mg", SPLIT_CFGS)
def test_split_path(tm, Mw, K, bits, bm, kf, gs, ags, zp, mg, act_f16, out_f16):
    """variants 0, 1, 2, 4, 5, 7 (tiled / fused layouts, MFMA and v_mqsad accumulate) and 3 (the reference-layout kernel): QLUT, LUT scales /
    biases and integer sums bit-exact, fp32 outputs within 2e-5 (variant 3: by bits), fp16 outputs the oracle's rounded once within 1e-3"""
    import torch
    L = tm.lib()
    case = orc.make_case(7000 + Mw + K + bits, Mw, K, bits=bits, gs=gs, ags=ags, zero_point=zp, m_groups=mg, fp16_values=act_f16)
    A = orc.preprocess_weights(case["w"], bits, bm, kf)
    S = orc.preprocess_scales(case["sc"], case["zr"] if zp else None, bits, bm) if mg == -1 else case["sc"]
    q, ls, lb, Cc, PS = oracle_case(case, A, S, Mw, K, bits, bm, kf, gs, ags, zp, mg)
    for variant in (0, 1, 2, 4, 5, 7, 3):
        tm.binding.check(L.tmac_hip_set_variant(variant))
        wr = tm.TMACGeMMWrapper(act_group_size=ags)
        wr.set_workspace(K, 1)

        def call(alloc):
            Bt = alloc.inp(case["B"], npdt(act_f16), name="B")
            Ct = alloc.out((1, Mw), npdt(out_f16), name="C")
            alloc.arm()
            wr.llama_cpp_init(Bt, Mw, K, 1, bits)
            wr.llama_cpp_compute(w, Ct, 1)

        def check_want(want):
            torch.cuda.synchronize()
            gq, gls, glb = wr.workspace.read(K, 1, ags)
            assert np.array_equal(gq, q), variant
            check_bits(gls, ls); check_bits(glb, lb)
            assert np.array_equal(np.asarray(wr.partial_sums(w, 1)).reshape(PS.shape), PS), variant
            if out_f16:
                assert rel_err(want["C"].astype(np.float32), Cc.astype(np.float16).astype(np.float32)) <= REL_TOL, variant
            else:
                assert rel_err(want["C"], Cc) <= 2e-5, variant
                if variant == 3:
                    check_bits(want["C"], Cc)

        # (no variant is excused: one the dispatcher refuses for a configuration of SPLIT_CFGS is an error of this test)
        w = wr.register_weights(A, S, Mw, K, bits, tm.KCfg.make(Mw, K, bits, bm, kf, gs, ags, zp, mg), scales_dtype=tm.F32, dev_dtype=tm.F32)
        try:
            fp.check_footprint(call, check_want=check_want)
        finally:
            L.tmac_hip_set_variant(0)
            w.free()


# -------------------------------------------------------------------------------------------------
# fused entry point, N = 1: k_gemv_quad / k_gemv_fused, LUT built inside the kernel from B_dev

QUAD_CONFIGS = {0: [(0, 0), (512, 1), (768, 3), (1024, 4)], 7: [(0, 0), (512, 1)], 4: [(0, 0)], 5: [(0, 0)]}      # (threads, waves per quad); v_mqsad: 512 only


@pytest.mark.parametrize("act_f16,out_f16", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("K", [1024, 2688])
@pytest.mark.parametrize("nmat", [1, 2, 3, 4])
def test_fused_decode(tm, nmat, K, act_f16, out_f16):
    """1 to 4 matrices of 512 / 256 / 128 / 64 rows sharing the activations (the last workgroups own the tail of one matrix and the head of
    the next), K = 2688 with the ragged last step, the launch configurations of k_gemv_quad forced in turn: outputs within 2e-5 (fp16: 1e-3)"""
    L = tm.lib()
    bits, bm, kf, gs, ags = 2, 128, 16, 128, 64
    rows = [512, 256, 128, 64][:nmat]
    cases = [orc.make_case(7100 + 10 * K + i, Mw, K, bits=bits, gs=gs, ags=ags, fp16_values=act_f16) for i, Mw in enumerate(rows)]
    B = cases[0]["B"]
    host = [(orc.preprocess_weights(c["w"], bits, bm, kf), orc.preprocess_scales(c["sc"], c["zr"], bits, bm)) for c in cases]
    refs = [oracle_case(dict(c, B=B), A, S, Mw, K, bits, bm, kf, gs, ags, True)[3] for c, (A, S), Mw in zip(cases, host, rows)]
    for variant in (0, 4, 5, 7):          # (no variant and no launch configuration is excused: a refusal is an error of this test)
        tm.binding.check(L.tmac_hip_set_variant(variant))
        wr = tm.TMACGeMMWrapper(act_group_size=ags)
        ws = []

        def call(alloc):
            Bt = alloc.inp(B, npdt(act_f16), name="B")
            outs = [alloc.out((1, Mw), npdt(out_f16), name=f"C{i}") for i, Mw in enumerate(rows)]
            alloc.arm()
            wr.fused(ws, Bt, outs, 1)

        def check_want(want):
            for i, ref in enumerate(refs):
                assert rel_err(want[f"C{i}"].astype(np.float32), ref) <= (REL_TOL if out_f16 else 2e-5), (variant, i)

        ws.extend(wr.register_weights(A, S, Mw, K, bits, tm.KCfg.make(Mw, K, bits, bm, kf, gs, ags, True)) for (A, S), Mw in zip(host, rows))
        try:
            for ft, wpq in QUAD_CONFIGS[variant]:
                tm.binding.check(L.tmac_hip_debug_quad_config(ft, wpq))
                fp.check_footprint(call, check_want=check_want)
        finally:
            L.tmac_hip_debug_quad_config(0, 0)
            L.tmac_hip_set_variant(0)
            for w in ws:
                w.free()


# -------------------------------------------------------------------------------------------------
# N > 1: k_gemm_planes (both forms), k_gemm_onehot (forced), their unified-scale flavours, through the split entry points

NS = [2, 5, 33, 70]
GEMM_CFGS = [  # Mw, K, bits, bm, gs, zp, mg
    (128, 1024, 2, 128, 128, True, -1), (64, 512, 2, 128, 256, True, -1), (320, 3200, 3, 192, 128, False, -1), (128, 1024, 1, 64, 128, True, -1),
    (256, 1024, 4, 256, 64, False, -1), (320, 3200, 2, 320, 128, False, 1), (160, 640, 2, 320, 128, False, 1),
]


@functools.lru_cache(maxsize=None)
def gemm_reference(Mw, K, bits, bm, gs, zp, mg):
    """case, A, S and the oracle's q / ls / lb / C / integer sums for max(NS) activation rows: computed once; the rows are independent
    GEMVs (qgemm.py:183-190), a call with N rows takes the first N"""
    N, ags = max(NS), (K if mg >= 1 else 64)
    case = orc.make_case(7200 + Mw + K + bits, Mw, K, N=N, bits=bits, gs=gs, ags=ags, zero_point=zp, m_groups=mg)
    A = orc.preprocess_weights(case["w"], bits, bm, 16)
    S = orc.preprocess_scales(case["sc"], case["zr"] if zp else None, bits, bm) if mg == -1 else case["sc"]
    q, ls, lb, Cc, PS = oracle_case(case, A, S, Mw, K, bits, bm, 16, gs, ags, zp, mg, N=N)
    rows = np.arange(Mw)
    comb = sum(PS[:, mrow(rows, p, bits), :].astype(np.int64) << p for p in range(bits))      # what k_gemm_planes accumulates: sum_p 2^p PS_p
    for a in (Cc, PS, comb):
        a.setflags(write=False)
    return case, A, S, Cc, PS, comb


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("Mw,K,bits,bm,gs,zp,mg", GEMM_CFGS)
def test_gemm(tm, Mw, K, bits, bm, gs, zp, mg, N):
    """N = 2 and 5 (a few rows of a 64-row tile), 33 (ragged against 32 and 64), 70 (two tiles, the second nearly empty); Mw = 64, 160 and
    320 against the 256-column tile; tmac_hip_debug_gemm_kernel 2 / 3 = k_gemm_planes(_us) with eight / four waves, 1 = k_gemm_onehot:
    integer sums array_equal; per-group outputs within 1e-5 (one-hot: 2e-5), unified-scale outputs by bits; fp16 outputs within 1e-3"""
    import torch
    L = tm.lib()
    case, A, S, Cc, PS, comb = gemm_reference(Mw, K, bits, bm, gs, zp, mg)
    Cc, PS, comb, B = Cc[:N], PS[:N], comb[:N], case["B"][:N]
    ags = K if mg >= 1 else 64
    tm.binding.check(L.tmac_hip_set_gemm_min_n(1))
    wr = tm.TMACGeMMWrapper(act_group_size=ags)
    wr.set_workspace(K, N)
    w = wr.register_weights(A, S, Mw, K, bits, tm.KCfg.make(Mw, K, bits, bm, 16, gs, ags, zp, mg, N), scales_dtype=tm.F32, dev_dtype=tm.F32)
    for kernel in (2, 3, 1):
        tm.binding.check(L.tmac_hip_debug_gemm_kernel(kernel))
        for out_f16 in (False, True):
            def call(alloc):
                Bt = alloc.inp(B, np.float32, name="B")
                Ct = alloc.out((N, Mw), npdt(out_f16), name="C")
                alloc.arm()
                wr.llama_cpp_init(Bt, Mw, K, N, bits)
                wr.llama_cpp_compute(w, Ct, N)

            def check_want(want):
                torch.cuda.synchronize()
                if kernel == 1:
                    assert np.array_equal(np.asarray(wr.partial_sums(w, N)).reshape(PS.shape), PS), kernel
                else:
                    assert np.array_equal(wr.comb_sums(w, N).astype(np.int64), comb), kernel
                if out_f16:
                    assert rel_err(want["C"].astype(np.float32), Cc) <= REL_TOL, kernel
                elif mg >= 1:
                    check_bits(want["C"], Cc)
                else:
                    assert rel_err(want["C"], Cc) <= (2e-5 if kernel == 1 else 1e-5), kernel

            fp.check_footprint(call, check_want=check_want)
    w.free()


@pytest.mark.parametrize("out_f16", [False, True])
@pytest.mark.parametrize("N", NS)
def test_gemm_through_the_fused_entry(tm, N, out_f16):
    """tmac_hip_qgemm_fused_dev, N > 1, three matrices of 256 / 128 / 64 rows sharing the activations: the library's own LUT build from
    B_dev (image or half tables) and one launch over the three outputs, whatever the dispatcher picks (0) and each GEMM kernel forced"""
    L = tm.lib()
    K, bits, bm, gs, rows = 1024, 2, 128, 128, [256, 128, 64]
    cases = [orc.make_case(7300 + i, Mw, K, N=N, bits=bits, gs=gs, ags=64) for i, Mw in enumerate(rows)]
    B = cases[0]["B"]
    host = [(orc.preprocess_weights(c["w"], bits, bm, 16), orc.preprocess_scales(c["sc"], c["zr"], bits, bm)) for c in cases]
    refs = [oracle_case(dict(c, B=B), A, S, Mw, K, bits, bm, 16, gs, 64, True, N=N)[3] for c, (A, S), Mw in zip(cases, host, rows)]
    tm.binding.check(L.tmac_hip_set_gemm_min_n(1))
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    ws = [wr.register_weights(A, S, Mw, K, bits, tm.KCfg.make(Mw, K, bits, bm, 16, gs, 64, True, -1, N)) for (A, S), Mw in zip(host, rows)]

    def call(alloc):
        Bt = alloc.inp(B, np.float32, name="B")
        outs = [alloc.out((N, Mw), npdt(out_f16), name=f"C{i}") for i, Mw in enumerate(rows)]
        alloc.arm()
        wr.fused(ws, Bt, outs, N)

    def check_want(want):
        for i, ref in enumerate(refs):
            assert rel_err(want[f"C{i}"].astype(np.float32), ref) <= (REL_TOL if out_f16 else 2e-5), i

    for kernel in (0, 2, 3, 1):
        tm.binding.check(L.tmac_hip_debug_gemm_kernel(kernel))
        fp.check_footprint(call, check_want=check_want)
    tm.binding.check(L.tmac_hip_cache_clear())
    for w in ws:
        w.free()


@pytest.mark.parametrize("N", [5, 11])
def test_split_entry_small_n(tm, N):
    """test_split_entry_small_n_matches_oracle's route with the thresholds left alone: below PLANES_MIN_N no LUT image, the row loop"""
    Mw, K, bits, bm, gs = 512, 1024, 2, 128, 128
    c = orc.make_case(80 + N, Mw, K, bits=bits, N=N, gs=gs, ags=64, zero_point=True)
    A = orc.preprocess_weights(c["w"], bits, bm, 16)
    S = orc.preprocess_scales(c["sc"], c["zr"], bits, bm)
    Cc = oracle_case(c, A, S, Mw, K, bits, bm, 16, gs, 64, True, N=N)[3]
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    wr.set_workspace(K, N)
    w = wr.register_weights(A, S, Mw, K, bits, tm.KCfg.make(Mw, K, bits, bm, 16, gs, 64, True, -1, N), scales_dtype=tm.F32, dev_dtype=tm.F32)

    def call(alloc):
        Bt = alloc.inp(c["B"], np.float32, name="B")
        Ct = alloc.out((N, Mw), np.float32, name="C")
        alloc.arm()
        wr.llama_cpp_init(Bt, Mw, K, N, bits)
        wr.llama_cpp_compute(w, Ct, N)

    def check_want(want):
        assert rel_err(want["C"], Cc) <= 2e-5

    fp.check_footprint(call, check_want=check_want)
    w.free()


# -------------------------------------------------------------------------------------------------
# fast aggregation

@pytest.mark.parametrize("variant", [0, 3])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("Mw,K,bits,bm,kf,gs,ags", [(256, 1024, 2, 128, 16, 128, 64), (256, 1024, 2, 128, 8, 128, 32)])
def test_fast_aggregation(tm, Mw, K, bits, bm, kf, gs, ags, mode, variant):
    """test_fast_aggregation_vs_oracle's bars: tree results array_equal, variant 3 by bits, mode 1 within 1e-3, mode 2 within 1e-4"""
    import torch
    L = tm.lib()
    case = orc.make_case(7400 + ags, Mw, K, bits=bits, gs=gs, ags=ags)
    A = orc.preprocess_weights(case["w"], bits, bm, kf)
    S = orc.preprocess_scales(case["sc"], case["zr"], bits, bm)
    q, ls, lb = orc.preprocessor(case["B"], ags)
    Cc, tap = orc.qgemm_float_fa(A, q, S, ls, lb, Mw, K, 1, bits, bm, kf, gs, ags, True, mode)
    tm.binding.check(L.tmac_hip_set_variant(variant))
    wr = tm.TMACGeMMWrapper(act_group_size=ags)
    wr.set_workspace(K, 1)
    w = wr.register_weights(A, S, Mw, K, bits, tm.KCfg.make(Mw, K, bits, bm, kf, gs, ags, True), fast_aggregation=mode)

    def call(alloc):
        Bt = alloc.inp(case["B"], np.float32, name="B")
        Ct = alloc.out((1, Mw), np.float32, name="C")
        alloc.arm()
        wr.llama_cpp_init(Bt, Mw, K, 1, bits)
        wr.llama_cpp_compute(w, Ct, 1)

    def check_want(want):
        torch.cuda.synchronize()
        assert np.array_equal(wr.partial_sums(w, 1), tap)
        if variant == 3:
            check_bits(want["C"], Cc)
        else:
            assert np.abs(want["C"] - Cc).max() <= (1e-3 if mode == 1 else 1e-4) * np.abs(Cc).max()

    fp.check_footprint(call, check_want=check_want)
    w.free()


# -------------------------------------------------------------------------------------------------
# persistent kernels: k_decode_chain, and k_lut_images(_us) + k_gemv_stream

def run_model(m, alloc, launches, want_stream):
    """record m's calls on buffers from alloc (outputs, external vectors and the tap buffer), launch `launches` times"""
    import torch
    m.allocate(out_alloc=lambda i, k, Mw, dt: alloc.out((Mw,), dt, name=f"out{i}.{k}"), ext_alloc=lambda i, x, dt: alloc.inp(x, dt, name=f"x{i}"))
    chain = m.record()
    assert chain.stream == want_stream and chain.nops == len(m.ops)
    tap = alloc.out((chain.tap_layout(len(m.ops))[0],), np.int32, name="tap", tile=False)
    alloc.arm()
    chain.set_tap(tap)
    try:
        for _ in range(launches):          # replays: the generation tag advances
            chain.launch()
        torch.cuda.synchronize()
        assert chain.status() == 0
    finally:
        chain.set_tap(None)
        chain.free()


def model_footprint(tm, ops, want_stream, launches=3, **kw):
    """Model.check / check_tap on ordinary tensors first (stand-alone launches by bits, the oracle within 1e-3, the kernel's own integers
    array_equal), then the guarded runs: outputs AND tap bit-identical to the plain run's, the tap's interior fully written"""
    import torch
    m = Model(tm, ops, **kw)
    chain = m.record()
    assert chain.stream == want_stream
    chain.launch()
    m.check(chain)
    m.check_tap(chain)
    # the launch that was just held to the oracle, once more with a tap buffer of this test's own (check_tap keeps its buffer to itself)
    total = chain.tap_layout(len(ops))[0]
    tap = torch.full((total,), -(2 ** 31), dtype=torch.int32, device="cuda")
    chain.set_tap(tap)
    chain.launch(); torch.cuda.synchronize()
    chain.set_tap(None)
    assert chain.status() == 0
    first = {f"out{i}.{k}": o.cpu().numpy() for i, os_ in enumerate(m.outs) for k, o in enumerate(os_)}
    first["tap"] = tap.cpu().numpy()
    assert not (first["tap"] == -(2 ** 31)).any(), "the tap buffer has elements the launch does not write"
    chain.free()

    def check_want(want):          # the three-launch run on ordinary buffers == the checked launch, tap included
        assert set(want) == set(first)
        for name, ref in first.items():
            assert np.array_equal(fp.bits(want[name]), fp.bits(ref)), name

    fp.check_footprint(lambda alloc: run_model(m, alloc, launches, want_stream), check_want=check_want, nbytes=32 << 20)
    m.free()


SMALL = [            # test_gpu_chain.SMALL: Mw = 64 (128-byte output) and K = 256 (512-byte activations) among them
    (1024, [512, 256], None), (512, [1024], (0, 0)), (1024, [2688, 512, 128], (1, 0)), (2688, [1024], (2, 0)), (1024, [64], (3, 0)),
    (256, [256, 256], (0, 1)), (256, [4096], (5, 1)), (4096, [1024, 1024], (6, 0)), (1024, [512], None),
]
CHAIN_US = [(3200, [640, 640], None), (640, [1024], (0, 1)), (1024, [64], (1, 0)), (3200, [256], None)]      # from test_gpu_chain.UNIFIED


@pytest.mark.parametrize("grid", [0, 7, 1])
@pytest.mark.parametrize("ext_f32", [False, True])
@pytest.mark.parametrize("bits,zp,mg", [(2, True, -1), (4, False, -1), (3, True, -1), (2, False, 1)])
def test_decode_chain(tm, bits, zp, mg, ext_f32, grid):
    """k_decode_chain on all of the device's workgroups, on 7 and on 1 (tmac_hip_debug_chain_grid): every workgroup then owns many row
    pairs of every output and the b16 / b32 / b64 stores of tmac_chain_core.h are chosen at other rows"""
    tm.binding.check(tm.lib().tmac_hip_debug_chain_grid(grid))
    try:
        model_footprint(tm, CHAIN_US if mg >= 1 else SMALL, False, bits=bits, zp=zp, mg=mg, ext_f32=ext_f32, seed=50 + bits + mg)
    finally:
        tm.lib().tmac_hip_debug_chain_grid(0)


STREAM = [(1024, [512, 256], None), (2688, [640], None), (128, [64], None), (256, [128, 64, 64, 128], None)]      # test_gpu_stream.INDEP at its smallest
STREAM_US = [(3200, [320], None), (640, [128, 64], None), (1024, [64], None)]


@pytest.fixture(params=["auto", "quad64"])
def _form(request, monkeypatch):
    """test_gpu_stream.py's two walk forms of k_gemv_stream: the default choice (quarter walk where it applies), row quad x 64 units forced"""
    if request.param == "quad64":
        monkeypatch.setenv("TMAC_STREAM_QW", "0")
    return request.param


@pytest.mark.parametrize("grid", [0, 1, 7, 13])
@pytest.mark.parametrize("out_f16", [True, False])
@pytest.mark.parametrize("bits,zp,mg", [(2, True, -1), (4, False, -1), (2, False, 1)])
def test_stream(tm, _form, bits, zp, mg, out_f16, grid):
    """k_lut_images / k_lut_images_us read the external vectors 16 bytes at a time, k_gemv_stream stores element by element: K = 128
    (256 bytes of fp16 activations), Mw = 64 outputs, K = 2688 with the ragged last step, on few workgroups and on all"""
    tm.binding.check(tm.lib().tmac_hip_debug_chain_grid(grid))
    try:
        model_footprint(tm, STREAM_US if mg >= 1 else STREAM, True, bits=bits, zp=zp, mg=mg, out_f16=out_f16, seed=70 + bits + mg)
    finally:
        tm.lib().tmac_hip_debug_chain_grid(0)


def test_deferred_queue(tm):
    """eight independent calls queued (tmac_hip_defer) and launched by one tmac_hip_flush as a stream: every output within 1e-3 of the oracle,
    and guarded like a recording"""
    import torch
    L = tm.lib()
    ops = [(1024, [256], None), (256, [128, 64], None), (2688, [128], None), (128, [64], None)] * 2
    m = Model(tm, ops, seed=77)

    def call(alloc):
        m.allocate(out_alloc=lambda i, k, Mw, dt: alloc.out((Mw,), dt, name=f"out{i}.{k}"), ext_alloc=lambda i, x, dt: alloc.inp(x, dt, name=f"x{i}"))
        alloc.arm()
        tm.binding.check(L.tmac_hip_defer(1))
        try:
            m.issue()
            st = [C.c_uint64(0) for _ in range(4)]
            tm.binding.check(L.tmac_hip_flush(None))
            tm.binding.check(L.tmac_hip_defer_stats(*[C.byref(x) for x in st]))
            assert st[2].value >= 1, "the flush launched no stream"
        finally:
            tm.binding.check(L.tmac_hip_defer(0))
        torch.cuda.synchronize()

    def check_want(want):
        for i in range(len(ops)):
            ref = m.oracle_outputs(i, m.x_host[i].astype(np.float16).astype(np.float32))
            for k in range(len(ops[i][1])):
                assert rel_err(want[f"out{i}.{k}"].astype(np.float32), ref[k]) <= 1e-3, (i, k)

    fp.check_footprint(call, check_want=check_want)
    tm.binding.check(L.tmac_hip_cache_clear())
    m.free()


# -------------------------------------------------------------------------------------------------
# chain transforms: x, x2, residual, gamma (inputs), residual_out and the three outputs

@pytest.mark.parametrize("grid", [0, 96, 7, 1])
def test_chain_transforms(tm, grid):
    """test_gpu_chain_xform._norm_and_glu_on_external_vectors' recording: the 16-byte loads of in2 / residual / gamma into LDS, and
    residual_out striped over however many workgroups exist -- t = x + residual array_equal, outputs within 2e-3 of the oracle"""
    import torch
    tm.binding.check(tm.lib().tmac_hip_debug_chain_grid(grid))
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    rng = np.random.default_rng(11)
    K, Mw = 1024, 512
    mats = [Mat(tm, wr, s, Mw, K) for s in (1, 2, 3)]
    xh, x2h = (rng.standard_normal(K).astype(np.float16) for _ in range(2))
    rh = rng.standard_normal(K).astype(np.float32)
    gh = (1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)

    def call(alloc):
        x, x2, res, gam = alloc.inp(xh, name="x"), alloc.inp(x2h, name="x2"), alloc.inp(rh, name="residual"), alloc.inp(gh, name="gamma")
        rout = alloc.out((K,), np.float32, name="residual_out")
        o = [alloc.out((Mw,), np.float16, name=f"out{i}") for i in range(3)]
        with wr.record_chain() as rec:
            wr.chain_xform("norm", residual=res, gamma=gam, eps=1e-5, residual_out=rout)
            wr.fused([mats[0].w], x, [o[0]], 1, act_dtype=tm.F16)
            wr.chain_xform("glu", in2=x2)
            wr.fused([mats[1].w], x, [o[1]], 1, act_dtype=tm.F16)
            wr.chain_xform("norm", residual=res)                       # add only
            wr.fused([mats[2].w], x, [o[2]], 1, act_dtype=tm.F16)
        alloc.arm()
        for _ in range(2):
            rec.chain.launch()
        torch.cuda.synchronize()
        assert rec.chain.status() == 0
        rec.chain.free()

    def check_want(want):
        xf, x2f = xh.astype(np.float32), x2h.astype(np.float32)
        t = xf + rh
        assert np.array_equal(want["residual_out"], t)
        assert rel_err(want["out0"].astype(np.float32), mats[0].oracle(np_norm(t, gh, 1e-5))) <= 2e-3
        assert rel_err(want["out1"].astype(np.float32), mats[1].oracle(np_glu(xf, x2f))) <= 2e-3
        assert rel_err(want["out2"].astype(np.float32), mats[2].oracle(t)) <= 2e-3

    try:
        fp.check_footprint(call, check_want=check_want)
    finally:
        tm.lib().tmac_hip_debug_chain_grid(0)
    for mt in mats:
        mt.w.free()


def test_decoder_segment(tm):
    """one segment of test_gpu_chain_xform.test_decoder_layers_with_an_operator_outside at (H, F) = (1024, 2560): o -> [+ residual, RMSNorm,
    kept] -> gate / up -> [silu(gate) * up] -> down -> [+ carried residual, RMSNorm, residual_out] -> q / k / v.  F = 2560: 640 row pairs,
    no multiple of the workgroup count, so the row-pair ranges are ragged; eight outputs, three of them handed over inside the launch"""
    import torch
    H, F, eps = 1024, 2560, 1e-5
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    La, Ln = Layer(tm, wr, 100, H, F), Layer(tm, wr, 200, H, F)
    rng = np.random.default_rng(5)
    ah, hh = rng.standard_normal(H).astype(np.float16), rng.standard_normal(H).astype(np.float32)
    g2h, g1h = La.g2.cpu().numpy(), Ln.g1.cpu().numpy()

    def call(alloc):
        attn, hin, g2, g1 = alloc.inp(ah, name="attn"), alloc.inp(hh, name="h"), alloc.inp(g2h, name="gamma2"), alloc.inp(g1h, name="gamma1")
        b = {n: alloc.out((F if n in ("gate", "up") else H,), np.float16, name=n) for n in ("o", "gate", "up", "down", "q", "k", "v")}
        h_out = alloc.out((H,), np.float32, name="h_out")
        with wr.record_chain() as rec:
            wr.fused([La.o.w], attn, [b["o"]], 1, act_dtype=tm.F16)
            wr.chain_xform("norm", residual=hin, gamma=g2, eps=eps, keep=True)
            wr.fused([La.gate.w, La.up.w], b["o"], [b["gate"], b["up"]], 1, act_dtype=tm.F16)
            wr.chain_xform("glu", in2=b["up"])
            wr.fused([La.down.w], b["gate"], [b["down"]], 1, act_dtype=tm.F16)
            wr.chain_xform("norm", residual=wr.CARRY, gamma=g1, eps=eps, residual_out=h_out)
            wr.fused([Ln.q.w, Ln.k.w, Ln.v.w], b["down"], [b["q"], b["k"], b["v"]], 1, act_dtype=tm.F16)
        alloc.arm()
        for _ in range(2):
            rec.chain.launch()
        torch.cuda.synchronize()
        assert rec.chain.status() == 0
        rec.chain.free()

    def check_want(want):
        f = {n: v.astype(np.float32) for n, v in want.items()}
        assert rel_err(f["o"], La.o.oracle(ah.astype(np.float32))) <= 2e-3
        t2 = f["o"] + hh
        x2 = np_norm(t2, g2h, eps)
        assert rel_err(f["gate"], La.gate.oracle(x2)) <= 2e-3 and rel_err(f["up"], La.up.oracle(x2)) <= 2e-3
        glu = np_glu(f["gate"], f["up"]).astype(np.float16).astype(np.float32)      # the hand-off image holds silu(gate) * up as fp16
        assert rel_err(f["down"], La.down.oracle(glu)) <= 2e-3
        t3 = f["down"] + t2
        assert np.array_equal(want["h_out"], t3)
        x3 = np_norm(t3, g1h, eps)
        for n, mt in (("q", Ln.q), ("k", Ln.k), ("v", Ln.v)):
            assert rel_err(f[n], mt.oracle(x3)) <= 2e-3

    fp.check_footprint(call, check_want=check_want)
    for L_ in (La, Ln):
        for mt in (L_.q, L_.k, L_.v, L_.o, L_.gate, L_.up, L_.down):
            mt.w.free()


# -------------------------------------------------------------------------------------------------
# tmac_hip_register_weights_dev: A_ref_dev and scales_ref_dev are the caller's

@pytest.mark.parametrize("dev_f16", [True, False])
@pytest.mark.parametrize("bits,bm", [(1, 128), (2, 128), (3, 192), (4, 256)])
def test_register_weights_from_device_memory(tm, bits, bm, dev_f16):
    """the re-tiling kernels read the reference-layout blobs out of guarded views; the matrix they make is then multiplied (fused entry,
    buffers guarded as well): same bits under both guard patterns, within 2e-5 of the oracle"""
    Mw, K, kf, gs, ags = 256, 1024, 16, 128, 64
    case = orc.make_case(7500 + bits, Mw, K, bits=bits, gs=gs, ags=ags, fp16_values=True)
    A = orc.preprocess_weights(case["w"], bits, bm, kf)
    S = orc.preprocess_scales(case["sc"], case["zr"], bits, bm)
    Cc = oracle_case(case, A, S, Mw, K, bits, bm, kf, gs, ags, True)[3]
    wr = tm.TMACGeMMWrapper(act_group_size=ags)

    def call(alloc):
        At = alloc.inp(np.ascontiguousarray(A, np.uint8).reshape(-1), name="A_ref")
        St = alloc.inp(np.ascontiguousarray(S, np.float32).reshape(-1), name="scales_ref")
        Bt = alloc.inp(case["B"], np.float32, name="B")
        Ct = alloc.out((1, Mw), np.float32, name="C")
        alloc.arm()
        w = wr.register_weights(At, St, Mw, K, bits, tm.KCfg.make(Mw, K, bits, bm, kf, gs, ags, True), scales_dtype=tm.F32,
                                dev_dtype=tm.F16 if dev_f16 else tm.F32, on_device=True)
        wr.fused([w], Bt, [Ct], 1)
        alloc.results()                  # (synchronises: the matrix is freed behind its launch)
        w.free()

    def check_want(want):
        assert rel_err(want["C"], Cc) <= 2e-5

    fp.check_footprint(call, check_want=check_want)


# -------------------------------------------------------------------------------------------------
# host pointers: layer (1) and the read-back taps write into the CALLER's heap

def _vp(a):
    return C.c_void_p(a.ctypes.data)


def test_host_pointer_layer(tm, tmp_path):
    """preprocessor_int8 / qgemm_lut_int8 tile by tile with B, QLUT, LUT scales / biases, A, Scales and C in a numpy arena: QLUT, scales and
    biases bit-exact, C within 2e-5"""
    L = tm.lib()
    Mw, K, bits, bm, kf, gs, ags = 512, 1024, 2, 128, 16, 128, 64
    ntile, rpt = Mw * bits // bm, bm // bits
    ini = tmp_path / "kcfg.ini"
    ini.write_text(f"[qgemm_lut_t1_int8_m{Mw * bits}_k{K}_n1_b2]\nbm = {bm}\nsimd_n_in = 16\nsimd_n_out = 8\nkfactor = {kf}\n"
                   f"group_size = {gs}\nlut_scales_size = {K // ags}\nscales_size = {Mw * K // gs * 2}\nn_tile_num = {ntile}\n")
    tm.binding.check(L.tmac_hip_load_kcfg(str(ini).encode()))
    case = orc.make_case(7600, Mw, K, bits=bits, gs=gs, ags=ags)
    A = np.ascontiguousarray(orc.preprocess_weights(case["w"], bits, bm, kf))
    S = np.ascontiguousarray(orc.preprocess_scales(case["sc"], case["zr"], bits, bm))
    q, ls, lb, Cc, _ = oracle_case(case, A, S, Mw, K, bits, bm, kf, gs, ags, True)

    def call(alloc):
        L.tmac_hip_cache_clear()
        Bh = alloc.inp(case["B"], np.float32, name="B")
        Ah, Sh = alloc.inp(A, name="A"), alloc.inp(S, name="Scales")
        lsh, lbh = alloc.out((K // ags,), np.float32, name="LUT_Scales"), alloc.out((K // ags,), np.float32, name="LUT_Biases")
        qh = alloc.out((K // 4, 16), np.int8, name="QLUT")
        ch = [alloc.out((rpt,), np.float32, name=f"C{t}") for t in range(ntile)]
        alloc.arm()
        assert L.preprocessor_int8(Mw * bits, K, 1, bits, _vp(Bh), _vp(lsh), _vp(lbh), _vp(qh)) == 0, L.tmac_hip_last_error()
        for t in range(ntile):
            assert L.qgemm_lut_int8(bm, K, 1, bits, _vp(Ah[t]), _vp(qh), _vp(Sh[t]), _vp(lsh), _vp(lbh), _vp(ch[t])) == 0, L.tmac_hip_last_error()

    def check_want(want):
        assert np.array_equal(want["QLUT"], q[0])
        check_bits(want["LUT_Scales"], ls[0]); check_bits(want["LUT_Biases"], lb[0])
        assert rel_err(np.concatenate([want[f"C{t}"] for t in range(ntile)]), Cc[0]) <= 2e-5

    fp.check_footprint(call, device="numpy", check_want=check_want, nbytes=8 << 20)
    L.tmac_hip_cache_clear()


def test_shape_named_host_pointer_kernel(tm, tmp_path):
    """preprocessor_t1_int8_m8192_k4096_n1_b2 on the reference's own prebuilt vector (test_host_pointer_cabi_matches_prebuilt_reference)"""
    d = dict(np.load(os.path.join(GOLD, "prebuilt_llama2_7b_w2_k4096.npz")))
    L = tm.lib()
    ini = tmp_path / "kcfg.ini"
    ini.write_text("[qgemm_lut_t1_int8_m8192_k4096_n1_b2]\nbm = 128\nsimd_n_in = 16\nsimd_n_out = 8\nkfactor = 16\n"
                   "group_size = 128\nlut_scales_size = 64\nscales_size = 262144\nn_tile_num = 64\n")
    tm.binding.check(L.tmac_hip_load_kcfg(str(ini).encode()))
    K = 4096
    fn = L.preprocessor_t1_int8_m8192_k4096_n1_b2
    fn.restype = C.c_int32

    def call(alloc):
        Bh = alloc.inp(d["B"][0], np.float32, name="B")
        lsh, lbh = alloc.out((64,), np.float32, name="LUT_Scales"), alloc.out((64,), np.float32, name="LUT_Biases")
        qh = alloc.out((K // 4, 16), np.int8, name="QLUT")
        alloc.arm()
        assert fn(_vp(Bh), _vp(lsh), _vp(lbh), _vp(qh)) == 0, L.tmac_hip_last_error()

    def check_want(want):
        assert np.array_equal(want["QLUT"], d["qlut"])
        check_bits(want["LUT_Scales"], d["lut_scales"]); check_bits(want["LUT_Biases"], d["lut_biases"])

    fp.check_footprint(call, device="numpy", check_want=check_want, nbytes=8 << 20)
    L.tmac_hip_cache_clear()


@pytest.mark.parametrize("N", [1, 5])
def test_host_readers(tm, N):
    """tmac_hip_workspace_read, tmac_hip_qgemm_partial_sums, tmac_hip_qgemm_fused_partial_sums and tmac_hip_debug_gemm_comb_sums copy device
    results into host buffers of the caller: carved numpy views, every integer against the oracle"""
    import torch
    L = tm.lib()
    Mw, K, bits, bm, kf, gs, ags = 128, 1024, 2, 128, 16, 128, 64
    case = orc.make_case(7700 + N, Mw, K, N=N, bits=bits, gs=gs, ags=ags)
    A = orc.preprocess_weights(case["w"], bits, bm, kf)
    S = orc.preprocess_scales(case["sc"], case["zr"], bits, bm)
    q, ls, lb, Cc, PS = oracle_case(case, A, S, Mw, K, bits, bm, kf, gs, ags, True, N=N)
    rows = np.arange(Mw)
    comb = sum(PS[:, mrow(rows, p, bits), :].astype(np.int64) << p for p in range(bits))
    tm.binding.check(L.tmac_hip_set_gemm_min_n(1))
    wr = tm.TMACGeMMWrapper(act_group_size=ags)
    wr.set_workspace(K, N)
    w = wr.register_weights(A, S, Mw, K, bits, tm.KCfg.make(Mw, K, bits, bm, kf, gs, ags, True, -1, N), scales_dtype=tm.F32, dev_dtype=tm.F32)
    Bt = torch.from_numpy(case["B"]).cuda()
    Ct = torch.empty((N, Mw), dtype=torch.float32, device="cuda")
    G = K // ags

    def call(alloc):
        flat = dict(tile=False)          # (no [N][Mw] matrices: plain 4096-byte guards)
        qh = alloc.out((N, K // 4, 16), np.int8, name="q", **flat)
        lsh, lbh = alloc.out((N, G), np.float32, name="ls", **flat), alloc.out((N, G), np.float32, name="lb", **flat)
        psh = alloc.out((N, Mw * bits, G), np.int32, name="PS", **flat)
        fps, flut = alloc.out((N, Mw * bits, G), np.int32, name="fused_PS", **flat), alloc.out((N, 2, G), np.float32, name="fused_lut", **flat)
        fc = alloc.out((N, Mw), np.float32, name="fused_C")
        cmb = alloc.out((N, Mw, K // 64), np.int32, name="comb", **flat) if N > 1 else None
        alloc.arm()
        tm.binding.check(L.tmac_hip_debug_gemm_kernel(2 if N > 1 else 0))
        wr.llama_cpp_init(Bt, Mw, K, N, bits)
        wr.llama_cpp_compute(w, Ct, N)
        tm.binding.check(L.tmac_hip_workspace_read(wr.workspace.handle, _vp(qh), _vp(lsh), _vp(lbh), K, N, ags, None))
        if N > 1:
            tm.binding.check(L.tmac_hip_debug_gemm_comb_sums(w.handle, wr.workspace.handle, _vp(cmb), N, None))
        tm.binding.check(L.tmac_hip_debug_gemm_kernel(0))
        tm.binding.check(L.tmac_hip_qgemm_partial_sums(w.handle, wr.workspace.handle, _vp(psh), N, None))
        tm.binding.check(L.tmac_hip_qgemm_fused_partial_sums(w.handle, Bt.data_ptr(), tm.F32, _vp(fps), _vp(fc), _vp(flut), N, None))

    def check_want(want):
        assert np.array_equal(want["q"], q)
        check_bits(want["ls"], ls); check_bits(want["lb"], lb)
        assert np.array_equal(want["PS"], PS) and np.array_equal(want["fused_PS"], PS)
        check_bits(want["fused_lut"][:, 0, :], ls); check_bits(want["fused_lut"][:, 1, :], lb)
        assert rel_err(want["fused_C"], Cc) <= 2e-5
        if N > 1:
            assert np.array_equal(want["comb"].astype(np.int64), comb)

    fp.check_footprint(call, device="numpy", check_want=check_want, nbytes=8 << 20)
    w.free()


# -------------------------------------------------------------------------------------------------
# the alignment contract (include/tmac_hip.h): refused with TMAC_HIP_E_ARG, the argument named, nothing launched, queued or recorded

E_ARG = -4


def _refused(tm, fn, name):
    with pytest.raises(tm.TMACHipError) as e:
        fn()
    assert e.value.code == E_ARG and name in str(e.value) and "aligned" in str(e.value), e.value


def test_misaligned_pointers_are_refused(tm):
    """an fp16 view one element into a tensor as B_dev and as C_dev, an fp32 output 8 bytes in; what the contract allows (fp16 output 8
    bytes in, everything 32 bytes in) is served"""
    import torch
    L = tm.lib()
    Mw, K, bits, bm = 128, 512, 2, 128
    case = orc.make_case(7800, Mw, K, bits=bits, fp16_values=True)
    A = orc.preprocess_weights(case["w"], bits, bm, 16)
    S = orc.preprocess_scales(case["sc"], case["zr"], bits, bm)
    Cc = oracle_case(case, A, S, Mw, K, bits, bm, 16, 128, 64, True)[3][0]
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    wr.set_workspace(K, 1)
    w = wr.register_weights(A, S, Mw, K, bits, tm.KCfg.make(Mw, K, bits, bm, 16, 128, 64, True))
    xa, xc = (torch.zeros(K + 64, dtype=torch.float16, device="cuda") for _ in range(2))
    ob = torch.full((Mw + 64,), float("nan"), dtype=torch.float16, device="cuda")
    ob32 = torch.full((Mw + 64,), float("nan"), dtype=torch.float32, device="cuda")
    x, x_odd, x_32 = xa[:K], xa[1:1 + K], xc[16:16 + K]          # x_odd: 2 bytes in (refused before anything reads it); x_32: 32 bytes in
    x.copy_(torch.from_numpy(case["B"][0]).half()); x_32.copy_(torch.from_numpy(case["B"][0]).half())
    _refused(tm, lambda: wr.fused([w], x_odd, [ob[:Mw]], 1), "B_dev")
    _refused(tm, lambda: wr.fused([w], x, [ob[1:1 + Mw]], 1), "C_dev[0]")
    _refused(tm, lambda: wr.fused([w], x, [ob32[2:2 + Mw]], 1), "C_dev[0]")           # fp32 outputs: 16 bytes
    _refused(tm, lambda: wr.llama_cpp_init(x_odd, Mw, K, 1, bits), "B_dev")
    wr.llama_cpp_init(x, Mw, K, 1, bits)
    _refused(tm, lambda: wr.llama_cpp_compute(w, ob[1:1 + Mw], 1), "C_dev")
    _refused(tm, lambda: wr.llama_cpp_compute(w, ob32[2:2 + Mw], 1), "C_dev")
    torch.cuda.synchronize()
    assert bool(torch.isnan(ob).all()) and bool(torch.isnan(ob32).all()), "a refused call launched something"
    for xs, os_ in ((x, ob[4:4 + Mw]), (x_32, ob[16:16 + Mw]), (x_32, ob32[8:8 + Mw])):      # 8 bytes in (fp16 output), 32 bytes in
        wr.fused([w], xs, [os_], 1)
        torch.cuda.synchronize()
        assert rel_err(os_.float().cpu().numpy(), Cc) <= REL_TOL
    w.free()


def test_misaligned_pointers_are_refused_when_queued(tm):
    """with deferral on: the code and message of the non-deferred call, at once; the queue is left alone and one flush launches the valid
    calls around the refused ones (test_gpu_defer.test_invalid_calls_are_refused_when_they_are_queued's scheme)"""
    import torch
    from test_gpu_defer import Calls, raw_fused, stats
    L = tm.lib()
    c = Calls(tm, [Model(tm, [(1024, [256], None), (512, [128], None), (1024, [512], None)], seed=72)])
    m = c.models[0]
    xb = torch.zeros(1024 + 8, dtype=torch.float16, device="cuda")
    ob = torch.full((256 + 8,), float("nan"), dtype=torch.float16, device="cuda")
    bad = [([m.ws[0][0]], xb[1:1025], [ob[:256]]), ([m.ws[0][0]], m.x_ext[0], [ob[1:257]])]
    off = [raw_fused(tm, *b) for b in bad]
    assert [rc for rc, _ in off] == [E_ARG, E_ARG] and "B_dev" in off[0][1] and "C_dev[0]" in off[1][1], off
    c.poison()
    tm.binding.check(L.tmac_hip_defer(1))
    try:
        s0 = stats(tm)
        c.issue(0)
        for j, (b, (rc_off, msg_off)) in enumerate(zip(bad, off)):
            assert raw_fused(tm, *b) == (rc_off, msg_off)
            c.issue(1 + j)
        assert stats(tm) == s0, "a refused call disturbed the queue"
        tm.binding.check(L.tmac_hip_flush(None))
        s1 = stats(tm)
        assert s1[0] == s0[0] + 1 and (s1[2] - s0[2], s1[3] - s0[3]) == (1, 0), (s0, s1)
        torch.cuda.synchronize()
    finally:
        L.tmac_hip_defer(0)
    assert bool(torch.isnan(ob).all()), "a refused call launched something"
    for j in range(3):
        c.check_right(j, "misaligned call refused at enqueue")
    c.free()


def test_misaligned_pointers_are_refused_while_recording(tm):
    """a recorded call with a misaligned B_dev or C_dev, a transform with a misaligned vector: refused, not recorded, and neither the
    refused call's transform nor the refused transform reaches the next call -- the chain holds the two valid calls and computes them"""
    import torch
    L = tm.lib()
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    K, Mw = 1024, 512
    m0, m1 = Mat(tm, wr, 5, Mw, K), Mat(tm, wr, 6, Mw, K)
    rng = np.random.default_rng(12)
    xh = rng.standard_normal(K).astype(np.float16)
    rh = rng.standard_normal(K + 8).astype(np.float32)
    x, xb = torch.from_numpy(xh).cuda(), torch.zeros(K + 8, dtype=torch.float16, device="cuda")
    res = torch.from_numpy(rh).cuda()
    o0, o1 = (torch.full((Mw,), float("nan"), dtype=torch.float16, device="cuda") for _ in range(2))
    ob = torch.full((Mw + 8,), float("nan"), dtype=torch.float16, device="cuda")
    tm.binding.check(L.tmac_hip_chain_begin())
    wr._recording = []
    try:
        wr.fused([m0.w], x, [o0], 1)
        wr.chain_xform("norm", residual=res[:K])                                    # belongs to the call refused next: dropped with it
        _refused(tm, lambda: wr.fused([m1.w], xb[1:1 + K], [ob[:Mw]], 1), "B_dev")
        _refused(tm, lambda: wr.fused([m1.w], x, [ob[1:1 + Mw]], 1), "C_dev[0]")
        for vec in ("residual", "gamma", "residual_out"):
            _refused(tm, lambda: wr.chain_xform("norm", **{vec: res[1:1 + K]}), vec)
        _refused(tm, lambda: wr.chain_xform("glu", in2=xb[1:1 + K]), "in2")
        wr.fused([m1.w], x, [o1], 1)
    finally:
        wr._recording = None
        h = C.c_void_p()
        rc = L.tmac_hip_chain_end(C.byref(h))
    tm.binding.check(rc)
    chain = tm.DecodeChain(h, None)
    assert chain.nops == 2
    chain.launch()
    torch.cuda.synchronize()
    assert chain.status() == 0
    assert bool(torch.isnan(ob).all())
    xf = xh.astype(np.float32)
    assert rel_err(o0.float().cpu().numpy(), m0.oracle(xf)) <= 2e-3
    assert rel_err(o1.float().cpu().numpy(), m1.oracle(xf)) <= 2e-3          # no transform was left pending: plain x, not x + residual
    chain.free()
    m0.w.free(); m1.w.free()
