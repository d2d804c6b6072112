"""BitNet master weights to handles on the GPU: tmac_hip_absmean_dev, tmac_hip_pack_absmean_dev, tmac_hip_register_weights_absmean_dev
(k_absmean, k_absmean_scales, k_pack_dense_weights in tmac_pack.hip) and what sits on top (wrapper.absmean / pack_bitnet,
Weights.from_bitnet, checkpoint.load_bitnet_dir).

The reference tree holds no BitNet quantiser, so the yardstick of the levels is convert.bitnet_absmean_quant, the published absmean rule in
numpy (float64 mean, float32 element-wise part; tests/test_bitnet_quant_cpu.py ties it to a float64 restatement and a table of ties):
1. the scale: within 1 fp32 ulp of float32(float64 mean |w|) per row block -- an fp64 sum of n <= 2^31 non-negative terms is off by at
   most n 2^-53 relative (3e-9 at BitNet-3B's largest matrix), far below half an fp32 ulp, so only the final rounding can differ -- and
   the same bits on every launch and stream;
2. the blob: byte for byte weights.preprocess_weights of the host reference's levels under the DEVICE's scale; ties, signed zero,
   infinities and NaN through the hand-written table at a given scale of 1.0;
3. the handle: bit for bit (torch.equal) the plain twin from_codes(levels, scales) on every route, and the twin is bit for bit
   orc.qgemm_scale_final, the bar of the unified-scale tests (test_gpu_parity.py, test_gpu_rows.py, test_gpu_gemm_planes.py);
4. refusals, 5. ordering behind the deferred queue, 6. footprint, 7. the checkpoint loader.
Shapes (Mw, K, bm, m_groups): (128, 256, 128) one tile, less than a wave of pairs; (160, 3200, 320) a last row tile of 32 rows, 800
tables = 12.5 tiles of tables, BitNet's ragged K, and a row block of four reduction chunks, the last short; (256, 2304, 128); (256, 1024,
128) with 1, 2 and 4 row blocks.  make_shape accepts all of them.  Every shape in fp32, fp16 and bf16.
"""
import ctypes as C

import numpy as np
import pytest

import bitnet_common as bc
import footprint as fp
import pack_common as pc
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
E_NOMATCH, E_ARG = -1, -4
KF = 16
SHAPES = [(128, 256, 128, 1), (160, 3200, 320, 1), (256, 2304, 128, 1), (256, 1024, 128, 1), (256, 1024, 128, 2), (256, 1024, 128, 4)]
QUAD_CONFIGS = [(512, 1), (512, 2), (768, 3), (1024, 4)]              # (threads, waves per quad)


@pytest.fixture(scope="module")
def tm():
    import torch
    import tmac_amd
    assert torch.cuda.is_available()
    return tmac_amd


def kcfg(tm, Mw, K, bm, mg):
    return tm.KCfg.make(Mw, K, 2, bm, KF, 128, K, False, mg)


def dev(st):
    """the storage form on the GPU as torch sees it (bf16 bit patterns -> a bfloat16 tensor)"""
    import torch
    if st.dtype == np.uint16:
        return torch.from_numpy(st.view(np.int16)).cuda().view(torch.bfloat16)
    return torch.from_numpy(st).cuda()


_CASES = {}


def case(tm, shape, src):
    """(storage masters, the device's scales as numpy, host levels under them, host blob A, S) of one shape and dtype: made once, shared"""
    from tmac_amd import wrapper
    key = (shape, src)
    if key not in _CASES:
        Mw, K, bm, mg = shape
        st = bc.masters(1000 + Mw + K + mg, Mw, K, src, mg)
        s_dev = wrapper.absmean(dev(st), mg).cpu().numpy()
        A, S, lv = bc.host_blob(st, bm, KF, mg, scale=s_dev)
        _CASES[key] = (st, s_dev, lv, A, S)
    return _CASES[key]


def to_np(t):
    return t.cpu().numpy()


# ---- 1. the scale -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", bc.SRCS)
@pytest.mark.parametrize("shape", SHAPES)
def test_scale_is_the_float64_mean_and_the_same_bits_every_time(tm, shape, src):
    import torch
    from tmac_amd import wrapper
    Mw, K, bm, mg = shape
    st, s_dev, _, _, _ = case(tm, shape, src)
    want = np.abs(bc.as_f32(st).astype(np.float64)).reshape(mg, -1).mean(axis=1).astype(np.float32)
    print("scale", shape, src, s_dev, want)
    assert s_dev.dtype == np.float32 and s_dev.shape == (mg,)
    assert np.all(np.abs(s_dev.astype(np.float64) - want.astype(np.float64)) <= np.spacing(want)), (s_dev, want)
    w = dev(st)
    torch.cuda.synchronize()
    again = to_np(wrapper.absmean(w, mg))
    side = torch.cuda.Stream()
    other = to_np(wrapper.absmean(w, mg, stream=side))
    a = torch.randn(256, 256, device="cuda")
    (a @ a).sum().item()                                   # other work in between
    after = to_np(wrapper.absmean(w, mg))
    for got in (again, other, after):
        assert np.array_equal(pc.raw_bits(got), pc.raw_bits(s_dev))


def test_scale_floor_is_eps(tm):
    from tmac_amd import wrapper
    tiny = np.full((128, 256), 2e-7, np.float32)
    assert np.array_equal(to_np(wrapper.absmean(tiny)), np.array([1e-5], np.float32))
    assert np.array_equal(to_np(wrapper.absmean(tiny, eps=1e-3)), np.array([1e-3], np.float32))


# ---- 2. the blob --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", bc.SRCS)
@pytest.mark.parametrize("shape", SHAPES)
def test_pack_bitnet_is_the_host_blob_under_the_device_scale(tm, shape, src):
    from tmac_amd import wrapper
    Mw, K, bm, mg = shape
    st, s_dev, lv, A, S = case(tm, shape, src)
    assert set(np.unique(lv)) == {1, 2, 3}
    gA, gS = wrapper.pack_bitnet(dev(st), kcfg(tm, Mw, K, bm, mg), mg)
    assert np.array_equal(pc.raw_bits(to_np(gS)), pc.raw_bits(s_dev)), "the blob stores the scale the reduction gives"
    assert np.array_equal(to_np(gA), A.reshape(-1))
    assert np.array_equal(pc.raw_bits(to_np(gS)), pc.raw_bits(S))
    # the scales handed in: the same blob, no reduction
    hA, hS = wrapper.pack_bitnet(dev(st), kcfg(tm, Mw, K, bm, mg), mg, scale=s_dev)
    assert np.array_equal(to_np(hA), A.reshape(-1)) and np.array_equal(pc.raw_bits(to_np(hS)), pc.raw_bits(S))


@pytest.mark.parametrize("src", bc.SRCS)
def test_tie_table_meets_the_device_code(tm, src):
    from tmac_amd import wrapper
    Mw, K, bm, mg = SHAPES[0]
    st, lv = bc.tie_matrix(src, Mw, K)
    A, S = pc.host_blob_codes(lv, np.ones(1, np.float32), None, 2, bm, KF)          # the table's own levels
    A2, _, lv2 = bc.host_blob(st, bm, KF, scale=1.0)                                 # ... which are the host reference's
    assert np.array_equal(lv2, lv) and np.array_equal(A2, A)
    gA, gS = wrapper.pack_bitnet(dev(st), kcfg(tm, Mw, K, bm, mg), scale=1.0)
    assert np.array_equal(to_np(gA), A.reshape(-1)) and np.array_equal(pc.raw_bits(to_np(gS)), pc.raw_bits(S))


def test_blob_scales_in_fp16(tm):
    """host_float = TMAC_F16 rounds the STORED scale; the levels still come from the fp32 one"""
    from tmac_amd import wrapper
    shape = SHAPES[4]
    Mw, K, bm, mg = shape
    st, s_dev, lv, A, S = case(tm, shape, "f16")
    gA, gS = wrapper.pack_bitnet(dev(st), kcfg(tm, Mw, K, bm, mg), mg, ref_dtype=tm.F16)
    assert np.array_equal(to_np(gA), A.reshape(-1)) and np.array_equal(pc.raw_bits(to_np(gS)), pc.raw_bits(S.astype(np.float16)))


# ---- 3. the handle ------------------------------------------------------------------------------------------------------------------
def acts(seed, N, K, dtype):
    import torch
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((N, K)).astype(np.float32)).cuda().to(dtype)


def run(wr, ws, x, N, out_dtype=None):
    import torch
    outs = [torch.full((N, w.Mw), 7.0, dtype=out_dtype or torch.float32, device="cuda") for w in ws]
    wr.fused(ws, x, outs, N)
    torch.cuda.synchronize()
    return outs


def pair(tm, shape, src):
    """(handle from the masters, the plain twin from the host reference's levels under the device's scale)"""
    Mw, K, bm, mg = shape
    st, s_dev, lv, A, S = case(tm, shape, src)
    cfg = kcfg(tm, Mw, K, bm, mg)
    return tm.Weights.from_bitnet(dev(st), cfg, mg), tm.Weights.from_codes(lv, s_dev, None, 2, cfg, tm.F32)


def oracle_out(shape, A, S, x):
    Mw, K, bm, mg = shape
    q, ls, lb = orc.preprocessor(np.ascontiguousarray(x, np.float32), K)
    return orc.qgemm_scale_final(A, q, S, ls[:, 0], lb[:, 0], Mw, K, x.shape[0], 2, bm, KF, mg)[0]


@pytest.mark.parametrize("src", bc.SRCS)
@pytest.mark.parametrize("shape", SHAPES)
def test_handle_is_the_plain_twin_bit_for_bit(tm, shape, src):
    import torch
    Mw, K, bm, mg = shape
    _, _, _, A, S = case(tm, shape, src)
    wb, wt = pair(tm, shape, src)
    assert wb.algorithmic_bytes() == wt.algorithmic_bytes()
    wr = tm.TMACGeMMWrapper(act_group_size=K)
    L = tm.lib()
    for dt in (torch.float32, torch.float16):
        x = acts(K + Mw, 1, K, dt)
        ref = oracle_out(shape, A, S, to_np(x.float()))
        for ft, wpq in [(0, 0)] + QUAD_CONFIGS:
            tm.binding.check(L.tmac_hip_debug_quad_config(ft, wpq))
            (cb,), (ct,) = run(wr, [wb], x, 1), run(wr, [wt], x, 1)
            assert torch.equal(cb, ct), (dt, ft, wpq, float((cb - ct).abs().max()))
            assert np.array_equal(pc.raw_bits(to_np(ct)), pc.raw_bits(ref)), (dt, ft, wpq, float(np.abs(to_np(ct) - ref).max()))
        tm.binding.check(L.tmac_hip_debug_quad_config(0, 0))
    for N in (5, 70):
        tm.binding.check(L.tmac_hip_reset_state())
        tm.binding.check(L.tmac_hip_set_gemm_min_n(12))
        x = acts(N + K, N, K, torch.float32)
        (cb,), (ct,) = run(wr, [wb], x, N), run(wr, [wt], x, N)
        assert torch.equal(cb, ct), (N, float((cb - ct).abs().max()))
        ref = oracle_out(shape, A, S, to_np(x))
        assert np.array_equal(pc.raw_bits(to_np(ct)), pc.raw_bits(ref)), (N, float(np.abs(to_np(ct) - ref).max()))
    wb.free(); wt.free()


def test_one_stream_mode_recording_of_three_handles(tm):
    import torch
    shapes = [(SHAPES[0], "f16"), (SHAPES[4], "bf16"), (SHAPES[1], "f32")]
    pairs = [pair(tm, s, src) for s, src in shapes]
    xs = [acts(40 + i, 1, s[1], torch.float16)[0].contiguous() for i, (s, _) in enumerate(shapes)]
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    outs = {}
    for which in (0, 1):
        o = [torch.full((s[0],), 7.0, dtype=torch.float16, device="cuda") for s, _ in shapes]
        with wr.record_chain() as rec:
            for p, x, oo in zip(pairs, xs, o):
                wr.fused([p[which]], x, [oo], 1)
        assert rec.chain.stream and rec.chain.nops == 3
        rec.chain.launch(); torch.cuda.synchronize()
        assert rec.chain.status() == 0
        rec.chain.free()
        outs[which] = o
    for i, (a, b) in enumerate(zip(outs[0], outs[1])):
        assert torch.equal(a, b), (i, float((a.float() - b.float()).abs().max()))
        (s, src) = shapes[i]
        ref = oracle_out(s, case(tm, s, src)[3], case(tm, s, src)[4], to_np(xs[i].float())[None, :])[0]
        assert np.abs(to_np(b.float()) - ref).max() <= 1e-3 * np.abs(ref).max()       # fp16 outputs: the project's bar for them
    for p in pairs:
        p[0].free(); p[1].free()


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------
def raw_absmean(tm, W, src, Mw, K, mg, eps, out):
    rc = tm.lib().tmac_hip_absmean_dev(W, src, Mw, K, mg, eps, out, None)
    return rc, tm.lib().tmac_hip_last_error().decode()


def raw_pack(tm, W, src, sin, eps, Mw, K, cfg, A, S, ref=0):
    rc = tm.lib().tmac_hip_pack_absmean_dev(W, src, sin, eps, Mw, K, C.byref(cfg), A, S, ref, None)
    return rc, tm.lib().tmac_hip_last_error().decode()


def raw_register(tm, h, W, src, sin, eps, Mw, K, cfg):
    rc = tm.lib().tmac_hip_register_weights_absmean_dev(C.byref(h), W, src, sin, eps, Mw, K, C.byref(cfg), 0, 0, None)
    return rc, tm.lib().tmac_hip_last_error().decode()


def test_refusals(tm):
    import torch
    from tmac_amd import wrapper
    Mw, K, bm, mg = SHAPES[0]
    st = bc.masters(77, Mw, K, "f16")
    cfg = kcfg(tm, Mw, K, bm, 1)
    ab, sb = wrapper.ref_blob_bytes(Mw, K, 2, cfg, tm.F32)
    # spare bytes behind each so that "+ 8" stays inside the allocation
    bufA = torch.full((ab + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    bufS = torch.full((sb + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    bufO = torch.full((64,), 0xFF, dtype=torch.uint8, device="cuda")                 # scales_out_dev of the reduction
    w = torch.from_numpy(st).cuda()
    w8 = torch.zeros(Mw * K + 32, dtype=torch.float16, device="cuda")                # a copy of the matrix 8 bytes into its allocation
    w8[4:4 + Mw * K] = w.reshape(-1)
    sin = torch.ones(8, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    pW, pA, pS, pO, pI = w.data_ptr(), bufA.data_ptr(), bufS.data_ptr(), bufO.data_ptr(), sin.data_ptr()
    SRC = bc.SRC_CODE["f16"]

    def untouched():
        torch.cuda.synchronize()
        return bool((bufA == 0xFF).all()) and bool((bufS == 0xFF).all()) and bool((bufO == 0xFF).all())

    def pack(code, names, W=pW, src=SRC, s_in=None, eps=1e-5, c=cfg, A=pA, S=pS, M=Mw):
        rc, msg = raw_pack(tm, W, src, s_in, eps, M, K, c, A, S)
        assert rc == code and all(n in msg for n in names) and untouched(), (rc, msg, names)
        if A == pA and S == pS:                                                       # the register form shares the checks of the inputs
            h = C.c_void_p()
            rc, msg = raw_register(tm, h, W, src, s_in, eps, M, K, c)
            assert rc == code and all(n in msg for n in names) and not h and untouched(), (rc, msg, names)

    def mean(code, names, W=pW, src=SRC, eps=1e-5, m=1, out=pO, M=Mw):
        rc, msg = raw_absmean(tm, W, src, M, K, m, eps, out)
        assert rc == code and all(n in msg for n in names) and untouched(), (rc, msg, names)

    pack(E_ARG, ["W_dev"], W=None)
    pack(E_ARG, ["A_ref_out"], A=None)
    pack(E_ARG, ["scales_ref_out"], S=None)
    pack(E_ARG, ["W_dev", "aligned"], W=w8.data_ptr() + 8)
    pack(E_ARG, ["scales_in_dev", "aligned"], s_in=pI + 4)
    pack(E_ARG, ["A_ref_out", "aligned"], A=pA + 8)
    pack(E_ARG, ["scales_ref_out", "aligned"], S=pS + 4)
    pack(E_ARG, ["src_dtype"], src=3)
    pack(E_ARG, ["src_dtype"], src=-1)
    for bad in (0.0, -1e-5, float("inf"), float("nan")):
        pack(E_ARG, ["eps"], eps=bad)
        mean(E_ARG, ["eps"], eps=bad)
    pack(E_ARG, ["m_groups", "per-group scales: register codes or GPTQ tensors"], c=tm.KCfg.make(Mw, K, 2, bm, KF, 128, 64, False, -1))
    pack(E_ARG, ["m_groups", "Mw"], c=kcfg(tm, Mw, K, bm, 3))
    # a shape refusal is make_shape's own: the code and the message registration gives for the same arguments
    bad = kcfg(tm, Mw, K, 96, 1)
    h = C.c_void_p()
    rc0 = tm.lib().tmac_hip_register_weights_dev(C.byref(h), pA, pS, Mw, K, 2, C.byref(bad), tm.F32, tm.F32, None)
    msg0 = tm.lib().tmac_hip_last_error().decode()
    assert rc0 == E_NOMATCH and not h
    pack(E_NOMATCH, [msg0], c=bad)
    rc = tm.lib().tmac_hip_register_weights_absmean_dev(None, pW, SRC, None, 1e-5, Mw, K, C.byref(cfg), 0, 0, None)
    assert rc == E_ARG and "out" in tm.lib().tmac_hip_last_error().decode()

    mean(E_ARG, ["W_dev"], W=None)
    mean(E_ARG, ["scales_out_dev"], out=None)
    mean(E_ARG, ["W_dev", "aligned"], W=w8.data_ptr() + 8)
    mean(E_ARG, ["scales_out_dev", "aligned"], out=pO + 4)
    mean(E_ARG, ["src_dtype"], src=3)
    mean(E_ARG, ["m_groups", "per-group scales: register codes or GPTQ tensors"], m=0)
    mean(E_ARG, ["m_groups", "Mw"], m=3)

    # and good calls on the same buffers write them
    rc, msg = raw_absmean(tm, pW, SRC, Mw, K, 1, 1e-5, pO)
    assert rc == 0, msg
    rc, msg = raw_pack(tm, pW, SRC, None, 1e-5, Mw, K, cfg, pA, pS)
    assert rc == 0, msg
    torch.cuda.synchronize()
    A, S, _ = bc.host_blob(st, bm, KF, scale=to_np(bufO[:4].view(torch.float32)))
    assert np.array_equal(to_np(bufA[:ab]), A.reshape(-1)) and np.array_equal(to_np(bufS[:4]), to_np(bufO[:4]))
    assert bool((bufA[ab:] == 0xFF).all()) and bool((bufS[sb:] == 0xFF).all()) and bool((bufO[4:] == 0xFF).all())


# ---- 5. ordering --------------------------------------------------------------------------------------------------------------------
def defer_stats(tm):
    st = [C.c_uint64(0) for _ in range(4)]
    tm.binding.check(tm.lib().tmac_hip_defer_stats(*[C.byref(x) for x in st]))
    return tuple(int(x.value) for x in st)          # flushes, cache hits, stream launches, single calls


def test_each_entry_point_flushes_the_deferred_queue_first(tm):
    import torch
    from tmac_amd import wrapper
    shape = SHAPES[0]
    Mw, K, bm, mg = shape
    st, s_dev, lv, A, S = case(tm, shape, "bf16")
    cfg = kcfg(tm, Mw, K, bm, mg)
    wr = tm.TMACGeMMWrapper(act_group_size=K)
    w = wr.register_bitnet(st, cfg)
    x = acts(3, 1, K, torch.float32)
    (want,) = run(wr, [w], x, 1)
    wd = dev(st)
    out = torch.zeros((1, Mw), dtype=torch.float32, device="cuda")
    tm.binding.check(tm.lib().tmac_hip_defer(1))
    results = []
    for entry in ("absmean", "pack", "register"):
        out.zero_()
        wr.fused([w], x, [out], 1)                              # queued
        before = defer_stats(tm)
        # a refused call leaves the queue alone
        rc, _ = raw_pack(tm, wd.data_ptr(), 3, None, 1e-5, Mw, K, cfg, None, None)
        assert rc == E_ARG and defer_stats(tm)[0] == before[0]
        rc, _ = raw_absmean(tm, wd.data_ptr(), 2, Mw, K, 0, 1e-5, None)
        assert rc == E_ARG and defer_stats(tm)[0] == before[0]
        if entry == "absmean":
            results.append(wrapper.absmean(wd))
        elif entry == "pack":
            results.append(wrapper.pack_bitnet(wd, cfg))
        else:
            results.append(tm.Weights.from_bitnet(wd, cfg))
        after = defer_stats(tm)
        assert after[0] == before[0] + 1, (entry, before, after)                # the flush happened AT the call
        tm.binding.check(tm.lib().tmac_hip_flush(None))
        assert defer_stats(tm)[0] == after[0], "nothing was left to flush"
        torch.cuda.synchronize()
        assert torch.equal(out, want), entry
    tm.binding.check(tm.lib().tmac_hip_defer(0))
    assert np.array_equal(pc.raw_bits(to_np(results[0])), pc.raw_bits(s_dev))
    assert np.array_equal(to_np(results[1][0]), A.reshape(-1))
    (got,) = run(wr, [results[2]], x, 1)
    assert torch.equal(got, want)
    w.free(); results[2].free()


def test_a_failed_flush_returns_its_status_and_launches_nothing(tm):
    """no flush fails on a healthy GPU: tmac_hip_debug_defer_fail(1) makes the next flush's launch attempt return TMAC_HIP_E_RUNTIME on the
    host side, before anything reaches the device (tests/test_gpu_defer.py)"""
    import torch
    from tmac_amd import wrapper
    E_RUNTIME = -3
    Mw, K, bm, mg = SHAPES[0]
    st = case(tm, SHAPES[0], "f32")[0]
    cfg = kcfg(tm, Mw, K, bm, mg)
    wr = tm.TMACGeMMWrapper(act_group_size=K)
    w = wr.register_bitnet(st, cfg)
    wd, x = dev(st), acts(4, 1, K, torch.float32)
    ab, sb = wrapper.ref_blob_bytes(Mw, K, 2, cfg, tm.F32)
    bufA = torch.full((ab,), 0xFF, dtype=torch.uint8, device="cuda")
    bufS = torch.full((16,), 0xFF, dtype=torch.uint8, device="cuda")
    out = torch.zeros((1, Mw), dtype=torch.float32, device="cuda")
    L = tm.lib()
    tm.binding.check(L.tmac_hip_defer(1))
    try:
        for entry in ("absmean", "pack", "register"):
            wr.fused([w], x, [out], 1)                          # queued
            tm.binding.check(L.tmac_hip_debug_defer_fail(1))
            h = C.c_void_p()
            if entry == "absmean":
                rc, _ = raw_absmean(tm, wd.data_ptr(), 0, Mw, K, 1, 1e-5, bufS.data_ptr())
            elif entry == "pack":
                rc, _ = raw_pack(tm, wd.data_ptr(), 0, None, 1e-5, Mw, K, cfg, bufA.data_ptr(), bufS.data_ptr())
            else:
                rc, _ = raw_register(tm, h, wd.data_ptr(), 0, None, 1e-5, Mw, K, cfg)
            assert rc == E_RUNTIME and not h, (entry, rc)
            tm.binding.check(L.tmac_hip_flush(None))            # the queue is empty after the failed flush
            torch.cuda.synchronize()
            assert bool((bufA == 0xFF).all()) and bool((bufS == 0xFF).all()), entry
    finally:
        L.tmac_hip_defer(0)
    w.free()


# ---- 6. footprint -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", bc.SRCS)
@pytest.mark.parametrize("shape", (SHAPES[1], SHAPES[0]))
def test_footprint(tm, shape, src):
    """Guard bands around W_dev, a given scales_in_dev, scales_out_dev, A_ref_out and scales_ref_out, at both placements, with both finite
    guard patterns and with 0xFF guards -- NaN in every source dtype: a master or a scale read from outside its buffer would poison the
    sum or a level."""
    from tmac_amd import wrapper
    Mw, K, bm, mg = shape
    st, s_dev, lv, A, S = case(tm, shape, src)
    cfg = kcfg(tm, Mw, K, bm, mg)
    ab, sb = wrapper.ref_blob_bytes(Mw, K, 2, cfg, tm.F32)
    assert ab == A.size and sb == 4 * mg
    code = bc.SRC_CODE[src]
    stored = st.view(np.int16) if src == "bf16" else st

    def call(alloc):
        tw, ti = alloc.inp(stored, name="W"), alloc.inp(s_dev, name="scales_in")
        o0 = alloc.out(mg, np.float32, "scales_out", tile=False)
        oA, oS = alloc.out(ab, np.uint8, "A_ref", tile=False), alloc.out(mg, np.float32, "scales_ref", tile=False)
        oA2, oS2 = alloc.out(ab, np.uint8, "A_ref_given", tile=False), alloc.out(mg, np.float32, "scales_ref_given", tile=False)
        alloc.arm()
        rc, msg = raw_absmean(tm, tw.data_ptr(), code, Mw, K, mg, 1e-5, o0.data_ptr())
        assert rc == 0, msg
        rc, msg = raw_pack(tm, tw.data_ptr(), code, None, 1e-5, Mw, K, cfg, oA.data_ptr(), oS.data_ptr())
        assert rc == 0, msg
        rc, msg = raw_pack(tm, tw.data_ptr(), code, ti.data_ptr(), 1e-5, Mw, K, cfg, oA2.data_ptr(), oS2.data_ptr())
        assert rc == 0, msg

    def check_want(want):
        for n in ("scales_out", "scales_ref", "scales_ref_given"):
            assert np.array_equal(pc.raw_bits(want[n]), pc.raw_bits(s_dev)), n
        assert np.array_equal(want["A_ref"], A.reshape(-1)) and np.array_equal(want["A_ref_given"], A.reshape(-1))

    fp.check_footprint(call, check_want=check_want, patterns=fp.PATTERNS + (0xFF,))


# ---- 7. the loader ------------------------------------------------------------------------------------------------------------------
def test_load_bitnet_dir(tm, tmp_path):
    import torch
    from tmac_amd import checkpoint, wrapper
    tensors, _ = bc.write_bitnet_checkpoint(str(tmp_path))
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    loaded = checkpoint.load_bitnet_dir(str(tmp_path), wr)
    assert list(loaded) == [bc.CKPT_LAYERS[i][0] for i in (0, 2, 1)]
    for name, seed, Mw, K, src in bc.CKPT_LAYERS:
        st = tensors[name + ".weight"]
        assert (loaded[name].Mw, loaded[name].K, loaded[name].bits) == (Mw, K, 2)
        direct = tm.Weights.from_bitnet(dev(st))
        x = acts(seed, 1, K, torch.float32)
        (a,), (b,) = run(wr, [loaded[name]], x, 1), run(wr, [direct], x, 1)
        assert torch.equal(a, b), name
        # ... and it is the host reference's matrix
        s_dev = to_np(wrapper.absmean(dev(st)))
        bm = tm.convert.default_bm(2, Mw)
        A, S, _ = bc.host_blob(st, bm, KF, scale=s_dev)
        ref = oracle_out((Mw, K, bm, 1), A, S, to_np(x))
        assert np.array_equal(pc.raw_bits(to_np(a)), pc.raw_bits(ref)), name
        if src == "bf16":       # the 16-bit words went up as they lie: the levels are those of the fp32 upcast
            gA, gS = wrapper.pack_bitnet(st)
            uA, uS = wrapper.pack_bitnet(bc.as_f32(st))
            assert torch.equal(gA, uA) and torch.equal(gS, uS)
        loaded[name].free(); direct.free()
