"""Dense fp32 / fp16 / bf16 matrices to W1 - W4 handles with per-group scales on the GPU: tmac_hip_rtn_params_dev, tmac_hip_pack_rtn_dev,
tmac_hip_register_weights_rtn_dev (k_rtn_params, k_pack_rtn_weights in tmac_pack.hip) and what sits on top (wrapper.rtn_params / pack_rtn,
Weights.from_dense, checkpoint.load_dense_dir).

The reference tree holds no quantiser, so the yardstick is convert.rtn_quant, GPTQ's round-to-nearest rule in numpy
(tests/test_rtn_quant_cpu.py ties it to a float64 restatement and a table of ties).  Minimum and maximum are exact and every later step is
one correctly rounded fp32 operation on both sides, so nothing here has a tolerance of its own:
1. the parameters: scales and zero codes array_equal to convert.rtn_params on the same masters;
2. the blob: byte for byte weights.preprocess_weights of the host reference's codes, scales and zeros; the tie table and the edge groups;
3. the handle: bit for bit (torch.equal) the plain twin from_codes(codes, scales, zeros) on every route the fused entry point plans --
   N = 1 under the heuristic and a forced configuration, N = 3, N = 70, a declared-independent stream recording -- and the twin within
   1e-3 of the oracle (the bar of test_gpu_pack.py) with its integer tap bit for bit;
4. invalid inputs and refusals, 5. ordering behind the deferred queue, 6. footprint, 7. the checkpoint loader.
Shapes (Mw, K, gs): (128, 256, 128) two row tiles of one table tile; (192, 384, 64) three row tiles, 1.5 table tiles, a group smaller than
an activation group's pair; (320, 1024, 128) five row tiles, four table tiles, a last M-tile; (192, 704, 64) a ragged K: 176 tables = 2.75
tiles.  make_shape accepts all of them for every width.
"""
import ctypes as C

import numpy as np
import pytest

import footprint as fp
import pack_common as pc
import rtn_common as rc
from oracle import oracle as orc
from tmac_amd import convert

pytestmark = pytest.mark.gpu
E_NOMATCH, E_ARG = -1, -4
KF, AGS = 16, 64
SHAPES = [(128, 256, 128), (192, 384, 64), (320, 1024, 128), (192, 704, 64)]
BITS = (1, 2, 3, 4)


@pytest.fixture(scope="module")
def tm():
    import torch
    import tmac_amd
    assert torch.cuda.is_available()
    return tmac_amd


def bm_of(bits, Mw):
    """convert.default_bm, and 192 for the one pair it has no M-tile for: 192 rows of 1 bit (the kernels do not care: the value only fixes
    the blob layout)"""
    return 192 if (bits, Mw) == (1, 192) else convert.default_bm(bits, Mw)


def kcfg(tm, Mw, K, bits, gs, zp):
    return tm.KCfg.make(Mw, K, bits, bm_of(bits, Mw), KF, gs, AGS, zp)


def dev(st):
    """the storage form on the GPU as torch sees it (bf16 bit patterns -> a bfloat16 tensor)"""
    import torch
    if st.dtype == np.uint16:
        return torch.from_numpy(st.view(np.int16)).cuda().view(torch.bfloat16)
    return torch.from_numpy(st).cuda()


def to_np(t):
    return t.cpu().numpy()


_MASTERS, _HOST = {}, {}


def masters(shape, src):
    if (shape, src) not in _MASTERS:
        Mw, K, gs = shape
        _MASTERS[(shape, src)] = rc.masters(2000 + Mw + K + gs, Mw, K, src)
    return _MASTERS[(shape, src)]


def host(shape, src, bits, zp, f16):
    """(A, S fp32, codes, scales, zeros) of the host route: made once, shared, never changed"""
    key = (shape, src, bits, zp, f16)
    if key not in _HOST:
        Mw, K, gs = shape
        _HOST[key] = rc.host_blob(masters(shape, src), bits, gs, zp, f16, bm_of(bits, Mw), KF)
    return _HOST[key]


# ---- 1. the parameters, 2. the blob ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("shape", SHAPES)
def test_parameters_and_blob_are_the_host_route(tm, shape, bits):
    from tmac_amd import wrapper
    Mw, K, gs = shape
    for src in rc.SRCS:
        st = masters(shape, src)
        w = dev(st)
        for zp in (True, False):
            cfg = kcfg(tm, Mw, K, bits, gs, zp)
            for f16 in (False, True):
                A, S, codes, sc, zr = host(shape, src, bits, zp, f16)
                _, zq, bad = convert.rtn_params(st, bits, gs, zp, f16)
                assert not bad.any()
                gsc, gzq, n = wrapper.rtn_params(w, bits, gs, zp, f16, count_invalid=True)
                assert np.array_equal(pc.raw_bits(to_np(gsc)), pc.raw_bits(sc)), (src, zp, f16, "scales")
                assert np.array_equal(to_np(gzq), zq) and int(n.item()) == 0, (src, zp, f16, "zero codes")
                gA, gS, n = wrapper.pack_rtn(w, bits, gs, zp, cfg, tm.F16 if f16 else tm.F32, count_invalid=True)
                assert int(n.item()) == 0
                assert np.array_equal(to_np(gA), A.reshape(-1)), (src, zp, f16, "weight bytes")
                with np.errstate(over="ignore"):
                    want = S.astype(np.float16) if f16 else S
                assert np.array_equal(pc.raw_bits(to_np(gS)), pc.raw_bits(want)), (src, zp, f16, "scales half")


def test_the_same_bits_on_every_launch_and_stream(tm):
    import torch
    from tmac_amd import wrapper
    shape = SHAPES[3]
    Mw, K, gs = shape
    w = dev(masters(shape, "bf16"))
    first = [to_np(t) for t in wrapper.pack_rtn(w, 3, gs, True)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    other = [to_np(t) for t in wrapper.pack_rtn(w, 3, gs, True, stream=side)]
    for a, b in zip(first, other):
        assert np.array_equal(pc.raw_bits(a), pc.raw_bits(b))


@pytest.mark.parametrize("zp", (True, False))
@pytest.mark.parametrize("bits", BITS)
def test_tie_table_meets_the_device_code(tm, bits, zp):
    from tmac_amd import wrapper
    Mw, K, gs = 128, 256, 64
    wt, sc, zq, cd = rc.tie_matrix(bits, zp, Mw, K, gs)
    bm = bm_of(bits, Mw)
    zr = ((zq - np.float32(2 ** (bits - 1))) * sc).astype(np.float32) if zp else None
    A, S = pc.host_blob_codes(cd, sc, zr, bits, bm, KF)                       # the table's own codes
    for src in rc.SRCS:
        w = dev(rc.storage(wt, src))
        gsc, gzq = wrapper.rtn_params(w, bits, gs, zp)
        assert np.array_equal(to_np(gsc), sc) and np.array_equal(to_np(gzq), zq), src
        gA, gS = wrapper.pack_rtn(w, bits, gs, zp, kcfg(tm, Mw, K, bits, gs, zp))
        assert np.array_equal(to_np(gA), A.reshape(-1)) and np.array_equal(pc.raw_bits(to_np(gS)), pc.raw_bits(S)), src


@pytest.mark.parametrize("src", rc.SRCS)
def test_edge_groups_through_the_device(tm, src):
    """all zero, all positive, all negative, one value, -0.0, fp16 subnormals, a subnormal fp32 scale, the largest finite values: the
    parameters, the blob and the count of invalid groups are the host rule's, invalid groups included"""
    from tmac_amd import wrapper
    Mw, K, gs = 128, 256, 64
    st = rc.edge_matrix(src, Mw, K, gs)
    w = dev(st)
    seen = 0
    for bits in BITS:
        for zp in (True, False):
            cfg = kcfg(tm, Mw, K, bits, gs, zp)
            for f16 in (False, True):
                sc, zq, bad = convert.rtn_params(st, bits, gs, zp, f16)
                gsc, gzq, n = wrapper.rtn_params(w, bits, gs, zp, f16, count_invalid=True)
                assert np.array_equal(pc.raw_bits(to_np(gsc)), pc.raw_bits(sc)) and np.array_equal(to_np(gzq), zq), (bits, zp, f16)
                assert int(n.item()) == int(bad.sum()), (bits, zp, f16)
                seen += int(bad.sum())
                A, S, _, _, _ = rc.host_blob(st, bits, gs, zp, f16, bm_of(bits, Mw), KF)
                gA, gS, n = wrapper.pack_rtn(w, bits, gs, zp, cfg, tm.F16 if f16 else tm.F32, count_invalid=True)
                assert int(n.item()) == int(bad.sum())
                with np.errstate(over="ignore"):
                    want = S.astype(np.float16) if f16 else S
                assert np.array_equal(to_np(gA), A.reshape(-1)) and np.array_equal(pc.raw_bits(to_np(gS)), pc.raw_bits(want)), (bits, zp, f16)
    assert seen > 0


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


def pair(tm, shape, src, bits, zp, dev_dtype):
    """(handle from the masters, the plain twin from the host reference's codes, scales and zeros)"""
    Mw, K, gs = shape
    f16 = dev_dtype == tm.F16
    _, _, codes, sc, zr = host(shape, src, bits, zp, f16)
    cfg = kcfg(tm, Mw, K, bits, gs, zp)
    return (tm.Weights.from_dense(dev(masters(shape, src)), bits, gs, zp, cfg, dev_dtype, AGS),
            tm.Weights.from_codes(codes, sc, zr, bits, cfg, dev_dtype, AGS))


def oracle_out(shape, bits, zp, A, S, x):
    Mw, K, gs = shape
    q, ls, lb = orc.preprocessor(np.ascontiguousarray(x, np.float32), AGS)
    return orc.qgemm_float(A, q, S, ls, lb, Mw, K, x.shape[0], bits, bm_of(bits, Mw), KF, gs, AGS, zp)


def stored(S, f16):
    """the scales half as the handle keeps it: fp16 device scales round the zeros (the scales are fp16 values already)"""
    return S.astype(np.float16).astype(np.float32) if f16 else S


@pytest.mark.parametrize("zp", (True, False))
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("shape", SHAPES)
def test_handle_is_the_plain_twin_bit_for_bit(tm, shape, bits, zp):
    import torch
    Mw, K, gs = shape
    wr = tm.TMACGeMMWrapper(act_group_size=AGS)
    L = tm.lib()
    for src in rc.SRCS:
        for dd in (tm.F32, tm.F16):
            wd, wt = pair(tm, shape, src, bits, zp, dd)
            assert wd.algorithmic_bytes() == wt.algorithmic_bytes()
            # the twin against the oracle: once per device dtype.  (1 bit without zero points: every code is the zero code -- the rule's,
            # tests/test_rtn_quant_cpu.py -- so the matrix is 0 and a bar relative to the largest output says nothing.)
            check_oracle = src == "f16" and (zp or bits > 1)
            A, S = host(shape, src, bits, zp, dd == tm.F16)[:2]
            x = acts(K + Mw, 1, K, torch.float16)
            for ft, wpq in ((0, 0), (512, 2)):             # the heuristic, a forced configuration
                tm.binding.check(L.tmac_hip_debug_quad_config(ft, wpq))
                (cd,), (ct,) = run(wr, [wd], x, 1), run(wr, [wt], x, 1)
                assert torch.equal(cd, ct), (src, dd, ft, wpq, float((cd - ct).abs().max()))
            tm.binding.check(L.tmac_hip_debug_quad_config(0, 0))
            if check_oracle:
                ref = oracle_out(shape, bits, zp, A, stored(S, dd == tm.F16), to_np(x.float()))
                assert np.abs(to_np(ct) - ref).max() <= 1e-3 * np.abs(ref).max(), (dd, float(np.abs(to_np(ct) - ref).max()))
                psd, _ = wr.fused_partial_sums(wd, x, 1)
                pst, _ = wr.fused_partial_sums(wt, x, 1)
                q, _, _ = orc.preprocessor(to_np(x.float()), AGS)
                want = orc.partial_sums(A, q[0], Mw, K, bits, bm_of(bits, Mw), KF, AGS)
                assert np.array_equal(psd, pst) and np.array_equal(pst[0], want), "integer tap"
            for N in (3, 70):
                xn = acts(N + K, N, K, torch.float32)
                (cd,), (ct,) = run(wr, [wd], xn, N), run(wr, [wt], xn, N)
                assert torch.equal(cd, ct), (src, dd, N, float((cd - ct).abs().max()))
                if check_oracle:
                    ref = oracle_out(shape, bits, zp, A, stored(S, dd == tm.F16), to_np(xn))
                    assert np.abs(to_np(ct) - ref).max() <= 1e-3 * np.abs(ref).max(), (dd, N)
            wd.free(); wt.free()


def test_one_declared_independent_recording_of_three_handles(tm):
    import torch
    # (the matrices of one recording share bits, zero points and scale dtype: the chain's own rule)
    cases = [(SHAPES[0], "f16", 2, True), (SHAPES[2], "bf16", 2, True), (SHAPES[1], "f32", 2, True)]
    pairs = [pair(tm, s, src, bits, zp, tm.F16) for s, src, bits, zp in cases]
    xs = [acts(40 + i, 1, c[0][1], torch.float16)[0].contiguous() for i, c in enumerate(cases)]
    wr = tm.TMACGeMMWrapper(act_group_size=AGS)
    outs = {}
    for which in (0, 1):
        o = [torch.full((c[0][0],), 7.0, dtype=torch.float16, device="cuda") for c in cases]
        with wr.record_chain(independent=True) as rec:
            for p, x, oo in zip(pairs, xs, o):
                wr.fused([p[which]], x, [oo], 1)
        assert rec.chain.stream and rec.chain.nops == 3
        rec.chain.launch(); torch.cuda.synchronize()
        assert rec.chain.status() == 0
        rec.chain.free()
        outs[which] = o
    for i, (a, b) in enumerate(zip(outs[0], outs[1])):
        assert torch.equal(a, b), (i, float((a.float() - b.float()).abs().max()))
        s, src, bits, zp = cases[i]
        A, S = host(s, src, bits, zp, True)[:2]
        ref = oracle_out(s, bits, zp, A, stored(S, True), to_np(xs[i].float())[None, :])[0]
        assert np.abs(to_np(b.float()) - ref).max() <= 1e-3 * np.abs(ref).max()       # fp16 outputs: the project's bar for them
    for p in pairs:
        p[0].free(); p[1].free()


# ---- 4. invalid inputs and refusals ---------------------------------------------------------------------------------------------------
def raw_params(tm, W, src, Mw, K, bits, gs, zp, f16, sc, zq, n=None):
    rc_ = tm.lib().tmac_hip_rtn_params_dev(W, src, Mw, K, bits, gs, zp, f16, sc, zq, n, None)
    return rc_, tm.lib().tmac_hip_last_error().decode()


def raw_pack(tm, W, src, Mw, K, bits, cfg, A, S, ref=0, n=None):
    rc_ = tm.lib().tmac_hip_pack_rtn_dev(W, src, Mw, K, bits, C.byref(cfg), A, S, ref, n, None)
    return rc_, tm.lib().tmac_hip_last_error().decode()


def raw_register(tm, h, W, src, Mw, K, bits, cfg, host_float=0, dev_float=0):
    rc_ = tm.lib().tmac_hip_register_weights_rtn_dev(C.byref(h), W, src, Mw, K, bits, C.byref(cfg), host_float, dev_float, None)
    return rc_, tm.lib().tmac_hip_last_error().decode()


def defer_stats(tm):
    st = [C.c_uint64(0) for _ in range(4)]
    tm.binding.check(tm.lib().tmac_hip_defer_stats(*[C.byref(x) for x in st]))
    return tuple(int(x.value) for x in st)          # flushes, cache hits, stream launches, single calls


def test_invalid_masters_are_counted_and_registration_is_refused(tm):
    """a NaN, an infinity, and a scale beyond fp16's range under dev_float = F16: the count in the message, no handle, the handle slot and
    the masters as they were.  The deferred queue: the refusal depends on the masters' VALUES, which queued work may still have to write,
    so the call flushes first like every accepted one -- the queued call runs once, with its own result, and nothing is left behind."""
    import torch
    from tmac_amd import wrapper
    shape = SHAPES[1]
    Mw, K, gs = shape
    bits = 2
    cfg = kcfg(tm, Mw, K, bits, gs, True)
    base = rc.as_f32(masters(shape, "f32")).copy()
    wr = tm.TMACGeMMWrapper(act_group_size=AGS)
    wq = wr.register_dense(dev(masters(shape, "f16")), bits, gs, True, cfg)
    x = acts(3, 1, K, torch.float32)
    (want,) = run(wr, [wq], x, 1)
    out = torch.zeros((1, Mw), dtype=torch.float32, device="cuda")

    def poisoned(values, where):
        v = base.copy()
        for (o, k), val in zip(where, values):
            v[o, k] = val
        return v

    spots = [(7, 11), (7, 12), (100, 300), (191, 383)]                      # two in one group: three groups
    cases = [("nan", poisoned([np.nan] * 4, spots), tm.F32, 3), ("inf", poisoned([np.inf, -np.inf, np.inf, -np.inf], spots), tm.F32, 3),
             ("f16 scale overflow", poisoned([3.0e5, -3.0e5, 4.0e5, -3.0e5], spots), tm.F16, 3)]
    for what, v, dd, count in cases:
        assert convert.rtn_invalid(v, bits, gs, True, dd == tm.F16) == count, what
        w = torch.from_numpy(v).cuda()
        before_w = w.clone()
        # counted, not refused, by the two that write caller memory
        _, _, n = wrapper.rtn_params(w, bits, gs, True, dd == tm.F16, count_invalid=True)
        assert int(n.item()) == count, what
        _, _, n = wrapper.pack_rtn(w, bits, gs, True, cfg, dd, count_invalid=True)
        assert int(n.item()) == count, what
        # refused by registration, behind a queued call
        tm.binding.check(tm.lib().tmac_hip_defer(1))
        try:
            out.zero_()
            wr.fused([wq], x, [out], 1)                                      # queued
            h = C.c_void_p(0xFFFFFFFFFFFFFFFF)
            rc_, msg = raw_register(tm, h, w.data_ptr(), 0, Mw, K, bits, cfg, 0, dd)
            assert rc_ == E_ARG and "{} groups".format(count) in msg and "cannot be quantised" in msg, (what, rc_, msg)
            assert h.value == 0xFFFFFFFFFFFFFFFF, "no handle is created: the slot stays at 0xFF"
            with pytest.raises(tm.TMACHipError, match="{} groups".format(count)):
                tm.Weights.from_dense(w, bits, gs, True, cfg, dd, AGS)
            tm.binding.check(tm.lib().tmac_hip_flush(None))
            torch.cuda.synchronize()
            assert torch.equal(out, want), "the queued call ran, once, with its own result"
        finally:
            tm.lib().tmac_hip_defer(0)
        assert torch.equal(w.view(torch.int32), before_w.view(torch.int32))
        if dd == tm.F16:                                                      # the same masters are fine with fp32 device scales
            ok = tm.Weights.from_dense(w, bits, gs, True, cfg, tm.F32, AGS)
            ok.free()
    wq.free()


def test_refusals(tm):
    import torch
    from tmac_amd import wrapper
    Mw, K, gs = SHAPES[0]
    bits = 2
    st = masters(SHAPES[0], "f16")
    cfg = kcfg(tm, Mw, K, bits, gs, True)
    ab, sb = wrapper.ref_blob_bytes(Mw, K, bits, cfg, tm.F32)
    items = Mw * (K // gs)
    # spare bytes behind each so that "+ 8" stays inside the allocation
    bufA = torch.full((ab + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    bufS = torch.full((sb + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    bufP = torch.full((4 * items + 64,), 0xFF, dtype=torch.uint8, device="cuda")      # scales_out_dev of the parameters
    bufZ = torch.full((4 * items + 64,), 0xFF, dtype=torch.uint8, device="cuda")      # zq_out_dev
    bufN = torch.full((64,), 0xFF, dtype=torch.uint8, device="cuda")                  # invalid_count_dev
    w = torch.from_numpy(st).cuda()
    w8 = torch.zeros(Mw * K + 32, dtype=torch.float16, device="cuda")                 # a copy of the matrix 8 bytes into its allocation
    w8[4:4 + Mw * K] = w.reshape(-1)
    torch.cuda.synchronize()
    pW, pA, pS, pP, pZ, pN = (t.data_ptr() for t in (w, bufA, bufS, bufP, bufZ, bufN))
    SRC = rc.SRC_CODE["f16"]
    flushes = defer_stats(tm)[0]

    def untouched():
        torch.cuda.synchronize()
        return all(bool((b == 0xFF).all()) for b in (bufA, bufS, bufP, bufZ, bufN)) and defer_stats(tm)[0] == flushes

    def pack(code, names, W=pW, src=SRC, c=cfg, A=pA, S=pS, n=pN, b=bits, ref=0):
        rc_, msg = raw_pack(tm, W, src, Mw, K, b, c, A, S, ref, n)
        assert rc_ == code and all(x in msg for x in names) and untouched(), (rc_, msg, names)
        if A == pA and S == pS and n == pN and ref == 0:                              # the register form shares the checks of the inputs
            h = C.c_void_p()
            rc_, msg = raw_register(tm, h, W, src, Mw, K, b, c)
            assert rc_ == code and all(x in msg for x in names) and not h and untouched(), (rc_, msg, names)

    def params(code, names, W=pW, src=SRC, b=bits, g=gs, sc=pP, zq=pZ, n=pN, k=K):
        rc_, msg = raw_params(tm, W, src, Mw, k, b, g, 1, 0, sc, zq, n)
        assert rc_ == code and all(x in msg for x in names) and untouched(), (rc_, msg, names)

    pack(E_ARG, ["W_dev"], W=None)
    pack(E_ARG, ["A_ref_out"], A=None)
    pack(E_ARG, ["scales_ref_out"], S=None)
    pack(E_ARG, ["W_dev", "aligned"], W=w8.data_ptr() + 8)
    pack(E_ARG, ["A_ref_out", "aligned"], A=pA + 8)
    pack(E_ARG, ["scales_ref_out", "aligned"], S=pS + 4)
    pack(E_ARG, ["invalid_count_dev", "aligned"], n=pN + 4)
    pack(E_ARG, ["src_dtype"], src=3)
    pack(E_ARG, ["src_dtype"], src=-1)
    pack(E_ARG, ["host_float"], ref=2)
    pack(E_ARG, ["m_groups", "tmac_hip_register_weights_absmean_dev"], c=tm.KCfg.make(Mw, K, bits, 128, KF, 128, K, False, 1))
    h = C.c_void_p()
    rc_, msg = raw_register(tm, h, pW, SRC, Mw, K, bits, cfg, 0, 2)
    assert rc_ == E_ARG and "dev_float" in msg and not h and untouched()
    rc_ = tm.lib().tmac_hip_register_weights_rtn_dev(None, pW, SRC, Mw, K, bits, C.byref(cfg), 0, 0, None)
    assert rc_ == E_ARG and "out" in tm.lib().tmac_hip_last_error().decode()
    # shape refusals are make_shape's own: the code and the message registration gives for the same arguments
    for bad_cfg, b in ((tm.KCfg.make(Mw, K, bits, 96, KF, gs, AGS, True), bits), (cfg, 5), (tm.KCfg.make(Mw, K, bits, 128, KF, 96, AGS, True), bits)):
        h = C.c_void_p()
        rc0 = tm.lib().tmac_hip_register_weights_dev(C.byref(h), pA, pS, Mw, K, b, C.byref(bad_cfg), tm.F32, tm.F32, None)
        msg0 = tm.lib().tmac_hip_last_error().decode()
        assert rc0 == E_NOMATCH and not h
        pack(E_NOMATCH, [msg0], c=bad_cfg, b=b)

    params(E_ARG, ["W_dev"], W=None)
    params(E_ARG, ["scales_out_dev"], sc=None)
    params(E_ARG, ["zq_out_dev"], zq=None)
    params(E_ARG, ["W_dev", "aligned"], W=w8.data_ptr() + 8)
    params(E_ARG, ["scales_out_dev", "aligned"], sc=pP + 4)
    params(E_ARG, ["zq_out_dev", "aligned"], zq=pZ + 8)
    params(E_ARG, ["invalid_count_dev", "aligned"], n=pN + 4)
    params(E_ARG, ["src_dtype"], src=3)
    params(E_ARG, ["bits"], b=0)
    params(E_ARG, ["bits"], b=5)
    for g in (0, -64, 6, 96):                                                        # not positive, no multiple of 4, no divisor of K
        params(E_ARG, ["group_size"], g=g)
    params(E_ARG, ["K="], k=0)

    # and good calls on the same buffers write them, and nothing else
    rc_, msg = raw_params(tm, pW, SRC, Mw, K, bits, gs, 1, 0, pP, pZ, pN)
    assert rc_ == 0, msg
    rc_, msg = raw_pack(tm, pW, SRC, Mw, K, bits, cfg, pA, pS, 0, None)
    assert rc_ == 0, msg
    torch.cuda.synchronize()
    A, S, _, sc, _ = host(SHAPES[0], "f16", bits, True, False)
    _, zq, _ = convert.rtn_params(st, bits, gs, True)
    assert np.array_equal(to_np(bufA[:ab]), A.reshape(-1)) and np.array_equal(to_np(bufS[:sb]).view(np.float32), S.reshape(-1))
    assert np.array_equal(to_np(bufP[:4 * items]).view(np.float32), sc.reshape(-1)) and np.array_equal(to_np(bufZ[:4 * items]).view(np.float32), zq.reshape(-1))
    assert np.array_equal(to_np(bufN[:4]).view(np.int32), [0])
    assert all(bool((b[n:] == 0xFF).all()) for b, n in ((bufA, ab), (bufS, sb), (bufP, 4 * items), (bufZ, 4 * items), (bufN, 4)))


# ---- 5. ordering --------------------------------------------------------------------------------------------------------------------
def test_each_entry_point_flushes_the_deferred_queue_first(tm):
    import torch
    from tmac_amd import wrapper
    shape = SHAPES[0]
    Mw, K, gs = shape
    bits = 4
    st = masters(shape, "bf16")
    A, S, codes, sc, zr = host(shape, "bf16", bits, True, True)
    cfg = kcfg(tm, Mw, K, bits, gs, True)
    wr = tm.TMACGeMMWrapper(act_group_size=AGS)
    w = wr.register_dense(st, bits, gs, True, cfg)
    x = acts(3, 1, K, torch.float32)
    (want,) = run(wr, [w], x, 1)
    wd = dev(st)
    out = torch.zeros((1, Mw), dtype=torch.float32, device="cuda")
    tm.binding.check(tm.lib().tmac_hip_defer(1))
    results = []
    try:
        for entry in ("params", "pack", "register"):
            out.zero_()
            wr.fused([w], x, [out], 1)                              # queued
            before = defer_stats(tm)
            # a refused call leaves the queue alone
            rc_, _ = raw_pack(tm, wd.data_ptr(), 3, Mw, K, bits, cfg, None, None)
            assert rc_ == E_ARG and defer_stats(tm)[0] == before[0]
            rc_, _ = raw_params(tm, wd.data_ptr(), 2, Mw, K, bits, gs, 1, 0, None, None)
            assert rc_ == E_ARG and defer_stats(tm)[0] == before[0]
            if entry == "params":
                results.append(wrapper.rtn_params(wd, bits, gs, True, True))
            elif entry == "pack":
                results.append(wrapper.pack_rtn(wd, bits, gs, True, cfg, tm.F16))
            else:
                results.append(tm.Weights.from_dense(wd, bits, gs, True, cfg))
            after = defer_stats(tm)
            assert after[0] == before[0] + 1, (entry, before, after)                # the flush happened AT the call
            tm.binding.check(tm.lib().tmac_hip_flush(None))
            assert defer_stats(tm)[0] == after[0], "nothing was left to flush"
            torch.cuda.synchronize()
            assert torch.equal(out, want), entry
    finally:
        tm.lib().tmac_hip_defer(0)
    assert np.array_equal(pc.raw_bits(to_np(results[0][0])), pc.raw_bits(sc))
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
    shape = SHAPES[0]
    Mw, K, gs = shape
    bits = 2
    st = masters(shape, "f32")
    cfg = kcfg(tm, Mw, K, bits, gs, True)
    wr = tm.TMACGeMMWrapper(act_group_size=AGS)
    w = wr.register_dense(st, bits, gs, True, cfg)
    wd, x = dev(st), acts(4, 1, K, torch.float32)
    ab, sb = wrapper.ref_blob_bytes(Mw, K, bits, cfg, tm.F32)
    items = Mw * (K // gs)
    bufA = torch.full((ab,), 0xFF, dtype=torch.uint8, device="cuda")
    bufS = torch.full((sb,), 0xFF, dtype=torch.uint8, device="cuda")
    bufP = torch.full((8 * items,), 0xFF, dtype=torch.uint8, device="cuda")
    out = torch.zeros((1, Mw), dtype=torch.float32, device="cuda")
    L = tm.lib()
    tm.binding.check(L.tmac_hip_defer(1))
    try:
        for entry in ("params", "pack", "register"):
            wr.fused([w], x, [out], 1)                          # queued
            tm.binding.check(L.tmac_hip_debug_defer_fail(1))
            h = C.c_void_p()
            if entry == "params":
                rc_, _ = raw_params(tm, wd.data_ptr(), 0, Mw, K, bits, gs, 1, 0, bufP.data_ptr(), bufP.data_ptr() + 4 * items)
            elif entry == "pack":
                rc_, _ = raw_pack(tm, wd.data_ptr(), 0, Mw, K, bits, cfg, bufA.data_ptr(), bufS.data_ptr())
            else:
                rc_, _ = raw_register(tm, h, wd.data_ptr(), 0, Mw, K, bits, cfg)
            assert rc_ == E_RUNTIME and not h, (entry, rc_)
            tm.binding.check(L.tmac_hip_flush(None))            # the queue is empty after the failed flush
            torch.cuda.synchronize()
            assert all(bool((b == 0xFF).all()) for b in (bufA, bufS, bufP)), entry
    finally:
        L.tmac_hip_defer(0)
    w.free()


# ---- 6. footprint -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", rc.SRCS)
@pytest.mark.parametrize("shape,bits", ((SHAPES[3], 3), (SHAPES[0], 4)))
def test_footprint(tm, shape, bits, src):
    """Guard bands around W_dev, both parameter outputs and both pack outputs, at both placements, with both finite guard patterns and with
    0xFF guards -- NaN in every source dtype: a master read from outside its buffer would move a minimum or a maximum, or invalidate a
    group."""
    from tmac_amd import wrapper
    Mw, K, gs = shape
    st = masters(shape, src)
    A, S, codes, sc, zr = host(shape, src, bits, True, False)
    _, zq, _ = convert.rtn_params(st, bits, gs, True)
    cfg = kcfg(tm, Mw, K, bits, gs, True)
    ab, sb = wrapper.ref_blob_bytes(Mw, K, bits, cfg, tm.F32)
    assert ab == A.size and sb == 4 * S.size
    code = rc.SRC_CODE[src]
    stored_ = st.view(np.int16) if src == "bf16" else st
    SG = K // gs

    def call(alloc):
        tw = alloc.inp(stored_, name="W")
        oP, oZ = alloc.out((Mw, SG), np.float32, "scales_out", tile=False), alloc.out((Mw, SG), np.float32, "zq_out", tile=False)
        oN = alloc.out(4, np.int32, "invalid", tile=False)
        oA, oS = alloc.out(ab, np.uint8, "A_ref", tile=False), alloc.out(sb // 4, np.float32, "scales_ref", tile=False)
        alloc.arm()
        rc_, msg = raw_params(tm, tw.data_ptr(), code, Mw, K, bits, gs, 1, 0, oP.data_ptr(), oZ.data_ptr(), oN.data_ptr())
        assert rc_ == 0, msg
        # the counter is one int32; the three behind it are the test's own, written here so that every output element has a value
        oN[1:] = 0
        rc_, msg = raw_pack(tm, tw.data_ptr(), code, Mw, K, bits, cfg, oA.data_ptr(), oS.data_ptr())
        assert rc_ == 0, msg

    def check_want(want):
        assert np.array_equal(pc.raw_bits(want["scales_out"]), pc.raw_bits(sc)) and np.array_equal(want["zq_out"], zq)
        assert np.array_equal(want["invalid"], [0, 0, 0, 0])
        assert np.array_equal(want["A_ref"], A.reshape(-1)) and np.array_equal(pc.raw_bits(want["scales_ref"]), pc.raw_bits(S))

    fp.check_footprint(call, check_want=check_want, patterns=fp.PATTERNS + (0xFF,))


# ---- 7. the loader ------------------------------------------------------------------------------------------------------------------
def test_load_dense_dir(tm, tmp_path):
    import torch
    from tmac_amd import checkpoint, wrapper
    tensors, _ = rc.write_dense_checkpoint(str(tmp_path))
    wr = tm.TMACGeMMWrapper(act_group_size=AGS)
    bits, gs = 4, 128
    loaded = checkpoint.load_dense_dir(str(tmp_path), wr, bits, gs)
    assert list(loaded) == [rc.CKPT_LAYERS[i][0] for i in (0, 2, 1)]
    for name, seed, Mw, K, src in rc.CKPT_LAYERS:
        st = tensors[name + ".weight"]
        assert (loaded[name].Mw, loaded[name].K, loaded[name].bits) == (Mw, K, bits)
        direct = tm.Weights.from_dense(dev(st), bits, gs, act_group_size=AGS)
        x = acts(seed, 1, K, torch.float32)
        (a,), (b,) = run(wr, [loaded[name]], x, 1), run(wr, [direct], x, 1)
        assert torch.equal(a, b), name
        # ... and it is the host reference's matrix
        bm = bm_of(bits, Mw)
        A, S, _, _, _ = rc.host_blob(st, bits, gs, True, True, bm, KF)
        ref = oracle_out((Mw, K, gs), bits, True, A, stored(S, True), to_np(x))
        assert np.abs(to_np(a) - ref).max() <= 1e-3 * np.abs(ref).max(), name
        if src == "bf16":       # the 16-bit words went up as they lie: the codes are those of the fp32 upcast
            gA, gS = wrapper.pack_rtn(st, bits, gs)
            uA, uS = wrapper.pack_rtn(rc.as_f32(st), bits, gs)
            assert torch.equal(gA, uA) and torch.equal(gS, uS)
        loaded[name].free(); direct.free()
    # a quantised directory is refused, naming the loader to use
    g = tmp_path / "gptq"
    g.mkdir()
    pc.write_gptq_checkpoint(str(g), [("model.layers.0.self_attn.q_proj", 41, 128, 256, 2, 128)])
    with pytest.raises(RuntimeError, match="load_gptq_dir"):
        checkpoint.load_dense_dir(str(g), wr, bits, gs)
