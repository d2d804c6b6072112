"""Packed ternary BitNet checkpoints to handles on the GPU: tmac_hip_pack_ternary_dev, tmac_hip_register_weights_ternary_dev
(k_pack_ternary_weights, k_pack_ternary_weights_x4 in tmac_pack.hip) and what sits on top (wrapper.pack_ternary,
Weights.from_bitnet_packed, checkpoint.load_bitnet_packed_dir).

The yardstick of the levels is convert.unpack_bitnet_packed, which tests/test_bitnet_packed_cpu.py holds to the bytes of the format's
authors.  Everything here is a permutation of bits, so every bar is exact:
1. the blob: byte for byte weights.preprocess_weights of the unpacked levels, scales_ref the given scales (rounded once for an fp16
   blob); where the read-once kernel applies (R4 = Mw / 4 a multiple of 16) under BOTH kernels, the forced general form torch.equal to it;
2. invalid fields (value 3): the counter is their number, the blob that of the clamped levels, with or without a counter; registration
   refuses the matrix;
3. the handle: bit for bit (torch.equal) the plain twin from_codes(levels, [s]) at N = 1 and N = 5, for both scale conventions and
   bf16 / fp16 / fp32 scales, and the twin is bit for bit orc.qgemm_scale_final, the bar of the unified-scale tests;
4. one recording over three handles, 5. refusals, 6. ordering behind the deferred queue, 7. footprint, 8. the checkpoint loader.
Shapes: bitnet_packed_common.SHAPES (what each reaches is said there).
"""
import ctypes as C

import numpy as np
import pytest

import bitnet_packed_common as bp
import footprint as fp
import pack_common as pc
from oracle import oracle as orc
from test_gpu_bitnet_pack import acts, defer_stats, run, to_np

pytestmark = pytest.mark.gpu
E_NOMATCH, E_RUNTIME, E_ARG = -1, -3, -4
KF = bp.KF


@pytest.fixture(scope="module")
def tm():
    import torch
    import tmac_amd
    assert torch.cuda.is_available()
    return tmac_amd


def kcfg(tm, Mw, K, bm, mg):
    return tm.KCfg.make(Mw, K, 2, bm, KF, 128, K, False, mg)


_CASES = {}


def case(shape):
    """(levels, packed bytes, fp32 scales, host blob A, S) of one shape: made once, shared, never changed"""
    if shape not in _CASES:
        Mw, K, bm, mg = shape
        lv, packed = bp.levels(2000 + Mw + K + mg, Mw, K)
        s = bp.scales(mg)
        A, S = pc.host_blob_codes(lv, s, None, 2, bm, KF)
        _CASES[shape] = (lv, packed, s, A, S)
    return _CASES[shape]


def general_form(tm, on):
    tm.binding.check(tm.lib().tmac_hip_debug_pack_ternary_kernel(1 if on else 0))


# ---- 1. the blob --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref", ["f32", "f16"])
@pytest.mark.parametrize("shape", bp.SHAPES)
def test_pack_ternary_is_the_host_blob_under_both_kernels(tm, shape, ref):
    import torch
    from tmac_amd import wrapper
    Mw, K, bm, mg = shape
    lv, packed, s, A, S = case(shape)
    assert set(np.unique(lv)) == {1, 2, 3}
    ref_dtype, S_want = (tm.F32, S) if ref == "f32" else (tm.F16, S.astype(np.float16))
    cfg = kcfg(tm, Mw, K, bm, mg)
    pd = torch.from_numpy(packed).cuda()
    gA, gS = wrapper.pack_ternary(pd, s, cfg, ref_dtype)
    assert np.array_equal(to_np(gA), A.reshape(-1))
    assert np.array_equal(pc.raw_bits(to_np(gS)), pc.raw_bits(S_want))
    if bp.reads_once(Mw):
        general_form(tm, True)
        try:
            hA, hS, n = wrapper.pack_ternary(pd, s, cfg, ref_dtype, count_invalid=True)
        finally:
            general_form(tm, False)
        assert torch.equal(hA, gA) and torch.equal(hS, gS) and int(n.item()) == 0
    # a numpy array is uploaded as it is
    nA, nS, n = wrapper.pack_ternary(packed, s, cfg, ref_dtype, count_invalid=True)
    assert torch.equal(nA, gA) and torch.equal(nS, gS) and int(n.item()) == 0


def test_the_default_configuration_is_from_bitnets(tm):
    from tmac_amd import wrapper
    Mw, K, bm, mg = bp.SHAPES[0]
    lv, packed, s, _, _ = case(bp.SHAPES[0])
    A, S = pc.host_blob_codes(lv, s, None, 2, tm.convert.default_bm(2, Mw), KF)
    gA, gS = wrapper.pack_ternary(packed, float(s[0]))
    assert np.array_equal(to_np(gA), A.reshape(-1)) and np.array_equal(pc.raw_bits(to_np(gS)), pc.raw_bits(S))


# ---- 2. invalid fields --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", (bp.SHAPES[2], bp.SHAPES[1]))
def test_invalid_fields_are_counted_and_clamped(tm, shape):
    """(320, 320): 2 x 2 workgroups of the read-once kernel, 5 x 2 of the general one; (160, 3200): the general kernel alone, 13 x 3"""
    import torch
    from tmac_amd import wrapper
    Mw, K, bm, mg = shape
    bad, lv, n = bp.with_invalid(77 + Mw, Mw, K, 301)
    assert n > 250
    tiles = set()
    for f in range(4):
        rows, cols = np.nonzero(((bad >> (2 * f)) & 3) == 3)
        assert rows.size, f                                                           # every field holds some
        tiles |= set(zip((rows // 64).tolist(), (cols // 256).tolist()))
    assert len(tiles) >= 4, "the 3s meet several workgroups of either kernel"
    s = bp.scales(mg)
    A, S = pc.host_blob_codes(lv, s, None, 2, bm, KF)
    cfg = kcfg(tm, Mw, K, bm, mg)
    pd = torch.from_numpy(bad).cuda()
    for general in ((False, True) if bp.reads_once(Mw) else (False,)):
        general_form(tm, general)
        try:
            gA, gS, cnt = wrapper.pack_ternary(pd, s, cfg, count_invalid=True)
            hA, hS = wrapper.pack_ternary(pd, s, cfg)                                 # a NULL counter: the same blob
            cnt2 = wrapper.pack_ternary(pd, s, cfg, count_invalid=True)[2]            # the counter is zeroed by every call
            h = C.c_void_p()
            sd = torch.from_numpy(s).cuda()
            rc = tm.lib().tmac_hip_register_weights_ternary_dev(C.byref(h), pd.data_ptr(), sd.data_ptr(), Mw, K, C.byref(cfg), 0, 0, None)
            msg = tm.lib().tmac_hip_last_error().decode()
            with pytest.raises(tm.TMACHipError) as e:
                tm.Weights.from_bitnet_packed(pd, float(s[0]), cfg)
        finally:
            general_form(tm, False)
        assert int(cnt.item()) == n and int(cnt2.item()) == n, (general, int(cnt.item()), n)
        assert np.array_equal(to_np(gA), A.reshape(-1)) and torch.equal(hA, gA) and torch.equal(hS, gS)
        assert np.array_equal(pc.raw_bits(to_np(gS)), pc.raw_bits(S))
        assert rc == E_ARG and not h and msg == "packed weight holds {} fields of value 3 (no ternary level)".format(n), (rc, msg)
        assert e.value.code == E_ARG and "holds {} fields of value 3".format(n) in str(e.value)


# ---- 3. the handle ------------------------------------------------------------------------------------------------------------------
def oracle_out(shape, A, S, x):
    Mw, K, bm, mg = shape
    q, ls, lb = orc.preprocessor(np.ascontiguousarray(x, np.float32), K)
    return orc.qgemm_scale_final(A, q, S, ls[:, 0], lb[:, 0], Mw, K, x.shape[0], 2, bm, KF, mg)[0]


@pytest.mark.parametrize("shape", bp.SHAPES)
def test_handle_is_the_plain_twin_bit_for_bit(tm, shape):
    import torch
    Mw, K, bm, mg = shape
    lv, packed, _, _, _ = case(shape)
    cfg = kcfg(tm, Mw, K, bm, mg)
    wr = tm.TMACGeMMWrapper(act_group_size=K)
    pd = torch.from_numpy(packed).cuda()
    xs = {N: acts(N + K + Mw, N, K, torch.float32) for N in (1, 5)}
    forms = bp.scale_forms(1.6875 if Mw % 256 else 0.73)
    for lc in bp.LINEAR_CLASSES:
        for form, (stored, v) in forms.items():
            s = tm.convert.bitnet_packed_scale(stored, lc)
            assert s == (v if lc == "autobitlinear" else np.float32(1.0) / v)
            sv = np.full(mg, s, np.float32)
            if form == "f32":
                ws = float(stored[0])
            elif form == "f16":
                ws = torch.from_numpy(stored)                                        # a one-element tensor, on the host
            else:
                ws = torch.from_numpy(stored.view(np.int16)).view(torch.bfloat16).cuda().reshape(())      # ... and a 0-d bf16 one on the GPU
            wb = wr.register_bitnet_packed(pd, ws, cfg, lc)
            wn = tm.Weights.from_bitnet_packed(packed, stored, cfg, lc)               # numpy: uint16 means bf16 bits
            wt = tm.Weights.from_codes(lv, sv, None, 2, cfg, tm.F32)
            assert wb.algorithmic_bytes() == wt.algorithmic_bytes() and (wb.Mw, wb.K, wb.bits) == (Mw, K, 2)
            A, S = pc.host_blob_codes(lv, sv, None, 2, bm, KF)
            for N, x in xs.items():
                (cb,), (cn,), (ct,) = run(wr, [wb], x, N), run(wr, [wn], x, N), run(wr, [wt], x, N)
                assert torch.equal(cb, ct) and torch.equal(cn, ct), (lc, form, N, float((cb - ct).abs().max()))
                ref = oracle_out(shape, A, S, to_np(x))
                assert np.array_equal(pc.raw_bits(to_np(ct)), pc.raw_bits(ref)), (lc, form, N, float(np.abs(to_np(ct) - ref).max()))
            wb.free(); wn.free(); wt.free()
    with pytest.raises(ValueError, match="linear_class"):
        tm.Weights.from_bitnet_packed(pd, 1.0, cfg, "linear")


# ---- 4. recording -------------------------------------------------------------------------------------------------------------------
def test_one_declared_independent_recording_of_three_handles(tm):
    """The declared form (record_chain(independent=True): stream mode or nothing) accepts unified-scale handles -- a plain declared
    recording is the undeclared one (tests/test_gpu_actorder_stream.py) -- so this is the declared form, not the fall-back.  Unified-scale
    outputs of stream mode are those of stand-alone launches (include/tmac_hip.h, "deferred launches"): torch.equal."""
    import torch
    shapes = [bp.SHAPES[0], bp.SHAPES[3], bp.SHAPES[1]]
    ws, twins = [], []
    for i, shape in enumerate(shapes):
        Mw, K, bm, mg = shape
        lv, packed, _, _, _ = case(shape)
        stored, v = bp.scale_forms(0.73 + i)[("bf16", "f16", "f32")[i]]
        lc = bp.LINEAR_CLASSES[i % 2]
        ws.append(tm.Weights.from_bitnet_packed(packed, stored, kcfg(tm, Mw, K, bm, mg), lc))
        twins.append(tm.Weights.from_codes(lv, np.full(mg, tm.convert.bitnet_packed_scale(stored, lc), np.float32), None, 2, kcfg(tm, Mw, K, bm, mg), tm.F32))
    xs = [acts(50 + i, 1, s[1], torch.float16)[0].contiguous() for i, s in enumerate(shapes)]
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    alone = [run(wr, [w], x[None, :], 1, torch.float16)[0][0] for w, x in zip(ws, xs)]
    alone_twin = [run(wr, [w], x[None, :], 1, torch.float16)[0][0] for w, x in zip(twins, xs)]
    outs = [torch.full((s[0],), 7.0, dtype=torch.float16, device="cuda") for s in shapes]
    with wr.record_chain(independent=True) as rec:
        for w, x, o in zip(ws, xs, outs):
            wr.fused([w], x, [o], 1)
    assert rec.chain.stream and rec.chain.nops == 3
    rec.chain.launch(); torch.cuda.synchronize()
    assert rec.chain.status() == 0
    rec.chain.free()
    for i, (o, a, t) in enumerate(zip(outs, alone, alone_twin)):
        assert torch.equal(a, t), i
        assert torch.equal(o, a), (i, float((o.float() - a.float()).abs().max()))
    for w in ws + twins:
        w.free()


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------
def raw_pack(tm, P, S_in, Mw, K, cfg, A, S, ref=0, cnt=None):
    rc = tm.lib().tmac_hip_pack_ternary_dev(P, S_in, Mw, K, C.byref(cfg) if cfg is not None else None, A, S, ref, cnt, None)
    return rc, tm.lib().tmac_hip_last_error().decode()


def raw_register(tm, h, P, S_in, Mw, K, cfg, ref=0, dev=0):
    rc = tm.lib().tmac_hip_register_weights_ternary_dev(C.byref(h), P, S_in, Mw, K, C.byref(cfg) if cfg is not None else None, ref, dev, None)
    return rc, tm.lib().tmac_hip_last_error().decode()


def test_refusals(tm):
    import torch
    from tmac_amd import wrapper
    shape = bp.SHAPES[0]
    Mw, K, bm, mg = shape
    lv, packed, s, A_want, S_want = case(shape)
    cfg = kcfg(tm, Mw, K, bm, 1)
    ab, sb = wrapper.ref_blob_bytes(Mw, K, 2, cfg, tm.F32)
    # spare bytes behind each so that "+ 8" stays inside the allocation
    bufA = torch.full((ab + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    bufS = torch.full((sb + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    bufN = torch.full((64,), 0xFF, dtype=torch.uint8, device="cuda")
    p = torch.from_numpy(packed).cuda()
    p8 = torch.zeros(packed.size + 64, dtype=torch.uint8, device="cuda")               # a copy of the matrix 8 bytes into its allocation
    p8[8:8 + packed.size] = p.reshape(-1)
    sin = torch.from_numpy(np.concatenate([s, np.ones(7, np.float32)])).cuda()
    torch.cuda.synchronize()
    pP, pA, pS, pN, pI = p.data_ptr(), bufA.data_ptr(), bufS.data_ptr(), bufN.data_ptr(), sin.data_ptr()
    before = defer_stats(tm)

    def untouched():
        torch.cuda.synchronize()
        return bool((bufA == 0xFF).all()) and bool((bufS == 0xFF).all()) and bool((bufN == 0xFF).all())

    def pack(code, names, P=pP, s_in=pI, c=cfg, A=pA, S=pS, M=Mw, ref=0, cnt=pN, reg=None):
        rc, msg = raw_pack(tm, P, s_in, M, K, c, A, S, ref, cnt)
        assert rc == code and all(n in msg for n in names) and untouched(), (rc, msg, names)
        if (A == pA and S == pS and cnt == pN) if reg is None else reg:               # the register form shares the checks of the inputs
            h = C.c_void_p()
            rc, msg = raw_register(tm, h, P, s_in, M, K, c, ref)
            assert rc == code and all(n in msg for n in names) and not h and untouched(), (rc, msg, names)

    pack(E_ARG, ["kcfg"], c=None)
    pack(E_ARG, ["packed_dev", "NULL"], P=None)
    pack(E_ARG, ["scales_dev", "NULL"], s_in=None)
    pack(E_ARG, ["A_ref_out", "NULL"], A=None)
    pack(E_ARG, ["scales_ref_out", "NULL"], S=None)
    pack(E_ARG, ["packed_dev", "aligned"], P=p8.data_ptr() + 8)
    pack(E_ARG, ["scales_dev", "aligned"], s_in=pI + 4)
    pack(E_ARG, ["A_ref_out", "aligned"], A=pA + 8)
    pack(E_ARG, ["scales_ref_out", "aligned"], S=pS + 4)
    pack(E_ARG, ["invalid_count_dev", "aligned"], cnt=pN + 4)
    pack(E_ARG, ["host_float"], ref=2)
    pack(E_ARG, ["host_float"], ref=-1)
    pack(E_ARG, ["m_groups", "per-group scales: register codes or GPTQ tensors"], c=tm.KCfg.make(Mw, K, 2, bm, KF, 128, 64, False, -1))
    pack(E_ARG, ["m_groups", "Mw"], c=kcfg(tm, Mw, K, bm, 3))
    # a shape refusal is make_shape's own: the code and the message registration gives for the same arguments
    bad = kcfg(tm, Mw, K, 96, 1)
    h = C.c_void_p()
    rc0 = tm.lib().tmac_hip_register_weights_dev(C.byref(h), pA, pS, Mw, K, 2, C.byref(bad), tm.F32, tm.F32, None)
    msg0 = tm.lib().tmac_hip_last_error().decode()
    assert rc0 == E_NOMATCH and not h
    pack(E_NOMATCH, [msg0], c=bad)
    # Mw is 4 x the packed rows: one that registration does not tile gets registration's refusal (Mw = 132: 33 packed rows)
    rc1 = tm.lib().tmac_hip_register_weights_dev(C.byref(h), pA, pS, 132, K, 2, C.byref(cfg), tm.F32, tm.F32, None)
    msg1 = tm.lib().tmac_hip_last_error().decode()
    assert rc1 == E_NOMATCH and not h
    pack(E_NOMATCH, [msg1], M=132)
    # the register form's own arguments
    rc = tm.lib().tmac_hip_register_weights_ternary_dev(None, pP, pI, Mw, K, C.byref(cfg), 0, 0, None)
    assert rc == E_ARG and "out" in tm.lib().tmac_hip_last_error().decode()
    for dv in (2, -1):
        rc, msg = raw_register(tm, h, pP, pI, Mw, K, cfg, 0, dv)
        assert rc == E_ARG and "dev_float" in msg and not h and untouched(), (rc, msg)
    rc = tm.lib().tmac_hip_debug_pack_ternary_kernel(2)
    assert rc == E_ARG and "mode" in tm.lib().tmac_hip_last_error().decode()
    assert defer_stats(tm) == before, "a refused call leaves the deferred queue as it was"

    # and a good call on the same buffers writes them, and nothing behind them
    rc, msg = raw_pack(tm, pP, pI, Mw, K, cfg, pA, pS, 0, pN)
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert np.array_equal(to_np(bufA[:ab]), A_want.reshape(-1)) and np.array_equal(to_np(bufS[:sb]), pc.raw_bits(S_want).view(np.uint8))
    assert int(bufN[:4].view(torch.int32).item()) == 0
    assert bool((bufA[ab:] == 0xFF).all()) and bool((bufS[sb:] == 0xFF).all()) and bool((bufN[4:] == 0xFF).all())


# ---- 6. ordering --------------------------------------------------------------------------------------------------------------------
def test_each_entry_point_flushes_the_deferred_queue_first(tm):
    import torch
    from tmac_amd import wrapper
    shape = bp.SHAPES[0]
    Mw, K, bm, mg = shape
    lv, packed, s, A, S = case(shape)
    cfg = kcfg(tm, Mw, K, bm, mg)
    wr = tm.TMACGeMMWrapper(act_group_size=K)
    w = wr.register_bitnet_packed(packed, float(s[0]), cfg)
    x = acts(3, 1, K, torch.float32)
    (want,) = run(wr, [w], x, 1)
    pd = torch.from_numpy(packed).cuda()
    out = torch.zeros((1, Mw), dtype=torch.float32, device="cuda")
    tm.binding.check(tm.lib().tmac_hip_defer(1))
    results = []
    try:
        for entry in ("pack", "register"):
            out.zero_()
            wr.fused([w], x, [out], 1)                              # queued
            before = defer_stats(tm)
            # a refused call leaves the queue alone
            rc, _ = raw_pack(tm, pd.data_ptr(), None, Mw, K, cfg, None, None)
            assert rc == E_ARG and defer_stats(tm)[0] == before[0]
            h = C.c_void_p()
            rc, _ = raw_register(tm, h, None, None, Mw, K, cfg)
            assert rc == E_ARG and defer_stats(tm)[0] == before[0]
            if entry == "pack":
                results.append(wrapper.pack_ternary(pd, s, cfg))
            else:
                results.append(tm.Weights.from_bitnet_packed(pd, float(s[0]), cfg))
            after = defer_stats(tm)
            assert after[0] == before[0] + 1, (entry, before, after)                # the flush happened AT the call
            tm.binding.check(tm.lib().tmac_hip_flush(None))
            assert defer_stats(tm)[0] == after[0], "nothing was left to flush"
            torch.cuda.synchronize()
            assert torch.equal(out, want), entry
    finally:
        tm.binding.check(tm.lib().tmac_hip_defer(0))
    assert np.array_equal(to_np(results[0][0]), A.reshape(-1))
    (got,) = run(wr, [results[1]], x, 1)
    assert torch.equal(got, want)
    w.free(); results[1].free()


def test_a_failed_flush_returns_its_status_and_launches_nothing(tm):
    """no flush fails on a healthy GPU: tmac_hip_debug_defer_fail(1) makes the next flush's launch attempt return TMAC_HIP_E_RUNTIME on the
    host side, before anything reaches the device (tests/test_gpu_defer.py)"""
    import torch
    from tmac_amd import wrapper
    shape = bp.SHAPES[0]
    Mw, K, bm, mg = shape
    lv, packed, s, _, _ = case(shape)
    cfg = kcfg(tm, Mw, K, bm, mg)
    wr = tm.TMACGeMMWrapper(act_group_size=K)
    w = wr.register_bitnet_packed(packed, float(s[0]), cfg)
    pd, sd, x = torch.from_numpy(packed).cuda(), torch.from_numpy(s).cuda(), acts(4, 1, K, torch.float32)
    ab, sb = wrapper.ref_blob_bytes(Mw, K, 2, cfg, tm.F32)
    bufA = torch.full((ab,), 0xFF, dtype=torch.uint8, device="cuda")
    bufS = torch.full((16,), 0xFF, dtype=torch.uint8, device="cuda")
    bufN = torch.full((16,), 0xFF, dtype=torch.uint8, device="cuda")
    out = torch.zeros((1, Mw), dtype=torch.float32, device="cuda")
    L = tm.lib()
    tm.binding.check(L.tmac_hip_defer(1))
    try:
        for entry in ("pack", "register"):
            wr.fused([w], x, [out], 1)                          # queued
            tm.binding.check(L.tmac_hip_debug_defer_fail(1))
            h = C.c_void_p()
            if entry == "pack":
                rc, _ = raw_pack(tm, pd.data_ptr(), sd.data_ptr(), Mw, K, cfg, bufA.data_ptr(), bufS.data_ptr(), 0, bufN.data_ptr())
            else:
                rc, _ = raw_register(tm, h, pd.data_ptr(), sd.data_ptr(), Mw, K, cfg)
            assert rc == E_RUNTIME and not h, (entry, rc)
            tm.binding.check(L.tmac_hip_flush(None))            # the queue is empty after the failed flush
            torch.cuda.synchronize()
            assert bool((bufA == 0xFF).all()) and bool((bufS == 0xFF).all()) and bool((bufN == 0xFF).all()), entry
    finally:
        L.tmac_hip_defer(0)
    w.free()


# ---- 7. footprint -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", (bp.SHAPES[1], bp.SHAPES[2]))
def test_footprint(tm, shape):
    """Guard bands around packed, the scales, the counter and both outputs, at both placements and with both guard patterns, on a matrix
    WITH invalid fields: (160, 3200) runs the general kernel, (320, 320) the read-once one and then the general one forced.  A packed byte
    read from outside its buffer would change a level or the count (0x7B holds a field of 3); a scale read from outside, the blob's."""
    from tmac_amd import wrapper
    Mw, K, bm, mg = shape
    bad, lv, n = bp.with_invalid(31 + Mw, Mw, K, 97)
    s = bp.scales(mg)
    A, S = pc.host_blob_codes(lv, s, None, 2, bm, KF)
    cfg = kcfg(tm, Mw, K, bm, mg)
    ab, sb = wrapper.ref_blob_bytes(Mw, K, 2, cfg, tm.F32)
    assert ab == A.size and sb == 4 * mg
    forms = (False, True) if bp.reads_once(Mw) else (False,)

    def call(alloc):
        tp, ts = alloc.inp(bad, name="packed"), alloc.inp(np.concatenate([s, np.zeros(4 - mg, np.float32)]), name="scales")     # 16 bytes: skew 32 keeps it aligned
        outs = []
        for g in forms:
            tag = "_general" if g else ""
            outs.append((g, alloc.out(ab, np.uint8, "A_ref" + tag, tile=False), alloc.out(4, np.float32, "scales_ref" + tag, tile=False),
                         alloc.out(4, np.int32, "invalid" + tag, tile=False)))
        alloc.arm()
        try:
            for g, oA, oS, oN in outs:
                general_form(tm, g)
                # the outputs the call does not own are written here, so that "never written" means what it says
                oS[mg:] = 0.5
                oN[1:] = 5
                rc, msg = raw_pack(tm, tp.data_ptr(), ts.data_ptr(), Mw, K, cfg, oA.data_ptr(), oS.data_ptr(), 0, oN.data_ptr())
                assert rc == 0, msg
        finally:
            general_form(tm, False)

    def check_want(want):
        for g in forms:
            tag = "_general" if g else ""
            assert np.array_equal(want["A_ref" + tag], A.reshape(-1)), tag
            assert np.array_equal(pc.raw_bits(want["scales_ref" + tag][:mg]), pc.raw_bits(S)) and np.all(want["scales_ref" + tag][mg:] == 0.5), tag
            assert want["invalid" + tag].tolist() == [n, 5, 5, 5], tag

    fp.check_footprint(call, check_want=check_want)


# ---- 8. the loader ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lc", bp.LINEAR_CLASSES)
def test_load_bitnet_packed_dir(tm, tmp_path, lc):
    import torch
    from tmac_amd import checkpoint
    made, _ = bp.write_packed_checkpoint(str(tmp_path), linear_class=lc)
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    loaded = checkpoint.load_bitnet_packed_dir(str(tmp_path), wr)
    assert list(loaded) == [bp.CKPT_LAYERS[i][0] for i in (0, 2, 1)]
    for name, seed, Mw, K, form, shp, value in bp.CKPT_LAYERS:
        lv, packed, stored, v = made[name]
        assert (loaded[name].Mw, loaded[name].K, loaded[name].bits) == (Mw, K, 2)
        s = v if lc == "autobitlinear" else np.float32(1.0) / v
        bm = tm.convert.default_bm(2, Mw)
        twin = tm.Weights.from_codes(lv, np.array([s], np.float32), None, 2, kcfg(tm, Mw, K, bm, 1), tm.F32)
        x = acts(seed, 1, K, torch.float32)
        (a,), (b,) = run(wr, [loaded[name]], x, 1), run(wr, [twin], x, 1)
        assert torch.equal(a, b), name
        loaded[name].free(); twin.free()
