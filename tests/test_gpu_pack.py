"""Device-side packing (tmac_pack.hip, tmac_hip_pack_*_dev, tmac_hip_register_weights_*_dev) on the GPU.

1. the blob, bit for bit: what the kernels write equals the host route -- convert.unpack_gptq + weights.preprocess_weights, which
   tests/test_convert.py and tests/test_oracle_vs_ref.py tie to the reference -- A byte for byte, the scales' raw bits;
2. handle equivalence: weights registered from GPTQ tensors behave as weights registered from the host blob, per layout variant;
3. footprint: nothing outside the two outputs is written, nothing outside the inputs reaches an output (tests/footprint.py);
4. refusals: return code, a message naming the argument or width, outputs untouched;
5. ordering: the pack calls flush the deferred queue first; a registration inside a recording is not recorded;
6. the checkpoint loader end to end.
Shapes are the smallest that cross every boundary of the kernels' 64-row x 64-table tiles: Mw 72 .. 384 (tails of 8 and 32 rows, several
M-tiles of several 32-row groups), K 192 .. 384 (K/4 = 48, 64, 80, 96: below, at and past one tile; K/4 > kfactor), 2-5 scale groups of 64
and 128, zero points on and off, one unified-scale (BitNet) configuration.
"""
import ctypes as C

import numpy as np
import pytest

import footprint as fp
import pack_common as pc
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
E_NOMATCH, E_ARG = -1, -4
# bits -> (Mw, K, bm, kfactor, gs, ags)
SHAPES = {1: (384, 384, 128, 16, 128, 64), 2: (160, 320, 64, 16, 64, 64), 3: (160, 192, 96, 16, 64, 64), 4: (72, 256, 96, 8, 64, 32)}


@pytest.fixture(scope="module")
def tm():
    import torch
    import tmac_amd
    assert torch.cuda.is_available()
    return tmac_amd


def kcfg(tm, bits, zp=True, m_groups=-1):
    Mw, K, bm, kf, gs, ags = SHAPES[bits]
    return tm.KCfg.make(Mw, K, bits, bm, kf, gs, K if m_groups >= 1 else ags, zp, m_groups)


@pytest.fixture(scope="module")
def gptq_cases():
    """{(bits, scales dtype): (qweight, scales, qzeros)}, made once"""
    return {(b, dt): pc.make_gptq(31 * b + (dt == np.float32), SHAPES[b][0], SHAPES[b][1], b, SHAPES[b][4], dt) for b in (1, 2, 4)
            for dt in (np.float16, np.float32)}


def to_np(t):
    return t.cpu().numpy()


# ---- 1. the blob, bit for bit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref_f16", (False, True))
@pytest.mark.parametrize("sdt", (np.float16, np.float32))
@pytest.mark.parametrize("v2", (True, False))
@pytest.mark.parametrize("bits", (1, 2, 4))
def test_pack_gptq_is_the_host_blob(tm, gptq_cases, bits, v2, sdt, ref_f16):
    from tmac_amd import wrapper
    Mw, K, bm, kf, gs, ags = SHAPES[bits]
    qw, sc, qz = gptq_cases[(bits, sdt)]
    A, S, _ = pc.host_blob_gptq(qw, sc, qz, v2, bm, kf)
    with np.errstate(over="ignore"):
        S = S.astype(np.float16 if ref_f16 else np.float32)
    gA, gS = wrapper.pack_gptq(qw, sc, qz, kcfg(tm, bits), v2, tm.F16 if ref_f16 else tm.F32)
    assert np.array_equal(to_np(gA), A.reshape(-1))
    assert np.array_equal(pc.raw_bits(to_np(gS)), pc.raw_bits(S))


def test_pack_gptq_without_zero_points(tm, gptq_cases):
    from tmac_amd import wrapper
    bits = 2
    Mw, K, bm, kf, gs, ags = SHAPES[bits]
    qw, sc, qz = gptq_cases[(bits, np.float16)]
    A, S, _ = pc.host_blob_gptq(qw, sc, qz, True, bm, kf, zero_point=False)
    gA, gS = wrapper.pack_gptq(qw, sc, None, kcfg(tm, bits, zp=False), True, tm.F16)
    assert np.array_equal(to_np(gA), A.reshape(-1)) and np.array_equal(pc.raw_bits(to_np(gS)), pc.raw_bits(S))


@pytest.mark.parametrize("zp", (True, False))
@pytest.mark.parametrize("bits", (1, 2, 3, 4))
def test_pack_codes_is_the_host_blob(tm, bits, zp):
    from tmac_amd import wrapper
    Mw, K, bm, kf, gs, ags = SHAPES[bits]
    for dt, ref in ((np.float32, tm.F32), (np.float16, tm.F32), (np.float32, tm.F16)):
        codes, sc, zr = pc.make_codes(17 * bits + zp, Mw, K, bits, gs, dt)
        A, S = pc.host_blob_codes(codes, sc, zr if zp else None, bits, bm, kf)
        gA, gS = wrapper.pack_codes(codes, sc, zr if zp else None, bits, kcfg(tm, bits, zp), ref)
        assert np.array_equal(to_np(gA), A.reshape(-1))
        assert np.array_equal(pc.raw_bits(to_np(gS)), pc.raw_bits(S.astype(np.float16 if ref == tm.F16 else np.float32)))


def test_pack_codes_unified_scale(tm):
    """the BitNet configuration: m_groups = 1, one act group per row -- the blob's scales are the m_groups values, copied"""
    from tmac_amd import wrapper
    bits = 2
    Mw, K, bm, kf, gs, ags = SHAPES[bits]
    codes, _, _ = pc.make_codes(3, Mw, K, bits, gs)
    s1 = np.array([0.0371], np.float32)
    A, S = pc.host_blob_codes(codes, s1, None, bits, bm, kf)
    gA, gS = wrapper.pack_codes(codes, s1, None, bits, kcfg(tm, bits, False, m_groups=1), tm.F32)
    assert np.array_equal(to_np(gA), A.reshape(-1)) and np.array_equal(pc.raw_bits(to_np(gS)), pc.raw_bits(S))


@pytest.mark.parametrize("bits", (1, 2, 4))
def test_preprocess_for_t_mac_gpu(tm, gptq_cases, tmp_path, bits):
    from tmac_amd import convert
    Mw, K, bm, kf, gs, ags = SHAPES[bits]
    if bits == 4:          # write_kcfg wants a shape convert.default_bm knows, whatever bm the section then names: 72 rows have none
        Mw, K, bm, kf, gs, ags = 64, 256, 128, 16, 128, 64
        qw, sc, qz = pc.make_gptq(4, Mw, K, bits, gs, np.float16)
    else:
        qw, sc, qz = gptq_cases[(bits, np.float16)]
    path = str(tmp_path / "kcfg.ini")
    convert.write_kcfg(path, [[bits, Mw, K, 1, -1]], group_size=gs, act_group_size=ags, zero_point=True, bm={(bits, Mw, K): bm}, kfactor=kf)
    with np.errstate(over="ignore"):
        w, s, z, b, g = convert.unpack_gptq(qw, sc, qz, gptq_v2=False)
        want = convert.preprocess_for_t_mac(path, w, s, z, bits=b)
    got = convert.preprocess_for_t_mac_gpu(path, qw, sc, qz, gptq_v2=False)
    assert got.dtype == np.uint8 and np.array_equal(got, want)


# ---- 2. handle equivalence ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", (0, 1, 3))
def test_handle_from_gptq_is_the_handle_from_the_blob(tm, variant):
    import torch
    bits, Mw, K, bm, kf, gs, ags = 2, 192, 384, 128, 16, 128, 64
    qw, sc, qz = pc.make_gptq(11, Mw, K, bits, gs, np.float16, hard=False)
    A, S, _ = pc.host_blob_gptq(qw, sc, qz, True, bm, kf)
    cfg = tm.KCfg.make(Mw, K, bits, bm, kf, gs, ags, True)
    tm.binding.check(tm.lib().tmac_hip_set_variant(variant))
    wr = tm.TMACGeMMWrapper(act_group_size=ags)
    wg = wr.register_gptq(torch.from_numpy(qw).cuda(), torch.from_numpy(sc).cuda(), torch.from_numpy(qz).cuda(), cfg, True, tm.F32)
    wh = wr.register_weights(A, S.astype(np.float32), Mw, K, bits, cfg, tm.F32, tm.F32)
    assert wg.algorithmic_bytes() == wh.algorithmic_bytes()
    x = np.random.default_rng(5).standard_normal((4, K)).astype(np.float32)
    xt = torch.from_numpy(x).cuda()
    q, _, _ = orc.preprocessor(x[:1], ags)
    want = orc.partial_sums(A, q[0], Mw, K, bits, bm, kf, ags)
    if variant == 1:
        # The fused entry point serves the fused layouts only: weights of the two-kernel layout are refused there, from either source
        # alike, and are compared on the path that serves them -- preprocessor + qgemm_lut, and its integer tap.
        refusals = []
        for w in (wg, wh):
            with pytest.raises(tm.TMACHipError) as e:
                wr.fused([w], xt[:1], [torch.zeros((1, Mw), dtype=torch.float32, device="cuda")], 1)
            refusals.append((e.value.code, str(e.value)))
        assert refusals[0] == refusals[1] and refusals[0][0] == E_NOMATCH
        wr.set_workspace(K, 4)
        for N in (1, 4):
            cg = torch.zeros((N, Mw), dtype=torch.float32, device="cuda")
            ch = torch.ones((N, Mw), dtype=torch.float32, device="cuda")
            wr.llama_cpp_init(xt[:N], Mw, K, N, bits)
            wr.llama_cpp_compute(wg, cg, N)
            wr.llama_cpp_compute(wh, ch, N)
            torch.cuda.synchronize()
            assert torch.equal(cg, ch), (variant, N)
        wr.llama_cpp_init(xt[:1], Mw, K, 1, bits)
        psg, psh = wr.partial_sums(wg, 1), wr.partial_sums(wh, 1)
    else:
        for N in (1, 4):
            cg = torch.zeros((N, Mw), dtype=torch.float32, device="cuda")
            ch = torch.ones((N, Mw), dtype=torch.float32, device="cuda")
            wr.fused([wg], xt[:N], [cg], N)
            wr.fused([wh], xt[:N], [ch], N)
            torch.cuda.synchronize()
            assert torch.equal(cg, ch), (variant, N)
        psg, _ = wr.fused_partial_sums(wg, xt[:1], 1)
        psh, _ = wr.fused_partial_sums(wh, xt[:1], 1)
    assert np.array_equal(psg, psh) and np.array_equal(psg[0], want)
    wg.free(); wh.free()


# ---- 3. footprint -------------------------------------------------------------------------------------------------------------------
def raw_pack_gptq(tm, qw, sc, qz, sdt_code, v2, Mw, K, bits, cfg, A, S, ref):
    rc = tm.lib().tmac_hip_pack_gptq_dev(qw, sc, qz, sdt_code, int(v2), Mw, K, bits, C.byref(cfg), A, S, ref, None)
    return rc, tm.lib().tmac_hip_last_error().decode()


def raw_pack_codes(tm, cd, sc, zr, dt_code, Mw, K, bits, cfg, A, S, ref):
    rc = tm.lib().tmac_hip_pack_codes_dev(cd, sc, zr, dt_code, Mw, K, bits, C.byref(cfg), A, S, ref, None)
    return rc, tm.lib().tmac_hip_last_error().decode()


def blob_sizes(tm, Mw, K, bits, cfg, ref):
    from tmac_amd import wrapper
    return wrapper.ref_blob_bytes(Mw, K, bits, cfg, ref)


@pytest.mark.parametrize("bits", (1, 2, 4))
def test_footprint_gptq(tm, bits):
    Mw, K, bm, kf, gs, ags = SHAPES[bits]
    # (tensors without the fp16 overflow of the bit-for-bit cases: check_footprint wants the unguarded run finite everywhere)
    qw, sc, qz = pc.make_gptq(77 + bits, Mw, K, bits, gs, np.float16, hard=False)
    cfg = kcfg(tm, bits)
    ab, sb = blob_sizes(tm, Mw, K, bits, cfg, tm.F32)
    A, S, _ = pc.host_blob_gptq(qw, sc, qz, True, bm, kf)
    assert ab == A.size and sb == S.size * 4

    def call(alloc):
        tq, ts, tz = alloc.inp(qw, name="qweight"), alloc.inp(sc, name="scales"), alloc.inp(qz, name="qzeros")
        oA, oS = alloc.out(ab, np.uint8, "A_ref", tile=False), alloc.out(sb // 4, np.float32, "scales_ref", tile=False)
        alloc.arm()
        rc, msg = raw_pack_gptq(tm, tq.data_ptr(), ts.data_ptr(), tz.data_ptr(), tm.F16, True, Mw, K, bits, cfg, oA.data_ptr(), oS.data_ptr(), tm.F32)
        assert rc == 0, msg

    def check_want(want):
        assert np.array_equal(want["A_ref"], A.reshape(-1))
        assert np.array_equal(pc.raw_bits(want["scales_ref"]), pc.raw_bits(S.astype(np.float32)))

    fp.check_footprint(call, check_want=check_want)


def test_footprint_codes(tm):
    bits = 3
    Mw, K, bm, kf, gs, ags = SHAPES[bits]
    codes, sc, zr = pc.make_codes(9, Mw, K, bits, gs, np.float32)
    cfg = kcfg(tm, bits)
    ab, sb = blob_sizes(tm, Mw, K, bits, cfg, tm.F16)
    A, S = pc.host_blob_codes(codes, sc, zr, bits, bm, kf)

    def call(alloc):
        tc, ts, tz = alloc.inp(codes, name="codes"), alloc.inp(sc, name="scales"), alloc.inp(zr, name="zeros")
        oA, oS = alloc.out(ab, np.uint8, "A_ref", tile=False), alloc.out(sb // 2, np.float16, "scales_ref", tile=False)
        alloc.arm()
        rc, msg = raw_pack_codes(tm, tc.data_ptr(), ts.data_ptr(), tz.data_ptr(), tm.F32, Mw, K, bits, cfg, oA.data_ptr(), oS.data_ptr(), tm.F16)
        assert rc == 0, msg

    def check_want(want):
        assert np.array_equal(want["A_ref"], A.reshape(-1))
        assert np.array_equal(pc.raw_bits(want["scales_ref"]), pc.raw_bits(S.astype(np.float16)))

    fp.check_footprint(call, check_want=check_want)


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(tm, gptq_cases):
    import torch
    bits = 2
    Mw, K, bm, kf, gs, ags = SHAPES[bits]
    qw, sc, qz = (torch.from_numpy(a).cuda() for a in gptq_cases[(bits, np.float16)])
    cfg, cfg_nozp = kcfg(tm, bits), kcfg(tm, bits, zp=False)
    ab, sb = blob_sizes(tm, Mw, K, bits, cfg, tm.F32)
    # 64 spare bytes in front so that "+ 8" stays inside the allocation
    bufA = torch.full((ab + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    bufS = torch.full((sb + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    spare = torch.zeros(qw.numel() * 4 + 64, dtype=torch.uint8, device="cuda")          # a copy of qweight that can be offset by 8 bytes
    spare[8:8 + qw.numel() * 4] = qw.view(torch.uint8).reshape(-1)
    torch.cuda.synchronize()
    pA, pS, pq, ps, pz = bufA.data_ptr(), bufS.data_ptr(), qw.data_ptr(), sc.data_ptr(), qz.data_ptr()

    def untouched():
        torch.cuda.synchronize()
        return bool((bufA == 0xFF).all()) and bool((bufS == 0xFF).all())

    def gptq(code, names, q=pq, s=ps, z=pz, A=pA, S=pS, b=bits, c=cfg, sdt=tm.F16):
        rc, msg = raw_pack_gptq(tm, q, s, z, sdt, True, Mw, K, b, c, A, S, tm.F32)
        assert rc == code and all(n in msg for n in names) and untouched(), (rc, msg, names)

    gptq(E_ARG, ["qweight"], q=None)
    gptq(E_ARG, ["scales"], s=None)
    gptq(E_ARG, ["A_ref_out"], A=None)
    gptq(E_ARG, ["scales_ref_out"], S=None)
    gptq(E_ARG, ["qweight", "aligned"], q=spare.data_ptr() + 8)
    gptq(E_ARG, ["scales", "aligned"], s=ps + 8)
    gptq(E_ARG, ["qzeros", "aligned"], z=pz + 8)
    gptq(E_ARG, ["A_ref_out", "aligned"], A=pA + 8)
    gptq(E_ARG, ["scales_ref_out", "aligned"], S=pS + 4)
    gptq(E_ARG, ["qzeros", "zero_point"], c=cfg_nozp)                      # present without zero points
    gptq(E_ARG, ["qzeros", "zero_point"], z=None)                          # absent with them
    gptq(E_ARG, ["m_groups"], c=kcfg(tm, bits, False, m_groups=1), z=None)
    gptq(E_ARG, ["scales_dtype"], sdt=2)
    # 3-bit GPTQ: refused by width, whatever the rest says
    gptq(E_NOMATCH, ["width 3"], b=3)
    # a shape refusal is make_shape's own: the code and the message registration gives for the same arguments
    bad = tm.KCfg.make(Mw, K, bits, 96, kf, gs, ags, True)
    h = C.c_void_p()
    rc0 = tm.lib().tmac_hip_register_weights_dev(C.byref(h), pA, pS, Mw, K, bits, C.byref(bad), tm.F32, tm.F32, None)
    msg0 = tm.lib().tmac_hip_last_error().decode()
    assert rc0 == E_NOMATCH and not h
    gptq(E_NOMATCH, [msg0], c=bad)

    codes = torch.zeros((Mw, K), dtype=torch.uint8, device="cuda")
    s2 = torch.ones((Mw, K // gs), dtype=torch.float32, device="cuda")

    def cds(code, names, cd=codes.data_ptr(), s=s2.data_ptr(), z=s2.data_ptr(), A=pA, c=cfg, b=bits):
        rc, msg = raw_pack_codes(tm, cd, s, z, tm.F32, Mw, K, b, c, A, pS, tm.F32)
        assert rc == code and all(n in msg for n in names) and untouched(), (rc, msg, names)

    cds(E_ARG, ["codes"], cd=None)
    cds(E_ARG, ["codes", "aligned"], cd=codes.data_ptr() + 4)
    cds(E_ARG, ["zeros", "zero_point"], c=cfg_nozp)
    cds(E_ARG, ["zeros", "zero_point"], z=None)
    cds(E_ARG, ["A_ref_out", "aligned"], A=pA + 8)
    cds(E_NOMATCH, [msg0], c=bad)

    # the register forms share the checks: nothing is registered
    L = tm.lib()
    rc = L.tmac_hip_register_weights_gptq_dev(C.byref(h), spare.data_ptr() + 8, ps, pz, tm.F16, 1, Mw, K, bits, C.byref(cfg), tm.F32, tm.F32, None)
    assert rc == E_ARG and "qweight" in L.tmac_hip_last_error().decode() and not h
    rc = L.tmac_hip_register_weights_gptq_dev(C.byref(h), pq, ps, pz, tm.F16, 1, Mw, K, 3, C.byref(cfg), tm.F32, tm.F32, None)
    assert rc == E_NOMATCH and "width 3" in L.tmac_hip_last_error().decode() and not h
    rc = L.tmac_hip_register_weights_codes_dev(C.byref(h), codes.data_ptr(), s2.data_ptr(), None, tm.F32, Mw, K, bits, C.byref(cfg), tm.F32, tm.F32, None)
    assert rc == E_ARG and "zeros" in L.tmac_hip_last_error().decode() and not h
    # and a good call on the same buffers writes them
    rc, msg = raw_pack_gptq(tm, pq, ps, pz, tm.F16, True, Mw, K, bits, cfg, pA, pS, tm.F32)
    assert rc == 0, msg
    assert not untouched()


# ---- 5. ordering --------------------------------------------------------------------------------------------------------------------
def defer_stats(tm):
    st = [C.c_uint64(0) for _ in range(4)]
    tm.binding.check(tm.lib().tmac_hip_defer_stats(*[C.byref(x) for x in st]))
    return tuple(int(x.value) for x in st)          # flushes, cache hits, stream launches, single calls


def small_matrix(tm, wr, seed, Mw=128, K=256, bits=2, gs=128, ags=64):
    """(Weights registered from GPTQ tensors, the host blob, cfg)"""
    bm, kf = 128, 16
    qw, sc, qz = pc.make_gptq(seed, Mw, K, bits, gs, np.float16, hard=False)
    cfg = tm.KCfg.make(Mw, K, bits, bm, kf, gs, ags, True)
    A, S, _ = pc.host_blob_gptq(qw, sc, qz, True, bm, kf)
    return (qw, sc, qz), (A, S.astype(np.float32)), cfg


def test_pack_flushes_the_deferred_queue_first(tm):
    import torch
    from tmac_amd import wrapper
    Mw, K, bits, ags = 128, 256, 2, 64
    wr = tm.TMACGeMMWrapper(act_group_size=ags)
    (qw, sc, qz), (A, S), cfg = small_matrix(tm, wr, 21)
    w = wr.register_gptq(qw, sc, qz, cfg, True, tm.F32)
    xs = [torch.from_numpy(np.random.default_rng(i).standard_normal(K).astype(np.float32)).cuda() for i in range(2)]
    want = [torch.zeros(Mw, dtype=torch.float32, device="cuda") for _ in xs]
    for x, o in zip(xs, want):
        wr.fused([w], x, [o], 1)
    torch.cuda.synchronize()
    outs = [torch.zeros(Mw, dtype=torch.float32, device="cuda") for _ in xs]
    dq, ds, dz = (torch.from_numpy(a).cuda() for a in (qw, sc, qz))
    tm.binding.check(tm.lib().tmac_hip_defer(1))
    for x, o in zip(xs, outs):
        wr.fused([w], x, [o], 1)
    before = defer_stats(tm)
    gA, gS = wrapper.pack_gptq(dq, ds, dz, cfg, True, tm.F32)
    after = defer_stats(tm)
    assert after[0] == before[0] + 1, (before, after)            # the flush happened AT the pack call
    tm.binding.check(tm.lib().tmac_hip_flush(None))
    assert defer_stats(tm)[0] == after[0], "nothing was left to flush"
    tm.binding.check(tm.lib().tmac_hip_defer(0))
    torch.cuda.synchronize()
    for o, r in zip(outs, want):
        assert float((o - r).abs().max()) <= 1e-3 * float(r.abs().max())
    assert np.array_equal(to_np(gA), A.reshape(-1)) and np.array_equal(pc.raw_bits(to_np(gS)), pc.raw_bits(S))
    w.free()


def test_registration_inside_a_recording_is_not_recorded(tm):
    import torch
    Mw, K, bits, ags = 128, 256, 2, 64
    wr = tm.TMACGeMMWrapper(act_group_size=ags)
    (qw, sc, qz), (A, S), cfg = small_matrix(tm, wr, 22)
    w = wr.register_gptq(qw, sc, qz, cfg, True, tm.F16)
    x0 = torch.from_numpy(np.random.default_rng(1).standard_normal(K).astype(np.float16)).cuda()
    x1 = torch.from_numpy(np.random.default_rng(2).standard_normal(K).astype(np.float16)).cuda()
    o0, o1 = (torch.zeros(Mw, dtype=torch.float16, device="cuda") for _ in range(2))
    with wr.record_chain() as rec:
        wr.fused([w], x0, [o0], 1)
        w2 = wr.register_gptq(qw, sc, qz, cfg, True, tm.F16)          # runs at once
        wr.fused([w], x1, [o1], 1)
    assert rec.chain.nops == 2
    rec.chain.launch(); torch.cuda.synchronize()
    r0, r1 = (torch.zeros(Mw, dtype=torch.float16, device="cuda") for _ in range(2))
    wr.fused([w2], x0, [r0], 1); wr.fused([w2], x1, [r1], 1)          # the handle registered meanwhile is whole
    torch.cuda.synchronize()
    for o, r in ((o0, r0), (o1, r1)):
        assert float((o.float() - r.float()).abs().max()) <= 2e-3 * float(r.float().abs().max())
    rec.chain.free(); w.free(); w2.free()


# ---- 6. the loader, end to end ------------------------------------------------------------------------------------------------------
def test_load_gptq_dir(tm, tmp_path):
    import torch
    from tmac_amd import checkpoint, convert
    ags, gs, kf = 64, 128, 16
    layers = [("model.layers.0.self_attn.q_proj", 41, 128, 256, 2, gs), ("model.layers.0.mlp.down_proj", 42, 64, 384, 4, gs)]
    tensors, _ = pc.write_gptq_checkpoint(str(tmp_path), layers)
    wr = tm.TMACGeMMWrapper(act_group_size=ags)
    loaded = checkpoint.load_gptq_dir(str(tmp_path), wr)
    assert sorted(loaded) == sorted(n for n, *_ in layers)
    for name, seed, Mw, K, bits, _ in layers:
        bm = convert.default_bm(bits, Mw)
        A, S, _ = pc.host_blob_gptq(tensors[name + ".qweight"], tensors[name + ".scales"], tensors[name + ".qzeros"], True, bm, kf)
        x = np.random.default_rng(seed).standard_normal((1, K)).astype(np.float32)
        out = torch.zeros((1, Mw), dtype=torch.float32, device="cuda")
        wr.fused([loaded[name]], torch.from_numpy(x).cuda(), [out], 1)
        torch.cuda.synchronize()
        q, ls, lb = orc.preprocessor(x, ags)
        ref = orc.qgemm_float(A, q, S.astype(np.float32), ls, lb, Mw, K, 1, bits, bm, kf, gs, ags, True)
        assert np.abs(to_np(out) - ref).max() <= 1e-3 * np.abs(ref).max()
        loaded[name].free()
