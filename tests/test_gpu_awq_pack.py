"""AutoAWQ checkpoints on the GPU (k_pack_awq_weights / k_pack_awq_scales, tmac_hip_pack_awq_dev, tmac_hip_register_weights_awq_dev,
Weights.from_awq, checkpoint.load_awq_dir).

1. the blob, bit for bit: what the kernels write equals the host route -- convert.unpack_awq + weights.preprocess_weights -- A byte for
   byte, the scales' raw bits, the zero's fp16 overflow to infinity included;
2. handle equivalence: from_awq is from_codes on the unpacked tensors, per layout variant, at N = 1, 4 and 70, integer tap included;
3. bias: rn(plain + b) bit for bit;
4. footprint: nothing outside the two outputs is written, nothing outside the three inputs reaches an output (tests/footprint.py);
5. refusals: return code, a message naming the argument, outputs untouched;
6. ordering: the pack call flushes the deferred queue first; a registration inside a recording is not recorded;
7. the checkpoint loader and the converter's blob, end to end.
Shapes (awq_common.SHAPES): A -- word loads, an 8-row tail in the second 64-row tile, 80 tables (a tile and a tail of 16), five scale
groups; B -- 16-byte loads, a 32-row tail; C -- a whole 256-row tile and two tiles of tables.
"""
import ctypes as C

import numpy as np
import pytest

import awq_common as ac
import footprint as fp
import pack_common as pc
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
E_NOMATCH, E_ARG = -1, -4


@pytest.fixture(scope="module")
def tm():
    import torch
    import tmac_amd
    assert torch.cuda.is_available()
    return tmac_amd


def kcfg(tm, shape, zp=True, bits=4):
    Mw, K, bm, kf, gs, ags = ac.SHAPES[shape]
    return tm.KCfg.make(Mw, K, bits, bm, kf, gs, ags, zp)


@pytest.fixture(scope="module")
def cases():
    """{(shape, scales dtype): (qweight, scales, qzeros)} with the fp16 overflow of pack_common.hard_scales, made once"""
    return {(n, dt): ac.make_awq(ord(n) + (dt == np.float32), s[0], s[1], s[4], dt)[0] for n, s in ac.SHAPES.items() for dt in (np.float16, np.float32)}


def to_np(t):
    return t.cpu().numpy()


# ---- 1. the blob, bit for bit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref_f16", (False, True))
@pytest.mark.parametrize("sdt", (np.float16, np.float32))
@pytest.mark.parametrize("shape", ("A", "B", "C"))
def test_pack_awq_is_the_host_blob(tm, cases, shape, sdt, ref_f16):
    from tmac_amd import wrapper
    Mw, K, bm, kf, gs, ags = ac.SHAPES[shape]
    qw, sc, qz = cases[(shape, sdt)]
    A, S, (_, _, zr, _, _) = ac.host_blob(qw, sc, qz, bm, kf)
    if sdt == np.float16:
        assert np.isinf(zr).any(), "a zero overflows fp16"
    with np.errstate(over="ignore"):
        S = S.astype(np.float16 if ref_f16 else np.float32)
    gA, gS = wrapper.pack_awq(qw, sc, qz, kcfg(tm, shape), tm.F16 if ref_f16 else tm.F32)
    assert np.array_equal(to_np(gA), A.reshape(-1))
    assert np.array_equal(pc.raw_bits(to_np(gS)), pc.raw_bits(S))


def test_pack_awq_without_zero_points_and_without_a_cfg(tm, cases):
    import torch
    from tmac_amd import wrapper
    Mw, K, bm, kf, gs, ags = ac.SHAPES["A"]
    qw, sc, qz = cases[("A", np.float16)]
    A, S, _ = ac.host_blob(qw, sc, qz, bm, kf, zero_point=False)
    gA, gS = wrapper.pack_awq(qw, sc, None, kcfg(tm, "A", zp=False), tm.F16)
    assert np.array_equal(to_np(gA), A.reshape(-1)) and np.array_equal(pc.raw_bits(to_np(gS)), pc.raw_bits(S))
    # no cfg: the shape is read off the tensors (CUDA tensors here), the M-tile is convert.default_bm's
    Mw, K, bm, kf, gs, ags = ac.SHAPES["C"]
    qw, sc, qz = cases[("C", np.float32)]
    A, S, _ = ac.host_blob(qw, sc, qz, tm.convert.default_bm(4, Mw), 16)
    gA, gS = wrapper.pack_awq(*(torch.from_numpy(a).cuda() for a in (qw, sc, qz)))
    assert np.array_equal(to_np(gA), A.reshape(-1)) and np.array_equal(pc.raw_bits(to_np(gS)), pc.raw_bits(S))


def test_a_cfg_without_n_tile_num_has_nothing_to_contradict(tm, cases):
    """the width a cfg describes is bm * n_tile_num / Mw; a cfg that leaves n_tile_num at 0 (a caller of the C-ABI that fills in what the
    library reads) is packed at 4 bits with its bm, as include/tmac_hip.h says -- the same blob as with the field filled in"""
    from tmac_amd import wrapper
    Mw, K, bm, kf, gs, ags = ac.SHAPES["B"]
    qw, sc, qz = cases[("B", np.float16)]
    A, S, _ = ac.host_blob(qw, sc, qz, bm, kf)
    cfg = kcfg(tm, "B")
    cfg.n_tile_num = 0
    gA, gS = wrapper.pack_awq(qw, sc, qz, cfg, tm.F16)
    assert np.array_equal(to_np(gA), A.reshape(-1)) and np.array_equal(pc.raw_bits(to_np(gS)), pc.raw_bits(S))


def test_preprocess_awq_for_t_mac_gpu(tm, cases, tmp_path):
    from tmac_amd import convert
    Mw, K, bm, kf, gs, ags = ac.SHAPES["C"]
    qw, sc, qz = cases[("C", np.float16)]
    path = str(tmp_path / "kcfg.ini")
    convert.write_kcfg(path, [[4, Mw, K, 1, -1]], group_size=gs, act_group_size=ags, zero_point=True, bm={(4, Mw, K): bm}, kfactor=kf)
    with np.errstate(over="ignore"):
        w, s, z, b, g = convert.unpack_awq(qw, sc, qz)
        want = convert.preprocess_for_t_mac(path, w, s, z, bits=b)
    got = convert.preprocess_awq_for_t_mac_gpu(path, qw, sc, qz)
    assert got.dtype == np.uint8 and np.array_equal(got, want)


# ---- 2. handle equivalence ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", (0, 1, 3))
def test_handle_from_awq_is_the_handle_from_the_codes(tm, variant):
    import torch
    bits, Mw, K, bm, kf, gs, ags = 4, 192, 384, 128, 16, 128, 64
    (qw, sc, qz), _ = ac.make_awq(11, Mw, K, gs, np.float16, hard=False)
    A, S, (w, s_u, z_u, _, _) = ac.host_blob(qw, sc, qz, bm, kf)
    cfg = tm.KCfg.make(Mw, K, bits, bm, kf, gs, ags, True)
    tm.binding.check(tm.lib().tmac_hip_set_variant(variant))
    try:
        wr = tm.TMACGeMMWrapper(act_group_size=ags)
        wa = wr.register_awq(torch.from_numpy(qw).cuda(), torch.from_numpy(sc).cuda(), torch.from_numpy(qz).cuda(), cfg, tm.F16)
        wc = wr.register_codes(w, s_u, z_u, bits, cfg, tm.F16)
        assert wa.algorithmic_bytes() == wc.algorithmic_bytes()
        x = np.random.default_rng(5).standard_normal((70, K)).astype(np.float32)
        xt = torch.from_numpy(x).cuda()
        q, _, _ = orc.preprocessor(x[:1], ags)
        want = orc.partial_sums(A, q[0], Mw, K, bits, bm, kf, ags)
        if variant == 1:
            # weights of the two-kernel layout are refused by the fused entry point, from either source alike, and are compared on the path
            # that serves them -- preprocessor + qgemm_lut, and its integer tap (as tests/test_gpu_pack.py does for GPTQ)
            refusals = []
            for h in (wa, wc):
                with pytest.raises(tm.TMACHipError) as e:
                    wr.fused([h], xt[:1], [torch.zeros((1, Mw), dtype=torch.float32, device="cuda")], 1)
                refusals.append((e.value.code, str(e.value)))
            assert refusals[0] == refusals[1] and refusals[0][0] == E_NOMATCH
            wr.set_workspace(K, 4)
            for N in (1, 4):
                ca = torch.zeros((N, Mw), dtype=torch.float32, device="cuda")
                cc = torch.ones((N, Mw), dtype=torch.float32, device="cuda")
                wr.llama_cpp_init(xt[:N], Mw, K, N, bits)
                wr.llama_cpp_compute(wa, ca, N)
                wr.llama_cpp_compute(wc, cc, N)
                torch.cuda.synchronize()
                assert torch.equal(ca, cc), (variant, N)
            wr.llama_cpp_init(xt[:1], Mw, K, 1, bits)
            psa, psc = wr.partial_sums(wa, 1), wr.partial_sums(wc, 1)
        else:
            for N in (1, 4, 70):
                ca = torch.zeros((N, Mw), dtype=torch.float32, device="cuda")
                cc = torch.ones((N, Mw), dtype=torch.float32, device="cuda")
                wr.fused([wa], xt[:N], [ca], N)
                wr.fused([wc], xt[:N], [cc], N)
                torch.cuda.synchronize()
                assert torch.equal(ca, cc), (variant, N)
                assert bool(torch.isfinite(ca).all()) and float(ca.abs().max()) > 0
            psa, _ = wr.fused_partial_sums(wa, xt[:1], 1)
            psc, _ = wr.fused_partial_sums(wc, xt[:1], 1)
        assert np.array_equal(psa, psc) and np.array_equal(psa[0], want)
        wa.free(); wc.free()
    finally:
        tm.binding.check(tm.lib().tmac_hip_set_variant(0))


# ---- 3. bias ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (1, 5))
def test_bias_is_rn_of_plain_plus_b(tm, N):
    import torch
    Mw, K, bm, kf, gs, ags = 128, 512, 256, 16, 128, 64
    (qw, sc, qz), _ = ac.make_awq(23, Mw, K, gs, np.float16, hard=False)
    cfg = tm.KCfg.make(Mw, K, 4, bm, kf, gs, ags, True)
    wr = tm.TMACGeMMWrapper(act_group_size=ags)
    b = np.random.default_rng(24).standard_normal(Mw).astype(np.float16)
    plain, biased = wr.register_awq(qw, sc, qz, cfg, tm.F16), wr.register_awq(qw, sc, qz, cfg, tm.F16, bias=b)
    assert biased.has_bias and not plain.has_bias
    x = torch.from_numpy(np.random.default_rng(25).standard_normal((N, K)).astype(np.float16)).cuda()
    b32 = torch.from_numpy(b).cuda().float()
    p32 = torch.zeros((N, Mw), dtype=torch.float32, device="cuda")
    wr.fused([plain], x, [p32], N)
    for dt in (torch.float32, torch.float16):
        got = torch.zeros((N, Mw), dtype=dt, device="cuda")
        wr.fused([biased], x, [got], N)
        torch.cuda.synchronize()
        want = (p32 + b32).to(dt)
        assert torch.equal(got, want), (N, dt, float((got.float() - want.float()).abs().max()))
        assert bool((got != p32.to(dt)).any())
    plain.free(); biased.free()


# ---- 4. footprint -------------------------------------------------------------------------------------------------------------------
def raw_pack_awq(tm, qw, sc, qz, sdt_code, Mw, K, cfg, A, S, ref):
    rc = tm.lib().tmac_hip_pack_awq_dev(qw, sc, qz, sdt_code, Mw, K, C.byref(cfg), A, S, ref, None)
    return rc, tm.lib().tmac_hip_last_error().decode()


@pytest.mark.parametrize("shape", ("A", "B"))
def test_footprint(tm, shape):
    """guard bands around the three inputs and the two outputs, at both placements of footprint.PLACEMENTS and under both guard bytes"""
    from tmac_amd import wrapper
    Mw, K, bm, kf, gs, ags = ac.SHAPES[shape]
    # (tensors without the fp16 overflow of the bit-for-bit cases: check_footprint wants the unguarded run finite everywhere)
    (qw, sc, qz), _ = ac.make_awq(77, Mw, K, gs, np.float16, hard=False)
    cfg = kcfg(tm, shape)
    ab, sb = wrapper.ref_blob_bytes(Mw, K, 4, cfg, tm.F32)
    A, S, _ = ac.host_blob(qw, sc, qz, bm, kf)
    assert ab == A.size and sb == S.size * 4 and len(fp.PLACEMENTS) == 2

    def call(alloc):
        tq, ts, tz = alloc.inp(qw, name="qweight"), alloc.inp(sc, name="scales"), alloc.inp(qz, name="qzeros")
        oA, oS = alloc.out(ab, np.uint8, "A_ref", tile=False), alloc.out(sb // 4, np.float32, "scales_ref", tile=False)
        alloc.arm()
        rc, msg = raw_pack_awq(tm, tq.data_ptr(), ts.data_ptr(), tz.data_ptr(), tm.F16, Mw, K, cfg, oA.data_ptr(), oS.data_ptr(), tm.F32)
        assert rc == 0, msg

    def check_want(want):
        assert np.array_equal(want["A_ref"], A.reshape(-1))
        assert np.array_equal(pc.raw_bits(want["scales_ref"]), pc.raw_bits(S.astype(np.float32)))

    fp.check_footprint(call, check_want=check_want)


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(tm, cases):
    import torch
    from tmac_amd import wrapper
    Mw, K, bm, kf, gs, ags = ac.SHAPES["B"]
    qw, sc, qz = (torch.from_numpy(a).cuda() for a in cases[("B", np.float16)])
    cfg, cfg_nozp = kcfg(tm, "B"), kcfg(tm, "B", zp=False)
    cfg2 = tm.KCfg.make(Mw, K, 2, 64, kf, gs, ags, True)          # a 2-bit configuration of the same matrix shape
    ab, sb = wrapper.ref_blob_bytes(Mw, K, 4, cfg, tm.F32)
    bufA = torch.full((ab + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    bufS = torch.full((sb + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    spare = torch.zeros(qw.numel() * 4 + 64, dtype=torch.uint8, device="cuda")          # a copy of qweight that can be offset by 8 bytes
    spare[8:8 + qw.numel() * 4] = qw.view(torch.uint8).reshape(-1)
    torch.cuda.synchronize()
    pA, pS, pq, ps, pz = bufA.data_ptr(), bufS.data_ptr(), qw.data_ptr(), sc.data_ptr(), qz.data_ptr()

    def untouched():
        torch.cuda.synchronize()
        return bool((bufA == 0xFF).all()) and bool((bufS == 0xFF).all())

    def awq(code, names, q=pq, s=ps, z=pz, A=pA, S=pS, c=cfg, sdt=tm.F16):
        rc, msg = raw_pack_awq(tm, q, s, z, sdt, Mw, K, c, A, S, tm.F32)
        assert rc == code and all(n in msg for n in names) and untouched(), (rc, msg, names)

    awq(E_ARG, ["qweight", "NULL"], q=None)
    awq(E_ARG, ["scales", "NULL"], s=None)
    awq(E_ARG, ["A_ref_out", "NULL"], A=None)
    awq(E_ARG, ["scales_ref_out", "NULL"], S=None)
    awq(E_ARG, ["qweight", "aligned"], q=spare.data_ptr() + 8)
    awq(E_ARG, ["scales", "aligned"], s=ps + 8)
    awq(E_ARG, ["qzeros", "aligned"], z=pz + 8)
    awq(E_ARG, ["A_ref_out", "aligned"], A=pA + 8)
    awq(E_ARG, ["scales_ref_out", "aligned"], S=pS + 4)
    awq(E_ARG, ["qzeros", "zero_point"], c=cfg_nozp)                       # present without zero points
    awq(E_ARG, ["qzeros", "zero_point"], z=None)                           # absent with them
    awq(E_ARG, ["scales_dtype"], sdt=2)
    awq(E_ARG, ["AWQ is packed at 4 bits"], c=cfg2)
    # a shape refusal is make_shape's own: the code and the message registration gives for the same arguments
    bad = tm.KCfg.make(Mw, K, 4, 160, kf, gs, ags, True)
    bad.n_tile_num = 0          # not filled in: nothing for the 4-bit rule to contradict
    h = C.c_void_p()
    rc0 = tm.lib().tmac_hip_register_weights_dev(C.byref(h), pA, pS, Mw, K, 4, C.byref(bad), tm.F32, tm.F32, None)
    msg0 = tm.lib().tmac_hip_last_error().decode()
    assert rc0 == E_NOMATCH and not h
    awq(E_NOMATCH, [msg0], c=bad)

    # the register form shares the checks: nothing is registered
    L = tm.lib()
    for names, args in ((["qweight", "aligned"], (spare.data_ptr() + 8, ps, pz, tm.F16, Mw, K, C.byref(cfg))),
                        (["qzeros", "NULL"], (pq, ps, None, tm.F16, Mw, K, C.byref(cfg))),
                        (["scales", "NULL"], (pq, None, pz, tm.F16, Mw, K, C.byref(cfg))),
                        (["qzeros", "zero_point"], (pq, ps, pz, tm.F16, Mw, K, C.byref(cfg_nozp))),
                        (["AWQ is packed at 4 bits"], (pq, ps, pz, tm.F16, Mw, K, C.byref(cfg2)))):
        rc = L.tmac_hip_register_weights_awq_dev(C.byref(h), *args, tm.F16, tm.F16, None)
        msg = L.tmac_hip_last_error().decode()
        assert rc == E_ARG and all(n in msg for n in names) and not h, (rc, msg, names)
    # and a good call on the same buffers writes them
    rc, msg = raw_pack_awq(tm, pq, ps, pz, tm.F16, Mw, K, cfg, pA, pS, tm.F32)
    assert rc == 0, msg
    assert not untouched()


# ---- 6. ordering --------------------------------------------------------------------------------------------------------------------
def defer_stats(tm):
    st = [C.c_uint64(0) for _ in range(4)]
    tm.binding.check(tm.lib().tmac_hip_defer_stats(*[C.byref(x) for x in st]))
    return tuple(int(x.value) for x in st)          # flushes, cache hits, stream launches, single calls


def small_matrix(tm, seed, Mw=128, K=256, gs=128, ags=64):
    bm, kf = 256, 16
    (qw, sc, qz), _ = ac.make_awq(seed, Mw, K, gs, np.float16, hard=False)
    cfg = tm.KCfg.make(Mw, K, 4, bm, kf, gs, ags, True)
    A, S, _ = ac.host_blob(qw, sc, qz, bm, kf)
    return (qw, sc, qz), (A, S.astype(np.float32)), cfg


def test_pack_flushes_the_deferred_queue_first(tm):
    import torch
    from tmac_amd import wrapper
    Mw, K, ags = 128, 256, 64
    wr = tm.TMACGeMMWrapper(act_group_size=ags)
    (qw, sc, qz), (A, S), cfg = small_matrix(tm, 21)
    w = wr.register_awq(qw, sc, qz, cfg, tm.F32)
    xs = [torch.from_numpy(np.random.default_rng(i).standard_normal(K).astype(np.float32)).cuda() for i in range(2)]
    want = [torch.zeros(Mw, dtype=torch.float32, device="cuda") for _ in xs]
    for x, o in zip(xs, want):
        wr.fused([w], x, [o], 1)
    torch.cuda.synchronize()
    outs = [torch.zeros(Mw, dtype=torch.float32, device="cuda") for _ in xs]
    dq, ds, dz = (torch.from_numpy(a).cuda() for a in (qw, sc, qz))
    tm.binding.check(tm.lib().tmac_hip_defer(1))
    try:
        for x, o in zip(xs, outs):
            wr.fused([w], x, [o], 1)
        before = defer_stats(tm)
        gA, gS = wrapper.pack_awq(dq, ds, dz, cfg, tm.F32)
        after = defer_stats(tm)
        assert after[0] == before[0] + 1, (before, after)            # the flush happened AT the pack call
        tm.binding.check(tm.lib().tmac_hip_flush(None))
        assert defer_stats(tm)[0] == after[0], "nothing was left to flush"
        # ... and at the registration call
        for x, o in zip(xs, outs):
            wr.fused([w], x, [o], 1)
        before = defer_stats(tm)
        w2 = wr.register_awq(dq, ds, dz, cfg, tm.F32)
        assert defer_stats(tm)[0] == before[0] + 1
        w2.free()
    finally:
        tm.binding.check(tm.lib().tmac_hip_defer(0))
    torch.cuda.synchronize()
    for o, r in zip(outs, want):
        assert float((o - r).abs().max()) <= 1e-3 * float(r.abs().max())
    assert np.array_equal(to_np(gA), A.reshape(-1)) and np.array_equal(pc.raw_bits(to_np(gS)), pc.raw_bits(S))
    w.free()


def test_registration_inside_a_recording_is_not_recorded(tm):
    import torch
    Mw, K, ags = 128, 256, 64
    wr = tm.TMACGeMMWrapper(act_group_size=ags)
    (qw, sc, qz), _, cfg = small_matrix(tm, 22)
    w = wr.register_awq(qw, sc, qz, cfg, tm.F16)
    x0 = torch.from_numpy(np.random.default_rng(1).standard_normal(K).astype(np.float16)).cuda()
    x1 = torch.from_numpy(np.random.default_rng(2).standard_normal(K).astype(np.float16)).cuda()
    o0, o1 = (torch.zeros(Mw, dtype=torch.float16, device="cuda") for _ in range(2))
    with wr.record_chain() as rec:
        wr.fused([w], x0, [o0], 1)
        w2 = wr.register_awq(qw, sc, qz, cfg, tm.F16)          # runs at once
        wr.fused([w], x1, [o1], 1)
    assert rec.chain.nops == 2
    rec.chain.launch(); torch.cuda.synchronize()
    r0, r1 = (torch.zeros(Mw, dtype=torch.float16, device="cuda") for _ in range(2))
    wr.fused([w2], x0, [r0], 1); wr.fused([w2], x1, [r1], 1)          # the handle registered meanwhile is whole
    torch.cuda.synchronize()
    for o, r in ((o0, r0), (o1, r1)):
        assert float((o.float() - r.float()).abs().max()) <= 2e-3 * float(r.float().abs().max())
    rec.chain.free(); w.free(); w2.free()


# ---- 7. the loader, end to end ------------------------------------------------------------------------------------------------------
def test_load_awq_dir(tm, tmp_path):
    import torch
    from tmac_amd import checkpoint, convert
    ags, gs, kf = 64, 128, 16
    Q, D = "model.layers.0.self_attn.q_proj", "model.layers.0.mlp.down_proj"
    layers = [(Q, 41, 128, 256, gs), (D, 42, 64, 384, gs)]
    tensors = ac.write_awq_checkpoint(str(tmp_path), layers, biases=(Q,))
    wr = tm.TMACGeMMWrapper(act_group_size=ags)
    loaded = checkpoint.load_awq_dir(str(tmp_path), wr)
    assert sorted(loaded) == sorted(n for n, *_ in layers)
    assert loaded[Q].has_bias and not loaded[D].has_bias
    for name, seed, Mw, K, _ in layers:
        bm = convert.default_bm(4, Mw)
        trip = [tensors[name + s] for s in (".qweight", ".scales", ".qzeros")]
        A, S, (w, s_u, z_u, _, _) = ac.host_blob(*trip, bm, kf)
        x = np.random.default_rng(seed).standard_normal((1, K)).astype(np.float32)
        xt = torch.from_numpy(x).cuda()
        out, twin_out = (torch.zeros((1, Mw), dtype=torch.float32, device="cuda") for _ in range(2))
        wr.fused([loaded[name]], xt, [out], 1)
        twin = wr.register_codes(w, s_u, z_u, 4, tm.KCfg.make(Mw, K, 4, bm, kf, gs, ags, True), tm.F16, bias=tensors.get(name + ".bias"))
        wr.fused([twin], xt, [twin_out], 1)
        torch.cuda.synchronize()
        assert torch.equal(out, twin_out)
        q, ls, lb = orc.preprocessor(x, ags)
        ref = orc.qgemm_float(A, q, S.astype(np.float32), ls, lb, Mw, K, 1, 4, bm, kf, gs, ags, True)
        if name + ".bias" in tensors:
            ref = ref + tensors[name + ".bias"].astype(np.float32)
        assert np.abs(to_np(out) - ref).max() <= 1e-3 * np.abs(ref).max()
        loaded[name].free(); twin.free()
    with pytest.raises(RuntimeError, match="load_awq_dir"):
        checkpoint.load_gptq_dir(str(tmp_path), wr)
