"""Vector transforms outside a chain: tmac_hip_qgemm_fused_xf_dev (include/tmac_hip.h) -- the N = 1 fused call with a residual add +
RMSNorm, or silu(in) * in2, applied to its activations inside k_gemv_quad, between the activation loads and the table build.

Bars (those of tests/test_gpu_chain_xform.py): every output within 2e-3 of max |C| of the ORACLE run on the vector transformed with
np_norm / np_glu below (tolerance, not bits: the mean square is summed in another order and exp differs in the last bit, which can move
a LUT entry by one step); the residual stream (fp32 adds only) bit for bit.  Where the transform has no rounding of its own -- NORM
without gamma -- the outputs are those of a plain call on the fp32 vector t, bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from footprint import check_footprint
from xf_common import Mat, dev, host, np_glu, np_norm, poison, rel_err

pytestmark = pytest.mark.gpu
BM = 128
XF_CONFIGS = [(512, 1), (512, 2), (768, 3), (1024, 4)]      # the (threads, waves per quad) with an XF instantiation (include/tmac_hip.h)


@pytest.fixture(scope="module")
def tm():
    import torch
    import tmac_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return tmac_amd


def vectors(K, seed, act_dtype):
    """in, in2 (act dtype), residual, gamma (fp32) on the device, and their fp32 host values"""
    import torch
    rng = np.random.default_rng(seed)
    x, x2 = (rng.standard_normal(K).astype(np.float32) for _ in range(2))
    res = rng.standard_normal(K).astype(np.float32)
    gam = (1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    xd, x2d = dev(x).to(act_dtype), dev(x2).to(act_dtype)
    return dict(x=xd, x2=x2d, res=dev(res), gam=dev(gam), xh=host(xd), x2h=host(x2d), resh=res, gamh=gam)


def run_norm_and_glu(tm, wr, mats, K, act_dtype, out_dtype, seed=3, eps=1e-5):
    """NORM with gamma and a residual (all matrices behind it), then GLU, each against the oracle; residual_out exact"""
    import torch
    v = vectors(K, seed, act_dtype)
    t = v["xh"] + v["resh"]
    outs = [poison(m.Mw, out_dtype) for m in mats]
    rout = poison(K, torch.float32)
    wr.fused_xf([m.w for m in mats], v["x"], outs, "norm", residual=v["res"], gamma=v["gam"], eps=eps, residual_out=rout)
    torch.cuda.synchronize()
    assert np.array_equal(rout.cpu().numpy(), t), "residual_out"
    xn = np_norm(t, v["gamh"], eps)
    for m, o in zip(mats, outs):
        e = rel_err(host(o), m.oracle(xn))
        assert e <= 2e-3, ("norm", e)
    outs = [poison(m.Mw, out_dtype) for m in mats]
    wr.fused_xf([m.w for m in mats], v["x"], outs, "glu", in2=v["x2"])
    torch.cuda.synchronize()
    xg = np_glu(v["xh"], v["x2h"])
    for m, o in zip(mats, outs):
        e = rel_err(host(o), m.oracle(xg))
        assert e <= 2e-3, ("glu", e)


def plain(tm, wr, mats, x, out_dtype):
    import torch
    outs = [poison(m.Mw, out_dtype) for m in mats]
    wr.fused([m.w for m in mats], x, outs, 1)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


# ---- 1. nothing changes without a transform ----------------------------------------------------------------------------------
def test_no_transform_is_the_plain_call(tm):
    import torch
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    m = Mat(tm, wr, 1, 512, 1024)
    v = vectors(1024, 1, torch.float16)
    want = plain(tm, wr, [m], v["x"], torch.float16)[0]
    assert np.isfinite(want).all()
    o = poison(512, torch.float16)
    wr.fused_xf([m.w], v["x"], [o], None)                                # xf = NULL
    torch.cuda.synchronize()
    assert np.array_equal(o.cpu().numpy(), want)
    o = poison(512, torch.float16)
    xf = tm.binding.XForm()                                               # kind = TMAC_XF_NONE
    wa, ca = (C.c_void_p * 1)(m.w.handle.value), (C.c_void_p * 1)(o.data_ptr())
    tm.binding.check(tm.lib().tmac_hip_qgemm_fused_xf_dev(wa, 1, v["x"].data_ptr(), tm.F16, C.byref(xf), ca, tm.F16, None))
    torch.cuda.synchronize()
    assert np.array_equal(o.cpu().numpy(), want)


# ---- 2. add-only NORM is exact -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["f16", "f32"])
def test_add_only_norm_is_exact(tm, act):
    """the LUT is built from identical fp32 values by identical code: any difference is a defect of the new prologue"""
    import torch
    act_dtype = torch.float16 if act == "f16" else torch.float32
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    K, Mw = 1024, 512
    m = Mat(tm, wr, 2, Mw, K)
    v = vectors(K, 2, act_dtype)
    tm.binding.check(tm.lib().tmac_hip_debug_quad_config(512, 2))
    t = v["xh"] + v["resh"]
    want = plain(tm, wr, [m], dev(t), torch.float16)[0]
    o, rout = poison(Mw, torch.float16), poison(K, torch.float32)
    wr.fused_xf([m.w], v["x"], [o], "norm", residual=v["res"], residual_out=rout)
    torch.cuda.synchronize()
    assert np.array_equal(rout.cpu().numpy(), t)
    assert np.array_equal(o.cpu().numpy(), want)
    want = plain(tm, wr, [m], v["x"], torch.float16)[0]
    o = poison(Mw, torch.float16)
    wr.fused_xf([m.w], v["x"], [o], "norm")
    torch.cuda.synchronize()
    assert np.array_equal(o.cpu().numpy(), want)


# ---- 3. NORM with gamma, and GLU, against the oracle -----------------------------------------------------------------------
SHAPES = [
    # id, K, Mw list, Mat keywords
    # The smallest matrix: 8 pairs, less than one wave, a grid of ONE workgroup (4 quads, (512,2) holds 4 per workgroup) -- residual_out
    # must be complete.  16 rows, not 4: registration tiles M = Mw * bits by bm >= 32, so no 2-bit matrix has fewer.
    ("one-workgroup", 64, [16], dict(gs=64)),
    ("k1024", 1024, [512], {}),
    ("k11008-ragged-nr6", 11008, [128], {}),
    ("k12288", 12288, [64], {}),
    ("k24576-kernel-limit", 24576, [64], {}),
    ("gs64", 256, [64], dict(gs=64)),
    ("w4", 512, [128], dict(bits=4)),
    ("w1", 256, [128], dict(bits=1)),
    ("w3", 256, [128], dict(bits=3)),
    ("bitnet-unified", 3200, [128], dict(m_groups=1)),
    ("three-matrices", 1024, [128, 64, 64], {}),
]


@pytest.mark.parametrize("name,K,mws,kw", SHAPES, ids=[s[0] for s in SHAPES])
def test_norm_and_glu_against_the_oracle(tm, name, K, mws, kw):
    import torch
    wr = tm.TMACGeMMWrapper(act_group_size=K if kw.get("m_groups", -1) >= 1 else 64)
    mats = [Mat(tm, wr, 10 + i, mw, K, **kw) for i, mw in enumerate(mws)]
    run_norm_and_glu(tm, wr, mats, K, torch.float16, torch.float16)


@pytest.mark.parametrize("ft,wpq", XF_CONFIGS)
def test_every_xf_configuration(tm, ft, wpq):
    """K = 6144: three 64-unit steps (3 waves per quad divide them evenly); the cross-wave sum depends on the wave count"""
    import torch
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    m = Mat(tm, wr, 20, 64, 6144)
    tm.binding.check(tm.lib().tmac_hip_debug_quad_config(ft, wpq))
    run_norm_and_glu(tm, wr, [m], 6144, torch.float16, torch.float16)


@pytest.mark.parametrize("act,out", [("f16", "f16"), ("f16", "f32"), ("f32", "f16"), ("f32", "f32")])
def test_dtypes(tm, act, out):
    import torch
    dt = {"f16": torch.float16, "f32": torch.float32}
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    m = Mat(tm, wr, 30, 256, 1024)
    run_norm_and_glu(tm, wr, [m], 1024, dt[act], dt[out])


# ---- 4. a decoder layer loop, call by call -----------------------------------------------------------------------------------
class Layer:
    def __init__(self, tm, wr, seed, H, F):
        self.q, self.k, self.v = (Mat(tm, wr, seed + i, H, H) for i in range(3))
        self.o = Mat(tm, wr, seed + 3, H, H)
        self.gate, self.up = Mat(tm, wr, seed + 4, F, H), Mat(tm, wr, seed + 5, F, H)
        self.down = Mat(tm, wr, seed + 6, H, F)
        rng = np.random.default_rng(seed)
        self.g1 = dev((1.0 + 0.1 * rng.standard_normal(H)).astype(np.float32))
        self.g2 = dev((1.0 + 0.1 * rng.standard_normal(H)).astype(np.float32))


def test_decoder_layers_call_by_call(tm):
    """o -> NORM -> gate/up -> GLU -> down -> NORM -> q/k/v, the residual stream alternating between two buffers (what
    test_decoder_layers_with_an_operator_outside runs as a chain, with the kept t read back from memory)"""
    import torch
    H, F, NL, eps = 1024, 2816, 3, 1e-5
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    layers = [Layer(tm, wr, 100 * (li + 1), H, F) for li in range(NL)]
    rng = np.random.default_rng(5)
    f16 = lambda n: torch.zeros(n, dtype=torch.float16, device="cuda")
    hbuf = [dev(rng.standard_normal(H).astype(np.float32)), torch.zeros(H, dtype=torch.float32, device="cuda")]
    attn, o, gate, up, down = f16(H), f16(H), f16(F), f16(F), f16(H)
    q, k, v = f16(H), f16(H), f16(H)
    cur = 0
    wr.fused_xf([layers[0].q.w, layers[0].k.w, layers[0].v.w], hbuf[0].half(), [q, k, v], "norm", gamma=layers[0].g1, eps=eps)
    torch.cuda.synchronize()
    hn = hbuf[0].cpu().numpy()
    x1 = np_norm(host(hbuf[0].half()), layers[0].g1.cpu().numpy(), eps)
    for m, got in ((layers[0].q, q), (layers[0].k, k), (layers[0].v, v)):
        assert rel_err(host(got), m.oracle(x1)) <= 2e-3
    for li in range(NL - 1):
        L, Ln = layers[li], layers[li + 1]
        attn.copy_((torch.tanh(q.float()) * 0.5 + 0.25 * k.float() - 0.25 * v.float()).half())     # stand-in for attention
        wr.fused([L.o.w], attn, [o], 1)
        wr.fused_xf([L.gate.w, L.up.w], o, [gate, up], "norm", residual=hbuf[cur], gamma=L.g2, eps=eps, residual_out=hbuf[cur ^ 1])
        cur ^= 1
        wr.fused_xf([L.down.w], gate, [down], "glu", in2=up)
        wr.fused_xf([Ln.q.w, Ln.k.w, Ln.v.w], down, [q, k, v], "norm", residual=hbuf[cur], gamma=Ln.g1, eps=eps, residual_out=hbuf[cur ^ 1])
        torch.cuda.synchronize()
        a, on = host(attn), host(o)
        assert rel_err(on, L.o.oracle(a)) <= 2e-3
        t2 = on + hn
        assert np.array_equal(hbuf[cur].cpu().numpy(), t2), f"layer {li}: residual stream (attention half)"
        x2 = np_norm(t2, L.g2.cpu().numpy(), eps)
        g, u = host(gate), host(up)
        assert rel_err(g, L.gate.oracle(x2)) <= 2e-3 and rel_err(u, L.up.oracle(x2)) <= 2e-3
        d = host(down)
        assert rel_err(d, L.down.oracle(np_glu(g, u))) <= 2e-3
        t3 = d + t2
        cur ^= 1
        assert np.array_equal(hbuf[cur].cpu().numpy(), t3), f"layer {li}: residual stream"
        x3 = np_norm(t3, Ln.g1.cpu().numpy(), eps)
        for m, got in ((Ln.q, q), (Ln.k, k), (Ln.v, v)):
            assert rel_err(host(got), m.oracle(x3)) <= 2e-3
        hn = t3
    assert np.isfinite(hn).all() and np.abs(hn).max() < 1e3


# ---- 5. recording ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("recorded", [True, False])
def test_three_calls_recorded_and_call_by_call(tm, recorded):
    """the three calls of test_gpu_chain_xform's _norm_and_glu_on_external_vectors through fused_xf: inside record_chain() they build a
    chain with transforms, outside they launch one by one; same bars"""
    import torch
    tm.binding.check(tm.lib().tmac_hip_debug_chain_config(0, 1 << 17))
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    K, Mw = 1024, 512
    m0, m1, m2 = Mat(tm, wr, 1, Mw, K), Mat(tm, wr, 2, Mw, K), Mat(tm, wr, 3, Mw, K)
    v = vectors(K, 11, torch.float16)
    rout = torch.zeros(K, dtype=torch.float32, device="cuda")
    o0, o1, o2 = (torch.zeros(Mw, dtype=torch.float16, device="cuda") for _ in range(3))

    def calls():
        wr.fused_xf([m0.w], v["x"], [o0], "norm", residual=v["res"], gamma=v["gam"], eps=1e-5, residual_out=rout)
        wr.fused_xf([m1.w], v["x"], [o1], "glu", in2=v["x2"])
        wr.fused_xf([m2.w], v["x"], [o2], "norm", residual=v["res"])                  # add only
    chain = None
    if recorded:
        with wr.record_chain() as rec:
            calls()
        chain = rec.chain
        nops = C.c_int32(0)
        tm.binding.check(tm.lib().tmac_hip_chain_info(chain.handle, 0, C.byref(nops), None, None, None))
        assert nops.value == 3 and not chain.stream, "a recording with transforms is a decode chain of its three calls"
        assert float(o0.abs().max()) == 0.0, "recorded, not launched"
        chain.launch()
        torch.cuda.synchronize()
        assert chain.status() == 0
    else:
        calls()
        torch.cuda.synchronize()
    t = v["xh"] + v["resh"]
    assert np.array_equal(rout.cpu().numpy(), t)
    assert rel_err(host(o0), m0.oracle(np_norm(t, v["gamh"], 1e-5))) <= 2e-3
    assert rel_err(host(o1), m1.oracle(np_glu(v["xh"], v["x2h"]))) <= 2e-3
    assert rel_err(host(o2), m2.oracle(t)) <= 2e-3
    if chain is not None:
        chain.free()


# ---- 6. deferral -----------------------------------------------------------------------------------------------------------
def defer_stats(tm):
    s = [C.c_uint64(0) for _ in range(4)]
    tm.binding.check(tm.lib().tmac_hip_defer_stats(*[C.byref(x) for x in s]))
    return [x.value for x in s]      # flushes, cache hits, stream launches, single calls


def test_deferral(tm):
    """a transformed call is never queued: it goes behind the queue (one flush, which launches the queued producer of its `in`), then
    launches; when that flush fails it returns the flush's status and launches nothing"""
    import torch
    L = tm.lib()
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    K = 1024
    m0, m1 = Mat(tm, wr, 40, K, K), Mat(tm, wr, 41, 256, K)
    v = vectors(K, 40, torch.float16)
    mid = poison(K, torch.float16)
    o = poison(256, torch.float16)
    tm.binding.check(L.tmac_hip_defer(1))
    try:
        f0 = defer_stats(tm)
        wr.fused([m0.w], v["x"], [mid], 1)                       # queued: writes the transformed call's `in`
        assert defer_stats(tm)[0] == f0[0]
        wr.fused_xf([m1.w], mid, [o], "norm", gamma=v["gam"], eps=1e-5)
        f1 = defer_stats(tm)
        assert f1[0] == f0[0] + 1, "one more flush"
        assert f1[3] == f0[3] + 1, "the queued plain call went out singly; the transformed call is not a queued call"
        torch.cuda.synchronize()
        assert defer_stats(tm) == f1
        midh = host(mid)
        assert rel_err(midh, m0.oracle(v["xh"])) <= 2e-3
        assert rel_err(host(o), m1.oracle(np_norm(midh, v["gamh"], 1e-5))) <= 2e-3
        # a failed flush: its status comes back, nothing of the call is launched
        o2 = poison(256, torch.float16)
        wr.fused([m0.w], v["x"], [mid], 1)
        tm.binding.check(L.tmac_hip_debug_defer_fail(1))
        with pytest.raises(tm.binding.TMACHipError) as ei:
            wr.fused_xf([m1.w], mid, [o2], "norm", gamma=v["gam"], eps=1e-5)
        assert ei.value.code == -3 and "injected" in str(ei.value)
        torch.cuda.synchronize()
        assert torch.isnan(o2).all(), "outputs keep their poison"
    finally:
        L.tmac_hip_debug_defer_fail(0)
        L.tmac_hip_defer(0)


# ---- 7. graph capture --------------------------------------------------------------------------------------------------------
def test_graph_capture(tm):
    import torch
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    K, Mw = 1024, 512
    m = Mat(tm, wr, 50, Mw, K)
    v = vectors(K, 50, torch.float16)
    o, rout = poison(Mw, torch.float16), poison(K, torch.float32)

    def call(stream=None):
        wr.fused_xf([m.w], v["x"], [o], "norm", residual=v["res"], gamma=v["gam"], eps=1e-5, residual_out=rout, stream=stream)
    call()
    torch.cuda.synchronize()
    want, want_r = o.cpu().numpy().copy(), rout.cpu().numpy().copy()
    assert np.isfinite(want).all()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            call(stream=s)
    for _ in range(2):
        o.fill_(float("nan")); rout.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(o.cpu().numpy(), want) and np.array_equal(rout.cpu().numpy(), want_r)


# ---- 8. footprint ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,Mw,gs", [(11008, 128, 128), (64, 16, 64)])      # (16 rows: the smallest a 2-bit matrix registers with)
@pytest.mark.parametrize("kind", ["norm", "glu"])
def test_footprint(tm, K, Mw, gs, kind):
    """guard bands around residual_out and every output, two placements (one 32-byte and not 64-byte aligned), two guard patterns:
    nothing outside the outputs is written -- the inputs among it -- and nothing outside an input reaches a result"""
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    mats = [Mat(tm, wr, 60, Mw, K, gs=gs), Mat(tm, wr, 61, Mw, K, gs=gs)]
    rng = np.random.default_rng(60)
    x, x2 = (rng.standard_normal(K).astype(np.float16) for _ in range(2))
    res = rng.standard_normal(K).astype(np.float32)
    gam = (1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)

    def call(al):
        xd = al.inp(x, name="in")
        ops = dict(in2=al.inp(x2, name="in2")) if kind == "glu" else dict(residual=al.inp(res, name="residual"), gamma=al.inp(gam, name="gamma"))
        outs = [al.out((m.Mw,), "float16", name=f"C{i}") for i, m in enumerate(mats)]
        if kind == "norm":
            ops["residual_out"] = al.out((K,), "float32", name="residual_out", tile=False)
        al.arm()
        wr.fused_xf([m.w for m in mats], xd, outs, kind, **ops)

    def check_want(want):
        xt = np_glu(x, x2) if kind == "glu" else np_norm(x.astype(np.float32) + res, gam, 1e-5)
        for i, m in enumerate(mats):
            assert rel_err(want[f"C{i}"].astype(np.float32), m.oracle(xt)) <= 2e-3
        if kind == "norm":
            assert np.array_equal(want["residual_out"], x.astype(np.float32) + res)
    check_footprint(call, check_want=check_want)


# ---- 9. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(tm):
    """each refusal launches nothing (outputs and residual_out keep their poison) and the next valid call runs"""
    import torch
    L = tm.lib()
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    K, Mw = 1024, 256
    m = Mat(tm, wr, 70, Mw, K)
    v = vectors(K, 70, torch.float32)
    o, rout = poison(Mw, torch.float32), poison(K + 8, torch.float32)
    wa, ca = (C.c_void_p * 1)(m.w.handle.value), (C.c_void_p * 1)(o.data_ptr())
    big = torch.zeros(2 * K + 8, dtype=torch.float32, device="cuda")     # for the misaligned / overlapping operands

    def raw(kind, in2=None, residual=None, gamma=None, residual_out=None, B=None, c=None):
        xf = tm.binding.XForm()
        xf.kind, xf.in2, xf.residual, xf.gamma, xf.eps, xf.residual_out, xf.keep = kind, in2, residual, gamma, 1e-5, residual_out, 0
        carr = ca if c is None else (C.c_void_p * 1)(c)
        rc = L.tmac_hip_qgemm_fused_xf_dev(wa, 1, v["x"].data_ptr() if B is None else B, tm.F32, C.byref(xf), carr, tm.F32, None)
        return rc, L.tmac_hip_last_error().decode()

    def untouched():
        torch.cuda.synchronize()
        return bool(torch.isnan(o).all()) and bool(torch.isnan(rout).all())
    rp, gp, resp = rout.data_ptr(), v["gam"].data_ptr(), v["res"].data_ptr()
    E_ARG, E_NOMATCH = -4, -1
    rc, msg = raw(1, residual=1, residual_out=rp)                        # CARRY outside a recording
    assert rc == E_ARG and "CARRY" in msg and untouched()
    rc, msg = raw(2, residual_out=rp)                                    # GLU without in2
    assert rc == E_ARG and untouched()
    rc, msg = raw(3, residual_out=rp)
    assert rc == E_ARG and "kind" in msg and untouched()
    for name, kw in (("in2", dict(kind=2, in2=big.data_ptr() + 8)), ("residual", dict(kind=1, residual=big.data_ptr() + 8, residual_out=rp)),
                     ("gamma", dict(kind=1, gamma=big.data_ptr() + 8, residual_out=rp)), ("residual_out", dict(kind=1, residual_out=rp + 8))):
        rc, msg = raw(**kw)
        assert rc == E_ARG and name in msg and untouched(), (name, rc, msg)
    # residual_out over B_dev, residual, gamma, C_dev[0]: by a whole vector, and by its last 16 bytes
    for name, kw in (("B_dev", dict(B=big.data_ptr(), residual_out=big.data_ptr())),
                     ("B_dev", dict(B=big.data_ptr(), residual_out=big.data_ptr() + 4 * K - 16)),
                     ("residual", dict(residual=big.data_ptr() + 4 * K - 16, residual_out=big.data_ptr())),
                     ("gamma", dict(gamma=big.data_ptr(), residual_out=big.data_ptr() + 4 * K - 16)),
                     ("C_dev[0]", dict(c=big.data_ptr() + 4 * K - 16, residual_out=big.data_ptr()))):
        rc, msg = raw(1, **kw)
        assert rc == E_ARG and "overlaps " + name in msg and untouched(), (name, rc, msg)
    assert float(big.abs().max()) == 0.0
    # weights with act groups of 32
    wr32 = tm.TMACGeMMWrapper(act_group_size=32)
    case = orc.make_case(71, Mw, K, bits=2, gs=128, ags=32, zero_point=True)
    w32 = wr32.register_weights(orc.preprocess_weights(case["w"], 2, BM, 8), orc.preprocess_scales(case["sc"], case["zr"], 2, BM), Mw, K, 2,
                                tm.KCfg.make(Mw, K, 2, BM, 8, 128, 32, True, -1))
    with pytest.raises(tm.binding.TMACHipError) as ei:
        wr32.fused_xf([w32], v["x"], [o], "norm", gamma=v["gam"], residual_out=rout[:K])
    assert ei.value.code == E_NOMATCH and untouched()
    # (no K above the limit: the kernel is served to gemv_quad_supported's own 24576)
    # a forced launch configuration without an XF instantiation
    tm.binding.check(L.tmac_hip_debug_quad_config(768, 1))
    rc, msg = raw(1, gamma=gp, residual_out=rp)
    assert rc == E_NOMATCH and untouched(), (rc, msg)
    tm.binding.check(L.tmac_hip_debug_quad_config(0, 0))
    # ... and the next valid call runs
    rc, msg = raw(1, residual=resp, gamma=gp, residual_out=rp)
    assert rc == 0, msg
    torch.cuda.synchronize()
    t = v["xh"] + v["resh"]
    assert np.array_equal(rout[:K].cpu().numpy(), t) and bool(torch.isnan(rout[K:]).all())
    assert rel_err(o.cpu().numpy(), m.oracle(np_norm(t, v["gamh"], 1e-5))) <= 2e-3
