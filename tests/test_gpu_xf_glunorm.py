"""TMAC_XF_GLU_NORM (include/tmac_hip.h) at N = 1 and in recordings: g = silu(in) * in2 followed by an RMSNorm of g with a weight vector --
the sub-layer norm BitNet b1.58 puts between silu(gate) * up and the down projection -- inside k_gemv_quad (tmac_hip_qgemm_fused_xf_dev)
and, in the producer form, inside k_decode_chain (tmac_hip_chain_xform).

Reference and bar, those of tests/test_gpu_xf.py: every output within 2e-3 of max |C| of the ORACLE run on the vector transformed in numpy --
np_glu as it stands, then np_norm on its fp32 result without a residual, with g rounded to fp16 first where the chain hands it over as fp16
(tests/test_gpu_chain_xform.py).  Where the 2e-3 bar would hide a defect -- a clamped lane's copy of the last pair added to the mean square
moves x by a factor the bar swallows at large K -- the kernel is compared bit for bit with its own NORM fed the same g.
"""
import ctypes as C

import numpy as np
import pytest

from footprint import check_footprint
from test_gpu_xf import XF_CONFIGS, vectors
from xf_common import Mat, dev, host, np_glu, np_norm, poison, rel_err

pytestmark = pytest.mark.gpu
EPS = 1e-5
E_ARG, E_NOMATCH = -4, -1


@pytest.fixture(scope="module")
def tm():
    import torch
    import tmac_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return tmac_amd


@pytest.fixture(autouse=True)
def _knobs(tm):
    """the launch configuration at its default, and a short spin: a lost hand-off reports through chain.status() instead of spinning"""
    L = tm.lib()
    tm.binding.check(L.tmac_hip_debug_quad_config(0, 0))
    tm.binding.check(L.tmac_hip_debug_chain_config(0, 1 << 17))
    yield
    tm.binding.check(L.tmac_hip_debug_quad_config(0, 0))


def np_glunorm(a, b, gamma, eps=EPS, handed_over_f16=False):
    g = np_glu(a, b)
    if handed_over_f16:
        g = g.astype(np.float16).astype(np.float32)
    return np_norm(g, gamma, eps)


def wrapper_for(tm, kw):
    return tm.TMACGeMMWrapper(act_group_size=64)      # (the default of llama_cpp_init alone: the fused calls take the matrices' own act groups)


def run_glunorm(tm, wr, mats, K, act_dtype, out_dtype, seed=3, label=""):
    import torch
    v = vectors(K, seed, act_dtype)
    outs = [poison(m.Mw, out_dtype) for m in mats]
    wr.fused_xf([m.w for m in mats], v["x"], outs, "glu_norm", in2=v["x2"], gamma=v["gam"], eps=EPS)
    torch.cuda.synchronize()
    xn = np_glunorm(v["xh"], v["x2h"], v["gamh"])
    for i, (m, o) in enumerate(zip(mats, outs)):
        e = rel_err(host(o), m.oracle(xn))
        print(f"glu_norm {label} K={K} matrix {i}: rel err vs oracle {e:.2e}")
        assert np.isfinite(host(o)).all() and e <= 2e-3, (label, i, e)


# ---- 1. against the oracle ---------------------------------------------------------------------------------------------------
SHAPES = [
    # id, K, Mw list, Mat keywords
    ("one-workgroup-8-pairs", 64, [16], dict(gs=64)),                 # nearly every lane clamped
    ("k1024", 1024, [512], {}),
    ("bitnet-k3200-400-pairs", 3200, [128], dict(m_groups=1)),        # 400 pairs < 512 threads, unified scale
    ("bitnet-down-k8640", 8640, [64], dict(m_groups=1)),              # 1080 pairs: P % 512 != 0
    ("k11008", 11008, [128], {}),
    ("k24576-kernel-limit", 24576, [64], {}),
    ("w4", 512, [128], dict(bits=4)),
    ("two-matrices", 1024, [128, 64], {}),
]


@pytest.mark.parametrize("name,K,mws,kw", SHAPES, ids=[s[0] for s in SHAPES])
def test_against_the_oracle(tm, name, K, mws, kw):
    import torch
    wr = wrapper_for(tm, kw)
    mats = [Mat(tm, wr, 10 + i, mw, K, **kw) for i, mw in enumerate(mws)]
    run_glunorm(tm, wr, mats, K, torch.float16, torch.float16, label=name)


# ---- 2. every XF configuration -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft,wpq", XF_CONFIGS)
def test_every_xf_configuration(tm, ft, wpq):
    """K = 6144, 768 pairs: (512, *) has clamped lanes in its second round, (768, 3) none, (1024, 4) a quarter of its lanes"""
    import torch
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    m = Mat(tm, wr, 20, 64, 6144)
    tm.binding.check(tm.lib().tmac_hip_debug_quad_config(ft, wpq))
    run_glunorm(tm, wr, [m], 6144, torch.float16, torch.float16, label=f"({ft},{wpq})")


# ---- 3. dtypes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act,out", [("f16", "f16"), ("f16", "f32"), ("f32", "f16"), ("f32", "f32")])
def test_dtypes(tm, act, out):
    import torch
    dt = {"f16": torch.float16, "f32": torch.float32}
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    m = Mat(tm, wr, 30, 256, 1024)
    run_glunorm(tm, wr, [m], 1024, dt[act], dt[out], label=f"{act}->{out}")


# ---- 4. decomposition: GLU_NORM == NORM on the same g, bit for bit -----------------------------------------------------------
@pytest.mark.parametrize("K,kw", [(3200, dict(m_groups=1)), (11008, {})], ids=["k3200", "k11008"])
@pytest.mark.parametrize("ft,wpq", [(512, 2), (1024, 4)])
def test_is_the_norm_of_its_own_glu(tm, K, kw, ft, wpq):
    """g as the N >= 2 tap shows it (kind GLU, the row repeated: the same expression as k_gemv_quad's), fed as fp32 activations to kind NORM
    with the same gamma, no residual, in the same launch configuration: the mean square then runs over the same numbers in the same order,
    and a clamped lane that leaked into kind 4's sum (K = 3200: 400 pairs under 512 threads; K = 11008: 1376 pairs in rounds of 512 or
    1024) would show in the bits.  `in` is zero on a random half of the elements: g is exactly zero there on any exp."""
    import torch
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    m = Mat(tm, wr, 35, 64, K, **kw)
    rng = np.random.default_rng(K)
    x = rng.standard_normal(K).astype(np.float16)
    x[rng.random(K) < 0.5] = 0
    x2 = rng.standard_normal(K).astype(np.float16)
    gam = dev((1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32))
    xd, x2d = dev(x), dev(x2)
    gt = poison(2 * K, torch.float32).view(2, K)
    wr.xf_rows_tap(xd.repeat(2).view(2, K).contiguous(), gt, "glu", K, 2, in2=x2d.repeat(2).view(2, K).contiguous())
    torch.cuda.synchronize()
    g = gt.cpu().numpy()
    assert np.array_equal(g[0], g[1]) and np.isfinite(g).all()
    gh = np_glu(x, x2)
    assert np.array_equal(g[0][x == 0], gh[x == 0]) and rel_err(g[0], gh) <= 1e-5
    tm.binding.check(tm.lib().tmac_hip_debug_quad_config(ft, wpq))
    a, b = poison(m.Mw, torch.float32), poison(m.Mw, torch.float32)
    wr.fused_xf([m.w], xd, [a], "glu_norm", in2=x2d, gamma=gam, eps=EPS)
    wr.fused_xf([m.w], gt[0].contiguous(), [b], "norm", gamma=gam, eps=EPS)
    torch.cuda.synchronize()
    ah, bh = a.cpu().numpy(), b.cpu().numpy()
    assert np.isfinite(ah).all()
    print(f"K={K} ({ft},{wpq}): kind 4 vs NORM on the tapped g: {int((ah != bh).sum())} of {ah.size} outputs differ, max |diff| {np.abs(ah - bh).max():.3e}")
    assert np.array_equal(ah, bh)
    assert rel_err(ah, m.oracle(np_norm(g[0], gam.cpu().numpy(), EPS))) <= 2e-3


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(tm):
    """each refusal is TMAC_HIP_E_ARG with a message naming the field, launches nothing (the outputs keep their poison), and the next valid
    call runs; 3 is still no kind"""
    import torch
    L = tm.lib()
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    K, Mw = 1024, 256
    m = Mat(tm, wr, 70, Mw, K)
    v = vectors(K, 70, torch.float32)
    o, rout = poison(Mw, torch.float32), poison(K, torch.float32)
    wa, ca = (C.c_void_p * 1)(m.w.handle.value), (C.c_void_p * 1)(o.data_ptr())
    big = torch.zeros(2 * K + 8, dtype=torch.float32, device="cuda")

    def raw(kind, in2=None, residual=None, gamma=None, residual_out=None, keep=0):
        xf = tm.binding.XForm()
        xf.kind, xf.in2, xf.residual, xf.gamma, xf.eps, xf.residual_out, xf.keep = kind, in2, residual, gamma, EPS, residual_out, keep
        rc = L.tmac_hip_qgemm_fused_xf_dev(wa, 1, v["x"].data_ptr(), tm.F32, C.byref(xf), ca, tm.F32, None)
        return rc, L.tmac_hip_last_error().decode()

    def untouched():
        torch.cuda.synchronize()
        return bool(torch.isnan(o).all()) and bool(torch.isnan(rout).all())
    i2, gp, resp, rp = v["x2"].data_ptr(), v["gam"].data_ptr(), v["res"].data_ptr(), rout.data_ptr()
    for name, kw in (("gamma", dict(in2=i2)),
                     ("in2", dict(gamma=gp)),
                     ("residual", dict(in2=i2, gamma=gp, residual=resp)),
                     ("residual_out", dict(in2=i2, gamma=gp, residual_out=rp)),
                     ("keep", dict(in2=i2, gamma=gp, keep=1)),
                     ("in2", dict(in2=big.data_ptr() + 8, gamma=gp)),
                     ("gamma", dict(in2=i2, gamma=big.data_ptr() + 8))):
        rc, msg = raw(4, **kw)
        assert rc == E_ARG and name in msg and untouched(), (name, kw, rc, msg)
    rc, msg = raw(3, in2=i2, gamma=gp)
    assert rc == E_ARG and "kind" in msg and untouched(), (rc, msg)
    rc, msg = raw(5, in2=i2, gamma=gp)
    assert rc == E_ARG and "kind" in msg and untouched(), (rc, msg)
    rc, msg = raw(4, in2=i2, gamma=gp)
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert rel_err(o.cpu().numpy(), m.oracle(np_glunorm(v["xh"], v["x2h"], v["gamh"]))) <= 2e-3
    assert bool(torch.isnan(rout).all())


# ---- 6. - 8. a decoder layer with the sub-layer norm ----------------------------------------------------------------------------
class Layer:
    def __init__(self, tm, wr, seed, H, F, kw):
        self.q, self.k, self.v = (Mat(tm, wr, seed + i, H, H, **kw) for i in range(3))
        self.o = Mat(tm, wr, seed + 3, H, H, **kw)
        self.gate, self.up = Mat(tm, wr, seed + 4, F, H, **kw), Mat(tm, wr, seed + 5, F, H, **kw)
        self.down = Mat(tm, wr, seed + 6, H, F, **kw)
        rng = np.random.default_rng(seed)
        self.g1, self.g2 = (dev((1.0 + 0.1 * rng.standard_normal(H)).astype(np.float32)) for _ in range(2))
        self.g3 = dev((1.0 + 0.1 * rng.standard_normal(F)).astype(np.float32))              # ffn_sub_norm


LAYER_SHAPES = {
    "llama-shaped": (1024, 2816, {}),
    # 432 row pairs of gate / up over the grid (ragged); K = 1728 of down is 27 act units: a partial step
    "bitnet-shaped": (640, 1728, dict(m_groups=1)),
}
_LAYERS = {}


def layers_of(tm, shape, NL=3):
    """the matrices of a shape, registered once and shared by the tests below (never changed)"""
    if shape not in _LAYERS:
        H, F, kw = LAYER_SHAPES[shape]
        wr = tm.TMACGeMMWrapper(act_group_size=64)
        _LAYERS[shape] = (wr, [Layer(tm, wr, 100 * (li + 1), H, F, kw) for li in range(NL)])
    return _LAYERS[shape]


def outside(attn, q, k, v):
    """stand-in for attention: some kernel of the stream between two segments"""
    import torch
    attn.copy_((torch.tanh(q.float()) * 0.5 + 0.25 * k.float() - 0.25 * v.float()).half())


def check_segment(L, Ln, a, on, g, u, d, hn, h_out, qkv, handed_over_f16, li):
    """every mpGEMM of one segment against the oracle on what it consumed; the residual stream bit for bit.  Returns the new stream."""
    assert rel_err(on, L.o.oracle(a)) <= 2e-3, f"layer {li}: o"
    t2 = on + hn
    x2 = np_norm(t2, L.g2.cpu().numpy(), EPS)
    eg, eu = rel_err(g, L.gate.oracle(x2)), rel_err(u, L.up.oracle(x2))
    assert eg <= 2e-3 and eu <= 2e-3, f"layer {li}: gate {eg:.2e} up {eu:.2e}"
    ed = rel_err(d, L.down.oracle(np_glunorm(g, u, L.g3.cpu().numpy(), handed_over_f16=handed_over_f16)))
    print(f"layer {li}: down behind GLU_NORM rel err vs oracle {ed:.2e}")
    assert ed <= 2e-3, f"layer {li}: down {ed:.2e}"
    t3 = d + t2
    assert np.array_equal(h_out, t3), f"layer {li}: residual stream"
    x3 = np_norm(t3, Ln.g1.cpu().numpy(), EPS)
    for m, got in zip((Ln.q, Ln.k, Ln.v), qkv):
        assert rel_err(got, m.oracle(x3)) <= 2e-3, f"layer {li}: next q/k/v"
    return t3


@pytest.mark.parametrize("shape", list(LAYER_SHAPES))
def test_recorded_segment_producer_form(tm, shape):
    """one launch per segment o -> NORM(keep) -> gate/up -> GLU_NORM -> down -> NORM(CARRY, residual_out) -> next q/k/v: the gate/up call
    publishes silu(gate) * up (fp16, like every handed-over vector) and the down projection norms it inside its LUT build"""
    import torch
    H, F, kw = LAYER_SHAPES[shape]
    wr, layers = layers_of(tm, shape)
    NL = len(layers)
    rng = np.random.default_rng(5)
    h = dev(rng.standard_normal(H).astype(np.float32))
    f16 = lambda n: torch.zeros(n, dtype=torch.float16, device="cuda")
    attn = f16(H)
    bufs = [dict(o=f16(H), gate=f16(F), up=f16(F), down=f16(H), q=f16(H), k=f16(H), v=f16(H), h_out=torch.zeros(H, dtype=torch.float32, device="cuda"))
            for _ in range(NL - 1)]
    q0, k0, v0 = f16(H), f16(H), f16(H)
    hx = h.half()
    wr.fused_xf([layers[0].q.w, layers[0].k.w, layers[0].v.w], hx, [q0, k0, v0], "norm", gamma=layers[0].g1, eps=EPS)
    chains = []
    for li in range(NL - 1):
        L, Ln, b = layers[li], layers[li + 1], bufs[li]
        hin = h if li == 0 else bufs[li - 1]["h_out"]
        with wr.record_chain() as rec:
            wr.fused([L.o.w], attn, [b["o"]], 1)
            wr.chain_xform("norm", residual=hin, gamma=L.g2, eps=EPS, keep=True)
            wr.fused([L.gate.w, L.up.w], b["o"], [b["gate"], b["up"]], 1)
            wr.chain_xform("glu_norm", in2=b["up"], gamma=L.g3, eps=EPS)
            wr.fused([L.down.w], b["gate"], [b["down"]], 1)
            wr.chain_xform("norm", residual=wr.CARRY, gamma=Ln.g1, eps=EPS, residual_out=b["h_out"])
            wr.fused([Ln.q.w, Ln.k.w, Ln.v.w], b["down"], [b["q"], b["k"], b["v"]], 1)
        assert not rec.chain.stream, "a recording with transforms is a decode chain (tmac_hip_chain_is_stream == 0)"
        nops = C.c_int32(0)
        tm.binding.check(tm.lib().tmac_hip_chain_info(rec.chain.handle, 0, C.byref(nops), None, None, None))
        assert nops.value == 4
        chains.append(rec.chain)
    torch.cuda.synchronize()
    hn = h.cpu().numpy()
    q, k, v = q0, k0, v0
    try:
        for li in range(NL - 1):
            L, Ln, b = layers[li], layers[li + 1], bufs[li]
            outside(attn, q, k, v)
            chains[li].launch()
            torch.cuda.synchronize()
            assert chains[li].status() == 0, f"layer {li}: a hand-off timed out"
            hn = check_segment(L, Ln, host(attn), host(b["o"]), host(b["gate"]), host(b["up"]), host(b["down"]), hn, b["h_out"].cpu().numpy(),
                               [host(b[n]) for n in "qkv"], True, li)
            q, k, v = b["q"], b["k"], b["v"]
        assert np.isfinite(hn).all() and np.abs(hn).max() < 1e3
    finally:
        for c in chains:
            c.free()


def down_calls(tm, shape):
    wr, layers = layers_of(tm, shape)
    H, F, kw = LAYER_SHAPES[shape]
    return wr, layers[0], H, F


@pytest.mark.parametrize("form", ["epilogue-off", "vectors-in-memory"])
def test_recording_refuses_the_reader_form(tm, form, monkeypatch):
    """tmac_hip_chain_end returns TMAC_HIP_E_NOMATCH and says why; the same calls issued one by one pass the bars of the oracle test"""
    import torch
    wr, L, H, F = down_calls(tm, "bitnet-shaped")
    rng = np.random.default_rng(17)
    x = dev(rng.standard_normal(H).astype(np.float16))
    gate, up, down = (torch.zeros(n, dtype=torch.float16, device="cuda") for n in (F, F, H))
    if form == "epilogue-off":
        monkeypatch.setenv("TMAC_CHAIN_GLU_EPILOGUE", "0")

        def calls():
            wr.fused([L.gate.w, L.up.w], x, [gate, up], 1)
            wr.fused_xf([L.down.w], gate, [down], "glu_norm", in2=up, gamma=L.g3, eps=EPS)
    else:
        wr.fused([L.gate.w, L.up.w], x, [gate, up], 1)

        def calls():
            wr.fused_xf([L.down.w], gate, [down], "glu_norm", in2=up, gamma=L.g3, eps=EPS)
            wr.fused([L.o.w], down, [torch.zeros(H, dtype=torch.float16, device="cuda")], 1)      # (a hand-off: not a candidate for stream mode)
    with pytest.raises(tm.binding.TMACHipError) as ei:
        with wr.record_chain():
            calls()
    assert ei.value.code == E_NOMATCH and "GLU_NORM" in str(ei.value), str(ei.value)
    torch.cuda.synchronize()
    assert float(down.abs().max()) == 0.0, "recorded and refused: nothing was launched"
    monkeypatch.delenv("TMAC_CHAIN_GLU_EPILOGUE", raising=False)
    if form == "epilogue-off":
        calls()
    else:
        wr.fused_xf([L.down.w], gate, [down], "glu_norm", in2=up, gamma=L.g3, eps=EPS)
    torch.cuda.synchronize()
    xh = host(x)
    g, u = host(gate), host(up)
    assert rel_err(g, L.gate.oracle(xh)) <= 2e-3 and rel_err(u, L.up.oracle(xh)) <= 2e-3
    assert rel_err(host(down), L.down.oracle(np_glunorm(g, u, L.g3.cpu().numpy()))) <= 2e-3


def test_layers_call_by_call(tm):
    """the BitNet-shaped segments issued one by one (what a caller does when tmac_hip_chain_end refuses): kind 4 in front of down, the
    residual stream alternating between two buffers"""
    import torch
    shape = "bitnet-shaped"
    H, F, kw = LAYER_SHAPES[shape]
    wr, layers = layers_of(tm, shape)
    NL = len(layers)
    rng = np.random.default_rng(5)
    f16 = lambda n: torch.zeros(n, dtype=torch.float16, device="cuda")
    hbuf = [dev(rng.standard_normal(H).astype(np.float32)), torch.zeros(H, dtype=torch.float32, device="cuda")]
    attn, o, gate, up, down = f16(H), f16(H), f16(F), f16(F), f16(H)
    q, k, v = f16(H), f16(H), f16(H)
    cur = 0
    wr.fused_xf([layers[0].q.w, layers[0].k.w, layers[0].v.w], hbuf[0].half(), [q, k, v], "norm", gamma=layers[0].g1, eps=EPS)
    torch.cuda.synchronize()
    hn = hbuf[0].cpu().numpy()
    for li in range(NL - 1):
        L, Ln = layers[li], layers[li + 1]
        outside(attn, q, k, v)
        wr.fused([L.o.w], attn, [o], 1)
        wr.fused_xf([L.gate.w, L.up.w], o, [gate, up], "norm", residual=hbuf[cur], gamma=L.g2, eps=EPS, residual_out=hbuf[cur ^ 1])
        cur ^= 1
        wr.fused_xf([L.down.w], gate, [down], "glu_norm", in2=up, gamma=L.g3, eps=EPS)
        wr.fused_xf([Ln.q.w, Ln.k.w, Ln.v.w], down, [q, k, v], "norm", residual=hbuf[cur], gamma=Ln.g1, eps=EPS, residual_out=hbuf[cur ^ 1])
        torch.cuda.synchronize()
        assert np.array_equal(hbuf[cur].cpu().numpy(), host(o) + hn), f"layer {li}: residual stream (attention half)"
        cur ^= 1
        hn = check_segment(L, Ln, host(attn), host(o), host(gate), host(up), host(down), hn, hbuf[cur].cpu().numpy(), [host(t) for t in (q, k, v)],
                           False, li)
    assert np.isfinite(hn).all() and np.abs(hn).max() < 1e3


# ---- 9. graph capture --------------------------------------------------------------------------------------------------------
def test_graph_capture(tm):
    import torch
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    K, Mw = 1024, 512
    m = Mat(tm, wr, 50, Mw, K)
    v = vectors(K, 50, torch.float16)
    o = poison(Mw, torch.float16)

    def call(stream=None):
        wr.fused_xf([m.w], v["x"], [o], "glu_norm", in2=v["x2"], gamma=v["gam"], eps=EPS, stream=stream)
    call()
    torch.cuda.synchronize()
    want = o.cpu().numpy().copy()
    assert np.isfinite(want).all()
    assert rel_err(want.astype(np.float32), m.oracle(np_glunorm(v["xh"], v["x2h"], v["gamh"]))) <= 2e-3
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            call(stream=s)
    for _ in range(2):
        o.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(o.cpu().numpy(), want)


# ---- 10. footprint -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,Mw,gs", [(11008, 128, 128), (64, 16, 64)])
def test_footprint(tm, K, Mw, gs):
    """guard bands around in, in2, gamma and every output, two placements, two guard patterns: nothing outside the outputs is written and
    nothing from outside an input -- a clamped lane's load among it -- reaches a result"""
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    mats = [Mat(tm, wr, 60, Mw, K, gs=gs), Mat(tm, wr, 61, Mw, K, gs=gs)]
    rng = np.random.default_rng(60)
    x, x2 = (rng.standard_normal(K).astype(np.float16) for _ in range(2))
    gam = (1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)

    def call(al):
        xd = al.inp(x, name="in")
        ops = dict(in2=al.inp(x2, name="in2"), gamma=al.inp(gam, name="gamma"), eps=EPS)
        outs = [al.out((m.Mw,), "float16", name=f"C{i}") for i, m in enumerate(mats)]
        al.arm()
        wr.fused_xf([m.w for m in mats], xd, outs, "glu_norm", **ops)

    def check_want(want):
        xt = np_glunorm(x, x2, gam)
        for i, m in enumerate(mats):
            assert rel_err(want[f"C{i}"].astype(np.float32), m.oracle(xt)) <= 2e-3
    check_footprint(call, check_want=check_want)
