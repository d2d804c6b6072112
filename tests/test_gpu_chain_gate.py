"""The gate of TMAC_XF_GLU / TMAC_XF_GLU_NORM inside k_decode_chain (tmac_hip_chain_xform, include/tmac_hip.h): the reader form (the call
that consumes the GLU evaluates gate(in) * in2 in its LUT build; the gate travels in ChainOp::xf_flags) and the producer form (the gate/up
call publishes gate(gate) * up itself; the gate travels in ChainOp::epi).  Launches that hold a gate other than silu run instances of the
kernel of their own.

Reference and bar, those of tests/test_gpu_chain_xform.py and tests/test_gpu_xf_glunorm.py: every output within 2e-3 of max |C| of the
oracle on the vector transformed in numpy -- g rounded to fp16 where the chain hands it over as fp16 -- and the residual stream bit for
bit.  relu^2 is exact, so the integers the kernel accumulates behind a reader-form relu^2 are held to the oracle's, array_equal
(tmac_hip_chain_set_tap; the tap does not cover the producer form, whose launches refuse it as before).
"""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from test_gpu_xf_glunorm import LAYER_SHAPES, layers_of, outside
from xf_common import KF, NP_GATE, Mat, dev, host, np_gated, np_norm, rel_err

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
    tm.binding.check(L.tmac_hip_debug_chain_grid(0))


_EXT = {}


def ext_mats(tm):
    if not _EXT:
        wr = tm.TMACGeMMWrapper(act_group_size=64)
        _EXT["v"] = (wr, [Mat(tm, wr, 1 + i, 512, 1024) for i in range(3)])
    return _EXT["v"]


# ---- 1. reader form ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [0, 7])
def test_reader_form_on_external_vectors(tm, grid):
    """three GLUs of one recording, one per gate, on vectors in memory: the consuming call applies the gate inside its LUT build.  grid 7:
    fewer workgroups than CUs.  Then the integers behind the relu^2 call from the launch's own tap, against the oracle's."""
    import torch
    tm.binding.check(tm.lib().tmac_hip_debug_chain_grid(grid))
    wr, mats = ext_mats(tm)
    K, Mw = 1024, 512
    rng = np.random.default_rng(11)
    x, x2 = (dev(rng.standard_normal(K).astype(np.float32)).half() for _ in range(2))
    outs = [torch.zeros(Mw, dtype=torch.float16, device="cuda") for _ in range(3)]
    kinds = ["glu:relu2", "glu:gelu", "glu:silu"]
    with wr.record_chain() as rec:
        for m, o, kind in zip(mats, outs, kinds):
            wr.chain_xform(kind, in2=x2)
            wr.fused([m.w], x, [o], 1)
    chain = rec.chain
    try:
        assert not chain.stream
        xh, x2h = host(x), host(x2)
        silu = lambda a, b: (a / (np.float32(1.0) + np.exp(-a))).astype(np.float32) * b
        want_x = [NP_GATE["relu2"](xh, x2h), NP_GATE["gelu"](xh, x2h), silu(xh, x2h)]
        for rep in range(2):
            for o in outs:
                o.zero_()
            chain.launch()
            torch.cuda.synchronize()
            assert chain.status() == 0
            for m, o, xt, kind in zip(mats, outs, want_x, kinds):
                e = rel_err(host(o), m.oracle(xt))
                print(f"reader form {kind} grid={grid}: rel err vs oracle {e:.2e}")
                assert np.isfinite(host(o)).all() and e <= 2e-3, (kind, e)
        # the tap's instance of the kernel: the integers of op 0 (relu^2: x is exact, so the tables are the oracle's)
        total, _ = chain.tap_layout(3)
        buf = torch.full((total,), -(2 ** 31), dtype=torch.int32, device="cuda")
        chain.set_tap(buf)
        try:
            chain.launch()
            torch.cuda.synchronize()
            assert chain.status() == 0
        finally:
            chain.set_tap(None)
        m = mats[0]
        off, cnt = chain.tap_layout(0)
        assert cnt == Mw * (K // 64)
        q, _, _ = orc.preprocessor(want_x[0][None, :], 64)
        PS = orc.partial_sums(m.A, q[0], Mw, K, m.bits, m.bm, KF, 64)
        r = np.arange(Mw)
        want = sum(PS[(r // 8) * 8 * m.bits + p * 8 + (r % 8)].astype(np.int64) << p for p in range(m.bits))
        assert np.array_equal(buf.cpu().numpy()[off:off + cnt].reshape(Mw, K // 64).astype(np.int64), want), "integer tap behind a relu^2 GLU != oracle"
        assert rel_err(host(outs[1]), mats[1].oracle(want_x[1])) <= 2e-3
    finally:
        chain.free()


# ---- 2. / 3. a decoder segment, recorded and call by call --------------------------------------------------------------------
def check_segment(kind, L, Ln, a, on, g, u, d, hn, h_out, qkv, handed_over_f16):
    """every mpGEMM of the segment against the oracle on what it consumed; the residual stream bit for bit"""
    assert rel_err(on, L.o.oracle(a)) <= 2e-3, "o"
    t2 = on + hn
    x2 = np_norm(t2, L.g2.cpu().numpy(), EPS)
    eg, eu = rel_err(g, L.gate.oracle(x2)), rel_err(u, L.up.oracle(x2))
    assert eg <= 2e-3 and eu <= 2e-3, f"gate {eg:.2e} up {eu:.2e}"
    ed = rel_err(d, L.down.oracle(np_gated(kind, g, u, L.g3.cpu().numpy(), EPS, handed_over_f16)))
    print(f"{kind}: down behind the gated product rel err vs oracle {ed:.2e}")
    assert np.isfinite(d).all() and ed <= 2e-3, f"down {ed:.2e}"
    t3 = d + t2
    assert np.array_equal(h_out, t3), "residual stream"
    x3 = np_norm(t3, Ln.g1.cpu().numpy(), EPS)
    for m, got in zip((Ln.q, Ln.k, Ln.v), qkv):
        assert rel_err(got, m.oracle(x3)) <= 2e-3, "next q/k/v"


def segment_inputs(tm, shape):
    import torch
    H, F, kw = LAYER_SHAPES[shape]
    wr, layers = layers_of(tm, shape)
    rng = np.random.default_rng(5)
    f16 = lambda n: torch.zeros(n, dtype=torch.float16, device="cuda")
    q, k, v = (dev(rng.standard_normal(H).astype(np.float16)) for _ in range(3))
    attn = f16(H)
    outside(attn, q, k, v)
    b = dict(o=f16(H), gate=f16(F), up=f16(F), down=f16(H), q=f16(H), k=f16(H), v=f16(H))
    h = dev(rng.standard_normal(H).astype(np.float32))
    return wr, layers[0], layers[1], H, F, attn, b, h


def run_recorded(tm, shape, kind, handed_over_f16):
    import torch
    wr, L, Ln, H, F, attn, b, h = segment_inputs(tm, shape)
    h_out = torch.zeros(H, dtype=torch.float32, device="cuda")
    ops = dict(in2=b["up"], gamma=L.g3, eps=EPS) if kind.startswith("glu_norm") else dict(in2=b["up"])
    with wr.record_chain() as rec:
        wr.fused([L.o.w], attn, [b["o"]], 1)
        wr.chain_xform("norm", residual=h, gamma=L.g2, eps=EPS, keep=True)
        wr.fused([L.gate.w, L.up.w], b["o"], [b["gate"], b["up"]], 1)
        wr.chain_xform(kind, **ops)
        wr.fused([L.down.w], b["gate"], [b["down"]], 1)
        wr.chain_xform("norm", residual=wr.CARRY, gamma=Ln.g1, eps=EPS, residual_out=h_out)
        wr.fused([Ln.q.w, Ln.k.w, Ln.v.w], b["down"], [b["q"], b["k"], b["v"]], 1)
    chain = rec.chain
    try:
        assert not chain.stream, "a recording with transforms is a decode chain"
        nops = C.c_int32(0)
        tm.binding.check(tm.lib().tmac_hip_chain_info(chain.handle, 0, C.byref(nops), None, None, None))
        assert nops.value == 4, "one segment: four calls, one launch"
        for rep in range(2):
            chain.launch()
            torch.cuda.synchronize()
            assert chain.status() == 0, "a hand-off timed out"
            check_segment(kind, L, Ln, host(attn), host(b["o"]), host(b["gate"]), host(b["up"]), host(b["down"]), h.cpu().numpy(), h_out.cpu().numpy(),
                          [host(b[n]) for n in "qkv"], handed_over_f16)
        if handed_over_f16:      # the producer form deals rows in gate / up pairs: no tap, as before
            buf = torch.zeros(16, dtype=torch.int32, device="cuda")
            with pytest.raises(tm.binding.TMACHipError) as ei:
                chain.set_tap(buf)
            assert ei.value.code == E_NOMATCH
    finally:
        chain.free()


@pytest.mark.parametrize("glu_in_producer", [1, 0])
def test_llama_shaped_layer_with_gelu(tm, glu_in_producer, monkeypatch):
    """(H, F) = (1024, 2816), GeGLU: the gate/up call publishes gelu(gate) * up (producer form, fp16 like every handed-over vector), or --
    TMAC_CHAIN_GLU_EPILOGUE=0 -- the down projection evaluates it in fp32 from the two handed-over vectors (reader form)"""
    monkeypatch.setenv("TMAC_CHAIN_GLU_EPILOGUE", str(glu_in_producer))
    run_recorded(tm, "llama-shaped", "glu:gelu", handed_over_f16=bool(glu_in_producer))


def test_bitnet_2b4t_shaped_segment_recorded(tm):
    """(H, F) = (640, 1728), unified scales, ffn_sub_norm(relu(gate)^2 * up) in front of down: one launch for the whole segment"""
    run_recorded(tm, "bitnet-shaped", "glu_norm:relu2", handed_over_f16=True)


def test_bitnet_2b4t_shaped_segment_call_by_call(tm):
    """the same segment issued one by one (what a caller does when tmac_hip_chain_end refuses): kind 4 | relu^2 in front of down"""
    import torch
    wr, L, Ln, H, F, attn, b, h = segment_inputs(tm, "bitnet-shaped")
    h1, h2 = torch.zeros(H, dtype=torch.float32, device="cuda"), torch.zeros(H, dtype=torch.float32, device="cuda")
    wr.fused([L.o.w], attn, [b["o"]], 1)
    wr.fused_xf([L.gate.w, L.up.w], b["o"], [b["gate"], b["up"]], "norm", residual=h, gamma=L.g2, eps=EPS, residual_out=h1)
    wr.fused_xf([L.down.w], b["gate"], [b["down"]], "glu_norm:relu2", in2=b["up"], gamma=L.g3, eps=EPS)
    wr.fused_xf([Ln.q.w, Ln.k.w, Ln.v.w], b["down"], [b["q"], b["k"], b["v"]], "norm", residual=h1, gamma=Ln.g1, eps=EPS, residual_out=h2)
    torch.cuda.synchronize()
    assert np.array_equal(h1.cpu().numpy(), host(b["o"]) + h.cpu().numpy())
    check_segment("glu_norm:relu2", L, Ln, host(attn), host(b["o"]), host(b["gate"]), host(b["up"]), host(b["down"]), h.cpu().numpy(), h2.cpu().numpy(),
                  [host(b[n]) for n in "qkv"], False)


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------
def test_reader_form_glu_norm_is_still_refused(tm):
    """vectors in memory: tmac_hip_chain_end returns TMAC_HIP_E_NOMATCH naming GLU_NORM, whatever the gate; nothing was launched"""
    import torch
    wr, L, Ln, H, F, attn, b, h = segment_inputs(tm, "bitnet-shaped")
    rng = np.random.default_rng(3)
    gate, up = (dev(rng.standard_normal(F).astype(np.float16)) for _ in range(2))
    with pytest.raises(tm.binding.TMACHipError) as ei:
        with wr.record_chain():
            wr.fused_xf([L.down.w], gate, [b["down"]], "glu_norm:relu2", in2=up, gamma=L.g3, eps=EPS)
            wr.fused([L.o.w], b["down"], [b["o"]], 1)      # (a hand-off: not a candidate for stream mode)
    assert ei.value.code == E_NOMATCH and "GLU_NORM" in str(ei.value), str(ei.value)
    torch.cuda.synchronize()
    assert float(b["down"].abs().max()) == 0.0, "recorded and refused: nothing was launched"


def test_gate_bits_on_a_norm_are_refused_and_nothing_stays_pending(tm):
    """tmac_hip_chain_xform: TMAC_HIP_E_ARG naming the gate -- also for a gate that is none of the three on a GLU; the next recorded call
    carries no transform: the recording is a plain pair of calls and gives their bits"""
    import torch
    wr, mats = ext_mats(tm)
    K, Mw = 1024, 512
    rng = np.random.default_rng(21)
    x = dev(rng.standard_normal(K).astype(np.float16))
    x2 = dev(rng.standard_normal(K).astype(np.float16))
    gam = dev((1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32))
    o0 = torch.zeros(K // 2, dtype=torch.float16, device="cuda")
    want = torch.zeros(Mw, dtype=torch.float16, device="cuda")
    wr.fused([mats[0].w], x, [want], 1)
    o = torch.zeros(Mw, dtype=torch.float16, device="cuda")
    with wr.record_chain() as rec:
        for kind, ops in ((1 | 0x100, dict(gamma=gam)), (2 | 0x300, dict(in2=x2)), (2 | 0x10000, dict(in2=x2)), (4 | 0x400, dict(in2=x2, gamma=gam))):
            with pytest.raises(tm.binding.TMACHipError) as ei:
                wr.chain_xform(kind, **ops)
            assert ei.value.code == E_ARG and "gate" in str(ei.value), (hex(kind), str(ei.value))
        with pytest.raises(tm.binding.TMACHipError) as ei:
            wr.chain_xform(3 | 0x100, in2=x2)
        assert ei.value.code == E_ARG and "unknown transform kind" in str(ei.value)
        wr.fused([mats[0].w], x, [o], 1)
        wr.fused([mats[1].w], x, [o0.new_zeros(Mw)], 1)
    chain = rec.chain
    try:
        chain.launch()
        torch.cuda.synchronize()
        if not chain.stream:
            assert chain.status() == 0
        assert rel_err(host(o), mats[0].oracle(host(x))) <= 1e-3
        assert rel_err(host(o), host(want)) <= 1e-3, "a pending transform would have changed the call"
    finally:
        chain.free()
