"""The gate of TMAC_XF_GLU / TMAC_XF_GLU_NORM at N = 1 (include/tmac_hip.h: bits 8..15 of tmac_hip_xform::kind): relu^2 -- BitNet b1.58 2B-4T's
ffn_sub_norm(relu(gate)^2 * up) -- and the tanh-approximated GELU of GeGLU decoders, inside k_gemv_quad (tmac_hip_qgemm_fused_xf_dev).

Reference and bar, those of tests/test_gpu_xf.py: every output within 2e-3 of max |C| of the ORACLE run on the vector transformed in numpy
(np_relu2 / np_gelu of tests/xf_common.py, float32, then np_norm for kind 4), all finite.  Where that bar cannot see a defect -- the mean square of kind 4
taken over other numbers than the gate produced -- the kernel is compared bit for bit with its own NORM fed the g the tap shows; relu^2, which
is exact arithmetic, is held to exact zeros.
"""
import ctypes as C

import numpy as np
import pytest

from footprint import check_footprint
from test_gpu_xf import XF_CONFIGS, vectors
from xf_common import NP_GATE, Mat, dev, host, np_gated, np_norm, poison, rel_err

pytestmark = pytest.mark.gpu
EPS = 1e-5
E_ARG = -4
GATES = ["relu2", "gelu"]
KINDS = ["glu", "glu_norm"]


@pytest.fixture(scope="module")
def tm():
    import torch
    import tmac_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return tmac_amd


@pytest.fixture(autouse=True)
def _knobs(tm):
    L = tm.lib()
    tm.binding.check(L.tmac_hip_debug_quad_config(0, 0))
    yield
    tm.binding.check(L.tmac_hip_debug_quad_config(0, 0))


_MATS = {}


def mats_of(tm, key, specs):
    """matrices registered once per shape and shared by the cases that use it (never changed)"""
    if key not in _MATS:
        wr = tm.TMACGeMMWrapper(act_group_size=64)
        _MATS[key] = (wr, [Mat(tm, wr, seed, Mw, K, **kw) for seed, Mw, K, kw in specs])
    return _MATS[key]


def run_gated(tm, wr, mats, K, kind, gate, act_dtype, out_dtype, seed=3, label=""):
    import torch
    v = vectors(K, seed, act_dtype)
    outs = [poison(m.Mw, out_dtype) for m in mats]
    ops = dict(in2=v["x2"])
    if kind == "glu_norm":
        ops.update(gamma=v["gam"], eps=EPS)
    wr.fused_xf([m.w for m in mats], v["x"], outs, f"{kind}:{gate}", **ops)
    torch.cuda.synchronize()
    xn = np_gated(f"{kind}:{gate}", v["xh"], v["x2h"], v["gamh"], EPS)
    for i, (m, o) in enumerate(zip(mats, outs)):
        e = rel_err(host(o), m.oracle(xn))
        print(f"{kind}:{gate} {label} K={K} matrix {i}: rel err vs oracle {e:.2e}")
        assert np.isfinite(host(o)).all() and e <= 2e-3, (label, i, e)


# ---- 1. against the oracle ---------------------------------------------------------------------------------------------------
SHAPES = [
    # id, K, Mw, Mat keywords
    ("one-workgroup-8-pairs", 64, 16, dict(gs=64)),                  # nearly every lane clamped
    ("bitnet-2b4t-down-k6912", 6912, 64, dict(m_groups=1)),          # 864 pairs: P % 512 != 0, unified scale
    ("k11008", 11008, 128, {}),
    ("w4", 512, 128, dict(bits=4)),
]


@pytest.mark.parametrize("gate", GATES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,K,Mw,kw", SHAPES, ids=[s[0] for s in SHAPES])
def test_against_the_oracle(tm, name, K, Mw, kw, kind, gate):
    import torch
    wr, mats = mats_of(tm, name, [(10, Mw, K, kw)])
    run_gated(tm, wr, mats, K, kind, gate, torch.float16, torch.float16, label=name)


# ---- 2. every XF configuration -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gate", GATES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ft,wpq", XF_CONFIGS)
def test_every_xf_configuration(tm, ft, wpq, kind, gate):
    """K = 6144, 768 pairs: (512, *) has clamped lanes in its second round, (768, 3) none, (1024, 4) a quarter of its lanes"""
    import torch
    wr, mats = mats_of(tm, "k6144", [(20, 64, 6144, {})])
    tm.binding.check(tm.lib().tmac_hip_debug_quad_config(ft, wpq))
    run_gated(tm, wr, mats, 6144, kind, gate, torch.float16, torch.float16, label=f"({ft},{wpq})")


# ---- 3. dtypes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gate", GATES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("act,out", [("f16", "f16"), ("f16", "f32"), ("f32", "f16"), ("f32", "f32")])
def test_dtypes(tm, act, out, kind, gate):
    import torch
    dt = {"f16": torch.float16, "f32": torch.float32}
    wr, mats = mats_of(tm, "k1024", [(30, 256, 1024, {})])
    run_gated(tm, wr, mats, 1024, kind, gate, dt[act], dt[out], label=f"{act}->{out}")


# ---- 4. decomposition: kind 4 with a gate == NORM on the tapped g, bit for bit -----------------------------------------------
@pytest.mark.parametrize("gate", GATES)
@pytest.mark.parametrize("ft,wpq", [(512, 2), (1024, 4)])
def test_is_the_norm_of_its_own_gated_product(tm, ft, wpq, gate):
    """g as the N >= 2 tap shows it (kind GLU with the gate, the row repeated: xf_rows_g8 and k_gemv_quad share the gate's expression), fed as
    fp32 activations to kind NORM with the same gamma, no residual, in the same launch configuration: the mean square then runs over the
    same numbers in the same order.  K = 6912 (BitNet 2B-4T's down), unified scale: 864 pairs in rounds of 512 or 1024, clamped lanes in the
    last.  The 2e-3 bar cannot make this check: a gate applied to the sum but not to the product, or a clamped lane in the sum, hides in it."""
    import torch
    K = 6912
    wr, (m,) = mats_of(tm, "bitnet-2b4t-down-k6912", [(10, 64, K, dict(m_groups=1))])
    rng = np.random.default_rng(K)
    x, x2 = (rng.standard_normal(K).astype(np.float16) for _ in range(2))
    gam = dev((1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32))
    xd, x2d = dev(x), dev(x2)
    gt = poison(2 * K, torch.float32).view(2, K)
    wr.xf_rows_tap(xd.repeat(2).view(2, K).contiguous(), gt, f"glu:{gate}", K, 2, in2=x2d.repeat(2).view(2, K).contiguous())
    torch.cuda.synchronize()
    g = gt.cpu().numpy()
    assert np.array_equal(g[0], g[1]) and np.isfinite(g).all()
    gh = NP_GATE[gate](x, x2)
    if gate == "relu2":
        assert np.array_equal(g[0], gh)
    else:
        assert rel_err(g[0], gh) <= 1e-5
    tm.binding.check(tm.lib().tmac_hip_debug_quad_config(ft, wpq))
    a, b = poison(m.Mw, torch.float32), poison(m.Mw, torch.float32)
    wr.fused_xf([m.w], xd, [a], f"glu_norm:{gate}", in2=x2d, gamma=gam, eps=EPS)
    wr.fused_xf([m.w], gt[0].contiguous(), [b], "norm", gamma=gam, eps=EPS)
    torch.cuda.synchronize()
    ah, bh = a.cpu().numpy(), b.cpu().numpy()
    assert np.isfinite(ah).all()
    print(f"{gate} ({ft},{wpq}): kind 4 vs NORM on the tapped g: {int((ah != bh).sum())} of {ah.size} outputs differ, max |diff| {np.abs(ah - bh).max():.3e}")
    assert np.array_equal(ah, bh)
    assert rel_err(ah, m.oracle(np_norm(g[0], gam.cpu().numpy(), EPS))) <= 2e-3


# ---- 5. relu^2 of a negative vector: exact zeros -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("act", ["f16", "f32"])
@pytest.mark.parametrize("flavour", ["per-group", "unified"])
def test_relu2_of_negative_inputs_is_exactly_zero(tm, flavour, act, kind):
    """`in` all negative: g = 0 * in2 = 0 exactly, so every output is exactly 0 and finite -- nothing from 0 * rsq(eps) in kind 4, no NaN from the
    table build's guard against a zero scale"""
    import torch
    dt = {"f16": torch.float16, "f32": torch.float32}[act]
    K = 1024
    if flavour == "per-group":
        wr, (m,) = mats_of(tm, "k1024", [(30, 256, K, {})])
    else:
        wr, (m,) = mats_of(tm, "k1024-unified", [(31, 256, K, dict(m_groups=1))])
    assert not m.oracle(np.zeros(K, dtype=np.float32)).any(), "the oracle on a zero vector is zero"
    v = vectors(K, 40, dt)
    xneg = (-v["x"].float().abs() - 0.25).to(dt)
    ops = dict(in2=v["x2"])
    if kind == "glu_norm":
        ops.update(gamma=v["gam"], eps=EPS)
    for out_dtype in (torch.float16, torch.float32):
        o = poison(m.Mw, out_dtype)
        wr.fused_xf([m.w], xneg, [o], f"{kind}:relu2", **ops)
        torch.cuda.synchronize()
        oh = host(o)
        assert np.isfinite(oh).all() and not oh.any(), (flavour, act, kind, out_dtype, np.abs(oh).max())


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(tm):
    """gate bits on a kind that takes none, a gate that is none of the three and a bit above 15 are TMAC_HIP_E_ARG naming the gate, at N = 1 and
    N = 2; 3 with a gate is still no kind; nothing is launched (the outputs keep their poison) and the next valid call runs"""
    import torch
    L = tm.lib()
    K, Mw = 1024, 256
    wr, (m,) = mats_of(tm, "k1024", [(30, Mw, K, {})])
    v = vectors(K, 70, torch.float32)
    x2 = torch.cat([v["x"], v["x"]]).contiguous()
    in2_2 = torch.cat([v["x2"], v["x2"]]).contiguous()
    o = poison(2 * Mw, torch.float32)
    wa, ca = (C.c_void_p * 1)(m.w.handle.value), (C.c_void_p * 1)(o.data_ptr())

    def raw(kind, N):
        xf = tm.binding.XForm()
        xf.kind, xf.in2, xf.gamma, xf.eps = kind, in2_2.data_ptr(), v["gam"].data_ptr(), EPS
        if N == 1:
            rc = L.tmac_hip_qgemm_fused_xf_dev(wa, 1, x2.data_ptr(), tm.F32, C.byref(xf), ca, tm.F32, None)
        else:
            rc = L.tmac_hip_qgemm_fused_xf_rows_dev(wa, 1, x2.data_ptr(), tm.F32, C.byref(xf), ca, tm.F32, N, None)
        return rc, L.tmac_hip_last_error().decode()

    def untouched():
        torch.cuda.synchronize()
        return bool(torch.isnan(o).all())
    for N in (1, 2):
        for kind in (1 | 0x100, 2 | 0x300, 2 | 0x10000, 4 | 0x300, 0x100, 4 | 0x8000):
            rc, msg = raw(kind, N)
            assert rc == E_ARG and "gate" in msg and untouched(), (N, hex(kind), rc, msg)
        rc, msg = raw(3 | 0x100, N)
        assert rc == E_ARG and "unknown transform kind" in msg and "gate" not in msg and untouched(), (N, rc, msg)
    rc, msg = raw(4 | 0x100, 1)
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert rel_err(o.cpu().numpy()[:Mw], m.oracle(np_gated("glu_norm:relu2", v["xh"], v["x2h"], v["gamh"], EPS))) <= 2e-3
    assert bool(torch.isnan(o[Mw:]).all())


def test_the_silu_alias_is_the_bare_kind(tm):
    """":silu" is the bare name: the same bits"""
    import torch
    wr, (m,) = mats_of(tm, "k1024", [(30, 256, 1024, {})])
    v = vectors(1024, 5, torch.float16)
    for kind, ops in (("glu", {}), ("glu_norm", dict(gamma=v["gam"], eps=EPS))):
        a, b = poison(m.Mw, torch.float32), poison(m.Mw, torch.float32)
        wr.fused_xf([m.w], v["x"], [a], kind, in2=v["x2"], **ops)
        wr.fused_xf([m.w], v["x"], [b], kind + ":silu", in2=v["x2"], **ops)
        torch.cuda.synchronize()
        assert np.isfinite(a.cpu().numpy()).all() and np.array_equal(a.cpu().numpy(), b.cpu().numpy())


# ---- 7. footprint ------------------------------------------------------------------------------------------------------------
def test_footprint(tm):
    """guard bands around in, in2, gamma and every output: nothing outside the outputs is written and nothing from outside an input -- a
    clamped lane's load among it (K = 3200: 400 pairs under 512 threads) -- reaches a result"""
    K, Mw = 3200, 128
    wr, mats = mats_of(tm, "k3200-x2", [(60, Mw, K, {}), (61, Mw, K, {})])
    rng = np.random.default_rng(60)
    x, x2 = (rng.standard_normal(K).astype(np.float16) for _ in range(2))
    gam = (1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)

    def call(al):
        xd = al.inp(x, name="in")
        ops = dict(in2=al.inp(x2, name="in2"), gamma=al.inp(gam, name="gamma"), eps=EPS)
        outs = [al.out((m.Mw,), "float16", name=f"C{i}") for i, m in enumerate(mats)]
        al.arm()
        wr.fused_xf([m.w for m in mats], xd, outs, "glu_norm:relu2", **ops)

    def check_want(want):
        xt = np_gated("glu_norm:relu2", x, x2, gam, EPS)
        for i, m in enumerate(mats):
            assert rel_err(want[f"C{i}"].astype(np.float32), m.oracle(xt)) <= 2e-3
    check_footprint(call, check_want=check_want)
