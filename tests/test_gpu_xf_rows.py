"""Vector transforms for N > 1 activation rows: tmac_hip_qgemm_fused_xf_rows_dev and its tap tmac_hip_debug_xf_rows (include/tmac_hip.h) --
residual add + RMSNorm, or silu(in) * in2, applied inside the activation load of the N > 1 LUT builders (k_lut_image, k_preprocess_pairs,
k_preprocess_pairs_row), behind one row pass (k_xf_rows) that writes residual_out and the rows' 1 / rms.

Bars:
  * the transform: NORM without gamma is fp32 addition, bit for bit numpy's; a row of an N-row call is that row of an N = 1 tap call, bit
    for bit; NORM with gamma within (K / 2 + 16) * 2^-24 of the float64 formula, element by element (a K-term fp32 sum of non-negative
    terms in any order, plus the single roundings behind it);
  * the LUT path: the outputs are those of the plain call on the same route fed the tapped x as fp32 activations, bit for bit;
  * every output within 2e-3 of max |C| of the oracle on the numpy-transformed rows (tests/test_gpu_xf.py's bar).

Shapes: Mw = 16 (the smallest 2-bit registration), one flavour with two matrices (16 + 32); K = 128 and 2112 (264 pairs: beyond the 256
threads of a k_preprocess_pairs workgroup), K = 4160 with unified scales (the second pair per thread of k_preprocess_pairs_row); N = 2, 3
(a k_gemv_rows group with a remainder), 33 (beyond k_lut_image's 32-row workgroup, 31 clamped padding rows behind it), 65 (the second
64-row tile).  W2 with zero points has gs = 128 at K = 128 and gs = 64 at K = 2112: 2112 = 33 x 64 has no group of 128.
"""
import ctypes as C

import numpy as np
import pytest

from footprint import check_footprint
from xf_common import Mat, dev, host, np_glu, np_norm, poison, rel_err

pytestmark = pytest.mark.gpu
E_ARG, E_NOMATCH, E_RUNTIME = -4, -1, -3
EPS = 1e-5


@pytest.fixture(scope="module")
def tm():
    import torch
    import tmac_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return tmac_amd


FLAVOURS = {
    # name: (K, Mw list, Mat keywords)
    "w2zp-k128": (128, [16, 32], dict(bits=2, gs=128)),
    "w2zp-k2112": (2112, [16], dict(bits=2, gs=64)),
    "w4-k128": (128, [16], dict(bits=4, gs=128, zp=False)),
    "bitnet-k4160": (4160, [16], dict(bits=2, m_groups=1)),
}


def make_mats(tm, flavour, seed=10):
    K, mws, kw = FLAVOURS[flavour]
    wr = tm.TMACGeMMWrapper(act_group_size=K if kw.get("m_groups", -1) >= 1 else 64)
    return wr, K, [Mat(tm, wr, seed + i, mw, K, **kw) for i, mw in enumerate(mws)]


_VEC = {}


def vectors(N, K, act, seed=7):
    """in, in2 [N][K] (act dtype), residual [N][K], gamma [K] (fp32): host values, computed once per (N, K, dtype) and never changed"""
    key = (N, K, act, seed)
    if key not in _VEC:
        rng = np.random.default_rng(seed + 1000 * N + K)
        dt = np.float16 if act == "f16" else np.float32
        x, x2 = (rng.standard_normal((N, K)).astype(dt) for _ in range(2))
        res = rng.standard_normal((N, K)).astype(np.float32)
        gam = (1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)
        _VEC[key] = dict(x=x, x2=x2, res=res, gam=gam)
    return _VEC[key]


def on_device(v):
    return {k: dev(a) for k, a in v.items()}


def set_route(tm, route):
    """every knob the routes differ in, set or back at its default (32 rows counts as "threshold not set")"""
    L = tm.lib()
    tm.binding.check(L.tmac_hip_set_gemm_min_n(2 if route in ("planes", "onehot") else 32))
    tm.binding.check(L.tmac_hip_debug_gemm_kernel(1 if route == "onehot" else 0))
    tm.binding.check(L.tmac_hip_debug_rows_kernel(2 if route == "rows" else 0))


ROUTE_CODE = {"planes": (0, 1), "onehot": (1, 2), "rows": (3, 2), "loop": (7, 2)}      # (enum Route, LUT build) of tmac_hip_debug_xf_rows_plan


def planned_route(tm, mats, outs, N):
    n = len(mats)
    wa = (C.c_void_p * n)(*[m.w.handle.value for m in mats])
    ca = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
    r, l = C.c_int32(-1), C.c_int32(-1)
    tm.binding.check(tm.lib().tmac_hip_debug_xf_rows_plan(wa, n, ca, N, C.byref(r), C.byref(l)))
    return r.value, l.value


def rows_launches(tm):
    n = C.c_uint64(0)
    tm.binding.check(tm.lib().tmac_hip_debug_rows_stats(C.byref(n)))
    return n.value


def tap(tm, wr, d, kind, K, N, act, with_rout=False):
    import torch
    x = poison((N, K), torch.float32)
    rout = poison((N, K), torch.float32) if with_rout else None
    if kind == "glu":
        wr.xf_rows_tap(d["x"], x, "glu", K, N, in2=d["x2"])
    elif kind == "add":
        wr.xf_rows_tap(d["x"], x, "norm", K, N, residual=d["res"], residual_out=rout)
    else:
        wr.xf_rows_tap(d["x"], x, "norm", K, N, residual=d["res"], gamma=d["gam"], eps=EPS, residual_out=rout)
    torch.cuda.synchronize()
    return x, rout


def xf_call(wr, mats, d, kind, N, outs, rout=None, stream=None):
    ws = [m.w for m in mats]
    if kind == "glu":
        wr.fused_xf_rows(ws, d["x"], outs, "glu", N, in2=d["x2"], stream=stream)
    elif kind == "add":
        wr.fused_xf_rows(ws, d["x"], outs, "norm", N, residual=d["res"], residual_out=rout, stream=stream)
    else:
        wr.fused_xf_rows(ws, d["x"], outs, "norm", N, residual=d["res"], gamma=d["gam"], eps=EPS, residual_out=rout, stream=stream)


def np_transform(v, kind):
    if kind == "glu":
        return np_glu(v["x"], v["x2"])
    t = v["x"].astype(np.float32) + v["res"]
    return t if kind == "add" else np_norm(t, v["gam"], EPS)


def plain_same_route(tm, wr, mats, route, xt, N, out_dtype):
    """the plain call of the route on the fp32 rows xt (device): the fused entry point for the GEMMs and the rows kernel, the split entry
    points on a caller's workspace for the row loop"""
    import torch
    outs = [poison((N, m.Mw), out_dtype) for m in mats]
    if route == "loop":
        wr.set_workspace(mats[0].K, N)
        wr.llama_cpp_init(xt, mats[0].Mw, mats[0].K, N, mats[0].bits, act_group_size=mats[0].ags)
        for m, o in zip(mats, outs):
            wr.llama_cpp_compute(m.w, o, N)
    else:
        wr.fused([m.w for m in mats], xt, outs, N)
    torch.cuda.synchronize()
    return outs


# ---- 1. the transform, exactly ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["f16", "f32"])
@pytest.mark.parametrize("N,K", [(3, 128), (33, 2112)])
def test_add_only_is_fp32_addition(tm, act, N, K):
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    v = vectors(N, K, act)
    x, rout = tap(tm, wr, on_device(v), "add", K, N, act, with_rout=True)
    t = v["x"].astype(np.float32) + v["res"]
    assert np.array_equal(x.cpu().numpy(), t) and np.array_equal(rout.cpu().numpy(), t)


@pytest.mark.parametrize("act", ["f16", "f32"])
@pytest.mark.parametrize("kind", ["norm", "glu"])
@pytest.mark.parametrize("N,K", [(3, 128), (65, 2112), (2, 4160)])
def test_a_row_is_a_row(tm, act, kind, N, K):
    """row n of an N-row tap == the N = 1 tap on that row alone; NORM with gamma also within the fp32 sum's bound of the float64 formula"""
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    v = vectors(N, K, act)
    d = on_device(v)
    x, _ = tap(tm, wr, d, kind, K, N, act)
    xh = x.cpu().numpy()
    for n in sorted({0, 1, N // 2, N - 1}):
        d1 = dict(x=d["x"][n:n + 1], x2=d["x2"][n:n + 1], res=d["res"][n:n + 1], gam=d["gam"])
        x1, _ = tap(tm, wr, d1, kind, K, 1, act)
        assert np.array_equal(x1.cpu().numpy()[0], xh[n]), (kind, n)
    if kind == "norm":
        t = (v["x"].astype(np.float32) + v["res"]).astype(np.float64)
        x64 = t * v["gam"].astype(np.float64)[None, :] / np.sqrt((t ** 2).mean(axis=1) + EPS)[:, None]
        excess = np.abs(xh.astype(np.float64) - x64) / ((K / 2 + 16) * 2.0 ** -24 * np.abs(x64))
        print(f"norm N={N} K={K} {act}: max |x - x64| / bound = {excess.max():.3f}")
        assert (excess <= 1.0).all(), float(excess.max())
    else:
        assert rel_err(xh, np_glu(v["x"], v["x2"])) <= 1e-5


# ---- 2. / 3. the LUT path exactly, and the oracle --------------------------------------------------------------------------------
ROUTE_N = [("planes", 33), ("planes", 65), ("onehot", 33), ("rows", 3), ("loop", 2), ("loop", 3)]


def run_route(tm, flavour, route, N, act="f16", out="f16", kinds=("norm", "glu")):
    import torch
    dt = {"f16": torch.float16, "f32": torch.float32}
    wr, K, mats = make_mats(tm, flavour)
    set_route(tm, route)
    v = vectors(N, K, act)
    d = on_device(v)
    for kind in kinds:
        xt, _ = tap(tm, wr, d, kind, K, N, act)
        outs = [poison((N, m.Mw), dt[out]) for m in mats]
        rout = poison((N, K), torch.float32) if kind == "norm" else None
        assert planned_route(tm, mats, outs, N) == ROUTE_CODE[route], (route, planned_route(tm, mats, outs, N))
        r0 = rows_launches(tm)
        xf_call(wr, mats, d, kind, N, outs, rout)
        torch.cuda.synchronize()
        if route == "rows":
            assert rows_launches(tm) > r0, "k_gemv_rows did not run"
        else:
            assert rows_launches(tm) == r0
        if rout is not None:
            assert np.array_equal(rout.cpu().numpy(), v["x"].astype(np.float32) + v["res"]), "residual_out"
        want = plain_same_route(tm, wr, mats, route, xt, N, dt[out])
        xn = np_transform(v, kind)
        for i, (m, o, w) in enumerate(zip(mats, outs, want)):
            assert np.isfinite(host(o)).all()
            assert np.array_equal(o.cpu().numpy(), w.cpu().numpy()), (kind, route, i, "differs from the plain call on the tapped x")
            e = rel_err(host(o), m.oracle(xn))
            print(f"{flavour} {route} N={N} {kind} matrix {i}: rel err vs oracle {e:.2e}")
            assert e <= 2e-3, (kind, route, i, e)


@pytest.mark.parametrize("flavour", list(FLAVOURS))
@pytest.mark.parametrize("route,N", ROUTE_N, ids=[f"{r}-n{n}" for r, n in ROUTE_N])
def test_routes(tm, flavour, route, N):
    run_route(tm, flavour, route, N)


@pytest.mark.parametrize("flavour,route,N", [("w2zp-k128", "planes", 33), ("w2zp-k2112", "loop", 3), ("bitnet-k4160", "loop", 3), ("bitnet-k4160", "planes", 33)])
@pytest.mark.parametrize("act,out", [("f16", "f32"), ("f32", "f16"), ("f32", "f32")])
def test_dtypes(tm, act, out, flavour, route, N):
    """fp32 activations through k_lut_image, k_preprocess_pairs and k_preprocess_pairs_row (both of its outputs), fp32 outputs"""
    run_route(tm, flavour, route, N, act, out)


def test_add_only_through_the_matrices(tm):
    """NORM without gamma launches the row pass for residual_out alone, and none without it"""
    import torch
    wr, K, mats = make_mats(tm, "w2zp-k2112")
    set_route(tm, "planes")
    N = 33
    v = vectors(N, K, "f16")
    d = on_device(v)
    t = v["x"].astype(np.float32) + v["res"]
    want = plain_same_route(tm, wr, mats, "planes", dev(t), N, torch.float16)
    for with_rout in (True, False):
        outs = [poison((N, m.Mw), torch.float16) for m in mats]
        rout = poison((N, K), torch.float32) if with_rout else None
        xf_call(wr, mats, d, "add", N, outs, rout)
        torch.cuda.synchronize()
        if with_rout:
            assert np.array_equal(rout.cpu().numpy(), t)
        assert np.array_equal(outs[0].cpu().numpy(), want[0].cpu().numpy())


# ---- 4. N = 1 and "no transform" are the existing calls ------------------------------------------------------------------------------
def test_n1_and_no_transform_are_the_existing_calls(tm):
    import torch
    wr, K, mats = make_mats(tm, "w2zp-k2112")
    m = mats[0]
    v = vectors(3, K, "f16")
    d = on_device(v)
    d1 = dict(x=d["x"][:1], x2=d["x2"][:1], res=d["res"][:1], gam=d["gam"])
    for kind in ("norm", "glu"):
        a, b = poison((1, m.Mw), torch.float16), poison((1, m.Mw), torch.float16)
        ra, rb = poison((1, K), torch.float32), poison((1, K), torch.float32)
        if kind == "norm":
            wr.fused_xf([m.w], d1["x"], [a], "norm", residual=d1["res"], gamma=d1["gam"], eps=EPS, residual_out=ra)
        else:
            wr.fused_xf([m.w], d1["x"], [a], "glu", in2=d1["x2"])
        xf_call(wr, [m], d1, kind, 1, [b], rb if kind == "norm" else None)
        torch.cuda.synchronize()
        assert np.isfinite(host(a)).all() and np.array_equal(a.cpu().numpy(), b.cpu().numpy()), kind
        if kind == "norm":
            assert np.array_equal(ra.cpu().numpy(), rb.cpu().numpy())
    a, b, c = (poison((3, m.Mw), torch.float16) for _ in range(3))
    wr.fused([m.w], d["x"], [a], 3)
    wr.fused_xf_rows([m.w], d["x"], [b], None, 3)                            # xf = NULL
    xf = tm.binding.XForm()                                                  # kind = TMAC_XF_NONE
    wa, ca = (C.c_void_p * 1)(m.w.handle.value), (C.c_void_p * 1)(c.data_ptr())
    tm.binding.check(tm.lib().tmac_hip_qgemm_fused_xf_rows_dev(wa, 1, d["x"].data_ptr(), tm.F16, C.byref(xf), ca, tm.F16, 3, None))
    torch.cuda.synchronize()
    assert np.isfinite(host(a)).all()
    assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()) and np.array_equal(a.cpu().numpy(), c.cpu().numpy())


# ---- 5. footprint --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,route", [(3, "loop"), (3, "rows"), (33, "planes"), (33, "onehot")])
@pytest.mark.parametrize("kind", ["norm", "glu"])
def test_footprint(tm, N, route, kind):
    """guard bands around in, in2, residual, gamma, residual_out and every output, two placements, two guard patterns: nothing outside an
    output or residual_out is written, and no value from outside an input reaches a result (N = 33: 31 clamped padding rows)"""
    wr, K, mats = make_mats(tm, "w2zp-k2112")
    mats.append(Mat(tm, wr, 31, 32, K, bits=2, gs=64))
    set_route(tm, route)
    import torch
    assert planned_route(tm, mats, [torch.empty(1, device="cuda") for _ in mats], N) == ROUTE_CODE[route]
    v = vectors(N, K, "f16")

    def call(al):
        xd = al.inp(v["x"], name="in")
        if kind == "glu":
            ops = dict(in2=al.inp(v["x2"], name="in2"))
        else:
            ops = dict(residual=al.inp(v["res"], name="residual"), gamma=al.inp(v["gam"], name="gamma"), eps=EPS)
        outs = [al.out((N, m.Mw), "float16", name=f"C{i}") for i, m in enumerate(mats)]
        if kind == "norm":
            ops["residual_out"] = al.out((N, K), "float32", name="residual_out", tile=False)
        al.arm()
        wr.fused_xf_rows([m.w for m in mats], xd, outs, kind, N, **ops)

    def check_want(want):
        xt = np_transform(v, kind)
        for i, m in enumerate(mats):
            assert rel_err(want[f"C{i}"].astype(np.float32), m.oracle(xt)) <= 2e-3
        if kind == "norm":
            assert np.array_equal(want["residual_out"], v["x"].astype(np.float32) + v["res"])
    check_footprint(call, check_want=check_want)


def test_footprint_unified_scales(tm):
    """the row-wise pair build: K = 4160, N = 33 through k_gemm_planes_us' image"""
    wr, K, mats = make_mats(tm, "bitnet-k4160")
    set_route(tm, "planes")
    N = 33
    v = vectors(N, K, "f16")

    def call(al):
        xd = al.inp(v["x"], name="in")
        res, gam = al.inp(v["res"], name="residual"), al.inp(v["gam"], name="gamma")
        outs = [al.out((N, m.Mw), "float16", name=f"C{i}") for i, m in enumerate(mats)]
        rout = al.out((N, K), "float32", name="residual_out", tile=False)
        al.arm()
        wr.fused_xf_rows([m.w for m in mats], xd, outs, "norm", N, residual=res, gamma=gam, eps=EPS, residual_out=rout)

    def check_want(want):
        assert rel_err(want["C0"].astype(np.float32), mats[0].oracle(np_transform(v, "norm"))) <= 2e-3
    check_footprint(call, check_want=check_want)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(tm):
    """each refusal launches nothing (outputs and residual_out keep their poison, no k_gemv_rows launch is counted) and the next valid
    call runs"""
    import torch
    L = tm.lib()
    wr, K, mats = make_mats(tm, "w2zp-k128")
    m = mats[0]
    N = 3
    tm.binding.check(L.tmac_hip_debug_rows_kernel(2))          # a launch of the planned kernel would be counted
    v = vectors(N, K, "f32")
    d = on_device(v)
    o, rout = poison((N, m.Mw), torch.float32), poison(N * K + 8, torch.float32)
    wa, ca = (C.c_void_p * 1)(m.w.handle.value), (C.c_void_p * 1)(o.data_ptr())
    big = torch.zeros(2 * N * K + 8, dtype=torch.float32, device="cuda")     # for the misaligned / overlapping operands
    r0 = rows_launches(tm)

    def raw(kind, in2=None, residual=None, gamma=None, residual_out=None, B=None, c=None, w=None, n=N):
        xf = tm.binding.XForm()
        xf.kind, xf.in2, xf.residual, xf.gamma, xf.eps, xf.residual_out, xf.keep = kind, in2, residual, gamma, EPS, residual_out, 0
        carr = ca if c is None else (C.c_void_p * 1)(c)
        warr = wa if w is None else (C.c_void_p * 1)(w.handle.value)
        rc = L.tmac_hip_qgemm_fused_xf_rows_dev(warr, 1, d["x"].data_ptr() if B is None else B, tm.F32, C.byref(xf), carr, tm.F32, n, None)
        return rc, L.tmac_hip_last_error().decode()

    def untouched():
        torch.cuda.synchronize()
        return bool(torch.isnan(o).all()) and bool(torch.isnan(rout).all()) and rows_launches(tm) == r0
    rp, gp, resp = rout.data_ptr(), d["gam"].data_ptr(), d["res"].data_ptr()
    bp, NK4 = big.data_ptr(), 4 * N * K
    rc, msg = raw(1, residual=1, residual_out=rp)                        # CARRY
    assert rc == E_ARG and "CARRY" in msg and untouched()
    rc, msg = raw(2, residual_out=rp)                                    # GLU without in2
    assert rc == E_ARG and untouched()
    rc, msg = raw(3, residual_out=rp)
    assert rc == E_ARG and "kind" in msg and untouched()
    for name, kw in (("in2", dict(kind=2, in2=bp + 8)), ("residual", dict(kind=1, residual=bp + 8, residual_out=rp)),
                     ("gamma", dict(kind=1, gamma=bp + 8, residual_out=rp)), ("residual_out", dict(kind=1, residual_out=rp + 8))):
        rc, msg = raw(**kw)
        assert rc == E_ARG and name in msg and untouched(), (name, rc, msg)
    # residual_out over B_dev, residual, gamma, in2, C_dev[0]: by the whole block, and by the last 16 bytes of its N rows
    for name, kw in (("B_dev", dict(B=bp, residual_out=bp)),
                     ("B_dev", dict(B=bp, residual_out=bp + NK4 - 16)),
                     ("residual", dict(residual=bp + NK4 - 16, residual_out=bp)),
                     ("gamma", dict(gamma=bp, residual_out=bp + 4 * K - 16)),
                     ("in2", dict(in2=bp + NK4 - 16, residual_out=bp)),
                     ("C_dev[0]", dict(c=bp + NK4 - 16, residual_out=bp))):
        rc, msg = raw(1, **kw)
        assert rc == E_ARG and "overlaps " + name in msg and untouched(), (name, rc, msg)
    assert float(big.abs().max()) == 0.0
    full = dict(residual=resp, gamma=gp, residual_out=rp)
    # outside the scope: act groups of 32; fast-aggregation weights; the reference-layout variant; unified scales beyond the row-wise build
    wr32 = tm.TMACGeMMWrapper(act_group_size=32)
    m32 = Mat(tm, wr32, 71, 16, K, ags=32)
    rc, msg = raw(1, w=m32.w, **full)
    assert rc == E_NOMATCH and untouched(), (rc, msg)
    mfa = Mat(tm, wr, 72, 16, K, fa=1)
    rc, msg = raw(1, w=mfa.w, **full)
    assert rc == E_NOMATCH and untouched(), (rc, msg)
    tm.binding.check(L.tmac_hip_set_variant(3))
    rc, msg = raw(1, **full)
    assert rc == E_NOMATCH and "reference" in msg and untouched(), (rc, msg)
    tm.binding.check(L.tmac_hip_set_variant(0))
    Kb = 12288 + 64
    wrb = tm.TMACGeMMWrapper(act_group_size=Kb)
    mb = Mat(tm, wrb, 73, 16, Kb, m_groups=1)
    xb = torch.zeros((2, Kb), dtype=torch.float32, device="cuda")
    gb = torch.ones(Kb, dtype=torch.float32, device="cuda")
    rc, msg = raw(1, w=mb.w, B=xb.data_ptr(), gamma=gb.data_ptr(), n=2)
    assert rc == E_NOMATCH and "12288" in msg and untouched(), (rc, msg)
    # ... and the next valid call runs
    rc, msg = raw(1, **full)
    assert rc == 0, msg
    torch.cuda.synchronize()
    t = v["x"] + v["res"]
    assert np.array_equal(rout[:N * K].cpu().numpy().reshape(N, K), t) and bool(torch.isnan(rout[N * K:]).all())
    assert rows_launches(tm) > r0
    assert rel_err(o.cpu().numpy(), m.oracle(np_norm(t, v["gam"], EPS))) <= 2e-3


def test_refused_while_recording(tm):
    """inside record_chain() the N = 2 call is refused, and the recording builds and runs as if it had never been made"""
    import torch
    tm.binding.check(tm.lib().tmac_hip_debug_chain_config(0, 1 << 17))
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    K, Mw = 1024, 512
    m0, m1 = Mat(tm, wr, 1, K, K), Mat(tm, wr, 2, Mw, K)
    v = vectors(2, K, "f16")
    d = on_device(v)
    mid = torch.zeros(K, dtype=torch.float16, device="cuda")
    o1 = torch.zeros(Mw, dtype=torch.float16, device="cuda")
    o2 = poison((2, Mw), torch.float16)
    with wr.record_chain() as rec:
        wr.fused([m0.w], d["x"][0], [mid], 1)
        with pytest.raises(tm.binding.TMACHipError) as ei:
            wr.fused_xf_rows([m1.w], d["x"], [o2], "norm", 2, gamma=d["gam"], eps=EPS)
        assert ei.value.code == E_NOMATCH
        wr.fused([m1.w], mid, [o1], 1)             # a pending transform would turn this into a NORM
    chain = rec.chain
    nops = C.c_int32(0)
    tm.binding.check(tm.lib().tmac_hip_chain_info(chain.handle, 0, C.byref(nops), None, None, None))
    assert nops.value == 2
    chain.launch()
    torch.cuda.synchronize()
    assert chain.status() == 0 and bool(torch.isnan(o2).all())
    midh = host(mid)
    assert rel_err(midh, m0.oracle(v["x"][:1])[0]) <= 2e-3
    assert rel_err(host(o1), m1.oracle(midh[None, :])[0]) <= 2e-3
    chain.free()


def defer_stats(tm):
    s = [C.c_uint64(0) for _ in range(4)]
    tm.binding.check(tm.lib().tmac_hip_defer_stats(*[C.byref(x) for x in s]))
    return [x.value for x in s]      # flushes, cache hits, stream launches, single calls


def test_deferral(tm):
    """a queued producer of B_dev is flushed first: the result is that of in-order launches; a failed flush returns its status and
    nothing is launched"""
    import torch
    L = tm.lib()
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    K, Mw, N = 1024, 16, 2
    m0, m1 = Mat(tm, wr, 40, K, K), Mat(tm, wr, 41, Mw, K)
    v = vectors(N, K, "f16")
    d = on_device(v)

    def sequence():
        mid = d["x2"].clone()                                       # row 1 as it is, row 0 from the producer
        o = poison((N, Mw), torch.float16)
        wr.fused([m0.w], d["x"][0], [mid[0]], 1)
        wr.fused_xf_rows([m1.w], mid, [o], "norm", N, gamma=d["gam"], eps=EPS)
        torch.cuda.synchronize()
        return mid, o
    mid_w, want = sequence()
    assert np.isfinite(host(want)).all()
    assert rel_err(host(want), m1.oracle(np_norm(host(mid_w), v["gam"], EPS))) <= 2e-3
    tm.binding.check(L.tmac_hip_defer(1))
    try:
        f0 = defer_stats(tm)
        mid, o = sequence()
        f1 = defer_stats(tm)
        assert f1[0] == f0[0] + 1 and f1[3] == f0[3] + 1, "one flush, which launched the queued producer"
        assert np.array_equal(mid.cpu().numpy(), mid_w.cpu().numpy()) and np.array_equal(o.cpu().numpy(), want.cpu().numpy())
        o2 = poison((N, Mw), torch.float16)
        wr.fused([m0.w], d["x"][0], [mid[0]], 1)
        tm.binding.check(L.tmac_hip_debug_defer_fail(1))
        with pytest.raises(tm.binding.TMACHipError) as ei:
            wr.fused_xf_rows([m1.w], mid, [o2], "norm", N, gamma=d["gam"], eps=EPS)
        assert ei.value.code == E_RUNTIME and "injected" in str(ei.value)
        torch.cuda.synchronize()
        assert torch.isnan(o2).all(), "outputs keep their poison"
    finally:
        L.tmac_hip_debug_defer_fail(0)
        L.tmac_hip_defer(0)


# ---- 7. graph capture ----------------------------------------------------------------------------------------------------------------
def test_graph_capture(tm):
    import torch
    wr, K, mats = make_mats(tm, "w2zp-k2112")
    N = 4
    v = vectors(N, K, "f16")
    d = on_device(v)
    outs = [poison((N, m.Mw), torch.float16) for m in mats]
    rout = poison((N, K), torch.float32)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        xf_call(wr, mats, d, "norm", N, outs, rout, stream=s)       # eager, on the stream that will be captured: its workspace exists afterwards
    torch.cuda.synchronize()
    want, want_r = [o.cpu().numpy().copy() for o in outs], rout.cpu().numpy().copy()
    assert all(np.isfinite(w.astype(np.float32)).all() for w in want)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            xf_call(wr, mats, d, "norm", N, outs, rout, stream=s)
    for _ in range(2):
        for o in outs:
            o.fill_(float("nan"))
        rout.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert all(np.array_equal(o.cpu().numpy(), w) for o, w in zip(outs, want)) and np.array_equal(rout.cpu().numpy(), want_r)
