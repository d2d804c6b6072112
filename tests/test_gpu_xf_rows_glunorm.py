"""TMAC_XF_GLU_NORM for N >= 2 activation rows: tmac_hip_qgemm_fused_xf_rows_dev and its tap tmac_hip_debug_xf_rows (include/tmac_hip.h).  The
row pass (k_xf_rows) forms g = silu(in) * in2 per (row, pair), sums g^2 in its existing order -- a function of K alone -- and writes the
row's r; the LUT builders recompute g with the same device function and take (g * gamma) * r in place of their activation load.

Bars (those of tests/test_gpu_xf_rows.py):
  * a row of an N-row call is that row of an N = 1 tap call, bit for bit; the tap within 1e-5 (of max |x|, rel_err below: the value and the
    form tests/test_gpu_xf_rows.py holds its tap to) of np_glu followed by np_norm, row by row;
  * the LUT path: the outputs are those of the plain call on the same route fed the tapped x as fp32 activations, bit for bit;
  * every output within 2e-3 of max |C| of the oracle on the numpy-transformed rows.
N = 5 for the small routes (k_gemm_onehot, k_gemv_rows forced, the row loop), N = 70 for k_gemm_planes: a second, padded tile whose rows
70..127 are clamped.
"""
import ctypes as C

import numpy as np
import pytest

from footprint import check_footprint
from test_gpu_xf_rows import EPS, FLAVOURS, ROUTE_CODE, make_mats, on_device, plain_same_route, planned_route, rows_launches, set_route, vectors
from xf_common import Mat, host, np_glu, np_norm, poison, rel_err

pytestmark = pytest.mark.gpu
E_ARG, E_NOMATCH = -4, -1


@pytest.fixture(scope="module")
def tm():
    import torch
    import tmac_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return tmac_amd


@pytest.fixture(autouse=True)
def _default_route(tm):
    yield
    set_route(tm, "loop")           # every knob of the routes back at its default


def np_glunorm_rows(v):
    return np_norm(np_glu(v["x"], v["x2"]), v["gam"], EPS)


def tap4(wr, d, K, N):
    import torch
    x = poison((N, K), torch.float32)
    wr.xf_rows_tap(d["x"], x, "glu_norm", K, N, in2=d["x2"], gamma=d["gam"], eps=EPS)
    torch.cuda.synchronize()
    return x


# ---- the transform ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["f16", "f32"])
@pytest.mark.parametrize("K", [3200, 11008])
@pytest.mark.parametrize("N", [2, 5, 70])
def test_a_row_is_a_row(tm, act, K, N):
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    v = vectors(N, K, act)
    d = on_device(v)
    xh = tap4(wr, d, K, N).cpu().numpy()
    assert np.isfinite(xh).all()
    for n in sorted({0, 1, N // 2, N - 1}):
        d1 = dict(x=d["x"][n:n + 1], x2=d["x2"][n:n + 1], gam=d["gam"])
        assert np.array_equal(tap4(wr, d1, K, 1).cpu().numpy()[0], xh[n]), n
    e = rel_err(xh, np_glunorm_rows(v))
    print(f"glu_norm tap N={N} K={K} {act}: rel err vs numpy {e:.2e}")
    assert e <= 1e-5, e


# ---- the LUT path exactly, and the oracle ----------------------------------------------------------------------------------------
ROUTE_N = [("planes", 70), ("onehot", 5), ("rows", 5), ("loop", 5)]


@pytest.mark.parametrize("flavour", list(FLAVOURS))
@pytest.mark.parametrize("route,N", ROUTE_N, ids=[f"{r}-n{n}" for r, n in ROUTE_N])
def test_routes(tm, flavour, route, N):
    """tmac_hip_debug_xf_rows_plan knows no kinds: it answers for this call what it answers for a NORM with gamma, and that route runs"""
    import torch
    wr, K, mats = make_mats(tm, flavour)
    set_route(tm, route)
    v = vectors(N, K, "f16")
    d = on_device(v)
    xt = tap4(wr, d, K, N)
    outs = [poison((N, m.Mw), torch.float16) for m in mats]
    assert planned_route(tm, mats, outs, N) == ROUTE_CODE[route], (route, planned_route(tm, mats, outs, N))
    r0 = rows_launches(tm)
    wr.fused_xf_rows([m.w for m in mats], d["x"], outs, "glu_norm", N, in2=d["x2"], gamma=d["gam"], eps=EPS)
    torch.cuda.synchronize()
    assert (rows_launches(tm) > r0) == (route == "rows"), "k_gemv_rows runs on its route alone"
    want = plain_same_route(tm, wr, mats, route, xt, N, torch.float16)
    xn = np_glunorm_rows(v)
    for i, (m, o, w) in enumerate(zip(mats, outs, want)):
        assert np.isfinite(host(o)).all()
        assert np.array_equal(o.cpu().numpy(), w.cpu().numpy()), (route, i, "differs from the plain call on the tapped x")
        e = rel_err(host(o), m.oracle(xn))
        print(f"{flavour} {route} N={N} glu_norm matrix {i}: rel err vs oracle {e:.2e}")
        assert e <= 2e-3, (route, i, e)


def test_fp32_rows(tm):
    """fp32 in / in2 and fp32 outputs through the row loop's pair build"""
    import torch
    wr, K, mats = make_mats(tm, "w2zp-k2112")
    set_route(tm, "loop")
    N = 5
    v = vectors(N, K, "f32")
    d = on_device(v)
    xt = tap4(wr, d, K, N)
    outs = [poison((N, m.Mw), torch.float32) for m in mats]
    wr.fused_xf_rows([m.w for m in mats], d["x"], outs, "glu_norm", N, in2=d["x2"], gamma=d["gam"], eps=EPS)
    torch.cuda.synchronize()
    want = plain_same_route(tm, wr, mats, "loop", xt, N, torch.float32)
    assert np.array_equal(outs[0].cpu().numpy(), want[0].cpu().numpy())
    assert rel_err(host(outs[0]), mats[0].oracle(np_glunorm_rows(v))) <= 2e-3


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(tm):
    """TMAC_HIP_E_ARG with a message naming the field, nothing launched (poison stays, no k_gemv_rows launch is counted), and the next valid
    call runs"""
    import torch
    L = tm.lib()
    wr, K, mats = make_mats(tm, "w2zp-k128")
    m = mats[0]
    N = 3
    tm.binding.check(L.tmac_hip_debug_rows_kernel(2))
    v = vectors(N, K, "f32")
    d = on_device(v)
    o, rout = poison((N, m.Mw), torch.float32), poison(N * K, torch.float32)
    wa, ca = (C.c_void_p * 1)(m.w.handle.value), (C.c_void_p * 1)(o.data_ptr())
    big = torch.zeros(2 * N * K + 8, dtype=torch.float32, device="cuda")
    r0 = rows_launches(tm)

    def raw(kind, in2=None, residual=None, gamma=None, residual_out=None, keep=0):
        xf = tm.binding.XForm()
        xf.kind, xf.in2, xf.residual, xf.gamma, xf.eps, xf.residual_out, xf.keep = kind, in2, residual, gamma, EPS, residual_out, keep
        rc = L.tmac_hip_qgemm_fused_xf_rows_dev(wa, 1, d["x"].data_ptr(), tm.F32, C.byref(xf), ca, tm.F32, N, None)
        return rc, L.tmac_hip_last_error().decode()

    def untouched():
        torch.cuda.synchronize()
        return bool(torch.isnan(o).all()) and bool(torch.isnan(rout).all()) and rows_launches(tm) == r0
    i2, gp, resp, rp = d["x2"].data_ptr(), d["gam"].data_ptr(), d["res"].data_ptr(), rout.data_ptr()
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
    # the tap takes the same rules
    xo = poison((N, K), torch.float32)
    xf = tm.binding.XForm()
    xf.kind, xf.in2, xf.eps = 4, i2, EPS
    assert L.tmac_hip_debug_xf_rows(d["x"].data_ptr(), tm.F32, C.byref(xf), K, N, xo.data_ptr(), None) == E_ARG
    assert "gamma" in L.tmac_hip_last_error().decode() and bool(torch.isnan(xo).all())
    rc, msg = raw(4, in2=i2, gamma=gp)
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert rows_launches(tm) > r0 and bool(torch.isnan(rout).all())
    assert rel_err(o.cpu().numpy(), m.oracle(np_glunorm_rows(v))) <= 2e-3


def test_refused_while_recording(tm):
    """inside record_chain() the N = 2 kind-4 call is TMAC_HIP_E_NOMATCH, and the recording builds and runs as if it had never been made"""
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
            wr.fused_xf_rows([m1.w], d["x"], [o2], "glu_norm", 2, in2=d["x2"], gamma=d["gam"], eps=EPS)
        assert ei.value.code == E_NOMATCH
        wr.fused([m1.w], mid, [o1], 1)             # a pending transform would turn this into a GLU_NORM, which the recording refuses
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


# ---- footprint -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["loop", "rows"])
def test_footprint(tm, route):
    """guard bands around in, in2, gamma and every output, two placements, two guard patterns, N = 5"""
    import torch
    wr, K, mats = make_mats(tm, "w2zp-k2112")
    mats.append(Mat(tm, wr, 31, 32, K, bits=2, gs=64))
    set_route(tm, route)
    N = 5
    assert planned_route(tm, mats, [torch.empty(1, device="cuda") for _ in mats], N) == ROUTE_CODE[route]
    v = vectors(N, K, "f16")

    def call(al):
        xd = al.inp(v["x"], name="in")
        ops = dict(in2=al.inp(v["x2"], name="in2"), gamma=al.inp(v["gam"], name="gamma"), eps=EPS)
        outs = [al.out((N, m.Mw), "float16", name=f"C{i}") for i, m in enumerate(mats)]
        al.arm()
        wr.fused_xf_rows([m.w for m in mats], xd, outs, "glu_norm", N, **ops)

    def check_want(want):
        xt = np_glunorm_rows(v)
        for i, m in enumerate(mats):
            assert rel_err(want[f"C{i}"].astype(np.float32), m.oracle(xt)) <= 2e-3
    check_footprint(call, check_want=check_want)
