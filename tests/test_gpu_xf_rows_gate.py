"""The gate of TMAC_XF_GLU / TMAC_XF_GLU_NORM for N >= 2 activation rows: tmac_hip_qgemm_fused_xf_rows_dev and its tap tmac_hip_debug_xf_rows
(include/tmac_hip.h).  One device function, xf_rows_g8, forms g = gate(in) * in2 for the row pass (k_xf_rows), the three LUT builders and
the tap; the gate comes with the argument block.

Bars (those of tests/test_gpu_xf_rows_glunorm.py):
  * relu^2 is exact arithmetic: the tap of "glu:relu2" is the float32 numpy expression, bit for bit;
  * a row of an N-row call is that row of an N = 1 tap call, bit for bit (the row pass sums the g^2 the builders recompute, in an order that
    depends on K alone);
  * the LUT path: the outputs are those of the plain call on the same route fed the tapped x as fp32 activations, bit for bit;
  * every output within 2e-3 of max |C| of the oracle on the numpy-transformed rows.
N = 5 for the small routes (k_gemm_onehot, k_gemv_rows forced, the row loop), N = 70 for k_gemm_planes: a second, padded tile.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_xf_rows import EPS, ROUTE_CODE, make_mats, on_device, plain_same_route, planned_route, rows_launches, set_route, vectors
from xf_common import Mat, host, np_gated, np_relu2, poison, rel_err

pytestmark = pytest.mark.gpu
E_NOMATCH = -1
GATES = ["relu2", "gelu"]


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


def np_rows(v, kind):
    """the rows a call of kind "glu:<gate>" / "glu_norm:<gate>" builds its tables from"""
    return np_gated(kind, v["x"], v["x2"], v["gam"], EPS)


def ops_of(d, kind):
    return dict(in2=d["x2"], gamma=d["gam"], eps=EPS) if kind.startswith("glu_norm") else dict(in2=d["x2"])


def tap(wr, d, kind, K, N):
    import torch
    x = poison((N, K), torch.float32)
    wr.xf_rows_tap(d["x"], x, kind, K, N, **ops_of(d, kind))
    torch.cuda.synchronize()
    return x


# ---- the transform ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["f16", "f32"])
def test_relu2_is_exact(tm, act):
    """m = max(v, 0); (m * m) * u with each product rounded to nearest: what numpy computes in float32"""
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    K, N = 3200, 5
    v = vectors(N, K, act)
    xh = tap(wr, on_device(v), "glu:relu2", K, N).cpu().numpy()
    want = np_relu2(v["x"], v["x2"])
    assert (want == 0).any() and (want != 0).any()
    assert np.array_equal(xh, want), int((xh != want).sum())


@pytest.mark.parametrize("gate", GATES)
@pytest.mark.parametrize("N", [2, 5, 70])
def test_a_row_is_a_row(tm, N, gate):
    kind = f"glu_norm:{gate}"
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    K = 3200
    v = vectors(N, K, "f16")
    d = on_device(v)
    xh = tap(wr, d, kind, K, N).cpu().numpy()
    assert np.isfinite(xh).all()
    for n in sorted({0, 1, N // 2, N - 1}):
        d1 = dict(x=d["x"][n:n + 1], x2=d["x2"][n:n + 1], gam=d["gam"])
        assert np.array_equal(tap(wr, d1, kind, K, 1).cpu().numpy()[0], xh[n]), n
    e = rel_err(xh, np_rows(v, kind))
    print(f"{kind} tap N={N} K={K}: rel err vs numpy {e:.2e}")
    assert e <= 1e-5, e


# ---- the LUT path exactly, and the oracle ----------------------------------------------------------------------------------------
ROUTE_N = [("planes", 70), ("onehot", 5), ("rows", 5), ("loop", 5)]


@pytest.mark.parametrize("kind", ["glu_norm:relu2", "glu:gelu"])
@pytest.mark.parametrize("flavour", ["w2zp-k2112", "bitnet-k4160"])
@pytest.mark.parametrize("route,N", ROUTE_N, ids=[f"{r}-n{n}" for r, n in ROUTE_N])
def test_routes(tm, flavour, route, N, kind):
    import torch
    wr, K, mats = make_mats(tm, flavour)
    set_route(tm, route)
    v = vectors(N, K, "f16")
    d = on_device(v)
    xt = tap(wr, d, kind, K, N)
    outs = [poison((N, m.Mw), torch.float16) for m in mats]
    assert planned_route(tm, mats, outs, N) == ROUTE_CODE[route], (route, planned_route(tm, mats, outs, N))
    r0 = rows_launches(tm)
    wr.fused_xf_rows([m.w for m in mats], d["x"], outs, kind, N, **ops_of(d, kind))
    torch.cuda.synchronize()
    assert (rows_launches(tm) > r0) == (route == "rows"), "k_gemv_rows runs on its route alone"
    want = plain_same_route(tm, wr, mats, route, xt, N, torch.float16)
    xn = np_rows(v, kind)
    for i, (m, o, w) in enumerate(zip(mats, outs, want)):
        assert np.isfinite(host(o)).all()
        assert np.array_equal(o.cpu().numpy(), w.cpu().numpy()), (route, i, "differs from the plain call on the tapped x")
        e = rel_err(host(o), m.oracle(xn))
        print(f"{flavour} {route} N={N} {kind} matrix {i}: rel err vs oracle {e:.2e}")
        assert e <= 2e-3, (route, i, e)


# ---- recording -------------------------------------------------------------------------------------------------------------------
def test_refused_while_recording(tm):
    """inside record_chain() an N = 2 gated call is TMAC_HIP_E_NOMATCH, and the recording builds and runs as if it had never been made"""
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
            wr.fused_xf_rows([m1.w], d["x"], [o2], "glu_norm:relu2", 2, in2=d["x2"], gamma=d["gam"], eps=EPS)
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
