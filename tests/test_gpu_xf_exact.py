"""The vector transforms (TMAC_XF_NORM / _GLU / _GLU_NORM with the silu, relu^2 and tanh-GELU gates, include/tmac_hip.h) held to the plain
path's bar on their three paths: k_gemv_quad's XF instantiations (N = 1, fused_xf), the N >= 2 LUT builds behind k_xf_rows (fused_xf_rows and
its tap) and k_decode_chain (chain_xform while recording).

Reference: the transform in float64, rounded once to fp32 (tests/xf_probe.py::ref_x), fed through the oracle.  Bar: every fp32 output within
2e-5 of max |C| -- what the untransformed calls are held to -- where the other transform tests allow 2e-3; NORM with gamma and GLU_NORM add
the bound of their scalar r, (K / 2 + 16) * 2^-24.  That bar is possible because every input is ROUNDING-SAFE: chosen on the CPU (pick_safe)
so that no table value lies within 127 * 4 eps of a half-integer, eps being the relative error of the GPU's x (measured, xf_probe.EPS_HW, and
asserted here on the tap), so the GPU's x and the reference x quantise to the same QLUT.  tests/test_xf_probe_cpu.py proves on the oracle
alone that this comparison rejects a reference that ignores eps or adds it outside the square root, drops or double-counts the last 8
elements of the mean square, shifts gamma by one index, swaps a GLU's operands, uses the erf GELU or rounds the product to fp16.

Regimes (xf_probe): `plain` N(0,1); `eps` mean(t^2) / eps in {1e-2, 1, 1e2} for eps in {1e-6, 1e-5} and eps = 1e-2 on an O(1) vector;
`sparse` one non-zero element with a weight distinct per index -- the pipeline is exactly linear in x_i; `tails` gate inputs on a fixed grid
over [-30, 30], one magnitude band per act group.  At N = 1 every regime runs fp16 and fp32 operands (k_gemv_quad loads them on
separate paths); fp32 alone where fp16 would go denormal.  Which test fails for which defect:
    eps ignored, hard-coded or outside the root   test_n1_eps, test_n1_every_configuration[eps-*], test_rows_eps, test_chain_reader_form[eps-*],
                                                  test_chain_producer_form_eps
    gamma off by one index                        test_n1_sparse, test_rows_sparse, test_chain_sparse (and every plain NORM case)
    last pair dropped from / counted twice in the mean square   the same three, at i = K - 8 and K - 1
    GLU operands swapped, a gate's tail wrong     test_n1_plain, test_n1_tails, test_rows_routes, test_rows_tails (element-wise on the tap),
                                                  test_chain_reader_form[plain-glu_* / tails-*]
The producer forms of GLU and GLU_NORM in the chain take `in` from a GPU-computed hand-off: no input can be chosen beforehand, they keep the
2e-3 bar and gain the eps regime.
"""
import numpy as np
import pytest

import xf_probe as P
from oracle import oracle as orc
from test_gpu_xf import XF_CONFIGS
from test_gpu_xf_glunorm import LAYER_SHAPES, layers_of
from test_gpu_xf_rows import FLAVOURS, ROUTE_CODE, ROUTE_N, make_mats, planned_route, set_route
from xf_common import KF, Mat, dev, host, np_gated, np_glu, np_norm, poison, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tm():
    import torch
    import tmac_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return tmac_amd


@pytest.fixture(autouse=True)
def _knobs(tm):
    """a short spin: a lost hand-off reports through chain.status() instead of spinning"""
    tm.binding.check(tm.lib().tmac_hip_debug_chain_config(0, 1 << 17))


# ---- shared pieces ---------------------------------------------------------------------------------------------------------------------
# the weight flavours, by K: W2 with zero points (gs = 64 where K has no group of 128), W4 / W1 / W3 / gs = 64 once each at K = 256, unified
N1_MATS = {
    64: [dict(Mw=16, gs=64)],
    128: [dict(Mw=16)],
    256: [dict(Mw=16, bits=4), dict(Mw=32, bits=1), dict(Mw=32, bits=3), dict(Mw=16, gs=64)],
    1024: [dict(Mw=16)],
    2112: [dict(Mw=16, gs=64)],
    3200: [dict(Mw=16, m_groups=1)],
    4160: [dict(Mw=16, gs=64)],
    6144: [dict(Mw=16)],
    12288: [dict(Mw=16)],
}
_MATS = {}


def mats_of(tm, K):
    """the matrices of a K, registered once and shared (never changed): [(wrapper, Mat)] per flavour"""
    if K not in _MATS:
        wr = tm.TMACGeMMWrapper(act_group_size=64)
        _MATS[K] = [(wr, Mat(tm, wr, 40 + i, K=K, **kw)) for i, kw in enumerate(N1_MATS[K])]
    return _MATS[K]


def chain_mat(tm, K):
    """the chain's matrix of a K: 256 rows, so that most workgroups of the persistent launch own some"""
    if ("chain", K) not in _MATS:
        wr = tm.TMACGeMMWrapper(act_group_size=64)
        _MATS[("chain", K)] = (wr, Mat(tm, wr, 60, 256, K, gs=128 if K % 128 == 0 else 64))
    return _MATS[("chain", K)]


def to_dev(inp):
    return {k: dev(inp[k]) for k in ("a", "b", "res", "gam") if inp.get(k) is not None}


def xf_ops(inp, d):
    """the operands of the case's transform as the wrapper's methods take them"""
    if inp["kind"] == "norm":
        return dict(residual=d.get("res"), gamma=d["gam"], eps=inp["eps"])
    ops = dict(in2=d["b"])
    if inp["kind"].startswith("glu_norm"):
        ops.update(gamma=d["gam"], eps=inp["eps"])
    return ops


def t_of(inp):
    """residual_out of a NORM: fp32(in) + residual, one fp32 add"""
    return inp["a"].astype(np.float32) + inp["res"]


def check_out(label, got, want, bar):
    ok, e = P.compare(got, want, bar)
    print(f"{label}: rel err {e:.3e} of max |C| (bar {bar:.3e})")
    assert ok, (label, e, bar)


def run_n1(tm, c, label=""):
    """fused_xf on the case's vectors, fp32 outputs, every flavour of its K: outputs at the tight bar, residual_out bit for bit"""
    import torch
    inp = P.resolve(c)
    d = to_dev(inp)
    K = c["K"]
    for wr, m in mats_of(tm, K):
        o = poison(m.Mw, torch.float32)
        rout = poison(K, torch.float32) if c["kind"] == "norm" else None
        wr.fused_xf([m.w], d["a"], [o], c["kind"], residual_out=rout, **xf_ops(inp, d))
        torch.cuda.synchronize()
        if rout is not None:
            assert np.array_equal(rout.cpu().numpy(), t_of(inp)), "residual_out"
        check_out(f"N=1 {label} {P.case_id(c)} W{m.bits} gs={m.gs} seed {inp['seed']}", o.cpu().numpy(), m.oracle(inp["x"]), P.tight_bar(c["kind"], K))


def test_host_mat_is_mat(tm):
    """xf_probe.HostMat, on which the CPU tests of the comparison run, builds the weights and scales of xf_common.Mat from the same arguments"""
    for kw in (dict(Mw=16, K=2112, gs=64), dict(Mw=16, K=1024), dict(Mw=16, K=3200, m_groups=1), dict(Mw=16, K=256, bits=4), dict(Mw=32, K=256, bits=3)):
        wr = tm.TMACGeMMWrapper(act_group_size=64)
        m, h = Mat(tm, wr, 5, **kw), P.HostMat(5, **kw)
        assert np.array_equal(m.A, h.A) and np.array_equal(m.S, h.S) and (m.bm, m.ags, m.zp) == (h.bm, h.ags, h.zp), kw


# ---- 1. N = 1: k_gemv_quad's XF instantiations ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", P.N1_PLAIN, ids=[P.case_id(c) for c in P.N1_PLAIN])
def test_n1_plain(tm, c):
    run_n1(tm, c)


@pytest.mark.parametrize("c", P.N1_EPS, ids=[P.case_id(c) for c in P.N1_EPS])
def test_n1_eps(tm, c):
    """eps in play: a kernel that ignored a.eps, hard-coded 1e-5 or added eps outside the root is off by 0.5 % to 10x here"""
    run_n1(tm, c)


@pytest.mark.parametrize("c", P.N1_TAILS, ids=[P.case_id(c) for c in P.N1_TAILS])
def test_n1_tails(tm, c):
    run_n1(tm, c)


@pytest.mark.parametrize("c", P.N1_CONFIG, ids=[P.case_id(c) for c in P.N1_CONFIG])
@pytest.mark.parametrize("ft,wpq", XF_CONFIGS)
def test_n1_every_configuration(tm, ft, wpq, c):
    """K = 4160: 520 pairs, a second round with eight live lanes under 512 threads; K = 6144: three even steps for (768, 3); K = 12288: the
    six-tables-per-thread forms; K = 2112 with eps in play: the cross-wave sum of the mean square depends on the wave count"""
    tm.binding.check(tm.lib().tmac_hip_debug_quad_config(ft, wpq))
    run_n1(tm, c, label=f"({ft},{wpq})")


@pytest.mark.parametrize("K", P.SPARSE_KS)
@pytest.mark.parametrize("act", P.ACTS)
@pytest.mark.parametrize("kind", ["norm", "glu_norm:silu", "glu_norm:relu2"])
@pytest.mark.parametrize("ft,wpq", XF_CONFIGS)
def test_n1_sparse(tm, ft, wpq, kind, act, K):
    """one non-zero element i, gamma distinct per index: the outputs carry x_i = t_i * gamma_i * r to fp32 precision.  i sweeps both ends,
    the pair boundaries and the first round's last lane and the second round's first (8 * threads - 1, 8 * threads)"""
    tm.binding.check(tm.lib().tmac_hip_debug_quad_config(ft, wpq))
    for c in P.sparse_cases(kind, K, ft, act=act):
        run_n1(tm, c, label=f"({ft},{wpq})")


# ---- 2. N >= 2: the LUT builds behind k_xf_rows, with the tap --------------------------------------------------------------------------
def check_tap(c, xt, ref, label):
    """the tapped x against float64, element by element, relative to |x_ref|: relu^2 to the bit, silu / GELU within the measured eps, NORM
    within r's float64 bound (tests/test_gpu_xf_rows.py::test_a_row_is_a_row), GLU_NORM within both"""
    base, _, gate = c["kind"].partition(":")
    assert np.isfinite(xt).all()
    if base == "glu" and gate == "relu2":
        assert np.array_equal(xt, ref), (label, "relu^2 is specified to the bit")
        return
    bound = (P.norm_bound(c["K"]) if base != "glu" else 0.0) + (P.eps_hw(c) if gate in ("silu", "gelu") else 0.0)
    r64 = np.abs(ref.astype(np.float64))
    d = np.abs(xt.astype(np.float64) - ref.astype(np.float64))
    worst = float((d[r64 > 0] / r64[r64 > 0]).max()) if (r64 > 0).any() else 0.0
    print(f"{label}: tap max |x - x_ref| / |x_ref| = {worst:.3e} (bound {bound:.3e})")
    assert (d <= bound * r64).all(), (label, worst, bound)


def run_rows(tm, wr, mats, c, N, route, inp=None):
    """the tap of x element by element, then the outputs of the same call at the tight bar; residual_out bit for bit"""
    import torch
    inp = P.rows_of(c, N) if inp is None else inp
    K = c["K"]
    d = to_dev(inp)
    ops = xf_ops(inp, d)
    label = f"{P.case_id(c)} {route} N={N}"
    xt = poison((N, K), torch.float32)
    wr.xf_rows_tap(d["a"], xt, c["kind"], K, N, **ops)
    torch.cuda.synchronize()
    check_tap(c, xt.cpu().numpy(), inp["x"], label)
    outs = [poison((N, m.Mw), torch.float32) for m in mats]
    rout = poison((N, K), torch.float32) if c["kind"] == "norm" else None
    assert planned_route(tm, mats, outs, N) == ROUTE_CODE[route], (route, planned_route(tm, mats, outs, N))
    wr.fused_xf_rows([m.w for m in mats], d["a"], outs, c["kind"], N, residual_out=rout, **ops)
    torch.cuda.synchronize()
    if rout is not None:
        assert np.array_equal(rout.cpu().numpy(), t_of(inp)), "residual_out"
    for i, (m, o) in enumerate(zip(mats, outs)):
        check_out(f"{label} matrix {i}", o.cpu().numpy(), m.oracle(inp["x"]), P.tight_bar(c["kind"], K))


ROWS_CASES = [(f, r, n, c) for f in FLAVOURS for r, n in ROUTE_N for c in P.ROWS_PLAIN[FLAVOURS[f][0]] if n <= P.rows_max_n(c)]


@pytest.mark.parametrize("flavour,route,N,c", ROWS_CASES, ids=[f"{f}-{r}-n{n}-{c['kind'].replace(':', '_')}" for f, r, n, c in ROWS_CASES])
def test_rows_routes(tm, flavour, route, N, c):
    """the routes tests/test_gpu_xf_rows.py forces (planes, onehot, rows, loop), N = 2, 3, 33, 65, every row rounding-safe"""
    wr, K, mats = make_mats(tm, flavour)
    set_route(tm, route)
    run_rows(tm, wr, mats, c, N, route)


@pytest.mark.parametrize("c", P.ROWS_EPS, ids=[P.case_id(c) for c in P.ROWS_EPS])
@pytest.mark.parametrize("route", ["loop", "planes"])
def test_rows_eps(tm, route, c):
    """eps in play in the row pass's r (k_xf_rows), behind the pair builds (loop) and k_lut_image (planes)"""
    wr, K, mats = make_mats(tm, "w2zp-k128")
    set_route(tm, route)
    run_rows(tm, wr, mats, c, 3, route)


@pytest.mark.parametrize("c", P.ROWS_TAILS, ids=[P.case_id(c) for c in P.ROWS_TAILS])
def test_rows_tails(tm, c):
    """the gates' tails and the neighbourhood of 0, element by element: hardware exp and rcp within the measured eps of float64"""
    wr, K, mats = make_mats(tm, "w2zp-k128")
    set_route(tm, "rows")
    run_rows(tm, wr, mats, c, 3, "rows")


@pytest.mark.parametrize("kind", ["norm", "glu_norm:silu"])
@pytest.mark.parametrize("route", ["rows", "planes"])
def test_rows_sparse(tm, route, kind):
    """seven rows, row n with its one non-zero element at the n-th index of the sweep: a row's r and gamma are its own"""
    wr, K, mats = make_mats(tm, "w2zp-k2112")
    set_route(tm, route)
    rows = [P.resolve(c) for c in P.sparse_cases(kind, K)]
    inp = dict(rows[0])
    for k in ("a", "b", "res", "x"):
        inp[k] = None if rows[0].get(k) is None else np.stack([r[k] for r in rows])
    run_rows(tm, wr, mats, P.case("sparse", kind, K, 64, i=-1), len(rows), route, inp=inp)


# ---- 3. the chain: reader form, vectors in memory ---------------------------------------------------------------------------------------
def comb_sums(m, x):
    """what tmac_hip_chain_set_tap shows of a call on per-group scales: comb[row][act group] = sum_p 2^p PS_p (tests/test_gpu_chain_gate.py)"""
    q, _, _ = orc.preprocessor(np.ascontiguousarray(x[None, :], np.float32), 64)
    PS = orc.partial_sums(m.A, q[0], m.Mw, m.K, m.bits, m.bm, KF, 64)
    r = np.arange(m.Mw)
    return sum(PS[(r // 8) * 8 * m.bits + p * 8 + (r % 8)].astype(np.int64) << p for p in range(m.bits))


class ReaderChain:
    """one recorded call with the case's transform in front, its vectors in device memory that later cases of the same shape overwrite"""

    def __init__(self, tm, c):
        import torch
        self.tm, self.K, self.kind = tm, c["K"], c["kind"]
        self.wr, self.m = chain_mat(tm, c["K"])
        inp = P.resolve(c)
        self.d = to_dev(inp)
        self.o = torch.zeros(self.m.Mw, dtype=torch.float32, device="cuda")
        self.rout = torch.zeros(self.K, dtype=torch.float32, device="cuda") if self.kind == "norm" else None
        with self.wr.record_chain() as rec:
            self.wr.chain_xform(self.kind, residual_out=self.rout, **xf_ops(inp, self.d))
            self.wr.fused([self.m.w], self.d["a"], [self.o], 1)
        self.chain = rec.chain
        assert not self.chain.stream, "a recording with a transform is a decode chain"

    def run(self, c):
        import torch
        inp = P.resolve(c)
        for k, t in self.d.items():
            t.copy_(dev(inp[k]))
        self.o.fill_(float("nan"))
        self.chain.launch()
        torch.cuda.synchronize()
        assert self.chain.status() == 0
        label = f"chain {P.case_id(c)} seed {inp['seed']}"
        if self.rout is not None:
            assert np.array_equal(self.rout.cpu().numpy(), t_of(inp)), "residual_out"
        check_out(label, self.o.cpu().numpy(), self.m.oracle(inp["x"]), P.tight_bar(c["kind"], self.K))
        # the integers the launch itself accumulated: the oracle's on ref_x, bit for bit.  Every reader-form recording here takes the tap
        # (set_tap raises otherwise: a recording that began to refuse it would fail here, not drop the check)
        total, _ = self.chain.tap_layout(1)
        buf = torch.full((total,), -(2 ** 31), dtype=torch.int32, device="cuda")
        self.chain.set_tap(buf)
        try:
            self.chain.launch()
            torch.cuda.synchronize()
            assert self.chain.status() == 0
        finally:
            self.chain.set_tap(None)
        off, cnt = self.chain.tap_layout(0)
        assert cnt == self.m.Mw * (self.K // 64)
        got = buf.cpu().numpy()[off:off + cnt].reshape(self.m.Mw, self.K // 64).astype(np.int64)
        assert np.array_equal(got, comb_sums(self.m, inp["x"])), (label, "integer tap != oracle on ref_x")
        print(f"{label}: integer tap == oracle on ref_x")


@pytest.mark.parametrize("c", P.CHAIN_CASES, ids=[P.case_id(c) for c in P.CHAIN_CASES])
def test_chain_reader_form(tm, c):
    """NORM with residual and gamma, and GLU with the three gates, on vectors in memory: the consuming call transforms them in its LUT build"""
    rc = ReaderChain(tm, c)
    try:
        rc.run(c)
    finally:
        rc.chain.free()


def test_chain_sparse(tm):
    """NORM in the chain, one non-zero element with a weight distinct per index, swept over both ends and the pair boundaries of K = 4160"""
    cases = P.sparse_cases("norm", P.CHAIN_SPARSE_K, 512)
    rc = ReaderChain(tm, cases[0])
    try:
        for c in cases:
            rc.run(c)
    finally:
        rc.chain.free()


# ---- 4. the chain: producer forms, eps in play -----------------------------------------------------------------------------------------
PRODUCER = [("bitnet-shaped", "glu_norm:silu", 1e-5), ("bitnet-shaped", "glu_norm:relu2", 1e-6), ("bitnet-shaped", "glu_norm:relu2", 1e-5),
            ("llama-shaped", "glu_norm:gelu", 1e-6), ("llama-shaped", "glu:gelu", 1e-5)]


@pytest.mark.parametrize("shape,kind,eps", PRODUCER, ids=[f"{s}-{k.replace(':', '_')}-eps{e:g}" for s, k, e in PRODUCER])
def test_chain_producer_form_eps(tm, shape, kind, eps):
    """gate/up -> gate(gate) * up published by the producer (fp16) -> [RMSNorm] -> down, the activations of the gate/up call scaled so that
    the product's mean square is about eps (BitNet's ffn_sub_norm).  The hand-off is computed on the GPU, so no input can be chosen
    beforehand: the existing 2e-3 bar, the GPU's own gate/up outputs feeding the reference (tests/test_gpu_chain_gate.py::check_segment)"""
    import torch
    H, F, kw = LAYER_SHAPES[shape]
    wr, layers = layers_of(tm, shape)
    L = layers[0]
    gate = kind.split(":")[1]
    x0 = np.random.default_rng(23).standard_normal(H).astype(np.float32)
    g0, u0 = L.gate.oracle(x0).astype(np.float64), L.up.oracle(x0).astype(np.float64)
    lo, hi = 1e-6, 1.0                  # the outputs are linear in the scale s of x; mean((gate(s g0) * s u0)^2) grows with s
    for _ in range(60):
        s = np.sqrt(lo * hi)
        lo, hi = (s, hi) if float((P.gate64(gate, s * g0, s * u0) ** 2).mean()) < eps else (lo, s)
    x = dev((x0 * s).astype(np.float16))
    g, u = (torch.zeros(F, dtype=torch.float16, device="cuda") for _ in range(2))
    d = torch.zeros(H, dtype=torch.float16, device="cuda")          # (one output dtype per chain: fp16, like the hand-off)
    ops = dict(in2=u, gamma=L.g3, eps=eps) if kind.startswith("glu_norm") else dict(in2=u)
    with wr.record_chain() as rec:
        wr.fused([L.gate.w, L.up.w], x, [g, u], 1)
        wr.chain_xform(kind, **ops)
        wr.fused([L.down.w], g, [d], 1)
    chain = rec.chain
    try:
        assert not chain.stream
        chain.launch()
        torch.cuda.synchronize()
        assert chain.status() == 0, "a hand-off timed out"
        gh, uh = host(g), host(u)
        assert rel_err(gh, L.gate.oracle(host(x))) <= 2e-3 and rel_err(uh, L.up.oracle(host(x))) <= 2e-3
        prod = P.gate64(gate, gh, uh)
        ratio = float((prod ** 2).mean()) / eps
        tiny = float(np.finfo(np.float16).tiny)
        assert 0.25 <= ratio <= 4.0, ratio
        if gate == "silu":      # (np_gated knows the two other gates; silu is np_glu, as in tests/test_gpu_xf_glunorm.py)
            xt = np_norm(np_glu(gh, uh).astype(np.float16).astype(np.float32), L.g3.cpu().numpy(), eps)
        else:
            xt = np_gated(kind, gh, uh, L.g3.cpu().numpy(), eps, handed_over_f16=True)
        e = rel_err(host(d), L.down.oracle(xt))
        print(f"{shape} {kind} eps={eps:g}: mean(g^2) / eps = {ratio:.2f}, {float(((prod != 0) & (np.abs(prod) < tiny)).mean()):.1%} of the products non-zero and below fp16's normals, "
              f"down rel err vs oracle {e:.2e}")
        assert np.isfinite(host(d)).all() and e <= 2e-3, e
        if kind.startswith("glu_norm"):      # the bar sees eps: the reference without it is far outside
            wrong = P.ref_x("glu_norm", gate, gh, uh, None, L.g3.cpu().numpy(), eps, handed_over_f16=True, mutant="no_eps")
            assert rel_err(host(d), L.down.oracle(wrong)) > 0.1
    finally:
        chain.free()
