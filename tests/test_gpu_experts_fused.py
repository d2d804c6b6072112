"""k_gemv_experts with its tables built in the launch (tmac_hip_qgemm_experts_fused_dev; wr.experts(build="kernel", glu=..., in2=...)):
the built tables are the image's, so every result equals the image path's BIT FOR BIT; the oracle and float64 numpy behind that; the GLU
in front of `down` against the fp32 vector the N >= 2 builds consume (bits) and against float64 (REL_TOL for relu^2, whose fp32 x numpy
reproduces exactly; 2e-3 of max|C| for silu and GELU, whose x is a GPU-computed transform: README, "Left at 2e-3")."""
import ctypes as C

import numpy as np
import pytest

import footprint as fp
from oracle import oracle as orc
from test_gpu_defer import stats
from test_gpu_experts import E, GATES, IDS, SHAPES, bank_of, dev, nan_out, refused, within
from test_gpu_parity import REL_TOL, tm  # noqa: F401  (tm: the module fixture)

pytestmark = pytest.mark.gpu
SIX = [n for n in SHAPES if n != "narrow"]
DOWN = ["ragged", "gs64", "long"]
KINDS = ["glu", "glu:relu2", "glu:gelu"]
F64_GATE = {"glu": lambda v: v / (1 + np.exp(-v)), "glu:relu2": lambda v: np.maximum(v, 0) ** 2,
            "glu:gelu": lambda v: v / (1 + np.exp(-1.5957691216 * v * (1 + 0.044715 * v * v)))}


def admits(tm, name, S, lut_rows, combine, kind=0):
    Mw, K, bits, _, gs, _, _ = SHAPES[name]
    return tm.lib().tmac_hip_debug_experts_fused_plan(K, bits, gs, (C.c_int * 1)(Mw), 1, S, lut_rows, int(combine), kind, None, None, None, None) == 0


def both(tm, name, x, ids, gates=None, f16_out=False):
    """the same call through the image path and with the tables built in the launch"""
    import torch
    wr, bank = bank_of(tm, name)[:2]
    shape = (bank.Mw,) if gates is not None else (len(ids), bank.Mw)
    got = []
    for build in ("image", "kernel"):
        out = nan_out(shape, f16_out)
        wr.experts(bank, x, dev(ids, np.int32), gates=gates, out=out if gates is not None else [out], build=build)
        got.append(out)
    torch.cuda.synchronize()
    return got


def glu_operands(name, S, f16, seed=0):
    """G, U [S][K]: N(0, 1) scaled so that values reach about +-8"""
    K = SHAPES[name][1]
    G, U = (2 * np.random.default_rng(40 + seed).standard_normal((2, S, K))).astype(np.float16 if f16 else np.float32)
    return G, U


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("form", ["shared", "per_slot", "combine"])
@pytest.mark.parametrize("S", list(IDS))
@pytest.mark.parametrize("name", SIX)
def test_the_built_tables_are_the_images(tm, name, S, form, f16):
    import torch
    wr, bank, X, _ = bank_of(tm, name)
    x = dev(X[5] if form == "shared" else X[:S])
    x = x.half() if f16 else x
    g = dev(GATES[:S], np.float32) if form == "combine" else None
    if not admits(tm, name, S, 1 if form == "shared" else S, form == "combine"):      # (S = 8 rows of K = 11008: as the image path refuses)
        out = nan_out((bank.Mw,) if g is not None else (S, bank.Mw))
        return refused(tm, -1, "do not fit LDS", lambda: wr.experts(bank, x, dev(IDS[S], np.int32), gates=g, out=out if g is not None else [out], build="kernel"), out)
    image, kernel = both(tm, name, x, IDS[S], g)
    assert torch.isfinite(image).all() and torch.equal(kernel, image)


@pytest.mark.parametrize("name", SIX)
def test_against_the_oracle(tm, name):
    import torch
    wr, bank, X, ref = bank_of(tm, name)
    ids = IDS[3]
    f16 = name == "w3"
    within(both(tm, name, dev(X[5]), ids, f16_out=f16)[1], np.stack([ref[e, 5] for e in ids]))
    within(both(tm, name, dev(X[:3]), ids, f16_out=f16)[1], np.stack([ref[e, s] for s, e in enumerate(ids)]))
    got = wr.experts(bank, dev(X[:3]), dev(ids, np.int32), gates=dev(GATES[:3], np.float32), out=nan_out((bank.Mw,)), build="kernel")
    torch.cuda.synchronize()
    want = sum(np.float64(np.float32(GATES[s])) * ref[e, s] for s, e in enumerate(ids))
    bound = REL_TOL * sum(abs(GATES[s]) * np.abs(ref[e, s]).max() for s, e in enumerate(ids))
    assert np.abs(got.cpu().numpy() - want).max() <= bound


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", DOWN)
def test_glu_bit_for_bit(tm, name, kind, f16):
    """down(gate(G) * U) in one launch == the image path fed the fp32 vector the N >= 2 builds form with the same xf_gate_mul"""
    import torch
    wr, bank = bank_of(tm, name)[:2]
    S, ids, g = 3, dev(IDS[3], np.int32), dev(GATES[:3], np.float32)
    G, U = (dev(a) for a in glu_operands(name, S, f16))
    xt = nan_out((S, bank.K))
    wr.xf_rows_tap(G, xt, kind, bank.K, S, in2=U)
    for gates in (None, g):
        shape = (bank.Mw,) if gates is not None else (S, bank.Mw)
        fused, image = nan_out(shape), nan_out(shape)
        wr.experts(bank, G, ids, gates=gates, out=fused if gates is not None else [fused], glu=kind, in2=U)
        wr.experts(bank, xt, ids, gates=gates, out=image if gates is not None else [image])
        torch.cuda.synchronize()
        assert torch.isfinite(image).all() and torch.equal(fused, image)


_down = {}


def down_bank(tm, name):
    """a bank of the shape with its experts' reference blobs kept: (wrapper, ExpertBank, [(A, S)] per expert)"""
    if name not in _down:
        Mw, K, bits, bm, gs, zp, sc16 = SHAPES[name]
        wr = tm.TMACGeMMWrapper(act_group_size=64)
        blobs = []
        for e in range(E):
            case = orc.make_case(3300 + 10 * len(_down) + e, Mw, K, N=1, bits=bits, gs=gs, ags=64, zero_point=zp, fp16_values=sc16)
            blobs.append((orc.preprocess_weights(case["w"], bits, bm, 16), orc.preprocess_scales(case["sc"], case["zr"] if zp else None, bits, bm)))
        ws = [wr.register_weights(A, S, Mw, K, bits, tm.KCfg.make(Mw, K, bits, bm, 16, gs, 64, zp), scales_dtype=tm.F32,
                                  dev_dtype=tm.F16 if sc16 else tm.F32) for A, S in blobs]
        _down[name] = (wr, tm.ExpertBank.from_handles(ws), blobs)
    return _down[name]


def glu_reference(name, blobs, kind, G, U, ids, gates):
    """x = gate(G) * U in float64 rounded to fp32 (relu^2: the two rounded fp32 products themselves), the oracle per expert on it, the
    gated sum in float64; returns (want [Mw], sum_s |g_s| max|y_s|)"""
    Mw, K, bits, bm, gs, zp, _ = SHAPES[name]
    G32, U32 = G.astype(np.float32), U.astype(np.float32)
    if kind == "glu:relu2":
        m = np.maximum(G32, 0)
        x = (m * m).astype(np.float32) * U32
    else:
        x = (F64_GATE[kind](G32.astype(np.float64)) * U32.astype(np.float64)).astype(np.float32)
    q, ls, lb = orc.preprocessor(x, 64)
    ys = [orc.qgemm_float(blobs[e][0], q, blobs[e][1], ls, lb, Mw, K, len(ids), bits, bm, 16, gs, 64, zp)[s].astype(np.float64) for s, e in enumerate(ids)]
    return sum(np.float64(np.float32(gates[s])) * y for s, y in enumerate(ys)), sum(abs(gates[s]) * np.abs(y).max() for s, y in enumerate(ys))


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", DOWN)
def test_glu_against_float64(tm, name, kind, f16):
    """relu^2: REL_TOL, as the image path is held (its fp32 x is exact in numpy).  silu, GELU: 2e-3 of max|C| (hardware exp and reciprocal
    in x; on the CPU the fp32-formula x against the float64 one moves C by at most 2.5e-4 of max|C| for these seeds -- one table entry of
    `long` on a rounding boundary -- and by 2e-7 elsewhere)"""
    import torch
    wr, bank, blobs = down_bank(tm, name)
    S, ids = 3, IDS[3]
    G, U = glu_operands(name, S, f16, seed=1)
    got = wr.experts(bank, dev(G), dev(ids, np.int32), gates=dev(GATES[:S], np.float32), out=nan_out((bank.Mw,)), glu=kind, in2=dev(U))
    torch.cuda.synchronize()
    want, scale = glu_reference(name, blobs, kind, G, U, ids, GATES)
    err = np.abs(got.cpu().numpy() - want).max()
    print(f"{name} {kind} f16={f16}: err {err:.3e}, REL_TOL bound {REL_TOL * scale:.3e}, 2e-3 bound {2e-3 * np.abs(want).max():.3e}")
    assert err <= (REL_TOL * scale if kind == "glu:relu2" else 2e-3 * np.abs(want).max())


@pytest.mark.parametrize("name", ["ragged", "long"])
def test_empty_slots_do_not_leak(tm, name):
    import torch
    wr, bank = bank_of(tm, name)[:2]
    G, U = glu_operands(name, 3, False)
    G[1], U[1] = np.nan, np.nan
    g = dev(GATES[:3], np.float32)
    c3 = wr.experts(bank, dev(G), dev([1, -1, 3], np.int32), gates=g, out=nan_out((bank.Mw,)), glu="glu", in2=dev(U))
    c2 = wr.experts(bank, dev(G[[0, 2]]), dev([1, 3], np.int32), gates=g[[0, 2]].contiguous(), out=nan_out((bank.Mw,)), glu="glu", in2=dev(U[[0, 2]]))
    s3 = wr.experts(bank, dev(G), dev([1, -1, 3], np.int32), out=[nan_out((3, bank.Mw))], build="kernel")[0]
    torch.cuda.synchronize()
    assert torch.isfinite(c2).all() and torch.equal(c3, c2)
    assert torch.equal(s3[1], torch.zeros_like(s3[1])) and torch.isfinite(s3[[0, 2]]).all()


def test_capture_on_a_cold_stream(tm):
    """no call of the library has seen `side` before the capture: the fused call needs no workspace there"""
    import torch
    wr, bank, X, _ = bank_of(tm, "long")
    G, U = (dev(a) for a in glu_operands("long", 3, False, seed=2))
    x, ids, g = dev(X[:3]), dev(IDS[3], np.int32), dev(GATES[:3], np.float32)
    xt = nan_out((3, bank.K))
    wr.xf_rows_tap(G, xt, "glu", bank.K, 3, in2=U)
    ys, yc, es, ec = nan_out((3, bank.Mw)), nan_out((bank.Mw,)), nan_out((3, bank.Mw)), nan_out((bank.Mw,))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        wr.experts(bank, x, ids, out=[ys], stream=side, build="kernel")
        wr.experts(bank, G, ids, gates=g, out=yc, stream=side, glu="glu", in2=U)
    for new_ids in ([0, 3, 1], [2, -1, 0], IDS[3]):
        ids.copy_(dev(new_ids, np.int32))                  # rewritten on the device, between replays
        ys.fill_(float("nan")); yc.fill_(float("nan"))
        graph.replay()
        wr.experts(bank, x, ids, out=[es])                 # eager, the image path
        wr.experts(bank, xt, ids, gates=g, out=ec)
        torch.cuda.synchronize()
        assert torch.isfinite(ec).all() and torch.equal(ys, es) and torch.equal(yc, ec)


@pytest.mark.parametrize("glu", [None, "glu:gelu"])
def test_footprint(tm, glu):
    wr, bank, X, _ = bank_of(tm, "ragged")
    G, U = glu_operands("ragged", 3, True)

    def call(alloc):
        x = alloc.inp(G if glu else X[:3], name="in")
        in2 = alloc.inp(U, name="in2") if glu else None
        ids = alloc.inp(np.array(IDS[3], np.int32), name="ids")
        g = alloc.inp(np.array(GATES[:3], np.float32), name="gates") if glu else None
        out = alloc.out((bank.Mw,) if glu else (3, bank.Mw), np.float32, name="C")
        alloc.arm()
        wr.experts(bank, x, ids, gates=g, out=out if glu else [out], build="kernel", glu=glu, in2=in2)
    fp.check_footprint(call)


def test_refusals(tm):
    import torch
    L = tm.lib()
    wr, bank, X, _ = bank_of(tm, "half_step")
    _, long_bank, XL, _ = bank_of(tm, "long")
    other = bank_of(tm, "narrow")[1]
    Mw, K = bank.Mw, bank.K
    x, ids, g = dev(X[:3]), dev(IDS[3], np.int32), dev(GATES[:3], np.float32)
    o1, o2, oc = nan_out((3, Mw)), nan_out((3, other.Mw)), nan_out((Mw,))
    flat = torch.zeros(3 * K + 4, device="cuda")
    before = stats(tm)
    refused(tm, -4, "TMAC_XF_NORM is not served", lambda: wr.experts(bank, x, ids, out=[o1], glu="norm"), o1)
    refused(tm, -4, "TMAC_XF_GLU_NORM is not served", lambda: wr.experts(bank, x, ids, out=[o1], glu="glu_norm", in2=x), o1)
    refused(tm, -4, "unknown gate", lambda: wr.experts(bank, x, ids, out=[o1], glu=0x302, in2=x), o1)
    refused(tm, -4, "GLU needs a second vector", lambda: wr.experts(bank, x, ids, out=[o1], glu="glu"), o1)
    refused(tm, -4, "one row of in and in2 per slot", lambda: wr.experts(bank, x[0], ids, out=[o1], glu="glu", in2=x[0]), o1)
    refused(tm, -4, "in2 must be 16-byte aligned", lambda: wr.experts(bank, x, ids, out=[o1], glu="glu", in2=flat[1:3 * K + 1].view(3, K)), o1)
    refused(tm, -4, "COMBINE", lambda: wr.experts([bank, other], x, ids, gates=g, out=[o1, o2], build="kernel"), o1, o2)
    refused(tm, -4, "one activation row per slot", lambda: wr.experts(bank, x[0], ids, gates=g, out=oc, build="kernel"), oc)
    o8 = nan_out((8, long_bank.Mw))
    refused(tm, -1, "do not fit LDS", lambda: wr.experts(long_bank, dev(XL), dev(IDS[8], np.int32), out=[o8], build="kernel"), o8)
    tm.binding.check(L.tmac_hip_chain_begin())
    try:
        refused(tm, -4, "tmac_hip_qgemm_experts_fused_dev cannot be recorded", lambda: wr.experts(bank, x[0], ids, out=[o1], build="kernel"), o1)
    finally:
        L.tmac_hip_chain_abort()
    assert stats(tm) == before, "a refused call flushed or launched"
    queued = nan_out((1, Mw))
    tm.binding.check(L.tmac_hip_defer(1))      # with deferral on the call runs behind the queue: it flushes it first
    try:
        f0 = stats(tm)[0]
        wr.fused([bank.experts[0]], dev(X[:1]), [queued], 1)
        assert stats(tm)[0] == f0
        wr.experts(bank, x[0], ids, out=[o1], build="kernel")
        assert stats(tm)[0] == f0 + 1
    finally:
        L.tmac_hip_defer(0)
    torch.cuda.synchronize()
    assert torch.isfinite(queued).all() and torch.isfinite(o1).all()
