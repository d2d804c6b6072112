"""k_gemv_rows (tmac_rows.hip): 2-8 activation rows per pass over QUAD-layout weights, behind the two stand-alone entry points.

Bars: the integers the kernel feeds into its float part (tmac_hip_debug_rows_comb_sums) array_equal to the oracle's per-plane partial
sums combined as integers (per-group scales: sum_p 2^p PS_p per act group; unified scales: the exact per-plane totals); outputs within
REL_TOL = 1e-3 of max|C| of orc.qgemm_float (the contract of test_gpu_parity.py / test_gpu_gemm_planes.py) and, for unified scales, equal
to orc.qgemm_scale_final bit for bit.  Unless a test says otherwise the kernel is forced (tmac_hip_debug_rows_kernel(2)) and
tmac_hip_debug_rows_stats shows that its launches happened: the counter is the only way to know which kernel ran.
"""
import ctypes as C

import numpy as np
import pytest

import footprint as fp
from oracle import oracle as orc
from test_gpu_gemm_planes import mrow
from test_gpu_parity import REL_TOL, check_bits, oracle_case, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tm():
    import torch
    import tmac_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert tmac_amd.lib().tmac_hip_device_count() > 0
    return tmac_amd


def launches(tm):
    n = C.c_uint64(0)
    tm.binding.check(tm.lib().tmac_hip_debug_rows_stats(C.byref(n)))
    return int(n.value)


def force(tm, mode=2):
    tm.binding.check(tm.lib().tmac_hip_debug_rows_kernel(mode))


def comb_of(PS, Mw, bits):
    """oracle_case's per-plane sums [N][M][G] -> sum_p 2^p PS_p, [N][Mw][G]"""
    rows = np.arange(Mw)
    return sum(PS[:, mrow(rows, p, bits), :].astype(np.int64) << p for p in range(bits))


def planes_of(PS, Mw, bits):
    """unified scales: oracle_case's totals [N][M][1] -> [N][Mw][bits]"""
    rows = np.arange(Mw)
    return np.stack([PS[:, mrow(rows, p, bits), 0].astype(np.int64) for p in range(bits)], axis=-1)


def setup(tm, case, Mw, K, bits, bm, gs, zp, N, mg=-1, scale_f16=False):
    ags = K if mg >= 1 else 64
    A = orc.preprocess_weights(case["w"], bits, bm, 16)
    S = orc.preprocess_scales(case["sc"], case["zr"] if zp else None, bits, bm) if mg == -1 else case["sc"]
    wr = tm.TMACGeMMWrapper(act_group_size=ags)
    wr.set_workspace(K, N)
    w = wr.register_weights(A, S, Mw, K, bits, tm.KCfg.make(Mw, K, bits, bm, 16, gs, ags, zp, mg, N), scales_dtype=tm.F32,
                            dev_dtype=tm.F16 if scale_f16 else tm.F32)
    return A, S, wr, w


def split(tm, wr, w, B, Mw, K, bits, N, out_f16=False, tap=True):
    """llama_cpp_init + llama_cpp_compute (+ the tap); returns (C fp32 [N][Mw], comb or None, launches of the untapped call)"""
    import torch
    Bt = torch.from_numpy(np.ascontiguousarray(B)).cuda()
    Ct = torch.full((N, Mw), float("nan"), dtype=torch.float16 if out_f16 else torch.float32, device="cuda")
    wr.llama_cpp_init(Bt, Mw, K, N, bits)
    l0 = launches(tm)
    wr.llama_cpp_compute(w, Ct, N)
    torch.cuda.synchronize()
    l1 = launches(tm)
    comb = wr.rows_comb_sums(w, N) if tap else None
    return Ct.float().cpu().numpy(), comb, l1 - l0


# -------------------------------------------------------------------------------------------------
# (a) integers and outputs, split entry points

SHAPES = [  # Mw, K, bits, bm, gs, zp
    (128, 1024, 2, 128, 128, True),      # half a step
    (320, 3200, 2, 320, 128, True),      # ragged last step
    (64, 512, 2, 128, 256, True),        # two weight groups
    (256, 1024, 4, 256, 64, False),      # one act group per weight group: two scale groups per lane and step
    (128, 1024, 1, 64, 128, True),       # 1-bit
    (192, 2048, 3, 192, 128, True),      # 3-bit
    (64, 11008, 2, 128, 128, True),      # six steps, LDS admits fewer than 8 rows
    (64, 24576, 2, 128, 128, True),      # largest K, smallest r_fit
    (704, 1024, 2, 128, 128, False),     # more quads than one pass of a small grid
]
NS = [2, 3, 5, 8, 9]     # 3: a part-filled capacity; 9: a second group with one live row (more groups at the two large K)

_oracle_cache = {}


def case_and_oracle(Mw, K, bits, bm, gs, zp):
    """one case of 9 rows per shape; the N-row calls use its first N rows (the oracle is row by row)"""
    key = (Mw, K, bits, bm, gs, zp)
    if key not in _oracle_cache:
        case = orc.make_case(9100 + Mw + K + bits, Mw, K, N=max(NS), bits=bits, gs=gs, ags=64, zero_point=zp)
        A = orc.preprocess_weights(case["w"], bits, bm, 16)
        S = orc.preprocess_scales(case["sc"], case["zr"] if zp else None, bits, bm)
        _, _, _, Cc, PS = oracle_case(case, A, S, Mw, K, bits, bm, 16, gs, 64, zp, N=max(NS))
        Cc.setflags(write=False); PS.setflags(write=False)
        _oracle_cache[key] = (case, Cc, comb_of(PS, Mw, bits))
    return _oracle_cache[key]


@pytest.mark.parametrize("Mw,K,bits,bm,gs,zp", SHAPES)
def test_integers_and_outputs(tm, Mw, K, bits, bm, gs, zp):
    case, Cc, comb = case_and_oracle(Mw, K, bits, bm, gs, zp)
    force(tm)
    A, S, wr, w = setup(tm, case, Mw, K, bits, bm, gs, zp, max(NS))
    for N in NS:
        C_, tap, nl = split(tm, wr, w, case["B"][:N], Mw, K, bits, N)
        assert nl >= 1, (N, "k_gemv_rows did not run")
        assert np.array_equal(tap.astype(np.int64), comb[:N]), N
        e = rel_err(C_, Cc[:N])
        print(f"ROWS split {Mw}x{K} W{bits} gs{gs} N={N}: rel err {e:.3g}, launches {nl}")
        assert e <= REL_TOL, (N, e)
    w.free()


# -------------------------------------------------------------------------------------------------
# (b) unified scales

@pytest.mark.parametrize("Mw,K,bits,bm,mg", [(320, 3200, 2, 320, 1), (128, 8640, 2, 128, 2)])
def test_unified_scales(tm, Mw, K, bits, bm, mg):
    Nmax = 9
    case = orc.make_case(9200 + K, Mw, K, N=Nmax, bits=bits, gs=128, ags=K, zero_point=False, m_groups=mg)
    force(tm)
    A, S, wr, w = setup(tm, case, Mw, K, bits, bm, 128, False, Nmax, mg=mg)
    _, _, _, Cc, PS = oracle_case(case, A, S, Mw, K, bits, bm, 16, 128, K, False, mg, N=Nmax)
    want = planes_of(PS, Mw, bits)
    for N in (2, 5, 9):
        C_, tap, nl = split(tm, wr, w, case["B"][:N], Mw, K, bits, N)
        assert nl >= 1, N
        assert np.array_equal(tap.astype(np.int64), want[:N]), N
        check_bits(C_, Cc[:N])
    w.free()


# -------------------------------------------------------------------------------------------------
# (c) a row is a row

@pytest.mark.parametrize("Mw,K", [(128, 1024), (64, 11008)])
def test_a_row_is_a_row(tm, Mw, K):
    bits, bm, gs, N = 2, 128, 128, 8
    case = orc.make_case(9300 + K, Mw, K, N=N, bits=bits, gs=gs, ags=64, zero_point=True)
    force(tm)
    A, S, wr, w = setup(tm, case, Mw, K, bits, bm, gs, True, N)
    B = case["B"].copy()
    B[6] = B[1]
    C1, _, nl = split(tm, wr, w, B, Mw, K, bits, N, tap=False)
    assert nl >= 1
    check_bits(C1[1], C1[6])                                   # identical activations, identical bits, whatever the position
    B2 = B.copy()
    B2[3] = -0.5 * B[3] + 0.25
    C2, _, _ = split(tm, wr, w, B2, Mw, K, bits, N, tap=False)
    keep = [n for n in range(N) if n != 3]
    check_bits(C1[keep], C2[keep])                             # only row 3 changed
    assert not np.array_equal(C1[3], C2[3])
    for n in range(N):                                         # the same vector as row 0 of an N = 2 call: another capacity, another group
        Bn = np.stack([B[n], B[(n + 1) % N]])
        Cn, _, nl = split(tm, wr, w, Bn, Mw, K, bits, 2, tap=False)
        assert nl >= 1
        check_bits(Cn[0], C1[n])
    w.free()


# -------------------------------------------------------------------------------------------------
# (d) dtypes, fused entry point

@pytest.mark.parametrize("scale_f16", [False, True])
@pytest.mark.parametrize("out_f16", [False, True])
@pytest.mark.parametrize("act_f16", [False, True])
def test_dtypes_fused(tm, act_f16, out_f16, scale_f16):
    import torch
    Mw, K, bits, bm, gs, N = 128, 1024, 2, 128, 128, 4
    case = orc.make_case(9400, Mw, K, N=N, bits=bits, gs=gs, ags=64, zero_point=True, fp16_values=True)
    force(tm)
    A, S, wr, w = setup(tm, case, Mw, K, bits, bm, gs, True, N, scale_f16=scale_f16)
    Cc = oracle_case(case, A, S, Mw, K, bits, bm, 16, gs, 64, True, N=N)[3]
    Bt = torch.from_numpy(case["B"]).cuda()
    if act_f16:
        Bt = Bt.half()
    Ct = torch.full((N, Mw), float("nan"), dtype=torch.float16 if out_f16 else torch.float32, device="cuda")
    l0 = launches(tm)
    wr.fused([w], Bt, [Ct], N)
    torch.cuda.synchronize()
    assert launches(tm) == l0 + 1
    assert rel_err(Ct.float().cpu().numpy(), Cc) <= REL_TOL
    w.free()


# -------------------------------------------------------------------------------------------------
# (e) several matrices, one launch

def test_three_matrices_one_launch(tm):
    import torch
    K, bits, bm, gs, N, rows = 1024, 2, 128, 128, 5, [128, 64, 64]
    cases = [orc.make_case(9500 + i, Mw, K, N=N, bits=bits, gs=gs, ags=64) for i, Mw in enumerate(rows)]
    B = cases[0]["B"]
    force(tm)
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    ws, refs = [], []
    for c, Mw in zip(cases, rows):
        A = orc.preprocess_weights(c["w"], bits, bm, 16)
        S = orc.preprocess_scales(c["sc"], c["zr"], bits, bm)
        refs.append(oracle_case(dict(c, B=B), A, S, Mw, K, bits, bm, 16, gs, 64, True, N=N)[3])
        ws.append(wr.register_weights(A, S, Mw, K, bits, tm.KCfg.make(Mw, K, bits, bm, 16, gs, 64, True, -1, N)))
    Bt = torch.from_numpy(B).cuda()
    outs = [torch.full((N, Mw), float("nan"), dtype=torch.float32, device="cuda") for Mw in rows]
    l0 = launches(tm)
    wr.fused(ws, Bt, outs, N)
    torch.cuda.synchronize()
    assert launches(tm) == l0 + 1
    for o, ref in zip(outs, refs):
        assert rel_err(o.cpu().numpy(), ref) <= REL_TOL
    for w in ws:
        w.free()


# -------------------------------------------------------------------------------------------------
# (f) routing and knobs

def test_routing_and_knobs(tm):
    import torch
    L = tm.lib()
    Mw, K, bits, bm, gs, N = 128, 1024, 2, 128, 128, 4
    case = orc.make_case(9600, Mw, K, N=N, bits=bits, gs=gs, ags=64, zero_point=True)
    A, S, wr, w = setup(tm, case, Mw, K, bits, bm, gs, True, N)
    Bt = torch.from_numpy(case["B"]).cuda()
    Ct = torch.zeros((N, Mw), dtype=torch.float32, device="cuda")
    # mode 1: the routing without the kernel
    force(tm, 1)
    l0 = launches(tm)
    C1, _, nl = split(tm, wr, w, case["B"], Mw, K, bits, N, tap=False)
    C1b, _, _ = split(tm, wr, w, case["B"], Mw, K, bits, N, tap=False)
    wr.fused([w], Bt, [Ct], N)
    torch.cuda.synchronize()
    assert launches(tm) == l0 and nl == 0
    check_bits(C1, C1b)
    # the per-plane taps never run the kernel, in any mode
    for mode in (0, 1, 2):
        force(tm, mode)
        wr.llama_cpp_init(Bt, Mw, K, N, bits)
        l0 = launches(tm)
        wr.partial_sums(w, N)
        wr.fused_partial_sums(w, Bt, N)
        assert launches(tm) == l0, mode
    # reset puts the mode back to auto and the counter to zero
    force(tm, 2)
    C2, _, nl = split(tm, wr, w, case["B"], Mw, K, bits, N, tap=False)
    assert nl >= 1 and launches(tm) >= 1
    assert rel_err(C2, C1) <= 2 * REL_TOL
    with pytest.raises(tm.TMACHipError) as e:
        tm.binding.check(L.tmac_hip_debug_rows_kernel(3))
    assert e.value.code == -4
    w.free()
    tm.binding.check(L.tmac_hip_reset_state())
    assert launches(tm) == 0
    # (mode 0 again: a forced-mode-only route would still count here)
    A, S, wr, w = setup(tm, case, Mw, K, bits, bm, gs, True, N)
    tm.binding.check(L.tmac_hip_set_gemm_min_n(1))          # N = 4 goes to a GEMM: with mode 2 still set the rows kernel would take it
    split(tm, wr, w, case["B"], Mw, K, bits, N, tap=False)
    assert launches(tm) == 0
    tm.binding.check(L.tmac_hip_set_gemm_min_n(32))
    # a recorded chain refuses an N = 4 call as before
    force(tm, 2)
    with pytest.raises(tm.TMACHipError) as e:
        with wr.record_chain():
            wr.fused([w], Bt.half(), [Ct], N)
    assert e.value.code == -1
    # deferred mode: an N = 4 call flushes what is queued, then runs
    x1 = Bt[0].half().contiguous()
    o1 = torch.zeros(Mw, dtype=torch.float16, device="cuda")
    st = [C.c_uint64(0) for _ in range(4)]

    def flushes():
        tm.binding.check(L.tmac_hip_defer_stats(*[C.byref(x) for x in st]))
        return int(st[0].value)
    tm.binding.check(L.tmac_hip_defer(1))
    try:
        wr.fused([w], x1, [o1], 1)
        f0, l0 = flushes(), launches(tm)
        wr.fused([w], Bt, [Ct], N)
        assert flushes() == f0 + 1
        assert launches(tm) == l0 + 1
    finally:
        tm.binding.check(L.tmac_hip_defer(0))
    torch.cuda.synchronize()
    assert rel_err(Ct.cpu().numpy(), C1) <= 2 * REL_TOL
    w.free()


# -------------------------------------------------------------------------------------------------
# (g) saturating inputs

@pytest.mark.parametrize("bits,bm", [(2, 128), (4, 256)])
@pytest.mark.parametrize("weights,acts", [("max", "const"), ("rows", "spike")])
def test_saturating(tm, weights, acts, bits, bm):
    Mw, K, gs, N = 128, 1024, 128, 5
    case = orc.make_hard_case(weights, acts, Mw, K, N=N, bits=bits, gs=gs, ags=64)
    force(tm)
    A, S, wr, w = setup(tm, case, Mw, K, bits, bm, gs, True, N)
    q, ls, lb, Cc, PS = oracle_case(case, A, S, Mw, K, bits, bm, 16, gs, 64, True, N=N)
    orc.assert_saturates(weights, acts, q[0], PS[0], 64, K)
    assert np.abs(Cc).max() > 100                       # the outputs do not cancel: rel_err means something
    C_, tap, nl = split(tm, wr, w, case["B"], Mw, K, bits, N)
    assert nl >= 1
    assert np.array_equal(tap.astype(np.int64), comb_of(PS, Mw, bits))
    assert rel_err(C_, Cc) <= REL_TOL
    w.free()


# -------------------------------------------------------------------------------------------------
# (h) footprint

@pytest.mark.parametrize("out_f16", [False, True])
@pytest.mark.parametrize("entry", ["split", "fused"])
def test_footprint(tm, entry, out_f16):
    """no store outside [C, C + N Mw), no guard value in a result: a part-filled group (5 of 8 rows) reads no image row beyond N"""
    Mw, K, bits, bm, gs, N = 512, 1024, 2, 128, 128, 5
    c = orc.make_case(9700, Mw, K, bits=bits, N=N, gs=gs, ags=64, zero_point=True)
    force(tm)
    A, S, wr, w = setup(tm, c, Mw, K, bits, bm, gs, True, N)
    Cc = oracle_case(c, A, S, Mw, K, bits, bm, 16, gs, 64, True, N=N)[3]
    seen = []

    def call(alloc):
        Bt = alloc.inp(c["B"], np.float32, name="B")
        Ct = alloc.out((N, Mw), np.float16 if out_f16 else np.float32, name="C")
        alloc.arm()
        l0 = launches(tm)
        if entry == "split":
            wr.llama_cpp_init(Bt, Mw, K, N, bits)
            wr.llama_cpp_compute(w, Ct, N)
        else:
            wr.fused([w], Bt, [Ct], N)
        seen.append(launches(tm) - l0)

    def check_want(want):
        assert rel_err(want["C"].astype(np.float32), Cc) <= REL_TOL

    fp.check_footprint(call, check_want=check_want)
    assert seen and all(s == 1 for s in seen)
    tm.binding.check(tm.lib().tmac_hip_cache_clear())
    w.free()


# -------------------------------------------------------------------------------------------------
# (i) graph capture

def test_graph_capture(tm):
    import torch
    Mw, K, bits, bm, gs, N = 128, 1024, 2, 128, 128, 4
    cases = [orc.make_case(9800 + i, Mw, K, N=N, bits=bits, gs=gs, ags=64, zero_point=True) for i in range(2)]
    force(tm)
    A, S, wr, w = setup(tm, cases[0], Mw, K, bits, bm, gs, True, N)
    x = torch.from_numpy(cases[0]["B"]).cuda().half()
    out = torch.zeros((N, Mw), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        wr.fused([w], x, [out], N)                      # warm-up: the library's per-stream workspace exists before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    l0 = launches(tm)
    with torch.cuda.graph(g, stream=side):
        wr.fused([w], x, [out], N)                      # a single linear chain: LUT build, then k_gemv_rows
    assert launches(tm) == l0 + 1
    for c in cases[::-1]:
        Bh = torch.from_numpy(c["B"]).cuda().half()
        x.copy_(Bh)
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        Cc = oracle_case(dict(c, B=Bh.float().cpu().numpy()), A, S, Mw, K, bits, bm, 16, gs, 64, True, N=N)[3]
        assert rel_err(out.cpu().numpy(), Cc) <= REL_TOL
    del g
    w.free()
