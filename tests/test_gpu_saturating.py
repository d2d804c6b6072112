"""Saturating inputs on every kernel: worst-case weights and tables (oracle.make_hard_case).

The other GPU files draw uniformly random weight levels and standard-normal activations: every integer partial sum is a random walk
around zero and no accumulator comes near its limit.  Here the weights are constant or alternate between the extremes (max, min, rows,
planes, kblocks) and the activations give tables of {+-127, +-64, 0} (const, negblocks) or of +-127 only (spike): a 16-lookup packed sum
sits at 16 x 254 (or 16 x 0) of its 12-bit field, an act group of 64 at +-2032, a unified-scale total at +-127 K / 4, the halving trees
at +-127, and k_gemm_planes' entry sums at their largest.

Every test first asserts ON THE ORACLE'S OWN RESULTS that its input saturates (orc.assert_saturates), then holds the kernel to the bars
the neighbouring file already uses for it (test_gpu_parity.py, test_gpu_gemm_planes.py, test_gpu_chain.py, test_gpu_stream.py): integers
array_equal, LUT scales / biases by bits, fp32 outputs within the fp32 re-association bound, unified-scale outputs by bits.  The oracle's
answers for these inputs are pinned to the reference's in tests/test_oracle_vs_ref.py (golden/ref/saturating.npz).
"""
import numpy as np
import pytest

from oracle import oracle as orc
from test_gpu_chain import BITS_BM, Model, tm, _short_spin, rel_err      # noqa: F401  (fixtures)
from test_gpu_gemm_planes import mrow, run as run_planes
from test_gpu_parity import REL_TOL, check_bits, oracle_case, run_case

pytestmark = pytest.mark.gpu

# weights x activations of the N = 1 tests
COMBOS = [(w, "const") for w in orc.HARD_WEIGHTS] + [("max", "spike"), ("rows", "spike"), ("max", "negblocks")]
COMBO_IDS = [f"{w}-{a}" for w, a in COMBOS]


def group_size(acts, gs):
    """negblocks under per-group scales, N = 1: with constant weights a weight group of 128 holds +0.75 x 64 and -0.75 x 64 under one
    scale and zero point, and EVERY output is exactly zero -- an error relative to max|C| would mean nothing.  Weight groups of 64, one
    per sign block, keep the outputs in the hundreds (the integer sums are the same either way)."""
    return 64 if acts == "negblocks" else gs


def sums_of_row0(PS):
    """oracle_case's integers of activation row 0: [M][K/ags], or the [M] totals of the unified-scale path"""
    return PS[0]


# -------------------------------------------------------------------------------------------------
# split path: preprocessor + GEMV, every variant

SPLIT_CFGS = [  # Mw, K, bits, bm, kf, gs, ags, zp, m_groups
    (256, 1024, 1, 128, 16, 128, 64, True, -1), (128, 1024, 2, 128, 16, 128, 64, True, -1),
    (128, 1024, 3, 192, 16, 128, 64, True, -1), (128, 1024, 4, 256, 16, 128, 64, True, -1),
    (128, 1024, 2, 128, 8, 128, 32, True, -1),            # act group 32: +-1016 per group
    (160, 3200, 2, 320, 16, 128, 3200, False, 1),         # unified scale: one running total across the whole K
    (64, 12288, 4, 256, 16, 128, 12288, False, 1), (64, 12288, 3, 192, 16, 128, 12288, False, 1),
    (128, 8640, 1, 128, 16, 128, 8640, False, 1),
]


@pytest.mark.parametrize("weights,acts", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("Mw,K,bits,bm,kf,gs,ags,zp,mg", SPLIT_CFGS)
def test_split_path(tm, Mw, K, bits, bm, kf, gs, ags, zp, mg, weights, acts):
    """every GEMV variant (0, 1, 2, 4, 5, 7: the tiled / fused layouts with the MFMA and the v_mqsad accumulate; 3: the reference-layout
    kernel) on saturated tables and constant weights: QLUT, scales, biases and integer sums bit-exact, outputs within 2e-5 (variant 3 and
    the unified-scale path: by bits).  Under a unified scale kblocks x const and max x negblocks do not saturate the total: it swings by
    +-2032 per 64-element block and ends at 0 (K = 8640, 135 blocks: +-2032), which assert_saturates pins; the outputs of kblocks x const are
    then the bias term alone (or nearly) and those of max x negblocks exactly zero (the activations sum to zero over the one act group),
    compared by bits like the others.  The negblocks cases with per-group scales take weight groups of 64
    (group_size)."""
    gs = group_size(acts, gs) if mg == -1 else gs
    case = orc.make_hard_case(weights, acts, Mw, K, bits=bits, gs=gs, ags=ags, zero_point=zp, m_groups=mg)
    A = orc.preprocess_weights(case["w"], bits, bm, kf)
    S = orc.preprocess_scales(case["sc"], case["zr"] if zp else None, bits, bm) if mg == -1 else case["sc"]
    q, ls, lb, Cc, PS = oracle_case(case, A, S, Mw, K, bits, bm, kf, gs, ags, zp, mg)
    orc.assert_saturates(weights, acts, q[0], sums_of_row0(PS), ags, K)
    # per-group scales: the outputs do not cancel, rel_err means something.  (Unified-scale outputs are compared by bits, which needs no
    # scale: they are exactly zero for max x negblocks, whose activations sum to zero over the one act group, and for 1-bit max weights,
    # whose real value (level - 1) is zero -- the saturated total and the bias term then cancel exactly, in the kernel as in the oracle.)
    assert mg != -1 or np.abs(Cc).max() > 100
    ran = []
    for variant in (0, 1, 2, 4, 5, 7, 3):
        try:
            r = run_case(tm, case, Mw, K, bits, bm, kf, gs, ags, zp, mg, variant=variant)
        except tm.binding.TMACHipError as e:
            if variant and e.code == -1:          # this variant has no kernel for the configuration
                tm.lib().tmac_hip_set_variant(0)
                continue
            raise
        ran.append(variant)
        assert np.array_equal(r["q"], q), variant
        check_bits(r["ls"], ls); check_bits(r["lb"], lb)
        assert np.array_equal(np.asarray(r["PS"]).reshape(PS.shape), PS), variant
        print(f"variant {variant}: rel_err {rel_err(r['C'], Cc):.3e}")
        assert rel_err(r["C"], Cc) <= 2e-5, variant
        if variant == 3 or mg != -1:
            check_bits(r["C"], Cc)
    assert 0 in ran


# -------------------------------------------------------------------------------------------------
# fused decode kernel (k_gemv_quad): LUT built inside the kernel

@pytest.mark.parametrize("weights,acts", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("act_f16", [False, True])
@pytest.mark.parametrize("bits,bm", [(2, 128), (4, 256)])
@pytest.mark.parametrize("K", [1024, 11008])
def test_fused_decode_kernel(tm, K, bits, bm, act_f16, weights, acts):
    """the in-kernel LUT build on the 63.5 tie and on tables of +-127 only, its biased half tables and packed accumulate with every nibble
    0 or 15, K = 11008 with the ragged last step: integer sums array_equal, LUT scales / biases by bits, C within 2e-5"""
    import torch
    Mw, kf, gs, ags = 128, 16, group_size(acts, 128), 64
    case = orc.make_hard_case(weights, acts, Mw, K, bits=bits, gs=gs, ags=ags)
    A = orc.preprocess_weights(case["w"], bits, bm, kf)
    S = orc.preprocess_scales(case["sc"], case["zr"], bits, bm)
    q, ls, lb, Cc, PSo = oracle_case(case, A, S, Mw, K, bits, bm, kf, gs, ags, True)
    orc.assert_saturates(weights, acts, q[0], sums_of_row0(PSo), ags, K)
    assert np.abs(Cc).max() > 100                       # the outputs do not cancel: rel_err means something
    Bt = torch.from_numpy(case["B"]).cuda()           # fp16-representable values: the fp16 path sees the same numbers
    if act_f16:
        Bt = Bt.half()
    for variant in (0, 7):                            # the quad kernel's MFMA (default) and v_mqsad accumulate
        tm.binding.check(tm.lib().tmac_hip_set_variant(variant))
        wr = tm.TMACGeMMWrapper(act_group_size=ags)
        wr.set_workspace(K, 1)
        w = wr.register_weights(A, S, Mw, K, bits, tm.KCfg.make(Mw, K, bits, bm, kf, gs, ags, True))
        PS, Cf = wr.fused_partial_sums(w, Bt)
        assert np.array_equal(PS, PSo), variant
        check_bits(wr.last_fused_lut[:, 0, :], ls)
        check_bits(wr.last_fused_lut[:, 1, :], lb)
        print(f"variant {variant}: rel_err {rel_err(Cf, Cc):.3e}")
        assert rel_err(Cf, Cc) <= 2e-5, variant
        w.free()
    tm.lib().tmac_hip_set_variant(0)


# -------------------------------------------------------------------------------------------------
# fast aggregation: the halving-adder trees with +-127 at every leaf

@pytest.mark.parametrize("variant", [0, 3])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("weights", ["max", "min", "rows"])
@pytest.mark.parametrize("bits,bm,kf,ags", [(2, 128, 16, 64), (4, 256, 16, 64), (2, 128, 8, 32)])
def test_fast_aggregation(tm, bits, bm, kf, ags, weights, mode, variant):
    """both flavours of the tree (test_fast_aggregation_vs_oracle's bars without its NMSE-vs-exact clause, a statement about random data):
    tree results array_equal and touching +-127, variant 3 by bits, mode 1 within 1e-3, mode 2 within 1e-4"""
    Mw, K, gs = 128, 2048, 128
    case = orc.make_hard_case(weights, "const", Mw, K, bits=bits, gs=gs, ags=ags)
    A = orc.preprocess_weights(case["w"], bits, bm, kf)
    S = orc.preprocess_scales(case["sc"], case["zr"], bits, bm)
    q, ls, lb = orc.preprocessor(case["B"], ags)
    orc.assert_saturates(weights, "const", q[0], orc.partial_sums(A, q[0], Mw, K, bits, bm, kf, ags), ags, K)
    Cc, tap = orc.qgemm_float_fa(A, q, S, ls, lb, Mw, K, 1, bits, bm, kf, gs, ags, True, mode)
    # the tree results sit at the extremes themselves: +127 (max), -127 (min), both (rows)
    assert tap.max() == (127 if weights != "min" else -127) and tap.min() == (-127 if weights != "max" else 127)
    r = run_case(tm, case, Mw, K, bits, bm, kf, gs, ags, True, variant=variant, fast_aggregation=mode)
    assert np.array_equal(r["q"], q)
    check_bits(r["ls"], ls); check_bits(r["lb"], lb)
    assert np.array_equal(r["PS"], tap)
    print(f"rel_err {rel_err(r['C'], Cc):.3e}")
    if variant == 3:
        check_bits(r["C"], Cc)
    elif mode == 1:
        assert rel_err(r["C"], Cc) < REL_TOL
    else:
        assert np.abs(r["C"] - Cc).max() <= 1e-4 * np.abs(Cc).max()


# -------------------------------------------------------------------------------------------------
# k_gemm_onehot (N > 1); activation rows cycle const, negblocks, spike, standard normal

@pytest.mark.parametrize("weights,acts", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("N", [5, 33])
@pytest.mark.parametrize("Mw,K,bits,bm,ags,zp,mg", [(256, 1024, 2, 128, 64, True, -1), (256, 1024, 4, 256, 64, True, -1),
                                                    (320, 3200, 2, 320, 3200, False, 1)])
def test_onehot_gemm(tm, Mw, K, bits, bm, ags, zp, mg, N, weights, acts):
    """one-hot(nibble) x QLUT on the matrix cores with every nibble 0 or 15: integer sums array_equal; per-group outputs within 2e-5,
    unified-scale outputs (and the row-wise build's scales / biases) by bits.  gemm_min_n = 1 alone would hand the untapped launch -- the
    one whose outputs are read -- to k_gemm_planes, which covers every shape here; tmac_hip_debug_gemm_kernel(1) keeps it on
    k_gemm_onehot, as test_gpu_gemm_planes.run(kernel=1) does.  (Unified scale, kblocks x const and max x negblocks: the totals of row 0
    cancel to 0 -- assert_saturates pins that -- and the other activation rows of the cycle carry the saturated totals.)"""
    case = orc.make_hard_case(weights, acts, Mw, K, N=N, bits=bits, gs=128, ags=ags, zero_point=zp, m_groups=mg)
    A = orc.preprocess_weights(case["w"], bits, bm, 16)
    S = orc.preprocess_scales(case["sc"], case["zr"], bits, bm) if mg == -1 else case["sc"]
    q, ls, lb, Cc, PS = oracle_case(case, A, S, Mw, K, bits, bm, 16, 128, ags, zp, m_groups=mg, N=N)
    orc.assert_saturates(weights, acts, q[0], sums_of_row0(PS), ags, K)
    assert np.abs(PS).max() == 127 * ags // 4          # some row of the cycle drives the sums to the limit whatever row 0 does
    assert np.abs(Cc).max() > 100
    tm.binding.check(tm.lib().tmac_hip_debug_gemm_kernel(1))
    try:
        r = run_case(tm, case, Mw, K, bits, bm, 16, 128, ags, zp, m_groups=mg, N=N, gemm_min_n=1)
    finally:
        tm.lib().tmac_hip_debug_gemm_kernel(0)
    assert np.array_equal(r["q"], q)
    assert np.array_equal(np.asarray(r["PS"]).reshape(PS.shape), PS)
    print(f"rel_err {rel_err(r['C'], Cc):.3e}")
    if mg == -1:
        assert rel_err(r["C"], Cc) <= 2e-5
    else:
        check_bits(r["ls"], ls); check_bits(r["lb"], lb)
        check_bits(r["C"], Cc)


# -------------------------------------------------------------------------------------------------
# k_gemm_planes / k_gemm_planes_us, both workgroup forms

PLANES_BM = {1: 64, 2: 128, 3: 192, 4: 256}
FORMS = [2, 3]


@pytest.mark.parametrize("weights", orc.HARD_WEIGHTS)
@pytest.mark.parametrize("N", [5, 70])
@pytest.mark.parametrize("Mw,K,bits,gs", [(128, 1024, 1, 128), (128, 1024, 2, 128), (192, 1024, 3, 128), (256, 1024, 4, 128),
                                          (128, 1024, 2, 256)])
def test_gemm_planes(tm, Mw, K, bits, gs, N, weights):
    """the bit-planes folded into one int8 operand with every plane at an extreme (planes: neighbouring planes at opposite extremes), the
    3- / 4-bit rows' BIASB x entry-sum correction with entry sums of +-127 x 128: LUT image (entries, scales, biases, entry sums)
    bit-exact, comb = sum_p 2^p PS_p array_equal, outputs within 1e-5"""
    bm = PLANES_BM[bits]
    case = orc.make_hard_case(weights, "const", Mw, K, N=N, bits=bits, gs=gs, ags=64)
    A = orc.preprocess_weights(case["w"], bits, bm, 16)
    S = orc.preprocess_scales(case["sc"], case["zr"], bits, bm)
    q, ls, lb = orc.preprocessor(case["B"], 64)
    PS = np.stack([orc.partial_sums(A, q[n], Mw, K, bits, bm, 16, 64) for n in range(N)])       # [N][M][G]
    orc.assert_saturates(weights, "const", q[0], PS[0], 64, K)
    rows = np.arange(Mw)
    comb = sum((PS[:, mrow(rows, p, bits), :].astype(np.int64) << p) for p in range(bits))
    Cc = orc.qgemm_float(A, q, S, ls, lb, Mw, K, N, bits, bm, 16, gs, 64, True)
    for form in FORMS:
        r = run_planes(tm, case, Mw, K, bits, bm, gs, True, N, kernel=form)
        h, gls, glb, hs = r["img"]
        assert np.array_equal(h, q[:, :, :8]), form
        check_bits(gls, ls); check_bits(glb, lb)
        assert np.array_equal(hs, q[:, :, :8].astype(np.int32).reshape(N, K // 64, 128).sum(-1).astype(np.float32)), form
        assert np.array_equal(r["comb"].astype(np.int64), comb), form
        print(f"form {form}: rel_err {rel_err(r['C'], Cc):.3e}")
        assert rel_err(r["C"], Cc) <= 1e-5, form


def run_planes_us(tm, case, Mw, K, bits, bm, N, form):
    """test_gemm_planes_unified_scale's launch: LUT image, combined totals and outputs of k_gemm_planes_us"""
    import torch
    L = tm.lib()
    tm.binding.check(L.tmac_hip_set_gemm_min_n(1))
    tm.binding.check(L.tmac_hip_debug_gemm_kernel(form))
    try:
        A = orc.preprocess_weights(case["w"], bits, bm, 16)
        cfg = tm.KCfg.make(Mw, K, bits, bm, 16, 128, K, False, 1, N)
        wr = tm.TMACGeMMWrapper(act_group_size=K)
        wr.set_workspace(K, N)
        w = wr.register_weights(A, case["sc"], Mw, K, bits, cfg, scales_dtype=tm.F32, dev_dtype=tm.F32)
        Bt = torch.from_numpy(case["B"]).cuda()
        Ct = torch.full((N, Mw), float("nan"), dtype=torch.float32, device="cuda")
        wr.llama_cpp_init(Bt, Mw, K, N, bits)
        wr.llama_cpp_compute(w, Ct, N)
        torch.cuda.synchronize()
        out = dict(img=wr.workspace.read_gemm_image(K, N, act_group_size=K), comb=wr.comb_sums(w, N), C=Ct.cpu().numpy())
        w.free()
        return out
    finally:
        L.tmac_hip_debug_gemm_kernel(0)
        L.tmac_hip_set_gemm_min_n(32)


@pytest.mark.parametrize("weights", orc.HARD_WEIGHTS)
@pytest.mark.parametrize("N", [5, 70])
@pytest.mark.parametrize("Mw,K,bits,bm", [(320, 3200, 2, 320), (192, 12288, 3, 192), (192, 12288, 4, 256)])
def test_gemm_planes_unified_scale(tm, Mw, K, bits, bm, N, weights):
    """k_gemm_planes_us with one total across K = 12288 and the largest entry sums the BIASB correction of 3- / 4-bit rows meets
    (+-127 x 8 x K / 4, carried as an fp32 number): LUT image and combined totals bit-exact, outputs BIT-IDENTICAL to scale-final"""
    case = orc.make_hard_case(weights, "const", Mw, K, N=N, bits=bits, ags=K, zero_point=False, m_groups=1)
    A = orc.preprocess_weights(case["w"], bits, bm, 16)
    q, ls, lb = orc.preprocessor(case["B"], K)
    Cc, cb = orc.qgemm_scale_final(A, q, case["sc"], ls[:, 0], lb[:, 0], Mw, K, N, bits, bm, 16, 1)      # cb: int32 [N][M] per-plane totals
    orc.assert_saturates(weights, "const", q[0], cb[0], K, K)
    rows = np.arange(Mw)
    want = sum((cb[:, mrow(rows, p, bits)].astype(np.int64) << p) for p in range(bits))
    for form in FORMS:
        r = run_planes_us(tm, case, Mw, K, bits, bm, N, form)
        h, gls, glb, hs = r["img"]
        assert np.array_equal(h, q[:, :, :8]), form
        check_bits(gls, ls); check_bits(glb, lb)
        assert np.array_equal(hs[:, 0], q[:, :, :8].astype(np.int32).reshape(N, -1).sum(-1).astype(np.float32)), form
        assert np.array_equal(r["comb"][:, :, 0].astype(np.int64), want), form
        check_bits(r["C"], Cc)


# -------------------------------------------------------------------------------------------------
# persistent kernels: k_gemv_stream (both item forms) and k_decode_chain

@pytest.fixture(params=["auto", "quad64"])
def _form(request, monkeypatch):
    """test_gpu_stream.py's two item forms of k_gemv_stream: the default choice, and row quad x 64 units forced"""
    if request.param == "quad64":
        monkeypatch.setenv("TMAC_STREAM_QW", "0")
    return request.param


STREAM_WEIGHTS = ["max", "rows", "min", "planes", "kblocks"]
STREAM_ACTS = ["const", "negblocks", "spike", "const", "spike"]


def pattern_names(i, m=0):
    """matrix m of op i takes weight pattern (i + m) mod 5 of STREAM_WEIGHTS, op i's external vector pattern i mod 5 of STREAM_ACTS
    (amplitude 0.75 / 3: the models below stay inside fp16, checked with the oracle by assert_model_in_range before anything runs).
    The negblocks vector (op 1) meets kblocks weights in every matrix of its op: weights constant along K would cancel to outputs of
    exactly zero under the model's weight groups of 128 (see group_size), while kblocks x negblocks keeps one sign -- and under a unified
    scale drives the running total to +-127 K / 4.  No matrix of the lists below shares its pattern with a matrix of the op before or
    after it (ops 0-3: max / rows, kblocks, min / planes, planes)."""
    a = STREAM_ACTS[i % 5]
    return ("kblocks" if a == "negblocks" else STREAM_WEIGHTS[(i + m) % 5]), a


def pattern_weights(i, m, Mw, K, bits):      # weights_fn of Model
    return orc.hard_weights(pattern_names(i, m)[0], Mw, K, bits)


def pattern_acts(i, K):                      # x_fn of Model
    return orc.hard_acts(pattern_names(i)[1], K)


def assert_model_in_range(m, names=pattern_names):
    """The oracle alone, on the CPU, op after op (handed-over vectors rounded to fp16 as the kernels store them): every output finite,
    non-zero somewhere and inside fp16 -- and the integers of every call fed by an external vector saturate."""
    outs = []
    for i, (K, rows, src) in enumerate(m.ops):
        x = m.x_ext[i].float().cpu().numpy() if src is None else outs[src[0]][src[1]]
        o = [c.astype(np.float16).astype(np.float32) for c in m.oracle_outputs(i, x)]
        for c in o:
            assert np.isfinite(c).all() and 0 < np.abs(c).max() < 65504, f"op {i}: the model leaves fp16"
        outs.append(o)
        if src is None:
            ags = K if m.mg >= 1 else 64
            q, _, _ = orc.preprocessor(x[None, :], ags)
            PS = orc.partial_sums(m.host[i][0][0], q[0], rows[0], K, m.bits, BITS_BM[m.bits], 16, ags)
            orc.assert_saturates(*names(i), q[0], PS, ags, K)


STREAM_OPS = [(1024, [256, 128], None), (2688, [128], None), (11008, [128], None), (4096, [256], None)]
STREAM_US_OPS = [(3200, [320], None), (8640, [128], None), (18432, [128, 128], None)]
STREAM_LARGE_OPS = [(18432, [128], None), (16384, [64, 128], None)]


def _run_stream(tm, ops, **kw):
    m = Model(tm, ops, weights_fn=pattern_weights, x_fn=pattern_acts, **kw)
    assert_model_in_range(m)
    chain = m.record()
    assert chain.stream
    chain.launch()
    m.check(chain)
    m.check_tap(chain)
    chain.free()
    m.free()


@pytest.mark.parametrize("bits,zp", [(2, True), (4, True), (2, False)])
def test_stream(tm, _form, bits, zp):
    """k_lut_images + k_gemv_stream, consecutive calls with different weight patterns and saturated tables, K = 2688 and 11008 with ragged
    last steps: every call bit-identical to its stand-alone launch (the quarter-walk form: within test_gpu_chain.Model.check's bound),
    within 1e-3 of the oracle, and the kernel's own integers array_equal to the oracle's"""
    _run_stream(tm, STREAM_OPS, bits=bits, zp=zp, seed=60 + bits + zp)


def _run_largest_K(tm, ops, form, monkeypatch, mg, seed):
    """test_stream_largest_K's bars (k_gemv_quad has no launch configuration of its own for these K): the oracle (1e-3; unified scales:
    bits), k_gemv_stream's own integers, and -- for the row quad x 64 form -- the same recording through k_decode_chain, bit for bit"""
    import torch
    if form == "quad64":
        monkeypatch.setenv("TMAC_STREAM_NCLS", "1")      # every row range visits every call, as k_decode_chain's workgroups do
    m = Model(tm, ops, mg=mg, seed=seed, zp=mg < 1, weights_fn=pattern_weights, x_fn=pattern_acts)
    assert_model_in_range(m)
    s = m.record()
    assert s.stream
    s.launch(); torch.cuda.synchronize()
    assert s.status() == 0
    got = [[o.clone() for o in os_] for os_ in m.outs]
    for i in range(len(ops)):
        want = m.oracle_outputs(i, m.x_ext[i].float().cpu().numpy())
        for k in range(len(want)):
            g = got[i][k].cpu().numpy()
            if mg >= 1:
                assert np.array_equal(g.view(np.uint16), want[k].astype(np.float16).view(np.uint16)), (i, k)
            assert rel_err(g.astype(np.float32), want[k]) <= 1e-3, (i, k)
    m.check_tap(s)
    if form == "quad64":
        for os_ in m.outs:
            for o in os_:
                o.zero_()
        monkeypatch.setenv("TMAC_CHAIN_STREAM", "0")
        c = m.record()
        monkeypatch.delenv("TMAC_CHAIN_STREAM")
        assert not c.stream
        c.launch(); torch.cuda.synchronize()
        assert c.status() == 0
        for x, y in zip(got, m.outs):
            for p, q in zip(x, y):
                assert torch.equal(p, q)
        c.free()
    s.free(); m.free()


def test_stream_unified_scale(tm, _form, monkeypatch):
    """k_lut_images_us + k_gemv_stream with one int32 total per plane across K = 3200 / 8640 / 18432: +-127 K / 4 = +-585216 at the
    persistent kernels' largest K.  The calls below K = 16384 also against their stand-alone launches (Model.check)."""
    _run_stream(tm, STREAM_US_OPS[:2], mg=1, zp=False, seed=71)
    _run_largest_K(tm, STREAM_US_OPS, _form, monkeypatch, 1, 72)


def test_stream_largest_K(tm, _form, monkeypatch):
    """per-group scales at K = 18432 and 16384: 288 / 256 act groups of +-2032 each, in both item forms"""
    _run_largest_K(tm, STREAM_LARGE_OPS, _form, monkeypatch, -1, 73)


CHAIN_OPS = [(1024, [1024], None), (1024, [256], (0, 0)), (256, [128, 64], (1, 0))]


@pytest.mark.parametrize("mg", [-1, 1])
def test_dependent_chain(tm, mg):
    """k_decode_chain: rows / max weights in turn; the saturated external vector feeds only op 0, the later ops consume what the chain
    produced (assert_model_in_range: the oracle alone keeps every vector finite, non-zero and inside fp16).  Every op bit-identical to
    its stand-alone launch, within 1e-3 of the oracle (unified scale, fp16 outputs: by bits), integers array_equal"""
    names = lambda i, m=0: (("rows", "max")[(i + m) % 2], "const")      # noqa: E731
    m = Model(tm, CHAIN_OPS, mg=mg, zp=mg < 1, seed=80 + mg, weights_fn=lambda i, k, Mw, K, bits: orc.hard_weights(names(i, k)[0], Mw, K, bits),
              x_fn=lambda i, K: orc.hard_acts("const", K))
    assert_model_in_range(m, names)
    chain = m.record()
    assert not chain.stream and chain.nops == len(CHAIN_OPS)
    for rep in range(2):
        chain.launch()
        m.check(chain, oracle_ops=None if rep == 0 else [])
    m.check_tap(chain)
    chain.free()
    m.free()
