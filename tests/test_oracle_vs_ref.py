"""Pins the scalar oracle (oracle/tmac_oracle.c) against the reference itself.

The reference's answers for the inputs drawn here -- its Python weight transform, its intrinsics (lut_ctor.cc / tbl.cc) and its
checked-in prebuilt kernel sets, compiled by `make -C oracle ref` -- are recorded in tests/golden/ref/oracle_vs_ref.npz by
tests/golden/make_golden.py, which builds its inputs with the helpers below.  Everything here is CPU-only.
"""
import os

import numpy as np
import pytest

from oracle import oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref", "oracle_vs_ref.npz")


@pytest.fixture(scope="module")
def ref():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


# ---- the inputs (shared with tests/golden/make_golden.py, which records the reference's answers for them) ----
PRE_CASES = [(256, 64), (4096, 64), (11008, 64), (1024, 32), (3200, 3200), (8640, 8640)]
PW_CASES = [(1, 128, 16), (2, 128, 16), (2, 256, 16), (3, 192, 16), (4, 256, 16), (2, 128, 8), (2, 320, 16)]


def preprocessor_input(K, ags):
    return np.random.default_rng(K + ags).standard_normal((1, K)).astype(np.float32)


def edge_input():
    # zero group (scale 0 -> t_scales 0), huge dynamic range, exact ties for RNE
    B = np.zeros((1, 256), np.float32)
    B[0, 64:128] = np.linspace(-3, 3, 64, dtype=np.float32)
    B[0, 128:192] = 1e-30
    B[0, 192:256] = np.tile(np.array([0.5, 1.5, 2.5, 127.0], np.float32), 16)
    return B


def pw_case(bits, bm, kfactor):
    Mw, K = bm // bits * 3 if bm != 320 else 480, 512
    return orc.make_case(7, Mw, K, bits=bits)


def float_case(bits, bm, kfactor, gs, ags, zp, fa=False):
    """(A, S, q, ls, lb, case) of the float-path tests; fa: the FastAggregation test's seed"""
    Mw, K = bm // bits * 2, 1024
    case = orc.make_case((5 * bits + ags + 1) if fa else (11 * bits + ags), Mw, K, bits=bits, gs=gs, ags=ags, zero_point=zp)
    A = orc.preprocess_weights(case["w"], bits, bm, kfactor)
    S = orc.preprocess_scales(case["sc"], case["zr"], bits, bm)
    q, ls, lb = orc.preprocessor(case["B"], ags)
    return A, S, q, ls, lb, case


def prebuilt_case(bits, bm, Mw, K):
    case = orc.make_case(0, Mw, K, bits=bits, zero_point=True)
    return orc.preprocess_weights(case["w"], bits, bm, 16), orc.preprocess_scales(case["sc"], case["zr"], bits, bm), case


def int32_case(bits, bm, Mw, K):
    case = orc.make_case(5, Mw, K, bits=bits, m_groups=1, ags=K, zero_point=False)
    A = orc.preprocess_weights(case["w"], bits, bm, 16)
    q, ls, lb = orc.preprocessor(case["B"], K)
    return A, q, ls, lb, case


def key(*parts):
    return "_".join(str(int(p) if isinstance(p, bool) else p) for p in parts)


@pytest.mark.parametrize("K,ags", PRE_CASES)
def test_preprocessor_bit_exact(ref, K, ags):
    B = preprocessor_input(K, ags)
    q, ls, lb = orc.preprocessor(B, ags)
    qr, lsr, lbr = (ref[key("pre", K, ags, n)] for n in ("q", "ls", "lb"))
    assert np.array_equal(q[0], qr)
    assert np.array_equal(ls[0].view(np.uint32), lsr.view(np.uint32))
    assert np.array_equal(lb[0].view(np.uint32), lbr.view(np.uint32))


def test_preprocessor_edge_values(ref):
    B, ags = edge_input(), 64
    q, ls, lb = orc.preprocessor(B, ags)
    qr, lsr, lbr = (ref[key("edge", n)] for n in ("q", "ls", "lb"))
    assert np.array_equal(q[0], qr) and np.array_equal(ls[0], lsr) and np.array_equal(lb[0], lbr)
    assert ls[0, 0] == 0 and not q[0, :16].any()
    # exact antisymmetry the GPU half-table relies on (lut_ctor.cc:152-155)
    assert np.array_equal(q[0][:, ::-1].astype(np.int16), -q[0].astype(np.int16))


@pytest.mark.parametrize("bits,bm,kfactor", PW_CASES)
def test_preprocess_weights_matches_reference_python(ref, bits, bm, kfactor):
    case = pw_case(bits, bm, kfactor)
    A = orc.preprocess_weights(case["w"], bits, bm, kfactor)
    assert np.array_equal(A, ref[key("pw", bits, bm, kfactor, "A")])
    S = orc.preprocess_scales(case["sc"], case["zr"], bits, bm)
    assert np.array_equal(S, ref[key("pw", bits, bm, kfactor, "S")].astype(np.float32))
    S1 = orc.preprocess_scales(case["sc"], None, bits, bm)
    assert np.array_equal(S1, ref[key("pw", bits, bm, kfactor, "S1")].astype(np.float32))


CFGS = [  # bits, bm, kfactor, gs, ags, zp
    (2, 128, 16, 128, 64, True), (2, 128, 16, 128, 64, False), (4, 256, 16, 128, 64, True),
    (1, 128, 16, 128, 64, True), (3, 192, 16, 128, 64, False), (2, 128, 8, 128, 32, True),
    (2, 128, 16, 128, 32, True), (4, 256, 8, 64, 32, True),
]


def has_int_partial_sums(bits, kfactor, ags):
    return ags % (4 * kfactor) == 0 and (kfactor, bits) in [(16, 1), (16, 2), (16, 3), (16, 4), (8, 2)]


@pytest.mark.parametrize("bits,bm,kfactor,gs,ags,zp", CFGS)
def test_float_path_bit_exact_vs_reference_intrinsics(ref, bits, bm, kfactor, gs, ags, zp):
    A, S, q, ls, lb, case = float_case(bits, bm, kfactor, gs, ags, zp)
    Mw, K = case["w"].shape
    Cor = orc.qgemm_float(A, q, S, ls, lb, Mw, K, 1, bits, bm, kfactor, gs, ags, zp)
    Cref = orc.combine_planes(ref[key("fp", bits, bm, kfactor, gs, ags, zp, "cbits")], Mw, bits)
    assert np.array_equal(Cor[0].view(np.uint32), Cref.view(np.uint32))
    # integer partial sums: scalar restatement == reference int32 intrinsic per act group
    if has_int_partial_sums(bits, kfactor, ags):
        PS = orc.partial_sums(A, q[0], Mw, K, bits, bm, kfactor, ags)
        assert np.array_equal(PS, ref[key("fp", bits, bm, kfactor, gs, ags, zp, "ps")])
    # and the statistical check of tests/test_e2e.py (NMSE <= 5e-4, qgemm.py:277-282)
    Cdq = orc.dequant_matmul(case["w"], case["sc"], case["zr"], case["B"], bits, gs)[0]
    nmse = np.mean((Cdq - Cor[0]) ** 2) / np.mean(Cdq ** 2)
    assert nmse < 5e-4


FA_CFGS = [  # bits, bm, kfactor, gs, ags, zp  (the FastAggregation = true instantiations of oracle/ref_shim.cc)
    (2, 128, 16, 128, 64, True), (2, 128, 16, 128, 64, False), (4, 256, 16, 128, 64, True), (4, 256, 16, 128, 64, False),
    (1, 128, 16, 128, 64, True), (3, 192, 16, 128, 64, True), (2, 128, 8, 128, 32, True), (2, 128, 16, 128, 32, True),
]


@pytest.mark.parametrize("bits,bm,kfactor,gs,ags,zp", FA_CFGS)
def test_fast_aggregation_bit_exact_vs_reference_intrinsics(ref, bits, bm, kfactor, gs, ags, zp):
    """(a9) the halving-adder tree, the ActK rescale and the analytic bias (tbl.cc:201-256,301-318,474-477):
    fa_mode 2 of the restatement == the reference's own FastAggregation build on an x86 host, to the bit."""
    A, S, q, ls, lb, case = float_case(bits, bm, kfactor, gs, ags, zp, fa=True)
    Mw, K = case["w"].shape
    Cor, tap = orc.qgemm_float_fa(A, q, S, ls, lb, Mw, K, 1, bits, bm, kfactor, gs, ags, zp, fa_mode=2)
    Cref = orc.combine_planes(ref[key("fa", bits, bm, kfactor, gs, ags, zp, "cbits")], Mw, bits)
    assert np.array_equal(Cor[0].view(np.uint32), Cref.view(np.uint32))
    assert tap.min() >= -128 and tap.max() <= 127


PREBUILT_CASES = [
    ("aarch64-llama-2-7b-2bit", 2, 128, 4096, 4096, 8192),     # BASELINE config #1 (tests/test_e2e.py)
    ("aarch64-llama-2-7b-2bit", 2, 128, 512, 11008, 8192),     # headline shape, 8 tiles
    ("aarch64-llama-2-7b-4bit", 4, 256, 512, 4096, 44032),     # bm=256 kernel only (SURVEY §8c caveat)
    ("aarch64-llama-3-8b-2bit", 2, 128, 256, 14336, 8192),
]


@pytest.mark.parametrize("setname,bits,bm,Mw,K,mname", PREBUILT_CASES)
def test_prebuilt_reference_kernels_bit_exact(ref, setname, bits, bm, Mw, K, mname):
    A, S, case = prebuilt_case(bits, bm, Mw, K)
    q, ls, lb, Cref = (ref[key("pb", setname, Mw, K, n)] for n in ("q", "ls", "lb", "C"))
    qo, lso, lbo = orc.preprocessor(case["B"], 64)
    assert np.array_equal(qo[0], q) and np.array_equal(lso[0], ls) and np.array_equal(lbo[0], lb)
    Cor = orc.qgemm_float(A, qo, S, lso, lbo, Mw, K, 1, bits, bm, 16, 128, 64, True)
    assert np.array_equal(Cor[0].view(np.uint32), Cref.view(np.uint32))
    Cdq = orc.dequant_matmul(case["w"], case["sc"], case["zr"], case["B"], bits, 128)[0]
    assert np.mean((Cdq - Cref) ** 2) / np.mean(Cdq ** 2) < 5e-4


INT32_CASES = [(2, 128, 256, 3200), (2, 320, 320, 3200), (2, 128, 128, 8640), (4, 256, 128, 1024),
               # the widths k_gemm_planes_us and the chain cover since rounds 3 / 4
               (1, 64, 128, 1024), (1, 64, 320, 8640), (3, 192, 192, 3200), (3, 192, 64, 12288), (4, 256, 192, 12288)]


@pytest.mark.parametrize("bits,bm,Mw,K", INT32_CASES)
def test_int32_scale_final_path(ref, bits, bm, Mw, K):
    A, q, ls, lb, case = int32_case(bits, bm, Mw, K)
    Cor, cb = orc.qgemm_scale_final(A, q, case["sc"], ls[:, 0], lb[:, 0], Mw, K, 1, bits, bm, 16, 1)
    assert np.array_equal(cb[0], ref[key("i32", bits, bm, Mw, K, "cb")])
    Cdq = orc.dequant_matmul(case["w"], case["sc"], None, case["B"], bits, 128, m_groups=1)[0]
    assert np.mean((Cdq - Cor[0]) ** 2) / np.mean(Cdq ** 2) < 5e-4


# ---- saturating inputs (oracle.make_hard_case): the reference's answers are recorded in golden/ref/saturating.npz ---------------------
SAT_GOLDEN = os.path.join(os.path.dirname(GOLDEN), "saturating.npz")
SAT_PRE_CASES = [(1024, 64), (1024, 32), (3200, 3200)]
SAT_WEIGHTS = ["max", "min", "rows", "planes"]
SAT_INT32_CASES = [(2, 320, 320, 3200), (4, 256, 192, 12288), (3, 192, 64, 12288), (1, 64, 320, 8640)]


@pytest.fixture(scope="module")
def sat():
    with np.load(SAT_GOLDEN) as z:
        return {k: z[k] for k in z.files}


def sat_float_case(bits, bm, kfactor, gs, ags, zp, weights):
    Mw, K = bm // bits * 2, 1024
    case = orc.make_hard_case(weights, "const", Mw, K, bits=bits, gs=gs, ags=ags, zero_point=zp, seed=11 * bits + ags)
    A = orc.preprocess_weights(case["w"], bits, bm, kfactor)
    S = orc.preprocess_scales(case["sc"], case["zr"], bits, bm)
    q, ls, lb = orc.preprocessor(case["B"], ags)
    return A, S, q, ls, lb, case


def sat_int32_case(bits, bm, Mw, K, weights):
    case = orc.make_hard_case(weights, "const", Mw, K, bits=bits, m_groups=1, ags=K, zero_point=False, seed=5)
    A = orc.preprocess_weights(case["w"], bits, bm, 16)
    q, ls, lb = orc.preprocessor(case["B"], K)
    return A, q, ls, lb, case


@pytest.mark.parametrize("acts", orc.HARD_ACTS)
@pytest.mark.parametrize("K,ags", SAT_PRE_CASES)
def test_preprocessor_saturating_inputs(sat, K, ags, acts):
    """tables of +-127 only (spike) and the 63.5 round-to-even tie in every table (const, negblocks)"""
    q, ls, lb = orc.preprocessor(orc.hard_acts(acts, K)[None, :], ags)
    assert np.abs(q).min() == 127 if acts == "spike" else sorted(np.unique(np.abs(q.astype(np.int32)))) == [0, 64, 127]
    qr, lsr, lbr = (sat[key("pre", acts, K, ags, n)] for n in ("q", "ls", "lb"))
    assert np.array_equal(q[0], qr)
    assert np.array_equal(ls[0].view(np.uint32), lsr.view(np.uint32))
    assert np.array_equal(lb[0].view(np.uint32), lbr.view(np.uint32))


@pytest.mark.parametrize("weights", SAT_WEIGHTS)
@pytest.mark.parametrize("bits,bm,kfactor,gs,ags,zp", CFGS)
def test_float_path_saturating_inputs(sat, bits, bm, kfactor, gs, ags, zp, weights):
    A, S, q, ls, lb, case = sat_float_case(bits, bm, kfactor, gs, ags, zp, weights)
    Mw, K = case["w"].shape
    PS = orc.partial_sums(A, q[0], Mw, K, bits, bm, kfactor, ags)
    orc.assert_saturates(weights, "const", q[0], PS, ags, K)
    Cor = orc.qgemm_float(A, q, S, ls, lb, Mw, K, 1, bits, bm, kfactor, gs, ags, zp)
    Cref = orc.combine_planes(sat[key("fp", weights, bits, bm, kfactor, gs, ags, zp, "cbits")], Mw, bits)
    assert np.array_equal(Cor[0].view(np.uint32), Cref.view(np.uint32))
    if has_int_partial_sums(bits, kfactor, ags):
        assert np.array_equal(PS, sat[key("fp", weights, bits, bm, kfactor, gs, ags, zp, "ps")])


@pytest.mark.parametrize("weights", SAT_WEIGHTS)
@pytest.mark.parametrize("bits,bm,kfactor,gs,ags,zp", FA_CFGS)
def test_fast_aggregation_saturating_inputs(sat, bits, bm, kfactor, gs, ags, zp, weights):
    """(a9) the halving-adder tree with +-127 at every leaf"""
    A, S, q, ls, lb, case = sat_float_case(bits, bm, kfactor, gs, ags, zp, weights)
    Mw, K = case["w"].shape
    orc.assert_saturates(weights, "const", q[0], orc.partial_sums(A, q[0], Mw, K, bits, bm, kfactor, ags), ags, K)
    Cor, tap = orc.qgemm_float_fa(A, q, S, ls, lb, Mw, K, 1, bits, bm, kfactor, gs, ags, zp, fa_mode=2)
    Cref = orc.combine_planes(sat[key("fa", weights, bits, bm, kfactor, gs, ags, zp, "cbits")], Mw, bits)
    assert np.array_equal(Cor[0].view(np.uint32), Cref.view(np.uint32))
    assert tap.max() == (127 if weights != "min" else -127) and tap.min() == (-127 if weights != "max" else 127)


@pytest.mark.parametrize("weights", ["max", "rows"])
@pytest.mark.parametrize("bits,bm,Mw,K", SAT_INT32_CASES)
def test_int32_scale_final_saturating_inputs(sat, bits, bm, Mw, K, weights):
    """one running total across the whole K: +-127 K / 4"""
    A, q, ls, lb, case = sat_int32_case(bits, bm, Mw, K, weights)
    _, cb = orc.qgemm_scale_final(A, q, case["sc"], ls[:, 0], lb[:, 0], Mw, K, 1, bits, bm, 16, 1)
    orc.assert_saturates(weights, "const", q[0], cb[0], K, K)
    assert np.array_equal(cb[0], sat[key("i32", weights, bits, bm, Mw, K, "cb")])
