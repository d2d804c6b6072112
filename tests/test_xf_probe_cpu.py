"""tests/xf_probe.py on the CPU: what tests/test_gpu_xf_exact.py rests on is itself under test, on the oracle alone.

  * lut_margin's restatement of the preprocessor rounds to the oracle's QLUT on every input the GPU file uses (the case lists are the
    helper's, so the two files cannot diverge), and every case is found by pick_safe within its seed budget;
  * the premise of the seed search: perturbing a chosen x by 4 eps, relative and element by element, leaves the oracle's QLUT and integer
    sums unchanged (and the outputs within the tight bar + 4 eps), for every case and every row;
  * every mutant of the reference is rejected by the GPU file's comparison in a regime meant for it, and the reference itself is accepted.

Which regime catches which mutant (MUTANT_CASES below; a mutant that no regime caught would be a gap to close with an input):
    no_eps, eps_outside        eps      mean(t^2) / eps of 1e-2 and 1: eps changes r by 10x and 1.41x; NORM and GLU_NORM
    drop_last8, double_last8   sparse   the one non-zero element sits among the last 8: the mean square goes to 0, or doubles
                               plain    K = 2112: 8 of 2112 elements move r by 0.2 %, a hundred times the bar
    gamma_shift                sparse   gamma is distinct per index, neighbours at least 18 % apart; the output is linear in x_i
                               plain    every element takes its neighbour's weight
    swap                       plain    gate(in2) * in for the three gates
                               tails    the gate's operand comes from the band, in2 from [0.5, 2]
    erf_gelu                   plain    the erf form is up to 4.7e-4 away from the tanh form
    f16_product                plain    the product rounded to fp16 (2^-11) moves table values a thousand times further than eps does
"""
import numpy as np
import pytest

import xf_probe as P
from oracle import oracle as orc


def mat_for(c, seed=5):
    K = c["K"]
    if c["ags"] == K and K > 64:
        return P.HostMat(seed, 16, K, m_groups=1)
    return P.HostMat(seed, 16, K, gs=128 if K % 128 == 0 else 64)


# ---- 1. the restatement and the search --------------------------------------------------------------------------------------------------
SEARCHED = P.searched_cases()


@pytest.mark.parametrize("c,n", SEARCHED, ids=[f"{P.case_id(c)}-n{n}" for c, n in SEARCHED])
def test_pick_safe_finds_the_case_and_the_margin_is_the_oracles(c, n):
    """every row within the seed budget (pick_safe raises otherwise); lut_q == the oracle's QLUT; the margin is what pick_safe was asked for"""
    rows = [P.resolve(c, r) for r in range(n)]
    assert len({r["seed"] for r in rows}) == n
    for r in rows:
        q, _, _ = orc.preprocessor(r["x"][None, :], c["ags"])
        assert np.array_equal(q[0], P.lut_q(r["x"], c["ags"])), P.case_id(c)
        assert P.lut_margin(r["x"], c["ags"]) >= P.margin_of(c)
        assert np.isfinite(r["x"]).all() and np.abs(r["x"]).max() > 0


def test_sparse_cases_are_one_hot():
    """|q| = 127 in the tables of element i, zero everywhere else: the margin is 0.5 and the pipeline linear in x_i"""
    for kind in ("norm", "glu_norm:silu", "glu_norm:relu2", "glu_norm:gelu"):
        for K in P.SPARSE_KS + (P.ROWS_SPARSE_K,):
            for ft, act in ((None, "f16"), (512, "f32"), (768, "f16"), (1024, "f32"), (512, "f16"), (768, "f32")):
                for c in P.sparse_cases(kind, K, ft, act=act):
                    inp = P.resolve(c)
                    assert inp["a"].dtype == P._dt(act)
                    q, _, _ = orc.preprocessor(inp["x"][None, :], 64)
                    assert np.array_equal(q[0], P.lut_q(inp["x"], 64))
                    assert set(np.unique(np.abs(q[0].astype(np.int32)))) == {0, 127} and np.count_nonzero(q[0]) == 16
                    assert np.count_nonzero(inp["x"]) == 1 and inp["x"][c["i"]] != 0
    g = P.sparse_gamma(12288)
    assert len(np.unique(g)) == 12288 and (np.abs(np.diff(g.astype(np.float64))) / g[1:] > 0.1).all()


def test_pick_safe_raises_instead_of_skipping():
    with pytest.raises(LookupError):
        P.pick_safe(lambda s: P.make_plain("glu:silu", 4160, 64, "f16", s), 0.4, 5)


def test_regimes_are_what_they_say():
    """eps: mean(t^2) / eps is the ratio asked for; every group's magnitudes within a factor of 4 outside `plain`; tails: the grid is fixed,
    fp16-exact, covers [-30, 30] for silu and relu^2, and only in2 depends on the seed"""
    for c in P.N1_EPS + P.ROWS_EPS:
        inp = P.resolve(c)
        base, _, gate = c["kind"].partition(":")
        t = (inp["a"].astype(np.float32) + inp["res"]).astype(np.float64) if base == "norm" else P.gate64(gate, inp["a"], inp["b"])
        assert abs(float((t ** 2).mean()) / c["eps"] / c["ratio"] - 1.0) < 0.01, P.case_id(c)
        g = np.abs(t).reshape(-1, 64)
        assert (g.max(axis=1) / g.min(axis=1) <= 4.0).all(), P.case_id(c)
    for gate in P.GATES:
        grid = np.concatenate([P.tail_band(c, gate) for c in P.tail_bands(gate)])
        assert grid.max() == 30.0 and grid.min() == (-9.5 if gate == "gelu" else -30.0) and np.abs(grid).min() < 2.0 ** -12
        for part in range(P.N_TAILS):
            a0, a1 = (P.make_tails(f"glu:{gate}", part, s) for s in (0, 1))
            assert np.array_equal(a0["a"], a1["a"]) and not np.array_equal(a0["b"], a1["b"])
            assert (np.abs(a0["b"].astype(np.float64)) >= 0.5).all() and (np.abs(a0["b"].astype(np.float64)) <= 2.0).all()
            if gate != "relu2":
                g = np.abs(a0["x"].astype(np.float64)).reshape(-1, 64)
                assert (g.max(axis=1) / g.min(axis=1) <= 4.0).all(), (gate, part)


# ---- 2. the premise: 4 eps of perturbation changes no table entry -----------------------------------------------------------------------
@pytest.mark.parametrize("c,n", SEARCHED, ids=[f"{P.case_id(c)}-n{n}" for c, n in SEARCHED])
def test_perturbation_by_four_eps_leaves_the_integers_alone(c, n):
    """every chosen x, every row: 24 independent relative perturbations of up to 4 eps per element give the same QLUT; on row 0 also the same
    integer sums and outputs within the tight bar + 4 eps"""
    X = np.stack([P.resolve(c, r)["x"] for r in range(n)])
    q0, _, _ = orc.preprocessor(X, c["ags"])
    rng = np.random.default_rng(1)
    e4 = 4 * P.eps_hw(c)
    for _ in range(24):
        Xp = (X.astype(np.float64) * (1.0 + e4 * rng.uniform(-1, 1, X.shape))).astype(np.float32)
        q, _, _ = orc.preprocessor(Xp, c["ags"])
        assert np.array_equal(q, q0), P.case_id(c)
    m = mat_for(c)
    x, xp = X[0], Xp[0]
    o0 = m.oracle(x)
    assert np.array_equal(m.sums(xp), m.sums(x))
    # with the integers equal the outputs are linear in ls and lb, which move by the perturbation itself: 4 eps here, on top of the plain bar
    ok, e = P.compare(m.oracle(xp), o0, P.TIGHT + e4)
    assert ok, e
    # ... and so does the common factor r at its bound: it rescales ls and moves no table value
    Xs = (X.astype(np.float64) * (1.0 + P.norm_bound(c["K"]))).astype(np.float32)
    assert np.array_equal(orc.preprocessor(Xs, c["ags"])[0], q0)
    assert P.compare(m.oracle(Xs[0]), o0, P.tight_bar("norm", c["K"]))[0]


# ---- 3. the mutant matrix ---------------------------------------------------------------------------------------------------------------
def _first(cases, **want):
    return next(c for c in cases if all(c.get(k) == v for k, v in want.items()))


def _sparse(kind, K, i):
    return P.case("sparse", kind, K, 64, i=i)


MUTANT_CASES = {
    "no_eps": [_first(P.N1_EPS, kind="norm", eps=1e-6, ratio=1.0), _first(P.N1_EPS, kind="glu_norm:silu", eps=1e-5, ratio=1e-2),
               _first(P.N1_EPS, kind="glu_norm:relu2", eps=1e-2, ratio=1e2), _first(P.ROWS_EPS, kind="norm", eps=1e-5, ratio=1.0),
               _first(P.CHAIN_CASES, regime="eps", eps=1e-6)],
    "eps_outside": [_first(P.N1_EPS, kind="norm", eps=1e-6, ratio=1.0), _first(P.N1_EPS, kind="glu_norm:gelu", eps=1e-5, ratio=1.0),
                    _first(P.N1_EPS, kind="norm", eps=1e-2, ratio=1e2), _first(P.ROWS_EPS, kind="glu_norm:silu", eps=1e-6, ratio=1e-2),
                    _first(P.CHAIN_CASES, regime="eps", eps=1e-2)],
    "drop_last8": [_sparse("norm", 4160, 4159), _sparse("glu_norm:silu", 12288, 12280), _sparse("norm", P.ROWS_SPARSE_K, P.ROWS_SPARSE_K - 1),
                   _first(P.N1_PLAIN, kind="norm", K=2112), _first(P.CHAIN_CASES, kind="norm", regime="plain")],
    "double_last8": [_sparse("norm", 4160, 4152), _sparse("glu_norm:relu2", 12288, 12287), _sparse("norm", P.ROWS_SPARSE_K, P.ROWS_SPARSE_K - 8),
                     _first(P.N1_PLAIN, kind="glu_norm:silu", K=2112), _first(P.CHAIN_CASES, kind="norm", regime="plain")],
    "gamma_shift": [_sparse("norm", 4160, 0), _sparse("norm", 4160, 4096), _sparse("glu_norm:silu", 12288, 6143), _sparse("norm", 12288, 8191),
                    _first(P.N1_PLAIN, kind="norm", K=64), _first(P.ROWS_PLAIN[128], kind="norm"), _first(P.CHAIN_CASES, kind="norm", regime="plain")],
    "swap": [_first(P.N1_PLAIN, kind="glu:silu", K=2112), _first(P.N1_PLAIN, kind="glu:relu2", K=64), _first(P.N1_PLAIN, kind="glu_norm:gelu", K=1024),
             _first(P.N1_TAILS, kind="glu:silu", part=9), _first(P.N1_TAILS, kind="glu:gelu", part=4), _first(P.CHAIN_CASES, kind="glu:silu")],
    "erf_gelu": [_first(P.N1_PLAIN, kind="glu:gelu", K=1024), _first(P.N1_PLAIN, kind="glu_norm:gelu", K=64), _first(P.ROWS_PLAIN[128], kind="glu:gelu"),
                 _first(P.CHAIN_CASES, kind="glu:gelu", regime="plain")],
    "f16_product": [_first(P.N1_PLAIN, kind="glu:silu", K=4160), _first(P.N1_PLAIN, kind="glu_norm:relu2", K=2112), _first(P.ROWS_PLAIN[2112], kind="glu:silu"),
                    _first(P.CHAIN_CASES, kind="glu:gelu", regime="plain")],
}
MATRIX = [(mu, c) for mu in P.MUTANTS for c in MUTANT_CASES[mu]]


def test_every_mutant_has_a_regime():
    assert set(MUTANT_CASES) == set(P.MUTANTS) and all(MUTANT_CASES[m] for m in P.MUTANTS)


@pytest.mark.parametrize("mutant,c", MATRIX, ids=[f"{mu}-{P.case_id(c)}" for mu, c in MATRIX])
def test_the_comparison_rejects_the_mutant(mutant, c):
    """compare(oracle(mutant x), oracle(ref x)) fails at the bar the GPU file uses for the case; compare(oracle(ref x), oracle(ref x)) passes"""
    inp = P.resolve(c)
    m = mat_for(c)
    bar = P.tight_bar(c["kind"], c["K"])
    want = m.oracle(inp["x"])
    assert np.abs(want).max() > 0
    assert P.compare(want, want, bar)[0]
    xm = P.case_ref(inp, mutant=mutant)
    assert not np.array_equal(xm, inp["x"]), "the mutant does not touch this case"
    ok, e = P.compare(m.oracle(xm), want, bar)
    print(f"{mutant} on {P.case_id(c)}: rel err {e:.3e} against a bar of {bar:.3e}")
    assert not ok, (mutant, P.case_id(c), e, bar)
    if c["kind"].startswith("glu:") and mutant in ("swap", "erf_gelu"):      # ... and by the tap's element-wise check at N >= 2
        d = np.abs(xm.astype(np.float64) - inp["x"].astype(np.float64))
        assert (d > P.eps_hw(c) * np.abs(inp["x"].astype(np.float64))).any()
