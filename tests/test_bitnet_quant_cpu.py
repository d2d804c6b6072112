"""convert.bitnet_absmean_quant -- the host reference of the device-side BitNet packing -- without a GPU.

The reference tree holds no BitNet quantiser (its conversion lives in a llama.cpp fork that is not part of it), so the yardstick is the
published absmean rule restated in float64 (bitnet_common.restated_levels): on matrices whose |w| / mean|w| keeps 1e-3 away from the
rounding points 0.5 and 1.5, float32 and float64 arithmetic must give the same levels.  What happens AT the rounding points, at signed
zero and at non-finite masters is fixed by a hand-written table.
"""
import numpy as np
import pytest

import bitnet_common as bc
from tmac_amd import convert


@pytest.mark.parametrize("m_groups", (1, 2, 4))
@pytest.mark.parametrize("src", bc.SRCS)
def test_levels_are_the_float64_rule(src, m_groups):
    Mw, K = 64, 320
    st = bc.masters(7 + m_groups, Mw, K, src, m_groups, clear_of_ties=True)
    v = bc.as_f32(st).astype(np.float64).reshape(m_groups, -1)
    r = np.abs(v) / np.abs(v).mean(axis=1)[:, None]
    assert np.abs(r - 0.5).min() >= 1e-3 and np.abs(r - 1.5).min() >= 1e-3
    want, s64 = bc.restated_levels(st, m_groups)
    got, s = convert.bitnet_absmean_quant(st, m_groups)
    assert got.dtype == np.uint8 and got.shape == (Mw, K) and s.dtype == np.float32 and s.shape == (m_groups,)
    assert np.array_equal(got, want)
    assert set(np.unique(got)) == {1, 2, 3}, "a matrix like a trained layer's uses all three levels"
    assert np.all(np.abs(s.astype(np.float64) - s64) <= np.spacing(s) / 2 * 1.0000001)        # the float64 mean, rounded once


@pytest.mark.parametrize("src", bc.SRCS)
def test_tie_table(src):
    st, want = bc.tie_table(src)
    got, s = convert.bitnet_absmean_quant(st.reshape(1, -1), scale=1.0)
    assert np.array_equal(got[0], want), (bc.as_f32(st), got[0], want)
    assert np.array_equal(s, np.ones(1, np.float32))
    mat, lv = bc.tie_matrix(src, 8, 64)
    assert np.array_equal(convert.bitnet_absmean_quant(mat, scale=np.ones(1, np.float32))[0], lv)


def test_masters_below_eps():
    w = np.full((8, 64), 3e-7, np.float32)
    w[::2] *= -1
    lv, s = convert.bitnet_absmean_quant(w)
    assert np.array_equal(s, np.array([1e-5], np.float32)) and np.all(lv == 2)
    lv, s = convert.bitnet_absmean_quant(np.zeros((8, 64), np.float16), eps=1e-3)
    assert np.array_equal(s, np.array([1e-3], np.float32)) and np.all(lv == 2)


@pytest.mark.parametrize("m_groups", (1, 2, 4))
def test_per_block_means(m_groups):
    Mw, K = 16, 64
    st = bc.masters(3, Mw, K, "f32", m_groups)
    lv, s = convert.bitnet_absmean_quant(st, m_groups)
    R = Mw // m_groups
    for g in range(m_groups):
        blk = st[g * R:(g + 1) * R]
        assert s[g] == np.float32(np.abs(blk.astype(np.float64)).mean())
        # the block's levels depend on the block alone
        assert np.array_equal(lv[g * R:(g + 1) * R], convert.bitnet_absmean_quant(blk)[0])
    if m_groups > 1:
        assert s[m_groups - 1] > 1.5 * s[0], "the blocks were drawn at different magnitudes"


def test_non_finite_masters_and_argument_rules():
    w = bc.as_f32(bc.masters(5, 8, 64, "f32"))
    w[3, 5] = np.inf
    lv, s = convert.bitnet_absmean_quant(w)
    assert np.isinf(s[0]) and np.all(lv == 2)                     # an infinite mean: 1 / s is 0, and inf * 0 is a NaN, which is 0
    w[3, 5] = np.nan
    lv, s = convert.bitnet_absmean_quant(w)
    assert s[0] == np.float32(1e-5) and lv[3, 5] == 2             # fmaxf drops the NaN mean
    with pytest.raises(ValueError):
        convert.bitnet_absmean_quant(w, m_groups=3)
    with pytest.raises(ValueError):
        convert.bitnet_absmean_quant(w, eps=0.0)
    with pytest.raises(TypeError):
        convert.bitnet_absmean_quant(w.astype(np.float64))
