"""convert.rtn_quant -- per-group round to nearest, the numpy yardstick of tmac_hip_pack_rtn_dev and Weights.from_dense -- without a GPU.

The reference tree holds no quantiser; the rule is GPTQ's published one (Quantizer.find_params with mse = False, then quantize).  Held here
1. to a float64 restatement (rtn_common.restated) on seeded matrices: float32 and float64 arithmetic can disagree only where the real
   quotient lies next to a half-integer -- |fl32(w / s) - w / s| <= (|w / s| + 1) 2^-22 covers the roundings of hi - lo, of the division
   by maxq and of w / s for |w / s| <= 2 maxq <= 30 -- so codes are compared wherever the float64 quotient is further than 1e-4 from a tie
   (at least 98 % of all values), zq likewise, and the scales at 2 fp32 ulp (two roundings);
2. to a hand-built table of ties (rtn_common.tie_groups): power-of-two scales, every quotient exactly an integer or an integer and a half,
   expected values from Python's round;
3. to the edge groups: all zero, all positive, all negative, a scale that underflows, fp16 subnormals, the invalid ones;
4. to the property of the rule, bits 1 - 4, with and without zero points: |w - (code - zq) scale| <= scale / 2 up to fp32 rounding.
"""
import numpy as np
import pytest

import rtn_common as rc
from tmac_amd import convert

BITS = (1, 2, 3, 4)


@pytest.mark.parametrize("src", rc.SRCS)
@pytest.mark.parametrize("zero_point", (True, False))
@pytest.mark.parametrize("bits", BITS)
def test_rule_meets_its_float64_restatement(bits, zero_point, src):
    Mw, K, gs = 96, 512, 64
    st = rc.masters(100 + bits, Mw, K, src)
    codes, sc, zr = convert.rtn_quant(st, bits, gs, zero_point)
    s32, zq, bad = convert.rtn_params(st, bits, gs, zero_point)
    assert codes.dtype == np.uint8 and sc.dtype == np.float32 and sc.shape == (Mw, K // gs) and not bad.any()
    assert np.array_equal(sc, s32) and (zr is None) == (not zero_point)
    q64, s64, z64 = rc.restated(st, bits, gs, zero_point)
    assert np.all(np.abs(sc.astype(np.float64) - s64) <= 2 * np.spacing(sc)), "scale: two roundings (hi - lo, / maxq) of at most one ulp together"
    zclear = np.abs(z64 - np.floor(z64) - 0.5) > 1e-4
    assert zclear.mean() > 0.99
    assert np.array_equal(zq[zclear], np.rint(z64)[zclear])
    want = np.clip(np.rint(q64) + np.rint(z64)[:, :, None], 0, 2 ** bits - 1)
    clear = (np.abs(q64 - np.floor(q64) - 0.5) > 1e-4) & zclear[:, :, None]
    print("clear of ties", bits, zero_point, src, clear.mean())
    assert clear.mean() > 0.98      # without zero points a group's extreme sits at exactly maxq / 2, a tie: one value in gs = 64
    assert np.array_equal(codes.reshape(q64.shape)[clear], want[clear].astype(np.uint8))
    if zero_point:
        assert np.array_equal(zr, ((zq - np.float32(2 ** (bits - 1))) * sc).astype(np.float32))
    if zero_point or bits > 1:      # symmetric 1-bit: w / scale lies in [-1/2, 1/2], every code is the zero code 1
        assert set(np.unique(codes)) == set(range(2 ** bits)), "every code occurs"


@pytest.mark.parametrize("zero_point", (True, False))
@pytest.mark.parametrize("bits", BITS)
def test_tie_table(bits, zero_point):
    w, sc, zq, cd = rc.tie_matrix(bits, zero_point, 16, 256)
    for src in rc.SRCS:
        st = rc.storage(w, src)
        assert np.array_equal(rc.as_f32(st), w), "every table value is exact in the dtype"
        for f16 in (False, True):                                  # power-of-two scales are fp16 values
            codes, s, zr = convert.rtn_quant(st, bits, 64, zero_point, f16)
            _, z, bad = convert.rtn_params(st, bits, 64, zero_point, f16)
            assert not bad.any()
            assert np.array_equal(s, sc) and np.array_equal(z, zq) and np.array_equal(codes, cd), (src, f16)


def test_table_holds_both_kinds_of_tie():
    """the table is not vacuous: quotients at k + 0.5 with k even and with k odd, positive and negative, and zero codes at a half"""
    for bits in (2, 3, 4):
        groups = rc.tie_groups(bits, True)
        q = np.concatenate([g / s for g, s, _, _ in groups])
        frac = q - np.floor(q)
        ks = np.floor(q[frac == 0.5]).astype(int)
        assert (ks % 2 == 0).any() and (ks % 2 == 1).any() and (ks < 0).any() and (ks >= 0).any()
        lo = np.array([-g.min() / s for g, s, _, _ in groups])
        assert ((lo - np.floor(lo)) == 0.5).sum() >= 2 ** bits - 1


@pytest.mark.parametrize("zero_point", (True, False))
@pytest.mark.parametrize("bits", BITS)
def test_edge_groups(bits, zero_point):
    f32 = np.float32
    maxq, mid, gs = f32(2 ** bits - 1), f32(2 ** (bits - 1)), 64
    s0 = f32(2.0) / maxq
    z0 = np.rint(f32(1.0) / s0) if zero_point else mid

    def one(group, f16=False):
        g = np.asarray(group)
        st = g.reshape(1, gs) if g.dtype in (np.float16, np.uint16) else g.astype(f32).reshape(1, gs)
        codes, s, zr = convert.rtn_quant(st, bits, gs, zero_point, f16)
        _, zq, bad = convert.rtn_params(st, bits, gs, zero_point, f16)
        return codes[0], s[0, 0], zq[0, 0], bool(bad[0, 0])

    # all zero (and -0.0): GPTQ's lo = -1, hi = +1; every code is the zero code, so w_real = 0
    for z in (0.0, -0.0):
        codes, s, zq, bad = one(np.full(gs, z))
        assert s == s0 and zq == z0 and not bad and np.all(codes == min(zq, maxq))
    rng = np.random.default_rng(3)
    pos = np.abs(rng.standard_normal(gs)).astype(f32) + f32(0.1)
    # all positive: lo = 0 -- zero code 0 with zero points; symmetric otherwise
    codes, s, zq, bad = one(pos)
    assert not bad and s == (f32(pos.max()) / maxq if zero_point else (pos.max() + pos.max()) / maxq)
    assert zq == (0 if zero_point else mid) and codes.max() == maxq
    # all negative: hi = 0 -- zero code maxq with zero points
    codes, s, zq, bad = one(-pos)
    # (1 bit without zero points: the minimum sits at -1/2, which rounds to even, 0 -- every code is the zero code 1)
    assert not bad and zq == (maxq if zero_point else mid) and codes.min() == (1 if bits == 1 and not zero_point else 0)
    # a range whose fp32 scale is subnormal: the all-zero group's parameters
    codes, s, zq, bad = one(rng.standard_normal(gs) * 1e-39)
    assert s == s0 and zq == z0 and not bad and np.all(codes == min(zq, maxq))
    # fp16 subnormals: multiples of 2^-24 are values like any other in fp32 ...
    sub = (rng.integers(0, 1024, gs) * 2.0 ** -24).astype(np.float16)
    sub[0], sub[1] = 0.0, np.float16(1023 * 2.0 ** -24)
    codes, s, zq, bad = one(sub)
    assert not bad and 0 < s < 2.0 ** -13 and codes.max() == maxq
    # ... and with the scale rounded to fp16 it is a subnormal fp16 itself, still the scale that divides
    codes, s, zq, bad = one(sub, f16=True)
    assert not bad and s == f32(np.float16(s)) and 0 < s < 2.0 ** -13
    # ... unless it rounds to 0: invalid
    tiny = np.zeros(gs, np.float16)
    tiny[5] = np.float16(2.0 ** -24)
    assert one(tiny, f16=False)[3] is False
    codes, s, zq, bad = one(tiny, f16=True)
    assert bad == (2.0 ** -24 / float(maxq) * (1 if zero_point else 2) <= 2.0 ** -25) and (not bad or (s == f32(np.float16(s0)) and np.all(codes <= maxq)))
    # an fp16 scale beyond 65504: invalid only where the scale is rounded to fp16
    wide = np.zeros(gs, f32)
    wide[2], wide[3] = -3.0e5, 9.0e5
    assert one(wide)[3] is False and one(wide, f16=True)[3] is True
    # non-finite masters: invalid, with the all-zero group's parameters; NaN codes 0, the infinities clamp
    for v, code in ((np.nan, 0), (np.inf, maxq), (-np.inf, 0)):
        g = pos.copy()
        g[11] = v
        codes, s, zq, bad = one(g)
        assert bad and s == s0 and zq == z0 and codes[11] == code
        assert convert.rtn_invalid(g.reshape(1, gs), bits, gs, zero_point) == 1


@pytest.mark.parametrize("src", rc.SRCS)
@pytest.mark.parametrize("zero_point", (True, False))
@pytest.mark.parametrize("bits", BITS)
def test_error_is_at_most_half_a_step(bits, zero_point, src):
    """|w - (code - zq) scale| <= scale / 2 for every w of the group: exact arithmetic gives 1/2; fl32(w / scale) is off by at most
    |w / scale| 2^-24 <= 2^-19 (|w / scale| <= 2 maxq <= 30), and hi - lo and its division by maxq move scale by 2^-23 relative, i.e. the
    quotient of hi by another maxq 2^-23 < 2^-19: bound (1/2 + 2^-18) scale.  With the scale rounded to fp16 -- 2^-11 relative for a
    normal fp16 -- the largest quotient moves by up to maxq 2^-11, which the clamp at maxq turns into error: bound (1/2 + 2^-18 + maxq 2^-11)."""
    Mw, K, gs = 64, 512, 128
    st = rc.masters(7 + bits, Mw, K, src)
    w = rc.as_f32(st).astype(np.float64).reshape(Mw, K // gs, gs)
    for f16 in (False, True):
        codes, sc, _ = convert.rtn_quant(st, bits, gs, zero_point, f16)
        _, zq, bad = convert.rtn_params(st, bits, gs, zero_point, f16)
        assert not bad.any()
        s = sc.astype(np.float64)[:, :, None]
        err = np.abs(w - (codes.reshape(w.shape).astype(np.float64) - zq.astype(np.float64)[:, :, None]) * s) / s
        bound = 0.5 + 2.0 ** -18 + ((2 ** bits - 1) * 2.0 ** -11 if f16 else 0.0)
        print("max error / scale", bits, zero_point, src, f16, err.max())
        assert err.max() <= bound
        assert err.max() > 0.45, "the bound is met, not missed by a mile"


def test_argument_rules():
    w = np.zeros((8, 64), np.float32)
    for bad in (dict(bits=0), dict(bits=5), dict(group_size=0), dict(group_size=6), dict(group_size=48)):
        with pytest.raises(ValueError):
            convert.rtn_quant(w, **{"bits": 2, "group_size": 64, **bad})
    with pytest.raises(TypeError):
        convert.rtn_quant(w.astype(np.float64), 2, 64)
    # bf16 words are widened exactly, never through fp16: a value below fp16's range keeps its scale
    st = rc.storage(np.full((8, 64), 3e-9, np.float32), "bf16")
    assert convert.rtn_quant(st, 2, 64)[1][0, 0] == rc.as_f32(st)[0, 0] / np.float32(3)
