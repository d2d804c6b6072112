"""The AutoAWQ GEMM format on the host (tmac_amd/convert.py: unpack_awq, pack_awq), against the statement of the format itself: field i
(bits 4i .. 4i+3) of qweight[k][c] is the code of weight row 8c + ORDER[i] at column k, ORDER = (0, 2, 4, 6, 1, 3, 5, 7); qzeros the same;
w = (q - z) * s with no + 1 on the zeros."""
import numpy as np

import awq_common as ac
from tmac_amd import convert

ORDER = (0, 2, 4, 6, 1, 3, 5, 7)
INV = (0, 4, 1, 5, 2, 6, 3, 7)


def test_order_and_inv_are_mutual_inverses():
    assert convert.AWQ_ORDER == ORDER and convert.AWQ_INV == INV
    assert sorted(ORDER) == list(range(8))
    for i in range(8):
        assert INV[ORDER[i]] == i and ORDER[INV[i]] == i


def test_known_answer_word():
    """0x76543210: field i holds i, so rows 8c .. 8c+7 get the codes 0, 4, 1, 5, 2, 6, 3, 7 -- for the weights and for the zeros"""
    K, gs = 4, 4
    qweight = np.full((K, 1), 0x76543210, np.uint32).view(np.int32)
    qzeros = np.full((1, 1), 0x76543210, np.uint32).view(np.int32)
    scales = np.ones((1, 8), np.float32)
    w, sc, zr, bits, g = convert.unpack_awq(qweight, scales, qzeros)
    assert bits == 4 and g == gs and w.shape == (8, K) and w.dtype == np.uint8
    want = np.array([0, 4, 1, 5, 2, 6, 3, 7])
    assert np.array_equal(w, np.repeat(want[:, None], K, axis=1))
    assert np.array_equal(zr[:, 0], (want - 8).astype(np.float32))


def test_unpack_is_the_inverse_of_pack():
    for name, (Mw, K, bm, kf, gs, ags) in ac.SHAPES.items():
        for dt in (np.float16, np.float32):
            (qw, sc, qz), (w, z) = ac.make_awq(len(name) + Mw, Mw, K, gs, dt, hard=False)
            assert qw.dtype == np.int32 and qw.shape == (K, Mw // 8) and qz.shape == (K // gs, Mw // 8) and sc.shape == (K // gs, Mw)
            gw, gsc, gzr, bits, g = convert.unpack_awq(qw, sc, qz)
            assert (bits, g) == (4, gs) and gsc.dtype == dt and gzr.dtype == dt
            assert np.array_equal(gw, w)
            assert np.array_equal(gsc, sc.T)
            assert np.array_equal(gzr, (z.astype(dt) - 8) * sc.T)
            # and back: the words themselves
            rq, rs, rz = convert.pack_awq(gw, gsc, z)
            assert np.array_equal(rq, qw) and np.array_equal(rs, sc) and np.array_equal(rz, qz)


def test_unpack_against_a_plain_loop_restatement():
    """(w - 8) * sc - zeros, T-MAC's dequantisation of what unpack_awq returns, is AWQ's (q - z) * s read off the words by the format's
    own rule, exactly in float64.  Scales are fp16-representable values held in float32, so (z - 8) * s is exact there."""
    Mw, K, gs = 24, 64, 32
    rng = np.random.default_rng(3)
    qweight = rng.integers(0, 2 ** 32, size=(K, Mw // 8), dtype=np.uint64).astype(np.uint32)
    qzeros = rng.integers(0, 2 ** 32, size=(K // gs, Mw // 8), dtype=np.uint64).astype(np.uint32)
    scales = (rng.integers(1024, 2048, size=(K // gs, Mw)) / 1024.0 * 2.0 ** -6).astype(np.float16).astype(np.float32)
    assert np.array_equal(scales, scales.astype(np.float16).astype(np.float32))
    want = np.zeros((Mw, K), np.float64)
    for k in range(K):
        for c in range(Mw // 8):
            for i in range(8):
                o = 8 * c + ORDER[i]
                q = (int(qweight[k, c]) >> (4 * i)) & 15
                z = (int(qzeros[k // gs, c]) >> (4 * i)) & 15
                want[o, k] = float(q - z) * float(scales[k // gs, o])
    w, sc, zr, bits, g = convert.unpack_awq(qweight.view(np.int32), scales, qzeros.view(np.int32))
    got = (w.astype(np.float64) - 8.0) * np.repeat(sc.astype(np.float64), gs, axis=1) - np.repeat(zr.astype(np.float64), gs, axis=1)
    assert np.array_equal(got, want)


def test_refused_shapes_and_dtypes():
    import pytest
    (qw, sc, qz), _ = ac.make_awq(1, 16, 64, 32, np.float16, hard=False)
    with pytest.raises(TypeError):
        convert.unpack_awq(qw.astype(np.int64), sc, qz)
    with pytest.raises(ValueError):
        convert.unpack_awq(qw[:, :1], sc, qz)
    with pytest.raises(ValueError):
        convert.unpack_awq(qw, sc, qz[:, :1])
    with pytest.raises(ValueError, match="qzeros"):
        convert.unpack_awq(qw, sc, None)
