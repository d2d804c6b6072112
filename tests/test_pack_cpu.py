"""The packers' index and nibble arithmetic without a GPU: tmac_amd/csrc/tmac_pack.h, the header the pack kernels (tmac_pack.hip) share,
compiled with plain g++ into tests/cpp/pack_main.cc, which packs whole matrices through it.  Required: the bytes of the host route --
weights.preprocess_weights, from convert.unpack_gptq for the GPTQ form -- for every width, M-tiles of several 32-row groups, both
kfactors and K with one, several and an odd number of kfactor blocks; the scales' raw bits, including fp16 zero products that round
and one that overflows.
"""
import os
import subprocess

import numpy as np
import pytest

import pack_common as pc

HERE = os.path.dirname(os.path.abspath(__file__))
# (bits, bm, Mw): at least 3 M-tiles of at least 2 groups of 32 M-space rows each
TILES = {1: (64, 192), 2: (64, 96), 3: (192, 192), 4: (64, 48)}
KS = (128, 192, 320)
GS = 64


@pytest.fixture(scope="module")
def packer(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pack") / "pack_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "cpp", "pack_main.cc")], check=True)
    return exe


def run(packer, d, form, Mw, K, bits, bm, kf, zp, v2, sdt, odt, wsrc, sc, zsrc):
    paths = [str(d / n) for n in ("w.bin", "s.bin", "z.bin", "A.bin", "S.bin")]
    wsrc.tofile(paths[0]); sc.tofile(paths[1])
    (zsrc if zsrc is not None else np.zeros(0, np.uint8)).tofile(paths[2])
    subprocess.run([packer, form] + [str(int(v)) for v in (Mw, K, bits, bm, kf, GS, zp, v2, sdt == np.float16, odt == np.float16)] + paths, check=True)
    return np.fromfile(paths[3], np.uint8), np.fromfile(paths[4], odt)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("kf", (8, 16))
@pytest.mark.parametrize("bits", (1, 2, 3, 4))
def test_codes_form_is_preprocess_weights(packer, tmp_path, bits, kf, K):
    bm, Mw = TILES[bits]
    assert Mw * bits // bm >= 3 and bm // 32 >= 2 and (K // 4) % kf == 0
    for zp in (True, False):
        codes, sc, zr = pc.make_codes(100 * bits + kf + K, Mw, K, bits, GS, np.float32)
        assert (codes >> bits).any(), "the codes carry bits above the width"
        A, S = pc.host_blob_codes(codes, sc, zr if zp else None, bits, bm, kf)
        gA, gS = run(packer, tmp_path, "codes", Mw, K, bits, bm, kf, zp, 0, np.float32, np.float32, codes, sc, zr if zp else None)
        assert np.array_equal(gA, A.reshape(-1))
        assert np.array_equal(pc.raw_bits(gS), pc.raw_bits(S))


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("kf", (8, 16))
@pytest.mark.parametrize("v2", (True, False))
@pytest.mark.parametrize("bits", (1, 2, 4))
def test_gptq_form_is_unpack_then_preprocess(packer, tmp_path, bits, v2, kf, K):
    bm, Mw = TILES[bits]
    for sdt in (np.float16, np.float32):
        qw, sc, qz = pc.make_gptq(7 * bits + kf + K + int(v2), Mw, K, bits, GS, sdt)
        A, S, (w, s_u, z_u, b, g) = pc.host_blob_gptq(qw, sc, qz, v2, bm, kf)
        assert b == bits and g == GS and S.dtype == sdt
        if sdt == np.float16:
            exact = z_u.astype(np.float64) == (z_u.astype(np.float64) / s_u.astype(np.float64)).round() * s_u.astype(np.float64)
            # (multipliers of 1- and 2-bit zeros are 0, +-1, +-2: only a 4-bit product can need more than 11 mantissa bits)
            assert bits < 4 or not exact[np.isfinite(z_u)].all(), "some fp16 zero product must have been rounded"
            assert np.isinf(z_u).any() == (bits > 1), "2- and 4-bit cases hold a zero that overflows fp16"
        gA, gS = run(packer, tmp_path, "gptq", Mw, K, bits, bm, kf, True, v2, sdt, sdt, qw, sc, qz)
        assert np.array_equal(gA, A.reshape(-1))
        assert np.array_equal(pc.raw_bits(gS), pc.raw_bits(S))
        # the other output dtype: the zero is rounded to the scales' dtype first, then converted
        odt = np.float32 if sdt == np.float16 else np.float16
        with np.errstate(over="ignore"):
            want = S.astype(odt)
        _, gS2 = run(packer, tmp_path, "gptq", Mw, K, bits, bm, kf, True, v2, sdt, odt, qw, sc, qz)
        assert np.array_equal(pc.raw_bits(gS2), pc.raw_bits(want))


def test_gptq_form_without_zero_points(packer, tmp_path):
    bits, kf, K = 2, 16, 192
    bm, Mw = TILES[bits]
    qw, sc, qz = pc.make_gptq(5, Mw, K, bits, GS, np.float16)
    A, S, _ = pc.host_blob_gptq(qw, sc, qz, True, bm, kf, zero_point=False)
    gA, gS = run(packer, tmp_path, "gptq", Mw, K, bits, bm, kf, False, True, np.float16, np.float16, qw, sc, None)
    assert np.array_equal(gA, A.reshape(-1)) and np.array_equal(pc.raw_bits(gS), pc.raw_bits(S))
