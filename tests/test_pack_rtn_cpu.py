"""The round-to-nearest packers' shared arithmetic without a GPU: tmac_amd/csrc/tmac_pack.h -- the rule (rtn_scale_zq, rtn_code, rtn_zero, the
fp16 rounding of the scale), the index of a (row, group) parameter and the blob's index arithmetic, the header k_rtn_params and
k_pack_rtn_weights (tmac_pack.hip) share -- compiled with plain g++ under AddressSanitizer and UBSan into tests/cpp/pack_rtn_main.cc, which
quantises and packs whole small matrices from fp32, fp16 and bf16 bit patterns.  Required: the bytes of the host route,
weights.preprocess_weights of convert.rtn_quant's codes, scales and zeros, and convert.rtn_params' parameters bit for bit -- minimum and
maximum are exact and every later step is one correctly rounded fp32 operation on both sides, so nothing is left to a tolerance.
"""
import os
import subprocess

import numpy as np
import pytest

import pack_common as pc
import rtn_common as rc
from tmac_amd import convert

HERE = os.path.dirname(os.path.abspath(__file__))
# (Mw, K, gs, kfactor): several M-tiles of several 32-row groups; K / 4 of one, several and an odd number of kfactor blocks; groups of one
# 16-byte load per lane, of several, of 8-byte loads (gs = 36 is no multiple of 8) and of more loads than a wave has lanes (gs = 1280)
SHAPES = [(64, 128, 64, 16), (96, 192, 32, 8), (32, 576, 192, 16), (32, 144, 36, 1), (32, 2560, 1280, 16)]


@pytest.fixture(scope="module")
def packer(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pack_rtn") / "pack_rtn_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(HERE, "cpp", "pack_rtn_main.cc")], check=True)
    return exe


def run(packer, d, src, st, bits, gs, zero_point, f16, bm, kf):
    paths = [str(d / n) for n in ("w.bin", "A.bin", "S.bin", "P.bin")]
    st.tofile(paths[0])
    Mw, K = st.shape
    subprocess.run([packer] + [str(v) for v in (rc.SRC_CODE[src], Mw, K, bits, gs, int(zero_point), int(f16), bm, kf)] + paths, check=True)
    P = np.fromfile(paths[3], np.float32).reshape(3, Mw, K // gs)
    return np.fromfile(paths[1], np.uint8), np.fromfile(paths[2], np.float32), P


def check(packer, d, src, st, bits, gs, zero_point, f16, kf):
    bm = 32 * bits
    gA, gS, P = run(packer, d, src, st, bits, gs, zero_point, f16, bm, kf)
    A, S, codes, sc, zr = rc.host_blob(st, bits, gs, zero_point, f16, bm, kf)
    _, zq, bad = convert.rtn_params(st, bits, gs, zero_point, f16)
    assert np.array_equal(pc.raw_bits(P[0]), pc.raw_bits(sc)), "scales"
    assert np.array_equal(P[1], zq) and np.array_equal(P[2] != 0, bad), "zero codes, invalid groups"
    assert np.array_equal(gA, A.reshape(-1)), "weight bytes"
    assert np.array_equal(pc.raw_bits(gS), pc.raw_bits(S)), "scales half of the blob"
    return codes, int(bad.sum())


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("src", rc.SRCS)
def test_rtn_form_is_quantise_then_preprocess(packer, tmp_path, src, shape):
    Mw, K, gs, kf = shape
    st = rc.masters(Mw + K + gs, Mw, K, src)
    for bits in (1, 2, 3, 4):
        for zero_point in (True, False):
            for f16 in (False, True):
                codes, nbad = check(packer, tmp_path, src, st, bits, gs, zero_point, f16, kf)
                assert nbad == 0
                if zero_point:
                    assert set(np.unique(codes)) == set(range(2 ** bits))


@pytest.mark.parametrize("zero_point", (True, False))
@pytest.mark.parametrize("bits", (1, 2, 3, 4))
def test_tie_table_through_the_shared_rule(packer, tmp_path, bits, zero_point):
    """the C++ of the header against the table itself"""
    Mw, K, gs, kf = SHAPES[0]
    w, sc, zq, cd = rc.tie_matrix(bits, zero_point, Mw, K, gs)
    for src in rc.SRCS:
        st = rc.storage(w, src)
        gA, gS, P = run(packer, tmp_path, src, st, bits, gs, zero_point, False, 32 * bits, kf)
        zr = ((zq - np.float32(2 ** (bits - 1))) * sc).astype(np.float32) if zero_point else None
        A, S = pc.host_blob_codes(cd, sc, zr, bits, 32 * bits, kf)
        assert np.array_equal(P[0], sc) and np.array_equal(P[1], zq) and not P[2].any()
        assert np.array_equal(gA, A.reshape(-1)) and np.array_equal(pc.raw_bits(gS), pc.raw_bits(S))


@pytest.mark.parametrize("src", rc.SRCS)
def test_edge_and_invalid_groups(packer, tmp_path, src):
    Mw, K, gs, kf = SHAPES[0]
    st = rc.edge_matrix(src, Mw, K, gs)
    seen = 0
    for bits in (1, 2, 3, 4):
        for zero_point in (True, False):
            for f16 in (False, True):
                seen += check(packer, tmp_path, src, st, bits, gs, zero_point, f16, kf)[1]
    assert seen > 0, "the edge matrix holds invalid groups"
    # non-finite masters
    for bad in (np.inf, -np.inf, np.nan):
        v = rc.as_f32(rc.masters(9, Mw, K, src))
        v[7, 11] = v[7, 12] = v[40, 100] = bad
        assert check(packer, tmp_path, src, rc.storage(v, src), 2, gs, True, False, kf)[1] == 2
