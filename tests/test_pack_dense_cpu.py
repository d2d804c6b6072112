"""The BitNet packers' shared arithmetic without a GPU: tmac_amd/csrc/tmac_pack.h -- the absmean rule and the blob's index arithmetic, the
header k_absmean and k_pack_dense_weights (tmac_pack.hip) share -- compiled with plain g++ under AddressSanitizer and UBSan into
tests/cpp/pack_dense_main.cc, which quantises and packs whole small matrices from fp32, fp16 and bf16 bit patterns.  Required: the bytes
of the host route, weights.preprocess_weights of convert.bitnet_absmean_quant's levels, and its scales.

The program adds a block's |w| in the device's order, numpy pairwise: both are fp64 sums of at most 2^17 non-negative terms, off by far
less than half an fp32 ulp, so their fp32 roundings agree except when the exact mean lies within ~1e-12 relative of a rounding boundary.
The scale is therefore compared at 1 fp32 ulp, and the blob under the program's own scale handed to the reference as ``scale=`` (as
tests/test_gpu_bitnet_pack.py does with the device's), where A and S must be equal byte for byte.
"""
import os
import subprocess

import numpy as np
import pytest

import bitnet_common as bc
import pack_common as pc

HERE = os.path.dirname(os.path.abspath(__file__))
# (Mw, K, bm, kfactor): several M-tiles of several 32-row groups; K / 4 of one, several and an odd number of kfactor blocks; a block of
# 160 x 320 = 51200 elements spans four reduction chunks, the last of them short
SHAPES = [(64, 128, 64, 16), (96, 192, 64, 8), (160, 320, 64, 16)]


@pytest.fixture(scope="module")
def packer(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pack_dense") / "pack_dense_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(HERE, "cpp", "pack_dense_main.cc")], check=True)
    return exe


def run(packer, d, src, st, bm, kf, m_groups=1, eps=1e-5, scale=None):
    paths = [str(d / n) for n in ("w.bin", "si.bin", "A.bin", "S.bin")]
    st.tofile(paths[0])
    (np.asarray(scale, np.float32) if scale is not None else np.zeros(0, np.float32)).tofile(paths[1])
    Mw, K = st.shape
    subprocess.run([packer] + [str(v) for v in (bc.SRC_CODE[src], Mw, K, bm, kf, m_groups, repr(float(np.float32(eps))), int(scale is not None))] + paths,
                   check=True)
    return np.fromfile(paths[2], np.uint8), np.fromfile(paths[3], np.float32)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("src", bc.SRCS)
def test_dense_form_is_quantise_then_preprocess(packer, tmp_path, src, shape):
    Mw, K, bm, kf = shape
    for m_groups in (1, 2, 4):
        st = bc.masters(Mw + K + m_groups, Mw, K, src, m_groups)
        gA, gS = run(packer, tmp_path, src, st, bm, kf, m_groups)
        mean = np.abs(bc.as_f32(st).astype(np.float64)).reshape(m_groups, -1).mean(axis=1).astype(np.float32)
        assert np.all(np.abs(gS.astype(np.float64) - mean.astype(np.float64)) <= np.spacing(mean)), (gS, mean)
        A, S, lv = bc.host_blob(st, bm, kf, m_groups, scale=gS)
        assert set(np.unique(lv)) == {1, 2, 3}
        assert np.array_equal(gA, A.reshape(-1))
        assert np.array_equal(pc.raw_bits(gS), pc.raw_bits(S))


@pytest.mark.parametrize("src", bc.SRCS)
def test_tie_table_through_the_shared_rule(packer, tmp_path, src):
    """ties, signed zero, infinities and NaN at a given scale of 1.0: the C++ of the header against the table itself"""
    Mw, K, bm, kf = SHAPES[0]
    st, lv = bc.tie_matrix(src, Mw, K)
    one = np.ones(1, np.float32)
    gA, gS = run(packer, tmp_path, src, st, bm, kf, scale=one)
    A, S = pc.host_blob_codes(lv, one, None, 2, bm, kf)
    assert np.array_equal(gA, A.reshape(-1)) and np.array_equal(pc.raw_bits(gS), pc.raw_bits(S))
    A2, _, lv2 = bc.host_blob(st, bm, kf, scale=one)
    assert np.array_equal(lv2, lv) and np.array_equal(A2, A)


def test_eps_floor_and_non_finite_masters(packer, tmp_path):
    Mw, K, bm, kf = SHAPES[0]
    tiny = np.full((Mw, K), 2e-7, np.float32)
    gA, gS = run(packer, tmp_path, "f32", tiny, bm, kf)
    A, S, lv = bc.host_blob(tiny, bm, kf)
    assert np.all(lv == 2) and gS[0] == np.float32(1e-5) and np.array_equal(gA, A.reshape(-1))
    for bad in (np.inf, np.nan):
        st = bc.as_f32(bc.masters(9, Mw, K, "f32"))
        st[7, 11] = bad
        gA, gS = run(packer, tmp_path, "f32", st, bm, kf)
        A, S, _ = bc.host_blob(st, bm, kf)
        assert np.array_equal(pc.raw_bits(gS), pc.raw_bits(S)) and np.array_equal(gA, A.reshape(-1))
