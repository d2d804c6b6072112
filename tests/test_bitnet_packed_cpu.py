"""The packed ternary BitNet format without a GPU.

1. The format against its authors' code: tests/golden/bitnet/bitnet_packed_ref.npz holds what ``transformers.integrations.bitnet.pack_weights``
   gives for a seeded 64 x 32 ternary matrix and for the worked example of ``unpack_weights``' docstring (written by
   tests/golden/make_bitnet_packed_ref.py; this test imports no transformers).  ``convert.unpack_bitnet_packed`` must return the recorded
   levels, ``convert.pack_bitnet_packed`` the recorded bytes.
2. Field value 3: counted, and level 3.
3. ``convert.bitnet_packed_scale``: both conventions on bf16 / fp16 / fp32 inputs against a float64 restatement rounded once to float32.
   The restatement of the reciprocal is float32(1 / float64(ws)): the float64 quotient of two float32 numbers rounded again to float32
   is the correctly rounded float32 quotient (double rounding is innocuous for division when the wide format has at least 2 p + 2 = 50
   bits of precision; float64 has 53), so the comparison is exact equality.
4. tmac_amd/csrc/tmac_pack.h through tests/cpp/pack_ternary_main.cc (plain g++ under AddressSanitizer and UBSan): whole matrices at the
   five shapes of the GPU test, in both formulations -- per weight row as the general kernel walks, four fields per byte as the read-once
   kernel walks -- byte for byte pack_common.host_blob_codes of the levels.
"""
import os
import subprocess

import numpy as np
import pytest

import bitnet_packed_common as bp
import pack_common as pc
from tmac_amd import convert

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(HERE, "golden", "bitnet", "bitnet_packed_ref.npz"))


@pytest.mark.parametrize("which", ["", "ex_"])
def test_format_is_the_authors(ref, which):
    ternary, packed = ref[which + "ternary"], ref[which + "packed"]
    assert packed.dtype == np.uint8 and packed.shape == (ternary.shape[0] // 4, ternary.shape[1])
    lv, invalid = convert.unpack_bitnet_packed(packed)
    assert invalid == 0 and lv.dtype == np.uint8
    assert np.array_equal(lv.astype(np.int8) - 2, ternary)
    assert np.array_equal(convert.pack_bitnet_packed((ternary + 2).astype(np.uint8)), packed)


def test_docstring_example_by_hand(ref):
    """the first byte of the example, 0b10100001, holds the first column of rows 0, 2, 4, 6: 0, -1, 1, 1"""
    lv, _ = convert.unpack_bitnet_packed(np.array([[0b10100001, 0b00011000], [0b10010000, 0b00001010]], np.uint8))
    assert (lv[:, 0].astype(int) - 2).tolist() == [0, -1, -1, -1, 1, 0, 1, 1]
    assert np.array_equal(lv.astype(np.int8) - 2, ref["ex_ternary"])


def test_field_value_3_is_counted_and_becomes_level_3():
    Mw, K = 64, 32
    lv, packed = bp.levels(5, Mw, K)
    got, invalid = convert.unpack_bitnet_packed(packed)
    assert invalid == 0 and np.array_equal(got, lv)
    bad, want, n = bp.with_invalid(5, Mw, K, 37)
    assert n >= 30
    got, invalid = convert.unpack_bitnet_packed(bad)
    assert invalid == n and np.array_equal(got, want)
    for f in range(4):                                       # every field took part
        assert (((bad >> (2 * f)) & 3) == 3).any()
    with pytest.raises(ValueError):
        convert.pack_bitnet_packed(np.zeros((4, 4), np.uint8))       # level 0 is no ternary level
    with pytest.raises(TypeError):
        convert.unpack_bitnet_packed(packed.astype(np.int32))


@pytest.mark.parametrize("value", [1.6875, 0.73, 2.3, 3.0, 1e-3, 417.0])
def test_packed_scale_both_conventions(value):
    for form, (stored, v) in bp.scale_forms(value).items():
        assert np.float32(v).dtype == np.float32
        v64 = float(v)                                       # exact
        mul = convert.bitnet_packed_scale(stored, "autobitlinear")
        div = convert.bitnet_packed_scale(stored, "bitlinear")
        assert mul.dtype == np.float32 and div.dtype == np.float32
        assert pc.raw_bits(mul)[0] == pc.raw_bits(np.float32(v64))[0], (form, value)
        assert pc.raw_bits(div)[0] == pc.raw_bits(np.float32(1.0 / v64))[0], (form, value)
        for shaped in (stored.reshape(()), stored.reshape(1, 1)):
            assert convert.bitnet_packed_scale(shaped, "bitlinear") == div
    assert convert.bitnet_packed_scale(value) == convert.bitnet_packed_scale(np.float32(value), "bitlinear")      # the default is BitNetQuantConfig's
    assert convert.bitnet_packed_scale(value, "autobitlinear") == np.float32(value)


def test_bitlinear_reciprocal_is_one_rounded_division():
    """1 / 3 is not exact: s must be the float32 nearest to it, not a float16 / bf16 reciprocal and not 1 / float64 kept wide"""
    three = np.array([3.0], np.float16)
    s = convert.bitnet_packed_scale(three, "bitlinear")
    assert s.dtype == np.float32 and s == np.float32(1.0) / np.float32(3.0) and pc.raw_bits(s)[0] == 0x3EAAAAAB
    assert float(s) != 1.0 / 3.0 and s != np.float32(np.float16(1.0) / np.float16(3.0))
    b = np.array([0x4040], np.uint16)                        # 3.0 as bf16
    assert pc.raw_bits(convert.bitnet_packed_scale(b, "bitlinear"))[0] == 0x3EAAAAAB


def test_packed_scale_refusals():
    with pytest.raises(ValueError, match="linear_class"):
        convert.bitnet_packed_scale(1.0, "linear")
    with pytest.raises(ValueError, match="one expected"):
        convert.bitnet_packed_scale(np.ones(2, np.float32))
    with pytest.raises(TypeError):
        convert.bitnet_packed_scale(np.array(["1"]))


# ---- the shared header through plain g++ ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def packer(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pack_ternary") / "pack_ternary_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(HERE, "cpp", "pack_ternary_main.cc")], check=True)
    return exe


def run(packer, d, form, packed, Mw, K, bm):
    paths = [str(d / n) for n in ("p.bin", "A.bin")]
    packed.tofile(paths[0])
    r = subprocess.run([packer] + [str(v) for v in (form, Mw, K, bm, bp.KF)] + paths, check=True, stdout=subprocess.PIPE)
    return np.fromfile(paths[1], np.uint8), int(r.stdout)


@pytest.mark.parametrize("shape", bp.SHAPES)
def test_both_formulations_are_unpack_then_preprocess(packer, tmp_path, shape):
    Mw, K, bm, mg = shape
    lv, packed = bp.levels(Mw + K, Mw, K)
    A, _ = pc.host_blob_codes(lv, bp.scales(mg), None, 2, bm, bp.KF)
    for form in (0, 1):
        gA, invalid = run(packer, tmp_path, form, packed, Mw, K, bm)
        assert invalid == 0 and np.array_equal(gA, A.reshape(-1)), form


def test_invalid_fields_through_the_shared_rule(packer, tmp_path):
    Mw, K, bm, mg = bp.SHAPES[2]
    bad, lv, n = bp.with_invalid(9, Mw, K, 301)
    A, _ = pc.host_blob_codes(lv, bp.scales(mg), None, 2, bm, bp.KF)
    for form in (0, 1):
        gA, invalid = run(packer, tmp_path, form, bad, Mw, K, bm)
        assert invalid == n and np.array_equal(gA, A.reshape(-1)), form
