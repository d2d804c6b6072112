"""The AWQ packer's index and nibble arithmetic without a GPU: the AWQ functions of tmac_amd/csrc/tmac_pack.h, the header the pack
kernels (tmac_pack.hip) share, compiled with plain g++ into tests/cpp/pack_awq_main.cc, which packs whole matrices through them.
Required: the bytes of the host route -- weights.preprocess_weights from convert.unpack_awq -- on the shapes of awq_common.SHAPES (a
word-load shape, a 16-byte-load shape, a whole wide tile), the scales' raw bits, including fp16 zero products that round and one that
overflows."""
import os
import subprocess

import numpy as np
import pytest

import awq_common as ac
import pack_common as pc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def packer(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pack_awq") / "pack_awq_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "cpp", "pack_awq_main.cc")], check=True)
    return exe


def run(packer, d, Mw, K, bm, kf, gs, zp, sdt, odt, qw, sc, qz):
    paths = [str(d / n) for n in ("w.bin", "s.bin", "z.bin", "A.bin", "S.bin")]
    qw.tofile(paths[0]); sc.tofile(paths[1])
    (qz if qz is not None else np.zeros(0, np.uint8)).tofile(paths[2])
    subprocess.run([packer] + [str(int(v)) for v in (Mw, K, bm, kf, gs, zp, sdt == np.float16, odt == np.float16)] + paths, check=True)
    return np.fromfile(paths[3], np.uint8), np.fromfile(paths[4], odt)


@pytest.mark.parametrize("sdt", (np.float16, np.float32))
@pytest.mark.parametrize("shape", ("A", "B", "C"))
def test_awq_form_is_unpack_then_preprocess(packer, tmp_path, shape, sdt):
    Mw, K, bm, kf, gs, ags = ac.SHAPES[shape]
    (qw, sc, qz), _ = ac.make_awq(ord(shape) + (sdt == np.float32), Mw, K, gs, sdt)
    A, S, (w, s_u, z_u, bits, g) = ac.host_blob(qw, sc, qz, bm, kf)
    assert bits == 4 and g == gs and S.dtype == sdt
    if sdt == np.float16:
        exact = z_u.astype(np.float64) == (z_u.astype(np.float64) / s_u.astype(np.float64)).round() * s_u.astype(np.float64)
        assert not exact[np.isfinite(z_u)].all(), "some fp16 zero product must have been rounded"
        assert np.isinf(z_u).any(), "a zero overflows fp16"
    gA, gS = run(packer, tmp_path, Mw, K, bm, kf, gs, True, sdt, sdt, qw, sc, qz)
    assert np.array_equal(gA, A.reshape(-1))
    assert np.array_equal(pc.raw_bits(gS), pc.raw_bits(S))
    # the other output dtype: the zero is rounded to the scales' dtype first, then converted
    odt = np.float32 if sdt == np.float16 else np.float16
    with np.errstate(over="ignore"):
        want = S.astype(odt)
    _, gS2 = run(packer, tmp_path, Mw, K, bm, kf, gs, True, sdt, odt, qw, sc, qz)
    assert np.array_equal(pc.raw_bits(gS2), pc.raw_bits(want))


def test_awq_form_without_zero_points(packer, tmp_path):
    Mw, K, bm, kf, gs, ags = ac.SHAPES["A"]
    (qw, sc, qz), _ = ac.make_awq(5, Mw, K, gs, np.float16)
    A, S, _ = ac.host_blob(qw, sc, qz, bm, kf, zero_point=False)
    gA, gS = run(packer, tmp_path, Mw, K, bm, kf, gs, False, np.float16, np.float16, qw, sc, None)
    assert np.array_equal(gA, A.reshape(-1)) and np.array_equal(pc.raw_bits(gS), pc.raw_bits(S))
