"""Packing through a K permutation (act-order) without a GPU: the index arithmetic tmac_amd/csrc/tmac_pack.h adds for the permuted pack
kernels (gptq_word_row, gptq_code, codes_four), compiled with plain g++ into tests/cpp/pack_perm_main.cc, which packs whole matrices
through it.  Required: the bytes of the host route on the matrix with its columns gathered,
weights.preprocess_weights(w[:, perm], sc, zr, ...), with w, sc, zr from convert.unpack_gptq for the GPTQ form.
"""
import os
import subprocess

import numpy as np
import pytest

import pack_common as pc

HERE = os.path.dirname(os.path.abspath(__file__))
GS, KF = 64, 16
BM = {1: 64, 2: 64, 3: 192, 4: 64}


@pytest.fixture(scope="module")
def packer(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pack_perm") / "pack_perm_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "cpp", "pack_perm_main.cc")], check=True)
    return exe


def perms(seed, K):
    """a random act-order permutation (exactly GS members per group), the reversal, and group 0 made of the last GS columns"""
    g = np.repeat(np.arange(K // GS, dtype=np.int32), GS)
    np.random.default_rng(seed).shuffle(g)
    rev = (np.arange(K, dtype=np.int32) // GS)[::-1]
    last = np.roll(np.arange(K, dtype=np.int32) // GS, -GS)       # the last GS columns are group 0, everything else moves up a group
    return [np.argsort(x, kind="stable").astype(np.int32) for x in (g, rev, last)]


def run(packer, d, form, Mw, K, bits, src, perm):
    paths = [str(d / n) for n in ("w.bin", "p.bin", "A.bin")]
    src.tofile(paths[0]); perm.tofile(paths[1])
    subprocess.run([packer, form] + [str(v) for v in (Mw, K, bits, BM[bits], KF)] + paths, check=True)
    return np.fromfile(paths[2], np.uint8)


@pytest.mark.parametrize("K", (256, 1024))
@pytest.mark.parametrize("Mw", (64, 256))
@pytest.mark.parametrize("bits", (1, 2, 4))
def test_gptq_form_packs_the_gathered_matrix(packer, tmp_path, bits, Mw, K):
    qw, sc, qz = pc.make_gptq(31 * bits + Mw + K, Mw, K, bits, GS, np.float16)
    _, _, (w, s_u, z_u, b, g) = pc.host_blob_gptq(qw, sc, qz, True, BM[bits], KF)
    assert (b, g) == (bits, GS)
    for perm in perms(bits + K, K):
        assert not np.array_equal(perm, np.arange(K))
        A, _ = pc.host_blob_codes(np.ascontiguousarray(w[:, perm]), s_u, z_u, bits, BM[bits], KF)
        assert np.array_equal(run(packer, tmp_path, "gptq", Mw, K, bits, qw, perm), A.reshape(-1))


@pytest.mark.parametrize("K", (256, 1024))
@pytest.mark.parametrize("Mw", (64, 256))
@pytest.mark.parametrize("bits", (1, 2, 3, 4))
def test_codes_form_packs_the_gathered_matrix(packer, tmp_path, bits, Mw, K):
    codes, sc, zr = pc.make_codes(17 * bits + Mw + K, Mw, K, bits, GS, np.float32)
    assert (codes >> bits).any(), "the codes carry bits above the width"
    for perm in perms(bits + K + 1, K):
        A, _ = pc.host_blob_codes(np.ascontiguousarray(codes[:, perm]), sc, zr, bits, BM[bits], KF)
        assert np.array_equal(run(packer, tmp_path, "codes", Mw, K, bits, codes, perm), A.reshape(-1))


def test_identity_is_the_plain_pack(packer, tmp_path):
    bits, Mw, K = 2, 64, 256
    qw, sc, qz = pc.make_gptq(3, Mw, K, bits, GS, np.float16)
    A, _, _ = pc.host_blob_gptq(qw, sc, qz, True, BM[bits], KF)
    assert np.array_equal(run(packer, tmp_path, "gptq", Mw, K, bits, qw, np.arange(K, dtype=np.int32)), A.reshape(-1))
