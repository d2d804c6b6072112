"""The K permutation of act-order (desc_act) GPTQ matrices without a GPU: tmac_amd/csrc/tmac_kperm.cpp compiled with plain g++ into a
stand-alone program (tests/cpp/kperm_main.cc: its own main, its own tmac_host::fail).  Required: perm == np.argsort(g_idx, kind="stable")
for random group assignments and for the identity; every refusal, naming the first offending group; equality by content, not by object.
And, in pure numpy float64, the DIRECTION of the permutation, independently of every kernel: GPTQ's own definition of the dense product
against the de-quantised permuted matrix on x[perm].
"""
import os
import subprocess

import numpy as np
import pytest

import pack_common as pc
from tmac_amd import convert

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
E_ARG = -4
SHAPES = ((256, 64), (512, 128), (1024, 128))


@pytest.fixture(scope="module")
def kperm(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kperm") / "kperm_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "cpp", "kperm_main.cc"),
                    os.path.join(ROOT, "tmac_amd", "csrc", "tmac_kperm.cpp")], check=True)
    return exe


def random_g_idx(seed, K, gs):
    """every group exactly gs members, in random places"""
    g = np.repeat(np.arange(K // gs, dtype=np.int32), gs)
    np.random.default_rng(seed).shuffle(g)
    return g


def build(exe, d, g_idx, K, gs):
    gp, pp = str(d / "g.bin"), str(d / "p.bin")
    np.asarray(g_idx, np.int32).tofile(gp)
    out = subprocess.run([exe, "build", str(K), str(gs), gp, pp], capture_output=True, text=True, check=True).stdout.rstrip("\n").split("\t")
    rc, msg, ident, pid = int(out[0]), out[1], int(out[2]), int(out[3])
    return rc, msg, bool(ident), pid, (np.fromfile(pp, np.int32) if rc == 0 else None)


def test_e_arg_is_the_librarys():
    with open(os.path.join(ROOT, "include", "tmac_hip.h")) as f:
        assert "#define TMAC_HIP_E_ARG ({})".format(E_ARG) in f.read()


@pytest.mark.parametrize("K,gs", SHAPES)
def test_perm_is_the_stable_argsort(kperm, tmp_path, K, gs):
    for seed in range(3):
        g = random_g_idx(1000 * seed + K, K, gs)
        rc, msg, ident, pid, perm = build(kperm, tmp_path, g, K, gs)
        assert rc == 0, msg
        assert np.array_equal(perm, np.argsort(g, kind="stable"))
        assert not ident and pid != 0
        assert (np.sort(perm) == np.arange(K)).all() and (g[perm] == np.arange(K) // gs).all()
    rc, msg, ident, pid, perm = build(kperm, tmp_path, np.arange(K, dtype=np.int32) // gs, K, gs)
    assert rc == 0 and ident and pid != 0 and np.array_equal(perm, np.arange(K))
    # the reversal is a permutation of whole groups and of the members inside them: not the identity
    rc, msg, ident, pid, perm = build(kperm, tmp_path, (np.arange(K, dtype=np.int32) // gs)[::-1], K, gs)
    assert rc == 0 and not ident and np.array_equal(perm, np.argsort((np.arange(K) // gs)[::-1], kind="stable"))


def test_refusals_name_the_first_offending_group(kperm, tmp_path):
    K, gs = 256, 64
    ok = np.arange(K, dtype=np.int32) // gs
    g = ok.copy(); g[5] = 4                                   # outside [0, K / gs)
    rc, msg, *_ = build(kperm, tmp_path, g, K, gs)
    assert rc == E_ARG and "g_idx[5] = 4" in msg and "outside [0, 4)" in msg
    g = ok.copy(); g[7] = -1
    rc, msg, *_ = build(kperm, tmp_path, g, K, gs)
    assert rc == E_ARG and "g_idx[7] = -1" in msg
    g = ok.copy(); g[200] = 1                                 # group 1 has 65 members, group 3 has 63: group 1 is named
    rc, msg, *_ = build(kperm, tmp_path, g, K, gs)
    assert rc == E_ARG and "group 1 has 65 members" in msg and "group_size = 64" in msg
    g = ok.copy(); g[0] = 2                                   # group 0 has 63
    rc, msg, *_ = build(kperm, tmp_path, g, K, gs)
    assert rc == E_ARG and "group 0 has 63 members" in msg
    rc, msg, *_ = build(kperm, tmp_path, ok, K, 96)           # K % group_size
    assert rc == E_ARG and "K=256 is no whole number of groups of 96" in msg
    rc, msg, *_ = build(kperm, tmp_path, ok, K, 0)
    assert rc == E_ARG and "must be positive" in msg


def test_equality_is_by_content(kperm, tmp_path):
    K, gs = 512, 128
    g = random_g_idx(7, K, gs)
    a, b, c = (str(tmp_path / n) for n in ("a.bin", "b.bin", "c.bin"))
    g.tofile(a); g.copy().tofile(b)
    eq, ia, ib = (int(v) for v in subprocess.run([kperm, "equal", str(K), str(gs), a, b], capture_output=True, text=True, check=True).stdout.split())
    assert eq == 1 and ia == ib != 0
    # one swapped pair of members of different groups: another permutation, another hash
    i, j = 0, int(np.nonzero(g != g[0])[0][0])
    g2 = g.copy(); g2[i], g2[j] = g2[j], g2[i]
    g2.tofile(c)
    eq, ia, ic = (int(v) for v in subprocess.run([kperm, "equal", str(K), str(gs), a, c], capture_output=True, text=True, check=True).stdout.split())
    assert eq == 0 and ia != ic


@pytest.mark.parametrize("v2", (True, False))
@pytest.mark.parametrize("bits", (2, 4))
def test_direction_of_the_permutation(bits, v2):
    """y = W x from GPTQ's definition, W[k, m] = scales[g_idx[k], m] * (q[k, m] - z[g_idx[k], m]) (z: the stored zero, + 1 for v1), against
    the de-quantised PERMUTED matrix -- the codes of convert.unpack_gptq with their columns gathered, groups contiguous -- times x[perm].  Both are float64 sums of the same K products per output in another order: |difference| <= K 2^-52 sum |terms|."""
    Mw, K, gs = 64, 512, 128
    qw, sc_g, qz = pc.make_gptq(bits * 10 + int(v2), Mw, K, bits, gs, np.float32, hard=False)
    g_idx = random_g_idx(bits, K, gs)
    perm = np.argsort(g_idx, kind="stable")
    x = np.random.default_rng(3).standard_normal(K)
    # GPTQ's definition, straight from the packed tensors
    q = convert._unpack_fields(qw, bits).transpose(0, 2, 1).reshape(K, Mw).astype(np.float64)          # [k][m]
    z = convert._unpack_fields(qz, bits).reshape(K // gs, Mw).astype(np.float64) + (0 if v2 else 1)    # [g][m]
    s = sc_g.astype(np.float64)                                                                       # [g][m]
    terms = s[g_idx] * (q - z[g_idx]) * x[:, None]
    y = terms.sum(axis=0)
    # the permuted matrix as the library holds it: codes from convert.unpack_gptq with their columns gathered, scale and zero of
    # position k' those of group k' // gs (de-quantised in float64 from the exact integers: the same K products per output)
    w, _, _, b, g = convert.unpack_gptq(qw, sc_g, qz, gptq_v2=v2)
    assert (b, g) == (bits, gs)
    grp = np.arange(K) // gs
    Wp = s.T[:, grp] * (w[:, perm].astype(np.float64) - z.T[:, grp])      # [m][k']
    yp = (Wp * x[perm][None, :]).sum(axis=1)
    bound = K * 2.0 ** -52 * np.abs(terms).sum(axis=0)
    assert (np.abs(y - yp) <= bound).all(), float(np.abs(y - yp).max())
    # and the direction matters: the inverse permutation misses by far more
    inv = np.argsort(perm)
    assert np.abs(y - (Wp * x[inv][None, :]).sum(axis=1)).max() > 1e3 * bound.max()
