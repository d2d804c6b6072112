"""experts_plan (tmac_launch_plan.cpp) without a GPU, through tests/cpp/experts_plan_main.cc built with plain g++.  The LDS rule is restated
from the layout against the 163,840 B budget of rows_lds_bytes: 8 rows fit up to K = 8192, 4 up to K = 18432."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "tmac_amd", "csrc")
LDS_MAX = 163840


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("experts_plan") / "experts_plan")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", os.path.join(HERE, "cpp", "experts_plan_main.cc"), os.path.join(CSRC, "tmac_launch_plan.cpp"),
                    "-o", exe], check=True)

    def ask(*queries):
        out = subprocess.run([exe], input="".join(" ".join(map(str, q)) + "\n" for q in queries), capture_output=True, text=True, check=True)
        return out.stdout.splitlines()
    return ask


def lds(K, rows):
    nst = (K // 32 + 63) // 64
    return rows * (4 * (nst * 64 + 1) * 16 + 4 * 2 * nst * 32) + 4 * 2 * 8 * 4


@pytest.mark.parametrize("S,mode", [(8, 0), (4, 1), (2, 1), (3, 0)])
def test_row_limit(ask, S, mode):
    Ks = [1408, 2048, 6144, 6208, 8192, 8256, 11008, 12288, 12352, 14336, 18432, 18496, 24576]
    got = ask(*[(K, 2, 64, 4096, 0, S, S, mode) for K in Ks])
    for K, line in zip(Ks, got):
        if lds(K, S) <= LDS_MAX:
            assert line.endswith("| inst 1") and int(line.split()[3]) == lds(K, S), (K, line)
        else:
            assert line.startswith("refuse") and "do not fit LDS" in line, (K, line)
    fits = [not l.startswith("refuse") for l in got]
    assert fits == sorted(fits, reverse=True)
    assert fits == [K <= {8: 8192, 4: 18432}.get(S, 24576) for K in Ks]
    shared = ask(*[(K, 2, 64, 4096, 0, S, 1, 0) for K in Ks])                # one x for all slots: one row of tables, whatever S
    assert all(int(l.split()[3]) == lds(K, 1) for K, l in zip(Ks, shared))


def test_waves_per_quad_by_the_shape_alone(ask):
    for K, Mw0, Mw1, want in [(1024, 128, 0, 1), (4096, 4096, 0, 2), (4096, 14336, 14336, 1), (14336, 4096, 0, 2), (11008, 64, 0, 4), (4096, 256, 0, 2),
                              (1408, 2048, 0, 1)]:
        nb = (1, Mw1) if Mw1 else (Mw0,)
        lines = ask(*[(K, 2, 128, Mw0, Mw1, S, lr, mode) for S in (1, 2, 3) for lr in {1, S} for mode in (0, 1) if not (mode and (lr != S or Mw1))])
        wpqs = {int(l.split()[0]) for l in lines}
        assert wpqs == {want}, (K, Mw0, Mw1, lines)                           # never by S, lut_rows or the mode
        quads = (Mw0 + Mw1) // 4
        for l in lines:                                                       # persistent grid: every item has a wave, at most 512 workgroups
            wpq, gx, items = (int(v) for v in l.split()[:3])
            assert items in (quads, 2 * quads, 3 * quads) and 1 <= gx <= 512 and gx <= -(-items * wpq // 8), (nb, l)


def test_refusals(ask):
    want = {(1024, 2, 128, 128, 64, 3, 3, 1): "COMBINE takes one bank", (1024, 2, 128, 128, 0, 3, 1, 1): "one activation row per slot",
            (1024, 2, 128, 128, 0, 9, 9, 0): "1 to 8 slots", (1024, 2, 128, 128, 0, 0, 0, 0): "1 to 8 slots", (1024, 2, 128, 128, 0, 4, 2, 0): "lut_rows",
            (1000, 2, 128, 128, 0, 2, 2, 0): "outside", (1024, 5, 128, 128, 0, 2, 2, 0): "outside", (1024, 2, 128, 130, 0, 2, 2, 0): "outside",
            (1024, 2, 96, 128, 0, 2, 2, 0): "outside", (1024, 2, 128, 128, 0, 2, 2, 2): "mode"}
    for q, line in zip(want, ask(*want)):
        assert line.startswith("refuse: ") and want[q] in line, (q, line)
