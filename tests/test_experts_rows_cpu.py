"""experts_rows_sizes (tmac_launch_plan.cpp) without a GPU, through tests/cpp/experts_rows_plan_main.cc built with plain g++: the tile bound
of a call shape and its limits."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "tmac_amd", "csrc")


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("experts_rows_plan") / "experts_rows_plan")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", os.path.join(HERE, "cpp", "experts_rows_plan_main.cc"), os.path.join(CSRC, "tmac_launch_plan.cpp"),
                    "-o", exe], check=True)

    def ask(*queries):
        out = subprocess.run([exe], input="".join(" ".join(map(str, q)) + "\n" for q in queries), capture_output=True, text=True, check=True)
        return out.stdout.splitlines()
    return ask


def test_tile_bound(ask):
    shapes = [(40, 2, 4), (70, 2, 8), (48, 4, 3), (5, 3, 4), (700, 3, 60), (1, 1, 256), (4096, 8, 256), (64, 2, 8), (256, 4, 60)]
    for (N, S, E), line in zip(shapes, ask(*[("sizes",) + q for q in shapes])):
        T = N * S // 64 + min(E, N * S)
        assert line == f"{T} {64 * T}", (N, S, E, line)
        # the bound holds for the worst split: every expert one slot past whole tiles
        assert T >= max(-(-(N * S - (k - 1)) // 64) + (k - 1) for k in range(1, min(E, N * S) + 1))
    want = {(4097, 8, 4): "at most 32768 slots", (40, 2, 257): "1 to 256 experts", (40, 9, 4): "1 to 8 slots", (0, 2, 4): "at least one token"}
    for q, line in zip(want, ask(*[("sizes",) + q for q in want])):
        assert line.startswith("refuse: ") and want[q] in line, (q, line)
