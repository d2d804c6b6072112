"""experts_gemm_plan (tmac_launch_plan.cpp) without a GPU, through tests/cpp/experts_gemm_plan_main.cc built with plain g++: the grid, the LDS
bytes and every refusal of the grouped expert GEMM."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "tmac_amd", "csrc")


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("experts_gemm_plan") / "experts_gemm_plan")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", os.path.join(HERE, "cpp", "experts_gemm_plan_main.cc"), os.path.join(CSRC, "tmac_launch_plan.cpp"),
                    "-o", exe], check=True)

    def ask(*queries):
        out = subprocess.run([exe], input="".join("plan " + " ".join(map(str, q)) + "\n" for q in queries), capture_output=True, text=True, check=True)
        return out.stdout.splitlines()
    return ask


def test_grid_and_lds(ask):
    # K bits gs ags nbanks Mw0 Mw1 N S E P: x = the banks' row-tile quartets, each bank rounded up on its own; y = T_max; 64 KB + 4 x 1 KB
    shapes = {(1024, 2, 128, 64, 1, 320, 0, 40, 2, 4, 320): (2, 5, 2, 0), (1024, 2, 128, 64, 2, 128, 64, 40, 2, 4, 320): (2, 5, 1, 2),
              (4096, 4, 64, 64, 2, 14336, 14336, 256, 2, 8, 1024): (112, 16, 56, 112), (2048, 3, 128, 64, 1, 132, 0, 1, 1, 4, 64): (1, 1, 1, 0)}
    for want, line in zip(shapes.values(), ask(*shapes)):
        assert line == " ".join(map(str, want)) + " 69632", line


def test_every_refusal_names_its_reason(ask):
    ok = [1024, 2, 128, 64, 1, 320, 0, 40, 2, 4, 320]

    def but(**kw):
        return [kw.get(k, v) for k, v in zip(("K", "bits", "gs", "ags", "nb", "Mw0", "Mw1", "N", "S", "E", "P"), ok)]
    want = [(but(P=256), "P is not 64 x T_max"), (but(P=384), "P is not 64 x T_max"), (but(gs=192), "outside what k_gemm_planes"),
            (but(ags=32), "outside what k_gemm_planes"), (but(bits=5), "outside what k_gemm_planes"), (but(nb=3), "one or two banks"),
            (but(Mw0=322), "multiple of 4"), (but(S=9), "1 to 8 slots"), (but(K=24576, N=16384, E=256, P=64 * 768), "position image reaches 2 GB"),
            (but(K=24576, bits=4, gs=128, Mw0=349528), "matrix reaches 2 GB")]
    for (q, word), line in zip(want, ask(*[q for q, _ in want])):
        assert line.startswith("refuse: ") and word in line, (q, line)
