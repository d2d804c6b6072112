"""The field rules of tmac_hip_xform without a GPU: tmac_amd/csrc/tmac_xform.cpp compiled with plain g++ into a stand-alone program
(tests/cpp/xf_resolve_main.cc: its own main, its own tmac_host::fail) and fed the recorded refusal grid, tests/golden/xf_refusals.json
(tests/golden/make_xf_refusals.py).  Replayed: every case the recorded library accepted, and every refusal the resolver alone decides --
kind, gate, operands, CARRY, alignment, overlap.  Required: the recorded return code and the recorded message, verbatim.  Pointers are
integers here (the arena's offsets above a fixed base) and nothing is dereferenced.
"""
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BASE = 0x7f0000000000          # where the arena "lies": 256-byte aligned like the device allocation the grid was recorded on
# the resolver's refusals (everything else in the file -- the tap's own argument check -- belongs to the entry points)
RESOLVER = ("unknown transform kind", "transform kind", "unknown gate", "GLU_NORM ", "GLU needs", "TMAC_XF_CARRY", "transform vector",
            "residual_out overlaps")
SITE_N = {"xf": 1, "rows": 2, "tap": 2, "chain": 1}


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "xf_refusals.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def resolver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("xf_resolve") / "xf_resolve")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "cpp", "xf_resolve_main.cc"),
                    os.path.join(ROOT, "tmac_amd", "csrc", "tmac_xform.cpp")], check=True)
    return exe


def test_resolver_replays_the_recorded_grid(golden, resolver):
    off, K, Mw = golden["off"], golden["K"], golden["Mw"]
    ptr = lambda v: 0 if v is None else 1 if v == "carry" else BASE + v
    cases = [c for c in golden["cases"] if c["rc"] == 0 or c["msg"].startswith(RESOLVER)]
    assert len(cases) > 300 and sum(1 for c in cases if c["rc"]) > 150, "the grid shrank"
    lines = []
    for c in cases:
        N, tap = SITE_N[c["site"]], c["site"] == "tap"
        out, out_bytes = (BASE + off["x_out"], N * K * 4) if tap else (BASE + off["C"], N * Mw * 4)
        lines.append(" ".join(str(v) for v in (c["site"], c["kind"], ptr(c["in2"]), ptr(c["residual"]), ptr(c["gamma"]), ptr(c["residual_out"]),
                                               c["keep"], BASE + off["B"], K, N, out, out_bytes)))
    got = subprocess.run([resolver], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
    assert len(got) == len(cases)
    bad = []
    for c, line in zip(cases, got):
        rc, _, msg = line.partition("\t")
        if int(rc) != c["rc"] or msg != c["msg"]:
            bad.append((c["site"], c["name"], (int(rc), msg), (c["rc"], c["msg"])))
    assert not bad, bad[:5]
