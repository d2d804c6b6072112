"""The refusals of the four transform sites, pinned: tests/golden/xf_refusals.json holds what the library answered to a fixed grid of
tmac_hip_xform values (tests/golden/make_xf_refusals.py: every kind and gate, every operand absent / present / off by 8 bytes, CARRY,
keep, residual_out over every vector a call reads and over its output) at tmac_hip_qgemm_fused_xf_dev, tmac_hip_qgemm_fused_xf_rows_dev
(N = 2), tmac_hip_debug_xf_rows and tmac_hip_chain_xform, before the field rules moved into tmac_amd/csrc/tmac_xform.cpp.  The grid is
replayed; required per case: the recorded return code, the recorded message verbatim, and -- after every non-zero code -- the arena as it
was before the call (outputs and residual_out keep their poison, nothing else is written).
"""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_the_recorded_grid_replays_verbatim():
    spec = importlib.util.spec_from_file_location("make_xf_refusals", os.path.join(HERE, "golden", "make_xf_refusals.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(gen.OUT) as f:
        golden = json.load(f)
    cases = golden["cases"]
    inputs = [{k: v for k, v in c.items() if k not in ("rc", "msg", "untouched")} for c in cases]
    assert inputs == gen.grid(), "the committed grid is the generator's"
    assert (golden["K"], golden["Mw"], golden["region"], golden["off"]) == (gen.K, gen.MW, gen.REGION, gen.OFF)
    bad = []
    for c, (rc, msg, untouched) in zip(cases, gen.replay(inputs)):
        if (rc, msg, untouched) != (c["rc"], c["msg"], c["untouched"]) or (rc and not untouched):
            bad.append((c["site"], c["name"], (rc, msg, untouched), (c["rc"], c["msg"], c["untouched"])))
    assert not bad, bad[:5]
