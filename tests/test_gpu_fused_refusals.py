"""The seven doors of the fused call, pinned: tests/golden/fused_refusals.json holds what the library answered to a fixed grid of matrix
lists and arguments (tests/golden/make_fused_refusals.py: every matrix set at N = 1, 2, 3 under the default knobs,
tmac_hip_set_gemm_min_n(2) and tmac_hip_debug_rows_kernel 1 and 2; every single fault; every pair of faults that can coexist in one call,
which pins the ORDER of a door's checks) at tmac_hip_qgemm_fused_dev -- plain, on act-order handles, while recording, while deferring --,
tmac_hip_qgemm_fused_xf_dev, tmac_hip_qgemm_fused_xf_rows_dev and tmac_hip_qgemm_fused_partial_sums, before the call became one value
(FusedCall) checked by named checks.  The grid is replayed; required per case: the recorded return code, the recorded message verbatim,
the recorded status of the door's closing call, the recorded tmac_hip_debug_route_stats delta, for an accepted case the recorded plan
(tmac_hip_debug_fused_plan / tmac_hip_debug_xf_rows_plan), and -- after every non-zero code -- the arena as it was before the call.
"""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_the_recorded_grid_replays_verbatim():
    spec = importlib.util.spec_from_file_location("make_fused_refusals", os.path.join(HERE, "golden", "make_fused_refusals.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(gen.OUT) as f:
        golden = json.load(f)
    inputs = gen.grid()
    assert golden["grid_sha256"] == gen.grid_digest(inputs), "the committed grid is the generator's"
    assert (golden["weights"], golden["off"]) == (json.loads(json.dumps(gen.WEIGHTS)), gen.OFF)
    recorded = gen.unpack(golden["classes"])
    assert sorted(recorded) == sorted((c["door"], c["name"]) for c in inputs), "one recorded answer per case of the grid"
    assert {d for d, _ in recorded} == set(gen.DOORS)
    assert sum(1 for v in recorded.values() if v[0]) > 1000 and sum(1 for v in recorded.values() if not v[0]) > 400
    bad = []
    for c, res in zip(inputs, gen.replay(inputs)):
        want = recorded[c["door"], c["name"]]
        got = tuple(list(r) if isinstance(r, (list, tuple)) else r for r in res)
        if got != want or (res[0] and not res[2]):
            bad.append((c["door"], c["name"], got, want))
    assert not bad, (len(bad), bad[:5])
