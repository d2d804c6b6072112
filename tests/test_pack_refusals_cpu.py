"""The fourteen doors in front of the pack kernels, pinned: tests/golden/pack_refusals.json holds what the library answered to a fixed grid
of faulty calls (tests/golden/make_pack_refusals.py: every single fault a door names; every pair of faults that can coexist in one call,
which pins the ORDER of a door's checks) before the six formats shared one pack_to and one register_from.  The grid is replayed without a
GPU: every answer was decided in front of the first call that touches a device, so the pointers are integers that nothing dereferences.
Required per case: the recorded return code and the recorded message verbatim.

Beside the recording, the rule every register door holds since that change: a dev_float other than TMAC_F32 / TMAC_F16 is refused, as the
last argument check.
"""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
E_NOMATCH, E_NODEVICE, E_ARG = -1, -2, -4


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_pack_refusals", os.path.join(HERE, "golden", "make_pack_refusals.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_recorded_grid_replays_verbatim(gen):
    with open(gen.OUT) as f:
        golden = json.load(f)
    inputs = gen.grid()
    assert golden["grid_sha256"] == gen.grid_digest(inputs), "the committed grid is the generator's"
    recorded = gen.unpack(golden["classes"])
    assert sorted(recorded) == sorted((c["door"], c["name"]) for c in inputs), "one recorded answer per case of the grid"
    assert {d for d, _ in recorded} == set(gen.DOORS) and len(gen.DOORS) == 14
    assert len(recorded) > 1000
    # decided in front of ensure_device: an argument refusal, never the answer of a machine without a device
    assert all(rc in (E_ARG, E_NOMATCH) and rc != E_NODEVICE and msg for rc, msg in recorded.values())
    bad = []
    for c, got in zip(inputs, gen.replay(inputs, recorded)):
        want = recorded[c["door"], c["name"]]
        if tuple(got) != want:
            bad.append((c["door"], c["name"], got, want))
    assert not bad, (len(bad), bad[:5])


DEV_FLOAT = "dev_float must be TMAC_F32 or TMAC_F16"
REGISTER_DOORS = ["register_gptq", "register_codes", "register_awq", "register_absmean", "register_ternary", "register_rtn",
                  "register_gptq_perm", "register_codes_perm"]


@pytest.mark.parametrize("door", REGISTER_DOORS)
def test_every_register_door_refuses_another_dev_float(gen, door):
    import tmac_amd
    L = tmac_amd.lib()
    c = dict(gen.base(door), dev=7)       # (the _perm_ doors: a NULL permutation)
    assert gen.run(L, tmac_amd.KCfg, c) == (E_ARG, DEV_FLOAT)
    # ... as the last argument check: whatever else the call is refused for wins
    faults = gen.faults(door)
    assert len(faults) >= 8
    for name, (_, do) in faults.items():
        if name == "dev-float-7":
            continue
        alone, both = gen.base(door), dict(gen.base(door), dev=7)
        do(alone); do(both)
        want = gen.run(L, tmac_amd.KCfg, alone)
        assert want[0] in (E_ARG, E_NOMATCH) and want[1] != DEV_FLOAT, (name, want)
        assert gen.run(L, tmac_amd.KCfg, both) == want, name
