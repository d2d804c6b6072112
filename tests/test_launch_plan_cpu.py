"""Launch planning without a GPU: tmac_amd/csrc/tmac_launch_plan.cpp compiled with plain g++ into a stand-alone program
(tests/cpp/launch_plan_main.cc: its own main) and fed the recorded grid, tests/golden/launch_plans.json -- the plans and refusals of
k_gemv_quad (heuristic, forced and XF, strict and lenient) and k_gemv_rows as the selection code chose them before the planners existed
(tests/golden/make_launch_plans.py says how it was recorded).  Required: every recorded plan and refusal, field for field; the grid at
its recorded size; the generator reproduces the file byte for byte; and every plan names an instantiation the policy predicate has.
"""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "launch_plans.json")
N_QUERIES = 19796           # the recorded grid
N_PLANS = 12298             # ... of which so many are plans, not refusals
N_ROWS_PLANS = 612          # ... of which so many answer rows_plan alone (no instantiation to name)


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_launch_plans", os.path.join(HERE, "golden", "make_launch_plans.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def program(gen, tmp_path_factory):
    return gen.build_program(str(tmp_path_factory.mktemp("launch_plan")))


@pytest.fixture(scope="module")
def replay(program, gen):
    """(query, recorded answer, answer, predicate column) of every query the FILE holds"""
    with open(GOLDEN) as f:
        golden = json.load(f)
    qs, want = [], []
    for template, axis, idx in golden["cases"]:
        values = golden["axes"][axis]
        assert len(idx) == len(values)
        qs += [template.replace("{}", str(v)) for v in values]
        want += [golden["answers"][i] for i in idx]
    got, inst = gen.answers(program, qs)
    return list(zip(qs, want, got, inst))


def test_every_recorded_plan_and_refusal(replay):
    assert len(replay) >= N_QUERIES, "the grid shrank"
    assert sum(1 for _, want, _, _ in replay if want != "refuse") >= N_PLANS, "the grid lost its plans"
    kinds = {q[0] for q, _, _, _ in replay}
    assert kinds == {"q", "x", "r", "p"}
    bad = [(q, want, got) for q, want, got, _ in replay if want != got]
    assert not bad, bad[:5]


def test_generator_reproduces_the_file(program, gen):
    with open(GOLDEN) as f:
        text = f.read()
    assert len(gen.queries(gen.cases())) >= N_QUERIES, "the generator's grid shrank"
    assert gen.record(program) == text


def test_every_plan_names_an_instantiation(replay):
    plans = [(q, got, inst) for q, _, got, inst in replay if got != "refuse" and q[0] != "p"]
    assert len(plans) >= N_PLANS - N_ROWS_PLANS
    bad = [(q, got) for q, got, inst in plans if inst != 1]
    assert not bad, bad[:5]
