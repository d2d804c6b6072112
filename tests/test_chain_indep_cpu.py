"""Which call ends a recording's independence, without a GPU: tmac_amd/csrc/tmac_chain_indep.h compiled with plain g++ into a stand-alone
program (tests/cpp/chain_indep_main.cc).  tmac_hip_chain_end decides stream mode with this verdict and, for a recording that was declared
independent (tmac_hip_chain_begin_independent), words its refusal from it: the FIRST call in recorded order that breaks the declaration is
named, its data flow before its transform, and an exchange step -- which belongs to no call -- only when every call is clean.
"""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
OK, FLOW, FLOW2, XFORM, EPILOGUE, EXCHANGE = range(6)
NONE = (-1, -1, 0, 0)                    # (src, src2, xf_kind, epi) of a call that reads memory and carries nothing


@pytest.fixture(scope="module")
def indep(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("indep") / "chain_indep_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "cpp", "chain_indep_main.cc")], check=True)

    def verdict(ops, exchange_steps=0):
        out = subprocess.run([exe, str(exchange_steps)] + [",".join(str(v) for v in o) for o in ops], capture_output=True, text=True, check=True).stdout
        return tuple(int(v) for v in out.split())
    return verdict


def test_independent_calls(indep):
    assert indep([NONE]) == (OK, -1, -1)
    assert indep([NONE] * 7) == (OK, -1, -1)
    assert indep([]) == (OK, -1, -1)


@pytest.mark.parametrize("ops,steps,want", [
    ([NONE, (0, -1, 0, 0)], 0, (FLOW, 1, 0)),                                   # op 1 reads op 0's output
    ([NONE, NONE, NONE, (1, -1, 0, 0), (0, -1, 0, 0)], 0, (FLOW, 3, 1)),        # the first reader is named, with ITS producer
    ([NONE, NONE, (-1, 1, 2, 0)], 0, (FLOW2, 2, 1)),                            # a GLU whose second vector is an output
    ([NONE, (0, 0, 2, 0)], 0, (FLOW, 1, 0)),                                    # both vectors handed over: the activations are named
    ([NONE, (-1, -1, 1, 0), (1, -1, 0, 0)], 0, (XFORM, 1, -1)),                 # a transform in front of a later flow: the earlier call
    ([(-1, -1, 4, 0)], 0, (XFORM, 0, -1)),
    ([NONE, (0, -1, 1, 0)], 0, (FLOW, 1, 0)),                                   # flow and transform on one call: its data flow first
    ([(-1, -1, 0, 1), NONE], 0, (EPILOGUE, 0, -1)),                             # a gate/up call that publishes the product
    ([NONE, NONE], 1, (EXCHANGE, -1, -1)),                                      # clean calls and an exchange step
    ([NONE, (0, -1, 0, 0)], 2, (FLOW, 1, 0)),                                   # a call is named before an exchange step is
])
def test_the_first_offending_call_is_named(indep, ops, steps, want):
    assert indep(ops, steps) == want
