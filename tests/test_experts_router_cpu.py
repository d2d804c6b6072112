"""The fused router without a GPU: its symbols, and its launch planner through tmac_hip_debug_experts_router_plan (pure, no device)."""
import ctypes as C
import os

import pytest

import tmac_amd


def plan(K, E, S, N, w=tmac_amd.F16, x=tmac_amd.F16):      # (rc, dict of the plan) of a call shape
    v, lds = [C.c_int32() for _ in range(5)], C.c_size_t()
    rc = tmac_amd.lib().tmac_hip_debug_experts_router_plan(K, E, S, N, w, x, *[C.byref(i) for i in v], C.byref(lds))
    return rc, dict(zip(("waves", "ctiles", "slices", "steps", "grid"), (i.value for i in v)), lds=lds.value)


def test_symbols_and_no_device():
    L = tmac_amd.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tmac_hip.h")).read()
    for name in ("tmac_hip_experts_router_dev", "tmac_hip_debug_experts_router_plan"):
        assert name + "(" in header and hasattr(L, name)
    assert "experts_router" in vars(tmac_amd.TMACGeMMWrapper)
    if L.tmac_hip_device_count() == 0:       # (with a device the GPU tests speak)
        assert L.tmac_hip_experts_router_dev(None, tmac_amd.F16, None, tmac_amd.F16, 1, 64, 8, 2, 0, None, None, None, None) == -2      # TMAC_HIP_E_NODEVICE


@pytest.mark.parametrize("E", [1, 8, 32, 33, 60, 64, 96, 128, 160, 200, 256])
@pytest.mark.parametrize("K", [64, 128, 192, 960, 2048, 4096, 7168])
def test_the_slices_cover_k_once_whatever_n(K, E):
    rc, p = plan(K, E, 1, 1)
    assert rc == 0 and p["ctiles"] == -(-E // 32) and p["waves"] == p["ctiles"] * p["slices"] <= 16
    # slice i owns the 64-value steps [i steps, (i + 1) steps), the last what is left: every step once, no slice empty
    assert (p["slices"] - 1) * p["steps"] < K // 64 <= p["slices"] * p["steps"]
    assert p["lds"] == 4 * p["slices"] * 32 * 32 * p["ctiles"] <= 163840
    for N, S in ((33, 1), (4096, min(E, 8))):
        rc, q = plan(K, E, S, N, tmac_amd.F32, tmac_amd.F16)
        assert rc == 0 and q == dict(p, grid=-(-N // 32))


@pytest.mark.parametrize("K,E,S,N,word", [(128, 257, 2, 3, "E: the router takes at most 256 experts"), (128, 16, 9, 3, "S: 1 to 8 experts"),
                                          (128, 8, 0, 3, "S: 1 to 8 experts"), (128, 3, 4, 3, "E: at least S experts"), (96, 8, 2, 3, "K: a multiple of 64"),
                                          (0, 8, 2, 3, "K: a multiple of 64"), (128, 8, 8, 4097, "N x S: the router takes at most 32768 slots"),
                                          (128, 8, 2, 0, "N: at least one token")])
def test_the_planner_refuses_by_name(K, E, S, N, word):
    rc, _ = plan(K, E, S, N)
    assert rc == -4 and word in tmac_amd.lib().tmac_hip_last_error().decode()
