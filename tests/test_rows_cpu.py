"""The row-group rule of k_gemv_rows (tmac_hip_debug_rows_plan): a pure host function, no device is touched.  Launches and the parity tap
group an N-row call by this function alone, so what holds here holds for every launch."""
import ctypes as C

import pytest

KS = [512, 1024, 3200, 4096, 11008, 14336, 24576]
LDS_MAX = 163840


@pytest.fixture(scope="module")
def L():
    import tmac_amd
    return tmac_amd.lib()


def plan(L, K, mg, N):
    r_fit, ng, lds = C.c_int32(0), C.c_int32(0), C.c_size_t(0)
    cap, live = (C.c_int32 * 32)(), (C.c_int32 * 32)()
    rc = L.tmac_hip_debug_rows_plan(K, mg, N, C.byref(r_fit), C.byref(ng), cap, live, C.byref(lds))
    assert rc == 0, (K, mg, N, L.tmac_hip_last_error())
    return r_fit.value, ng.value, list(cap[:ng.value]), list(live[:ng.value]), lds.value


@pytest.mark.parametrize("mg", [-1, 1])
def test_row_groups(L, mg):
    fits = []
    for K in KS:
        r_fits = set()
        for N in range(1, 18):
            r_fit, ng, cap, live, lds = plan(L, K, mg, N)
            assert (r_fit, ng, cap, live, lds) == plan(L, K, mg, N)          # deterministic
            assert r_fit in (2, 4, 8) and 0 < lds <= LDS_MAX
            assert ng == -(-N // r_fit)
            rows = []
            n0 = 0
            for g in range(ng):
                assert 1 <= live[g] <= cap[g] and cap[g] in (2, 4, 8)
                rows += list(range(n0, n0 + live[g]))
                n0 += live[g]
            assert rows == list(range(N))                                    # rows 0 .. N-1 exactly once
            assert all(live[g] == r_fit and cap[g] == r_fit for g in range(ng - 1))
            assert cap[-1] == min(c for c in (2, 4, 8) if c >= live[-1])     # the smallest capacity that takes the remainder
            r_fits.add(r_fit)
        assert len(r_fits) == 1                                              # r_fit is a function of K alone
        fits.append(r_fits.pop())
    assert fits == sorted(fits, reverse=True)                                # monotone non-increasing in K
    assert fits[-1] >= 2                                                     # K = 24576, the largest K the quad layout's kernels admit


def test_refusals(L):
    for K, mg, N in [(1000, -1, 4), (1024, 0, 4), (1024, -1, 0), (1 << 20, -1, 4)]:
        assert L.tmac_hip_debug_rows_plan(K, mg, N, None, None, None, None, None) == -4, (K, mg, N)
