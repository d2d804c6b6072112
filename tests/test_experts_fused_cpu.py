"""tmac_hip_debug_experts_fused_plan without a GPU: the plan of an experts call does not know how its tables are made -- for every kind
the fused entry point takes it is tmac_hip_debug_experts_plan's, field for field, or that function's refusal -- and the transform's own
refusals need no device."""
import ctypes as C

import pytest

SHAPES = [(1024, 2, 128, 128), (3200, 2, 128, 320), (1024, 4, 64, 256), (2048, 3, 128, 192), (11008, 2, 128, 64), (1024, 2, 128, 704),
          (14336, 2, 128, 4096)]      # K, bits, group size, Mw: tests/test_gpu_experts.py's six and Mixtral's down
KINDS = [0, 2, 0x102, 0x202]


def plan(fn, K, bits, gs, Mw, S, lut_rows, combine, *kind):
    out = [C.c_int32(-1) for _ in range(3)] + [C.c_size_t(0)]
    rc = fn(K, bits, gs, (C.c_int * 1)(Mw), 1, S, lut_rows, combine, *kind, *[C.byref(o) for o in out])
    return rc, tuple(o.value for o in out)


@pytest.mark.parametrize("K,bits,gs,Mw", SHAPES)
def test_the_plan_does_not_know_the_table_source(K, bits, gs, Mw):
    import tmac_amd
    L = tmac_amd.lib()
    for S in (1, 2, 3, 8):
        for lut_rows, combine in ((1, 0), (S, 0), (S, 1)):
            want = plan(L.tmac_hip_debug_experts_plan, K, bits, gs, Mw, S, lut_rows, combine)
            for kind in KINDS:
                if kind and lut_rows != S:
                    continue
                assert plan(L.tmac_hip_debug_experts_fused_plan, K, bits, gs, Mw, S, lut_rows, combine, kind) == want, (S, lut_rows, combine, kind)
    assert plan(L.tmac_hip_debug_experts_plan, 11008, 2, 128, 64, 8, 8, 0)[0] == -1      # (the refusal is shared too: 8 rows of K = 11008)


@pytest.mark.parametrize("kind,S,lut_rows,word", [(1, 2, 2, "TMAC_XF_NORM is not served"), (4, 2, 2, "TMAC_XF_GLU_NORM is not served"),
                                                  (0x104, 2, 2, "TMAC_XF_GLU_NORM is not served"), (0x302, 2, 2, "unknown gate"),
                                                  (0x100, 2, 2, "takes no gate"), (3, 2, 2, "unknown transform kind"),
                                                  (2, 3, 1, "one row of in and in2 per slot")])
def test_refusals_of_the_transform(kind, S, lut_rows, word):
    import tmac_amd
    L = tmac_amd.lib()
    rc, out = plan(L.tmac_hip_debug_experts_fused_plan, 1024, 2, 128, 128, S, lut_rows, 0, kind)
    assert rc == -4 and word in L.tmac_hip_last_error().decode() and out == (-1, -1, -1, 0)
