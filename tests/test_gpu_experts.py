"""k_gemv_experts behind tmac_hip_qgemm_experts_dev: top-k expert GEMVs, the expert of a slot read on the GPU.  Banks of E = 4 distinct
random experts against the oracle per expert (orc.qgemm_float on the row the slot reads; REL_TOL * max|C|, the contract of
test_gpu_parity.py: a wrong pick misses by orders of magnitude) and float64 numpy; slots, empty slots and COMBINE bit for bit."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from test_gpu_defer import stats
from test_gpu_parity import REL_TOL, rel_err, tm  # noqa: F401  (tm: the module fixture)

pytestmark = pytest.mark.gpu
E, ROWS = 4, 8
SHAPES = {  # name: Mw, K, bits, bm, gs, zp, fp16 device scales
    "half_step": (128, 1024, 2, 128, 128, True, False),
    "ragged": (320, 3200, 2, 320, 128, True, True),
    "gs64": (256, 1024, 4, 256, 64, False, False),
    "w3": (192, 2048, 3, 192, 128, True, False),
    "long": (64, 11008, 2, 128, 128, True, False),       # six steps, four waves per quad, 8 rows do not fit LDS
    "passes": (704, 1024, 2, 128, 128, False, False),    # more quads than one pass
    "narrow": (64, 1024, 2, 64, 128, True, False),       # second bank of "half_step": same K and config, other Mw
}
IDS = {1: [3], 2: [1, 2], 3: [2, 0, 2], 8: [3, 1, 0, 2, 2, 1, 3, 0]}
GATES = [0.37, 0.21, 0.29, 0.05, 0.11, 0.43, 0.17, 0.31]

_banks = {}


def bank_of(tm, name):
    """(wrapper, ExpertBank, X fp32 [ROWS][K], oracle fp64 [E][ROWS][Mw]) of a shape: built and computed once, left unchanged"""
    if name not in _banks:
        Mw, K, bits, bm, gs, zp, sc16 = SHAPES[name]
        wr = tm.TMACGeMMWrapper(act_group_size=64)
        ws, ref = [], []
        X = np.random.default_rng(K).standard_normal((ROWS, K)).astype(np.float32)      # by K alone: banks of one call share it
        for e in range(E):
            case = orc.make_case(2700 + 10 * len(_banks) + e, Mw, K, N=ROWS, bits=bits, gs=gs, ags=64, zero_point=zp,
                                 fp16_values=sc16)      # (fp16 device scales hold these values exactly)
            A = orc.preprocess_weights(case["w"], bits, bm, 16)
            S = orc.preprocess_scales(case["sc"], case["zr"] if zp else None, bits, bm)
            ws.append(wr.register_weights(A, S, Mw, K, bits, tm.KCfg.make(Mw, K, bits, bm, 16, gs, 64, zp), scales_dtype=tm.F32,
                                          dev_dtype=tm.F16 if sc16 else tm.F32))
            q, ls, lb = orc.preprocessor(X, 64)
            ref.append(orc.qgemm_float(A, q, S, ls, lb, Mw, K, ROWS, bits, bm, 16, gs, 64, zp).astype(np.float64))
        X.setflags(write=False)
        _banks[name] = (wr, tm.ExpertBank.from_handles(ws), X, np.stack(ref))
    return _banks[name]


def admits(tm, name, S, lut_rows, combine=False):
    Mw, K, bits, _, gs, _, _ = SHAPES[name]
    return tm.lib().tmac_hip_debug_experts_plan(K, bits, gs, (C.c_int * 1)(Mw), 1, S, lut_rows, int(combine), None, None, None, None) == 0


def dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.array(a, dtype)).cuda()


def nan_out(shape, f16=False):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float16 if f16 else torch.float32, device="cuda")


def slots(tm, name, ids, rows, f16=False):
    """a SLOTS call on one bank: slot s reads X[rows[s]] (rows an int: every slot reads that one row); returns the [S][Mw] tensor"""
    import torch
    wr, bank, X, _ = bank_of(tm, name)
    x = dev(X[rows]) if isinstance(rows, int) else dev(X[list(rows)])
    out = wr.experts(bank, x, dev(ids, np.int32), out=[nan_out((len(ids), bank.Mw), f16)])[0]
    torch.cuda.synchronize()
    return out


def within(out, want):
    assert rel_err(out.float().cpu().numpy(), want) <= REL_TOL


@pytest.mark.parametrize("name", [n for n in SHAPES if n != "narrow"])
def test_slots_against_the_oracle(tm, name):
    ref = bank_of(tm, name)[3]
    served = 0
    for S, ids in IDS.items():
        f16 = name == "w3" and S == 3                                          # fp16 output on one case
        within(slots(tm, name, ids, 5, f16), np.stack([ref[e, 5] for e in ids]))            # one x shared by the slots
        if admits(tm, name, S, S):
            within(slots(tm, name, ids, range(S), f16), np.stack([ref[e, s] for s, e in enumerate(ids)]))   # slot s reads row s
            served += 1
    assert served == (3 if name == "long" else 4)      # S = 8 rows of K = 11008 do not fit LDS: refused by the plan, below by the call


def test_two_banks_share_the_ids(tm):
    import torch
    (wr, gate, X, rg), (_, up, _, ru) = bank_of(tm, "half_step"), bank_of(tm, "narrow")
    ids = IDS[3]
    og, ou = wr.experts([gate, up], dev(X[2]), dev(ids, np.int32), out=[nan_out((3, gate.Mw)), nan_out((3, up.Mw))])
    torch.cuda.synchronize()
    within(og, np.stack([rg[e, 2] for e in ids]))
    within(ou, np.stack([ru[e, 2] for e in ids]))


@pytest.mark.parametrize("name", ["half_step", "long"])
def test_a_slot_is_a_slot(tm, name):
    import torch
    ids = IDS[3]
    full = slots(tm, name, ids, range(3))
    back = slots(tm, name, ids[::-1], [2, 1, 0])
    for s, e in enumerate(ids):
        assert torch.equal(full[s], slots(tm, name, [e], [s])[0])             # the only slot of an S = 1 call
        assert torch.equal(full[s], back[2 - s])                              # at another position


@pytest.mark.parametrize("name", ["ragged", "long"])
def test_empty_slots(tm, name):
    import torch
    wr, bank, X, _ = bank_of(tm, name)
    got, want = slots(tm, name, [1, -1, 3], range(3)), slots(tm, name, [1, 3], [0, 2])
    assert torch.equal(got[1], torch.zeros_like(got[1]))
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[1])
    g = dev(GATES[:3], np.float32)
    c3 = wr.experts(bank, dev(X[:3]), dev([1, -1, 3], np.int32), gates=g, out=nan_out((bank.Mw,)))
    c2 = wr.experts(bank, dev(X[[0, 2]]), dev([1, 3], np.int32), gates=g[[0, 2]].contiguous(), out=nan_out((bank.Mw,)))
    torch.cuda.synchronize()
    assert torch.isfinite(c2).all() and torch.equal(c3, c2)


@pytest.mark.parametrize("name", ["ragged", "gs64", "long", "passes"])
def test_combine_is_the_gated_sum_of_the_slots(tm, name):
    import torch
    wr, bank, X, ref = bank_of(tm, name)
    ids = IDS[3]
    y = slots(tm, name, ids, range(3)).cpu().numpy()
    got = wr.experts(bank, dev(X[:3]), dev(ids, np.int32), gates=dev(GATES[:3], np.float32), out=nan_out((bank.Mw,)))
    torch.cuda.synchronize()
    acc = np.zeros(bank.Mw, np.float32)
    for s in range(3):      # two roundings per slot, slot order, from 0
        acc = (acc + (np.float32(GATES[s]) * y[s]).astype(np.float32)).astype(np.float32)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), acc.view(np.uint32))
    want = sum(np.float64(np.float32(GATES[s])) * ref[e, s] for s, e in enumerate(ids))
    bound = REL_TOL * sum(abs(GATES[s]) * np.abs(ref[e, s]).max() for s, e in enumerate(ids))
    assert np.abs(got.cpu().numpy() - want).max() <= bound


def refused(tm, code, word, call, *outs):
    import torch
    with pytest.raises(tm.TMACHipError) as ei:
        call()
    torch.cuda.synchronize()
    assert ei.value.code == code and word in str(ei.value), ei.value
    assert all(torch.isnan(o).all() for o in outs), "a refused call wrote an output"


def test_refusals(tm):
    import torch
    L = tm.lib()
    wr, bank, X, _ = bank_of(tm, "half_step")
    _, long_bank, XL, _ = bank_of(tm, "long")
    other = bank_of(tm, "narrow")[1]
    refused(tm, -4, "expert 1: Mw", lambda: tm.ExpertBank.from_handles([bank.experts[0], other.experts[0]]))
    refused(tm, -4, "at least one expert", lambda: tm.ExpertBank.from_handles([]))
    Mw, K = bank.Mw, bank.K
    case = orc.make_case(2790, Mw, K, N=1, bits=2, gs=128, ags=64, zero_point=True)
    A, S = orc.preprocess_weights(case["w"], 2, 128, 16), orc.preprocess_scales(case["sc"], case["zr"], 2, 128)
    biased = wr.register_weights(A, S, Mw, K, 2, tm.KCfg.make(Mw, K, 2, 128, 16, 128, 64, True))
    biased._set_bias(np.ones(Mw, np.float32))
    refused(tm, -4, "expert 1: handles with a bias", lambda: tm.ExpertBank.from_handles([bank.experts[0], biased]))
    ucase = orc.make_case(2791, Mw, K, N=1, bits=2, gs=128, ags=K, zero_point=False, m_groups=1)
    unified = tm.TMACGeMMWrapper(act_group_size=K).register_weights(orc.preprocess_weights(ucase["w"], 2, 128, 16), ucase["sc"], Mw, K, 2,
                                                                  tm.KCfg.make(Mw, K, 2, 128, 16, 128, K, False, 1))
    refused(tm, -1, "expert 0: unified-scale", lambda: tm.ExpertBank.from_handles([unified]))
    ids, g = dev(IDS[3], np.int32), dev(GATES[:3], np.float32)
    o1, o2 = nan_out((3, Mw)), nan_out((3, other.Mw))
    refused(tm, -4, "COMBINE", lambda: wr.experts([bank, other], dev(X[:3]), ids, gates=g, out=[o1, o2]), o1, o2)
    o8 = nan_out((8, long_bank.Mw))
    refused(tm, -1, "do not fit LDS", lambda: wr.experts(long_bank, dev(XL), dev(IDS[8], np.int32), out=[o8]), o8)
    tm.binding.check(L.tmac_hip_chain_begin())
    try:
        refused(tm, -4, "tmac_hip_qgemm_experts_dev cannot be recorded", lambda: wr.experts(bank, dev(X[0]), ids, out=[o1]), o1)
    finally:
        L.tmac_hip_chain_abort()
    queued = nan_out((1, Mw))
    tm.binding.check(L.tmac_hip_defer(1))      # with deferral on the call runs behind the queue: it flushes it first
    try:
        f0 = stats(tm)[0]
        wr.fused([bank.experts[0]], dev(X[:1]), [queued], 1)
        assert stats(tm)[0] == f0
        wr.experts(bank, dev(X[0]), ids, out=[o1])
        assert stats(tm)[0] == f0 + 1
    finally:
        L.tmac_hip_defer(0)
    torch.cuda.synchronize()
    assert torch.isfinite(queued).all() and torch.isfinite(o1).all()
    biased.free(); unified.free()


def test_graph_replays_follow_the_ids(tm):
    import torch
    wr, bank, X, _ = bank_of(tm, "long")
    x, ids, g = dev(X[:3]), dev(IDS[3], np.int32), dev(GATES[:3], np.float32)
    ys, yc = nan_out((3, bank.Mw)), nan_out((bank.Mw,))
    side = torch.cuda.Stream()

    def calls():
        wr.experts(bank, x, ids, out=[ys], stream=side)
        wr.experts(bank, x, ids, gates=g, out=yc, stream=side)
    with torch.cuda.stream(side):
        calls()                      # warm-up on the stream that is captured: its workspace exists afterwards
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        calls()
    for new_ids in ([0, 3, 1], [2, -1, 0], IDS[3]):
        ids.copy_(dev(new_ids, np.int32))                  # rewritten on the device, between replays
        ys.fill_(float("nan")); yc.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        got_s, got_c = ys.clone(), yc.clone()
        with torch.cuda.stream(side):
            calls()
        torch.cuda.synchronize()
        assert torch.isfinite(got_c).all() and torch.equal(got_s, ys) and torch.equal(got_c, yc)
