"""Expert banks for token batches: k_experts_route and k_experts_combine behind TMACGeMMWrapper.experts_route / experts_combine.  The routing
against a numpy restatement, element for element, -1 tails included; the gated sum bit for bit against the same fp32 operations in torch
and against float64."""
import numpy as np
import pytest

from test_gpu_experts import dev, nan_out
from test_gpu_parity import REL_TOL, tm  # noqa: F401  (tm: the module fixture)

pytestmark = pytest.mark.gpu
N, S, E = 40, 2, 4
IDS = np.zeros((N, S), np.int32)                      # expert 0: 66 slots, two tiles; expert 2 none; two empty slots; tile 4 of 5 unused
IDS[26:, 1] = [1, 3, 1, 3, -1, 3, 1, 1, 3, 3, 1, -1, 3, 1]
GATES = np.random.default_rng(28).uniform(0.05, 0.6, (N, S)).astype(np.float32)


def route_np(ids, n_exp):
    """stable counting sort of the flat slots by expert, segments padded to 64: tile_expert [T_max], src [64 T_max], pos [N S]"""
    f = ids.reshape(-1)
    T = f.size // 64 + min(n_exp, f.size)
    te, src, pos = (np.full(n, -1, np.int32) for n in (T, 64 * T, f.size))
    p = 0
    for e in range(n_exp):
        idx = np.flatnonzero(f == e)
        src[p:p + idx.size], pos[idx] = idx, p + np.arange(idx.size)
        tiles = -(-idx.size // 64)
        te[p // 64:p // 64 + tiles] = e
        p += 64 * tiles
    return te, src, pos


def route_cases():
    a = np.full(140, -1, np.int32)                    # 64 of expert 1, 65 of expert 5, a few of 7, the rest empty; 140 = 2 * 64 + 12
    a[3:131:2], a[0:130:2], a[131:136] = 1, 5, 7
    rng = np.random.default_rng(5)
    return {"64_and_65": (a.reshape(70, 2), 8), "one_takes_all": (np.full((48, 4), 2, np.int32), 3),
            "under_a_tile": (rng.integers(-1, 4, (5, 3)).astype(np.int32), 4), "many_waves": (rng.integers(-1, 60, (700, 3)).astype(np.int32), 60),
            "skewed": (IDS, E)}


@pytest.mark.parametrize("case", list(route_cases()))
def test_route_is_the_stable_sort(tm, case):
    ids, n_exp = route_cases()[case]
    assert case != "64_and_65" or sorted(np.bincount(ids[ids >= 0])[[1, 5]]) == [64, 65]
    got = tm.TMACGeMMWrapper(act_group_size=64).experts_route(dev(ids), n_exp)
    for g, w in zip(got, route_np(ids, n_exp)):
        assert np.array_equal(g.cpu().numpy(), w)


@pytest.mark.parametrize("Mw,f16", [(320, False), (132, True)])
def test_combine_is_the_gated_sum(tm, Mw, f16):
    import torch
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    route = wr.experts_route(dev(IDS), E)
    pos, P = route[2].cpu().numpy(), int(route[1].numel())
    rows = np.random.default_rng(Mw).standard_normal((P, Mw)).astype(np.float32)
    rows[route[1].cpu().numpy() < 0] = np.nan        # padding positions and the unused tile: never read
    c, g = dev(rows), dev(GATES)
    got = wr.experts_combine(c, route, g, out=nan_out((N, Mw), f16))
    torch.cuda.synchronize()
    p = route[2].view(N, S).long()
    acc = torch.zeros((N, Mw), device="cuda")
    for s in range(S):                                # a rounded multiply, a rounded add, slot order, from 0; empty slots add nothing
        acc = torch.where(p[:, s:s + 1] >= 0, acc + g[:, s:s + 1] * c[p[:, s].clamp(min=0)], acc)
    assert torch.equal(got, acc.half() if f16 else acc) and (pos < 0).any() and torch.isfinite(got).all()
    if not f16:                                       # fp32 sums of S terms against float64: S roundings of 2^-24 each on the terms' magnitude
        live = (pos >= 0).reshape(N, S)
        want = sum(np.where(live[:, s:s + 1], np.float64(GATES[:, s:s + 1]) * rows[np.maximum(pos.reshape(N, S)[:, s], 0)], 0) for s in range(S))
        assert np.abs(got.cpu().numpy() - want).max() <= REL_TOL * GATES.sum(1).max() * np.nanmax(np.abs(rows))


def test_graph_replays_follow_the_ids(tm):
    import torch
    wr, Mw = tm.TMACGeMMWrapper(act_group_size=64), 128
    ids, g = dev(IDS), dev(GATES)
    P = 64 * (N * S // 64 + E)
    route = tuple(torch.empty(n, dtype=torch.int32, device="cuda") for n in (P // 64, P, N * S))
    c, y = dev(np.random.default_rng(3).standard_normal((P, Mw)).astype(np.float32)), nan_out((N, Mw))
    side = torch.cuda.Stream()

    def calls():
        wr.experts_route(ids, E, out=route, stream=side)
        wr.experts_combine(c, route, g, out=y, stream=side)
    with torch.cuda.stream(side):
        calls()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        calls()
    for shift in (1, 2, 3):
        new = np.where(IDS >= 0, (IDS + shift) % E, -1).astype(np.int32)
        ids.copy_(dev(new))                           # rewritten on the device, between replays
        y.fill_(float("nan"))
        for t in route:
            t.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        got = y.clone()
        for r, w in zip(route, route_np(new, E)):
            assert np.array_equal(r.cpu().numpy(), w)
        with torch.cuda.stream(side):
            calls()
        torch.cuda.synchronize()
        assert torch.isfinite(got).all() and torch.equal(got, y)


@pytest.mark.parametrize("case", ["recording", "slots_limit", "experts_limit", "misaligned"])
def test_refusals(tm, case):
    import torch
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    route = wr.experts_route(dev(IDS), E)
    c, y = torch.zeros((320, 64), device="cuda"), nan_out((N, 64))
    marks = tuple(torch.full((n,), -7, dtype=torch.int32, device="cuda") for n in (5, 320, 80))
    code, word, call = {
        "recording": (-4, "tmac_hip_experts_route_dev cannot be recorded", lambda: wr.experts_route(dev(IDS), E, out=marks)),
        "slots_limit": (-4, "at most 32768 slots", lambda: wr.experts_route(torch.zeros((4097, 8), dtype=torch.int32, device="cuda"), E, out=marks)),
        "experts_limit": (-4, "1 to 256 experts", lambda: wr.experts_route(dev(IDS), 257, out=marks)),
        "misaligned": (-4, "y_dev 16-byte aligned", lambda: wr.experts_combine(c, route, dev(GATES), out=nan_out((N * 64 + 1,))[1:].view(N, 64)))}[case]
    if case == "recording":
        tm.binding.check(tm.lib().tmac_hip_chain_begin())
    try:
        with pytest.raises(tm.TMACHipError) as ei:
            call()
    finally:
        if case == "recording":
            tm.lib().tmac_hip_chain_abort()
    torch.cuda.synchronize()
    assert ei.value.code == code and word in str(ei.value), ei.value
    assert torch.isnan(y).all() and all((m == -7).all() for m in marks), "a refused call wrote an output"
