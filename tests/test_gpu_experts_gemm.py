"""k_lut_image_pos + k_gemm_experts behind TMACGeMMWrapper.experts_rows: the grouped GEMM over routed positions.  Banks, inputs and oracle
results are test_gpu_experts.bank_of's (E = 4, eight activation rows per shape), the routing is test_gpu_experts_rows' (N = 40, S = 2:
expert 0 holds one full tile + 2, expert 2 nothing, two empty slots, one unused tile); token n reads X[n % 8].  The bar is REL_TOL * max|C|.
The bank with a ragged last tile has Mw = 136 (W4, bm = 32), not 132: the oracle's weight preprocessing takes row counts of 8 alone."""
import numpy as np
import pytest

from test_gpu_experts import ROWS, SHAPES, bank_of, dev, nan_out
from test_gpu_experts_rows import E, GATES, IDS, N, S, route_np
from test_gpu_parity import REL_TOL, rel_err, tm  # noqa: F401  (tm: the module fixture)

pytestmark = pytest.mark.gpu
TE, SRC, POS = route_np(IDS, E)
P = SRC.size
LIVE, USED = SRC >= 0, np.repeat(TE >= 0, 64)
ROW = (np.maximum(SRC, 0) // S) % ROWS                   # the row of X a position reads
EXP = np.repeat(np.maximum(TE, 0), 64)
assert (USED & ~LIVE).any() and (~USED).any()


def bank(tm, name):
    if name == "tile136":                               # 2 full row tiles + 8 rows, built the way bank_of builds
        SHAPES.setdefault(name, (136, 1024, 4, 32, 128, True, False))
    return bank_of(tm, name)


def tokens(X):
    return dev(X[np.arange(N) % ROWS])


def check(out, ref):
    got = out.float().cpu().numpy()
    assert rel_err(got[LIVE], ref[EXP, ROW][LIVE]) <= REL_TOL
    pad = got[USED & ~LIVE]
    assert np.array_equal(pad.view(np.uint32), np.zeros_like(pad, np.uint32)), "a padding position is not +0"
    assert np.isnan(got[~USED]).all(), "the unused tile was written"


@pytest.mark.parametrize("name", ["half_step", "ragged", "gs64", "w3", "long", "tile136"])
def test_positions_against_the_oracle(tm, name):
    import torch
    wr, b, X, ref = bank(tm, name)
    route = wr.experts_route(dev(IDS), E)
    out = wr.experts_rows(b, tokens(X), route, S, out=[nan_out((P, b.Mw), name == "w3")])[0]
    torch.cuda.synchronize()
    check(out, ref)


def test_two_banks_share_a_routing(tm):
    import torch
    (wr, gate, X, rg), (_, up, _, ru) = bank(tm, "half_step"), bank(tm, "narrow")
    og, ou = wr.experts_rows([gate, up], tokens(X), wr.experts_route(dev(IDS), E), S, out=[nan_out((P, gate.Mw)), nan_out((P, up.Mw))])
    torch.cuda.synchronize()
    check(og, rg)
    check(ou, ru)


def test_position_major_activations(tm):
    import torch
    wr, b, X, ref = bank(tm, "ragged")
    xp = np.full((P, b.K), np.nan, np.float32)          # rows at padding positions and in the unused tile are never read
    xp[LIVE] = X[ROW[LIVE]]
    out = wr.experts_rows(b, dev(xp), wr.experts_route(dev(IDS), E), S, out=[nan_out((P, b.Mw))])[0]
    torch.cuda.synchronize()
    check(out, ref)


def test_a_row_is_a_row(tm):
    import torch
    wr, b, X, _ = bank(tm, "long")
    full = wr.experts_rows(b, tokens(X), wr.experts_route(dev(IDS), E), S)[0]
    for n, s in ((0, 0), (27, 1), (39, 1)):             # experts 0, 3 and 1; the first sits in the full tile of expert 0
        one = dev(IDS[n:n + 1, s:s + 1])
        r1 = wr.experts_route(one, E)
        alone = wr.experts_rows(b, dev(X[n % ROWS][None]), r1, 1)[0]
        torch.cuda.synchronize()
        assert IDS[n, s] >= 0 and torch.equal(full[POS[n * S + s]], alone[int(r1[2][0])])


def test_graph_replay_follows_the_routing(tm):
    import torch
    wr, b, X, _ = bank(tm, "half_step")
    ids, x, g = dev(IDS), tokens(X), dev(GATES)
    route = tuple(torch.empty(n, dtype=torch.int32, device="cuda") for n in (P // 64, P, N * S))
    c, y = torch.zeros((P, b.Mw), device="cuda"), nan_out((N, b.Mw))
    side = torch.cuda.Stream()

    def calls():
        wr.experts_route(ids, E, out=route, stream=side)
        wr.experts_rows(b, x, route, S, out=[c], stream=side)
        wr.experts_combine(c, route, g, out=y, stream=side)
    with torch.cuda.stream(side):
        calls()                                         # warm-up on the captured stream: its workspace exists afterwards
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        calls()
    for shift in (1, 2, 3):                             # several replays, each against the eager calls
        ids.copy_(dev(np.where(IDS >= 0, (IDS + shift) % E, -1).astype(np.int32)))      # rewritten on the device
        y.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        got = y.clone()
        with torch.cuda.stream(side):
            calls()
        torch.cuda.synchronize()
        assert torch.isfinite(got).all() and torch.equal(got, y)


@pytest.mark.parametrize("case", ["recording", "x_rows", "positions", "banks_K", "misaligned"])
def test_refusals_launch_nothing(tm, case):
    import torch
    wr, b, X, _ = bank(tm, "half_step")
    route = wr.experts_route(dev(IDS), E)
    c = nan_out((P, b.Mw))
    short = tuple(t[:n] for t, n in zip(route, (P // 64 - 1, P - 64, N * S)))
    odd = nan_out((P * b.Mw + 1,))[1:].view(P, b.Mw)
    word, call, outs = {
        "recording": ("tmac_hip_qgemm_experts_rows_dev cannot be recorded", lambda: wr.experts_rows(b, tokens(X), route, S, out=[c]), [c]),
        "x_rows": ("x_rows=41", lambda: wr.experts_rows(b, dev(np.zeros((N + 1, b.K), np.float32)), route, S, out=[c]), [c]),
        "positions": ("P is not 64 x T_max", lambda: wr.experts_rows(b, tokens(X), short, S, out=[c[:P - 64]]), [c]),
        "banks_K": ("share K", lambda: wr.experts_rows([b, bank(tm, "long")[1]], tokens(X), route, S, out=[c, c[:, :64].contiguous()]), [c]),
        "misaligned": ("C_dev[0] must be 16-byte aligned", lambda: wr.experts_rows(b, tokens(X), route, S, out=[odd]), [c, odd])}[case]
    if case == "recording":
        tm.binding.check(tm.lib().tmac_hip_chain_begin())
    try:
        with pytest.raises(tm.TMACHipError) as ei:
            call()
    finally:
        if case == "recording":
            tm.lib().tmac_hip_chain_abort()
    torch.cuda.synchronize()
    assert word in str(ei.value), ei.value
    assert all(torch.isnan(o).all() for o in outs), "a refused call wrote an output"
