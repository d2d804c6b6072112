"""k_experts_router behind TMACGeMMWrapper.experts_router: logits, softmax and top-S in one launch, against float64 numpy (logits, a stable
argsort on (-logit, id), softmax).  Measured on an MI355X (profiles/r32_experts_router.txt): see the docstrings of the first two tests."""
import numpy as np
import pytest

from test_gpu_experts import bank_of, dev, nan_out
from test_gpu_parity import tm  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu
F16, F32 = np.float16, np.float32


def reference(x, w, S, renorm):      # (logits, ids, gates) in float64; among equal logits the lower id (a stable sort; -0 == +0)
    lg = x.astype(np.float64) @ w.astype(np.float64).T
    ids = np.argsort(-lg, axis=1, kind="stable")[:, :S]
    p = np.exp(lg - lg.max(1, keepdims=True))
    g = np.take_along_axis(p / p.sum(1, keepdims=True), ids, 1)
    return lg, ids.astype(np.int32), g / g.sum(1, keepdims=True) if renorm else g


def route(tm, x, w, S, renorm=False):      # one call on marked outputs -> (logits, ids, gates) as numpy
    import torch
    N, E = x.shape[0], w.shape[0]
    ids, gates, lg = torch.full((N, S), -7, dtype=torch.int32, device="cuda"), nan_out((N, S)), nan_out((N, E))
    tm.TMACGeMMWrapper(act_group_size=64).experts_router(dev(x), dev(w), S, renorm=renorm, out=(ids, gates), logits=lg)
    torch.cuda.synchronize()
    return lg.cpu().numpy(), ids.cpu().numpy(), gates.cpu().numpy()


ES = [(8, 2), (60, 4), (64, 8), (128, 8), (256, 8), (8, 8)]        # under a column tile, a ragged tile, one to four logits per lane, S = E
DT = [(F16, F16), (F32, F16), (F16, F32)]                          # (x, Wr)
GRID = [(E, S, K, (1, 33)[(i + rep) % 2], (i + i // 3 + rep) % 3, (i // 3 + rep) % 2)
        for rep in (0, 1) for i, ((E, S), K) in enumerate((es, k) for es in ES for k in (64, 192, 2048))]      # K: one step, ragged slices, many


@pytest.mark.parametrize("E,S,K,N,dt,renorm", GRID)
def test_exact_grid(tm, E, S, K, N, dt, renorm):
    """integers in [-4, 4] times integers / 64: every sum is exact in fp32 in any order, and ties are common.  Measured: the largest
    |gate - ref| over the largest reference gate of its token was 1.7e-7 over these cases."""
    rng = np.random.default_rng(E * K + N)
    x = rng.integers(-4, 5, (N, K)).astype(DT[dt][0])
    w = (rng.integers(-4, 5, (E, K)) / 64).astype(DT[dt][1])
    rl, ri, rg = reference(x, w, S, renorm)
    lg, ids, gates = route(tm, x, w, S, renorm)
    err = (np.abs(gates - rg) / rg.max(1, keepdims=True)).max()
    print(f"exact_grid E={E} S={S} K={K} N={N} dt={dt} renorm={renorm}: gate err / max gate {err:.3e}")
    assert np.array_equal(lg, rl.astype(F32)) and np.array_equal(ids, ri) and err <= 2e-5


# one seed per token row (each row N(0, 1)), chosen on the CPU so that every token's selected logits and its (S + 1)-th lie further apart than
# twice the summation bound, in fp16 and in fp32 data
ROW_SEEDS = {(60, 4, 2048): sorted(set(range(93)) - {0, 2, 4, 8, 9, 10, 16, 31, 35, 40, 41, 48, 50, 59, 60, 64, 71, 72, 75, 77, 81, 86, 88}),      # N = 70
             (128, 8, 4096): [44, 50, 75, 83, 85]}                                                                                       # N = 5


@pytest.mark.parametrize("shape", list(ROW_SEEDS))
@pytest.mark.parametrize("dtype", [F16, F32])
def test_random_data(tm, shape, dtype):
    """N(0, 1) x, N(0, 1) / sqrt(K) Wr.  |logit - ref| <= 2 gamma_K sum_k |x_k w_k|, gamma_K = K u / (1 - K u), u = 2^-24: the any-order fp32
    summation bound with a factor 2 for what the matrix core does inside a block.  Measured: the largest |logit - ref| / bound was 2.0e-4."""
    E, S, K = shape
    x = np.stack([np.random.default_rng(s).standard_normal(K) for s in ROW_SEEDS[shape]]).astype(dtype)
    w = (np.random.default_rng(E).standard_normal((E, K)) / np.sqrt(K)).astype(dtype)
    rl, ri, _ = reference(x, w, S, False)
    bound = 2 * (K * 2.0 ** -24 / (1 - K * 2.0 ** -24)) * (np.abs(x.astype(np.float64)) @ np.abs(w.astype(np.float64)).T)
    top = -np.sort(-rl, axis=1)[:, :S + 1]
    assert ((top[:, :-1] - top[:, 1:]).min(1) > 2 * bound.max(1)).all(), "the reference's own gaps: pick other seeds"
    lg, ids, _ = route(tm, x, w, S)
    print(f"random_data {shape} {dtype.__name__}: max |logit - ref| / bound {(np.abs(lg - rl) / bound).max():.3e}")
    assert (np.abs(lg - rl) <= bound).all() and np.array_equal(ids, ri)


@pytest.mark.parametrize("E,S,K,dt", [(60, 4, 2048, 0), (256, 8, 192, 1)])
def test_a_token_is_a_token(tm, E, S, K, dt):      # a token's logits, ids and gates are the same bits alone and at any place of a batch
    rng = np.random.default_rng(K)
    x = rng.standard_normal((70, K)).astype(DT[dt][0])
    w = (rng.standard_normal((E, K)) / np.sqrt(K)).astype(DT[dt][1])
    batch = route(tm, x, w, S, True)
    for n in (0, 31, 32, 69):
        for one, full in zip(route(tm, x[n:n + 1], w, S, True), batch):
            assert np.array_equal(one[0].view(np.int32), full[n].view(np.int32))


def test_any_bits_in_valid_ids_out(tm):
    E, S, K, rng = 60, 4, 192, np.random.default_rng(4)
    x = np.zeros((4, K), F16)
    x[0], x[1], x[2] = np.nan, np.inf, np.where(rng.random(K) < 0.5, np.inf, -np.inf)      # row 3: zeros, an E-way tie
    _, ids, _ = route(tm, x, (rng.standard_normal((E, K)) / 8).astype(F16), S)
    assert ((ids >= 0) & (ids < E)).all() and all(len(set(r)) == S for r in ids.tolist()) and ids[3].tolist() == list(range(S))


def test_capture_on_a_cold_stream(tm):      # no call of the library has seen `side` before the capture; replays follow x rewritten on the device
    import torch
    E, S, K, N, rng = 60, 4, 192, 33, np.random.default_rng(5)
    w = (rng.standard_normal((E, K)) / np.sqrt(K)).astype(F16)
    wr, wd, x = tm.TMACGeMMWrapper(act_group_size=64), dev(w), dev(rng.standard_normal((N, K)).astype(F16))
    out = (torch.full((N, S), -7, dtype=torch.int32, device="cuda"), nan_out((N, S)))
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        wr.experts_router(x, wd, S, renorm=True, out=out, stream=side)
    for _ in range(2):
        new = rng.standard_normal((N, K)).astype(F16)
        x.copy_(dev(new))
        out[0].fill_(-7); out[1].fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        _, ids, gates = route(tm, new, w, S, True)
        assert np.array_equal(out[0].cpu().numpy(), ids) and np.array_equal(out[1].cpu().numpy(), gates) and np.array_equal(ids, reference(new, w, S, True)[1])


def test_hand_over(tm):      # the router's ids and gates go into experts_route / experts_rows / experts_combine as they are
    import torch
    wr, bank, X, _ = bank_of(tm, "half_step")
    x, S, w = dev(X[:3]), 2, (np.random.default_rng(6).standard_normal((bank.E, bank.K)) / 32).astype(F32)
    ids, gates = wr.experts_router(x, dev(w), S, renorm=True)

    def layer(ids):
        r = wr.experts_route(ids, bank.E)
        return wr.experts_combine(wr.experts_rows(bank, x, r, S)[0], r, gates)
    got, want = layer(ids), layer(dev(reference(X[:3], w, S, True)[1]))
    torch.cuda.synchronize()
    assert torch.isfinite(got).all() and torch.equal(got, want)


@pytest.mark.parametrize("case", ["E=257", "S=9", "S>E", "K=96", "N*S", "flag", "misaligned_x", "null_ids", "recording"])
def test_refusals(tm, case):
    import torch
    L, x, w = tm.lib(), torch.zeros(4097 * 128 + 8, dtype=torch.float16, device="cuda"), torch.zeros(257 * 128, dtype=torch.float16, device="cuda")
    ids, gates = torch.full((4097 * 8,), -7, dtype=torch.int32, device="cuda"), nan_out((4097 * 8,))
    a = dict(N=3, K=128, E=8, S=2, flags=0, x=x.data_ptr(), ids=ids.data_ptr())
    word = {"E=257": (dict(E=257), "E: the router takes at most 256 experts"), "S=9": (dict(S=9, E=16), "S: 1 to 8 experts"),
            "S>E": (dict(S=4, E=3), "E: at least S experts"), "K=96": (dict(K=96), "K: a multiple of 64"),
            "N*S": (dict(N=4097, S=8), "N x S: the router takes at most 32768 slots"), "flag": (dict(flags=2), "flags=0x2: unknown bits"),
            "misaligned_x": (dict(x=x.data_ptr() + 2), "x_dev must be 16-byte aligned"), "null_ids": (dict(ids=None), "null Wr_dev, x_dev, ids_dev"),
            "recording": ({}, "tmac_hip_experts_router_dev cannot be recorded")}[case]
    a.update(word[0])
    if case == "recording":
        tm.binding.check(L.tmac_hip_chain_begin())
    try:
        rc = L.tmac_hip_experts_router_dev(w.data_ptr(), tm.F16, a["x"], tm.F16, a["N"], a["K"], a["E"], a["S"], a["flags"], a["ids"], gates.data_ptr(), None, None)
    finally:
        if case == "recording":
            L.tmac_hip_chain_abort()
    torch.cuda.synchronize()
    assert rc == -4 and word[1] in L.tmac_hip_last_error().decode(), L.tmac_hip_last_error()
    assert (ids == -7).all() and torch.isnan(gates).all(), "a refused call wrote an output"
