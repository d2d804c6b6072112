"""The router of a mixture-of-experts layer: the fused call against what a caller writes today.
  (a) experts_router (k_experts_router: logits, softmax, top-k, renormalise, int32 ids in one launch), graph replay
  (b) torch: linear, softmax, topk, renormalise, cast to int32; eager, wall clock
  (c) the same torch sequence, graph replay
fp16 x and Wr, renormalised gates.  Rounds alternate the columns; a column's figure is its best round with the spread over the rounds
behind it, us per call.  Before the timing every shape's ids are compared with torch's (counted, not asserted: torch leaves ties open) and
the gates held to 2e-5.  usage: bench_experts_router.py [rounds]"""
import os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tmac_amd

dev = torch.device("cuda")
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
REPS = 20
wr = tmac_amd.TMACGeMMWrapper(act_group_size=64)


def graph_us(fn):
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        fn(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for _ in range(REPS):
            fn(side)
    g.replay(); torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        g.replay()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (10 * REPS)


def eager_us(fn):
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10 * REPS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / (10 * REPS)


print("us per call, best of", ROUNDS, "alternating rounds (spread): (a) experts_router, graph | (b) torch, eager | (c) torch, graph; a/c")
for name, E, K, S in [("mixtral", 8, 4096, 2), ("qwen-moe", 60, 2048, 4), ("qwen3-moe", 128, 2048, 8)]:
    Wr = (torch.randn(E, K, device=dev) / K ** 0.5).half()
    for N in (1, 16, 256):
        x = torch.randn(N, K, device=dev).half()
        ids, gates = torch.empty(N, S, dtype=torch.int32, device=dev), torch.empty(N, S, device=dev)
        t_ids, t_gates = torch.empty(N, S, dtype=torch.int32, device=dev), torch.empty(N, S, device=dev)

        def fused(st):
            wr.experts_router(x, Wr, S, renorm=True, out=(ids, gates), stream=st)

        def today(st=None):
            p = torch.softmax(torch.nn.functional.linear(x, Wr).float(), dim=-1)
            g, i = torch.topk(p, S, dim=-1)
            torch.div(g, g.sum(-1, keepdim=True), out=t_gates)
            t_ids.copy_(i)

        fused(None); today(); torch.cuda.synchronize()
        same = int((ids == t_ids).all(1).sum())
        gerr = float((gates - t_gates)[(ids == t_ids)].abs().max())
        runs = [[], [], []]
        for _ in range(ROUNDS):
            for col, v in zip(runs, (graph_us(fused), eager_us(today), graph_us(today))):
                col.append(v)
        a, b, c = (min(r) for r in runs)
        sp = " ".join(f"{(max(r) - min(r)) / min(r):.0%}" for r in runs)
        print(f"{name:10s} E={E:3d} K={K} S={S} N={N:3d}: (a) {a:7.2f} | (b) {b:7.2f} | (c) {c:7.2f}   a/c {a / c:.2f}{'  MISSED' if a > c else ''}   spread {sp}"
              f"   tokens with torch's ids {same}/{N}, max |gate - torch| {gerr:.1e}", flush=True)
