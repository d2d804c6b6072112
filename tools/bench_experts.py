"""Top-k expert GEMVs of one token (mixture-of-experts layers): tmac_hip_qgemm_experts_dev against what a caller does without it.
  (a) the experts call: ids read on the GPU, one launch per projection group (gate + up as two banks; down with the gated sum), graph replay
  (b) today's caller: ids copied to the host and waited for, then S plain fused calls per projection (+ torch multiply-adds for the
      gated sum); eager, wall clock per layer step -- the wait rules a graph out
  (c) the same S plain calls with the ids known in advance, no wait, graph replay: the bound a host-routed caller cannot beat
  (a') the experts call with its tables built in the launch (build="kernel": tmac_hip_qgemm_experts_fused_dev), graph replay
Rounds alternate the columns; a column's figure is its best round, us per call group, with the spread of its rounds behind it.
A last row per shape is the whole layer step for one token, graph replay: today's five launches (pair build, gate + up, a torch silu(g) * u,
pair build, down with the gated sum) against the two fused calls (gate + up from x; down from silu(G) * U with the gated sum).
usage: bench_experts.py [rounds]"""
import os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tmac_amd
from tmac_amd import KCfg, F16

dev = torch.device("cuda")
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
wr = tmac_amd.TMACGeMMWrapper(act_group_size=64)


def experts(E, Mw, K, bits):
    bm = {2: 128, 4: 256}[bits]
    ws = []
    for _ in range(E):
        A = torch.randint(0, 256, (Mw * bits // bm, K // 4, bm // 2), dtype=torch.uint8, device=dev)
        S = (torch.randn((Mw * bits // bm, K // 128, bm // bits // 8, 2, 8), device=dev) * 0.01).half().contiguous()
        ws.append(tmac_amd.Weights(A, S, Mw, K, bits, KCfg.make(Mw, K, bits, bm), scales_dtype=F16, dev_dtype=F16, on_device=True))
    return ws


def graph_us(fn, reps=20):
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        fn(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for _ in range(reps):
            fn(side)
    g.replay(); torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record(); g.replay(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def eager_us(fn, reps=50):
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps


def col(v):
    return f"{min(v):7.1f} ({min(v):.1f}-{max(v):.1f})"


print("us per call group, best of", ROUNDS, "alternating rounds (spread): (a) experts call | (a') tables built in the launch | (b) host-routed with the "
      "wait | (c) host-routed, ids known; a/c, a'/a, a'/c")
for name, E, S, H, F, bits in [("mixtral W2", 8, 2, 4096, 14336, 2), ("mixtral W4", 8, 2, 4096, 14336, 4), ("qwen-moe W4", 60, 4, 2048, 1408, 4)]:
    gate, up, down = experts(E, F, H, bits), experts(E, F, H, bits), experts(E, H, F, bits)
    bg, bu, bd = (tmac_amd.ExpertBank.from_handles(w) for w in (gate, up, down))
    ids = torch.randperm(E, device=dev)[:S].int().contiguous()
    gates = torch.rand(S, device=dev) + 0.1
    gates_h = gates.half()
    x, h = torch.randn(1, H, device=dev).half(), torch.randn(S, F, device=dev).half()
    og, ou = (torch.empty(S, F, dtype=torch.float16, device=dev) for _ in range(2))
    od = torch.empty(H, dtype=torch.float16, device=dev)
    ys = torch.empty(S, H, dtype=torch.float16, device=dev)
    known = ids.tolist()

    def gu_plain(idl, stream=None):
        for s, e in enumerate(idl):
            wr.fused([gate[e], up[e]], x, [og[s:s + 1], ou[s:s + 1]], 1, stream=stream)

    def down_plain(idl, stream=None):
        for s, e in enumerate(idl):
            wr.fused([down[e]], h[s:s + 1], [ys[s:s + 1]], 1, stream=stream)
        torch.mv(ys.t(), gates_h, out=od)            # the gated sum as a torch kernel

    cols = {"gate_up": [lambda st: wr.experts([bg, bu], x, ids, out=[og, ou], stream=st), lambda: gu_plain(ids.tolist()),
                        lambda st: gu_plain(known, st), lambda st: wr.experts([bg, bu], x, ids, out=[og, ou], stream=st, build="kernel")],
            "down": [lambda st: wr.experts(bd, h, ids, gates=gates, out=od, stream=st), lambda: down_plain(ids.tolist()),
                     lambda st: down_plain(known, st),      # (graph_us makes `st` the current stream: the torch kernel follows)
                     lambda st: wr.experts(bd, h, ids, gates=gates, out=od, stream=st, build="kernel")]}
    for proj, (fa, fb, fc, fk) in cols.items():
        r = [[], [], [], []]
        for _ in range(ROUNDS):
            for v, t in zip(r, (graph_us(fa), eager_us(fb), graph_us(fc), graph_us(fk))):
                v.append(t)
        a, b, c, k = (min(v) for v in r)
        print(f"{name:12s} {proj:8s} S={S} E={E}: (a) {col(r[0])} | (a') {col(r[3])} | (b) {col(r[1])} | (c) {col(r[2])}   a/c {a / c:.2f}  a'/a {k / a:.2f}  "
              f"a'/c {k / c:.2f}", flush=True)

    hb = torch.empty(S, F, dtype=torch.float16, device=dev)

    def layer5(st):
        wr.experts([bg, bu], x, ids, out=[og, ou], stream=st)
        torch.mul(torch.nn.functional.silu(og), ou, out=hb)
        wr.experts(bd, hb, ids, gates=gates, out=od, stream=st)

    def layer2(st):
        wr.experts([bg, bu], x, ids, out=[og, ou], stream=st, build="kernel")
        wr.experts(bd, og, ids, gates=gates, out=od, stream=st, glu="glu", in2=ou)
    r = [[], []]
    for _ in range(ROUNDS):
        r[0].append(graph_us(layer5)); r[1].append(graph_us(layer2))
    print(f"{name:12s} layer    S={S} E={E}: five launches {col(r[0])} | two fused launches {col(r[1])}   fused / five {min(r[1]) / min(r[0]):.2f}", flush=True)
    for b in (bg, bu, bd):
        b.free()
    for w in gate + up + down:
        w.free()
