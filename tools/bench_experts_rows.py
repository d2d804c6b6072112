"""A mixture-of-experts layer over a token batch: the grouped GEMM over routed positions against what a caller does without it.
  (a) experts_route + experts_rows([gate, up]) + experts_rows(down) on position-major rows + experts_combine: ids read on the GPU, graph replay
  (b) today's caller: ids copied to the host and waited for, per live expert one plain fused call for gate + up and one for down on
      index_selected rows, the gated sum in torch (index_add_); eager, wall clock -- the wait rules a graph out
  (c) the same plain calls with the ids known in advance, no wait, graph replay: the bound a host-routed caller cannot beat
The GLU between up and down is left out of all three (down reads a fixed buffer).  Rounds alternate the columns; a column's figure is its
best round with the spread over the rounds behind it, us per layer.  usage: bench_experts_rows.py [rounds]"""
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


def graph_us(fn, reps=5):
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


def eager_us(fn, reps=5):
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps


print("us per layer, best of", ROUNDS, "alternating rounds (spread): (a) grouped GEMM | (b) host-routed with the wait | (c) host-routed, ids known; a/c")
for name, E, S, H, F, bits in [("mixtral W2", 8, 2, 4096, 14336, 2), ("mixtral W4", 8, 2, 4096, 14336, 4), ("qwen-moe W4", 60, 4, 2048, 1408, 4)]:
    gate, up, down = experts(E, F, H, bits), experts(E, F, H, bits), experts(E, H, F, bits)
    bg, bu, bd = (tmac_amd.ExpertBank.from_handles(w) for w in (gate, up, down))
    for N in (16, 64, 256):
        gen = torch.Generator(device="cpu").manual_seed(N)
        ids = torch.stack([torch.randperm(E, generator=gen)[:S] for _ in range(N)]).int().to(dev).contiguous()      # uniform, distinct per token
        gates = (torch.rand(N, S, device=dev) + 0.1).contiguous()
        x = torch.randn(N, H, device=dev).half()
        route = wr.experts_route(ids, E)
        P = int(route[1].numel())
        og, ou = (torch.empty(P, F, dtype=torch.float16, device=dev) for _ in range(2))
        hp = torch.randn(P, F, device=dev).half()                # down's position-major input (the GLU's output)
        cd, y = torch.empty(P, H, device=dev), torch.empty(N, H, dtype=torch.float16, device=dev)
        hs, yd, yacc = torch.randn(N * S, F, device=dev).half(), torch.empty(N * S, H, device=dev), torch.zeros(N, H, device=dev)

        def layer(st):
            wr.experts_route(ids, E, out=route, stream=st)
            wr.experts_rows([bg, bu], x, route, S, out=[og, ou], stream=st)
            wr.experts_rows(bd, hp, route, S, out=[cd], stream=st)
            wr.experts_combine(cd, route, gates, out=y, stream=st)

        def groups(idl):                                         # per live expert: its tokens, their gates, its rows in the flat buffers
            out, o = [], 0
            for e in range(E):
                tok, slot = (idl == e).nonzero(as_tuple=True)
                if tok.numel():
                    out.append((e, tok, gates[tok, slot].unsqueeze(1).contiguous(), o, int(tok.numel())))
                    o += int(tok.numel())
            return out

        def plain(gr, st=None):
            yacc.zero_()
            for e, tok, gw, o, n in gr:
                wr.fused([gate[e], up[e]], x.index_select(0, tok), [og[o:o + n], ou[o:o + n]], n, stream=st)
                wr.fused([down[e]], hs[o:o + n], [yd[o:o + n]], n, stream=st)
                yacc.index_add_(0, tok, yd[o:o + n] * gw)

        known = groups(ids)
        fa, fb, fc = layer, lambda: plain(groups(ids.cpu().to(dev))), lambda st: plain(known, st)
        runs = [[], [], []]
        for _ in range(ROUNDS):
            for col, v in zip(runs, (graph_us(fa), eager_us(fb), graph_us(fc))):
                col.append(v)
        a, b, c = (min(r) for r in runs)
        sp = " ".join(f"{(max(r) - min(r)) / min(r):.0%}" for r in runs)
        print(f"{name:12s} N={N:3d} S={S} E={E} P={P:4d}: (a) {a:8.1f} | (b) {b:8.1f} | (c) {c:8.1f}   a/c {a / c:.2f}   a/b {a / b:.2f}   spread {sp}", flush=True)
    for bk in (bg, bu, bd):
        bk.free()
    for w in gate + up + down:
        w.free()
