"""Act-order (g_idx) handles against what a caller could do before them: llama-2-7B shapes, W2 and W4, N = 1, 4 and 64 activation rows,
hipGraph replay over rotating distinct weight sets.  us per call of
  (a) the plain handle on a pre-gathered vector: the floor (no permutation work at all);
  (b) the permuted handle: the gather inside the LUT build (k_gemv_quad's GA instantiations for N = 1, the gathered pair build / LUT image
      for N >= 2);
  (c) what a caller can do without it: a torch index_select into scratch, followed by the plain call.
Reported: (b) / (a) and (b) / (c) per shape.  The yardstick is (c) from the same run; DESIGN.md 4.11 holds the numbers and what they say.
Second part: registration through the permutation (tmac_hip_register_weights_gptq_perm_dev) against the plain registration, host-clock ms
around the call with the tensors already on the device, first run and the median of the following three (tools/bench_register.py's
method for its column (b), without the upload).  No bar: the word-wise gather reads 8 / bits times the plain pack's qweight bytes, once.
--stream: act-order handles in stream mode instead (a recording declared independent, record_chain(independent=True)): NL calls per launch
over NL distinct weight sets and activation vectors, ten launches per event pair, mean and best of ten pairs (DESIGN.md 4.4's method), us per
call and fraction of the 8 TB/s HBM peak on the algorithmic bytes of
  (a) plain handles in a stream on pre-gathered vectors: the floor;
  (b) permuted handles in a declared-independent stream: k_lut_images gathers;
  (c) one torch index_select per call into scratch, then the plain stream: what a caller could do before (replayed from a hipGraph);
  (d) the permuted handles called stand-alone (k_gemv_quad's gather instantiations), replayed from a hipGraph: their route before.
--launches N (with --stream): N timed event pairs per variant instead of ten (a profiler run: k_lut_images' own duration with and
without the gather is read from its kernel trace, the two instantiations have two names).
usage: bench_actorder.py [--out FILE] [--bits 2,4] [--shapes o,qkv,gate_up,down] [--stream [--nl 96] [--launches 10]]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tmac_amd  # noqa: E402
from tmac_amd import F16, KCfg, convert  # noqa: E402

SHAPES = {"o": (4096, 4096, 1), "qkv": (4096, 4096, 3), "gate_up": (11008, 4096, 2), "down": (4096, 11008, 1)}     # (Mw, K, matrices per call)
GS, AGS, NSETS = 128, 64, 8
dev = torch.device("cuda")


def synthetic(seed, Mw, K, bits):
    rng = np.random.default_rng(seed)
    qw = rng.integers(-2 ** 31, 2 ** 31, size=(K * bits // 32, Mw), dtype=np.int64).astype(np.int32)
    qz = rng.integers(-2 ** 31, 2 ** 31, size=(K // GS, Mw * bits // 32), dtype=np.int64).astype(np.int32)
    sc = (np.abs(rng.standard_normal((K // GS, Mw))) * 0.02 + 0.005).astype(np.float16)
    return tuple(torch.from_numpy(a).to(dev) for a in (qw, sc, qz))


def random_g_idx(seed, K):
    g = np.repeat(np.arange(K // GS, dtype=np.int32), GS)
    np.random.default_rng(seed).shuffle(g)
    return g


def timeit(fns, rounds=3):
    """fns: one closure per weight set; a graph of `rounds` passes over all of them; the best of five replays"""
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for fn in fns:
            fn(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for _ in range(rounds):
            for fn in fns:
                fn(side)
    g.replay(); torch.cuda.synchronize()
    best = 1e9
    for _ in range(5):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); g.replay(); e1.record(); torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / (rounds * len(fns)))
    return best


def register_ms(tensors, cfg, kperm):
    out = []
    for _ in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = tmac_amd.Weights.from_gptq(*tensors, cfg, True, F16, g_idx=kperm)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
        h.free()
    return out[0], float(np.median(out[1:]))


def algorithmic_bytes(Mw, K, bits, cnt):
    """SURVEY 8d's bytes of one fused call of cnt matrices (tools/bench_stream.py): weights, scales and zeros, the LUT once, the outputs"""
    return cnt * (Mw * K * bits // 8 + Mw * (K // GS) * 2 * 2 + Mw * 2) + K // 4 * 16 + (K // AGS) * 4


def device_gptq(gen, Mw, K, bits):
    qw = torch.randint(-2 ** 31, 2 ** 31 - 1, (K * bits // 32, Mw), dtype=torch.int32, device=dev, generator=gen)
    qz = torch.randint(-2 ** 31, 2 ** 31 - 1, (K // GS, Mw * bits // 32), dtype=torch.int32, device=dev, generator=gen)
    sc = (torch.randn((K // GS, Mw), device=dev, generator=gen).abs() * 0.02 + 0.005).half()
    return qw, sc, qz


def event_pairs(fn, pairs, per_pair=10):
    """fn() enqueues one launch of NL calls: us per launch, (mean, best) over `pairs` event pairs of per_pair launches, after three warm-up pairs"""
    ts = []
    for r in range(pairs + 3):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per_pair):
            fn()
        e1.record(); torch.cuda.synchronize()
        if r >= 3:
            ts.append(e0.elapsed_time(e1) * 1e3 / per_pair)
    return float(np.mean(ts)), float(np.min(ts))


def stream_part(args):
    wr = tmac_amd.TMACGeMMWrapper(act_group_size=AGS)
    NL = args.nl
    gen = torch.Generator(device=dev); gen.manual_seed(11)
    lines = [f"# tools/bench_actorder.py --stream: {NL} calls per launch over {NL} distinct weight sets and vectors, 10 launches per event pair, mean (best) of "
             f"{args.launches} pairs; fp16 activations and outputs",
             f"# device: {torch.cuda.get_device_name(0)}; group size {GS}; random g_idx with exactly {GS} members per group; frac = of the 8 TB/s HBM peak",
             "# (a) plain stream, pre-gathered x | (b) permuted handles, declared-independent stream | (c) torch index_select per call + plain stream (hipGraph) | "
             "(d) permuted handles stand-alone (hipGraph)",
             "shape     bits |  (a) us/call   frac |  (b) us/call   frac |  (c) us/call   frac |  (d) us/call   frac | (b)/(a)  (b)/(c)  (b)/(d)"]
    for name in args.shapes.split(","):
        Mw, K, nshare = SHAPES[name]
        for bits in (int(b) for b in args.bits.split(",")):
            cfg = KCfg.make(Mw, K, bits, convert.default_bm(bits, Mw), 16, GS, AGS, True)
            kperm = tmac_amd.KPerm(random_g_idx(K + bits, K), GS)
            perm = torch.from_numpy(kperm.perm().astype(np.int64)).to(dev)
            plain_sets, perm_sets = [], []
            for s in range(NL):
                ts = [device_gptq(gen, Mw, K, bits) for _ in range(nshare)]
                plain_sets.append([tmac_amd.Weights.from_gptq(*t, cfg, True, F16) for t in ts])
                perm_sets.append([tmac_amd.Weights.from_gptq(*t, cfg, True, F16, g_idx=kperm) for t in ts])
                del ts
            xs = [torch.randn(K, device=dev, generator=gen).half() for _ in range(NL)]
            xg = [x.index_select(0, perm).contiguous() for x in xs]
            scratch = [torch.empty(K, dtype=torch.float16, device=dev) for _ in range(NL)]
            outs = [[torch.empty(Mw, dtype=torch.float16, device=dev) for _ in range(nshare)] for _ in range(NL)]

            def chain_of(sets, vecs):
                with wr.record_chain(independent=True) as rec:
                    for ws, v, o in zip(sets, vecs, outs):
                        wr.fused(ws, v, o, 1, act_dtype=F16, out_dtype=F16)
                assert rec.chain.stream
                return rec.chain

            ca, cb, cc = chain_of(plain_sets, xg), chain_of(perm_sets, xs), chain_of(plain_sets, scratch)
            side = torch.cuda.Stream()

            def select_then_stream():
                for x, sc in zip(xs, scratch):
                    torch.index_select(x, 0, perm, out=sc)
                cc.launch(side)

            def stand_alone():
                for ws, x, o in zip(perm_sets, xs, outs):
                    wr.fused(ws, x, o, 1, act_dtype=F16, out_dtype=F16, stream=side)

            graphs = []
            for fn in (select_then_stream, stand_alone):
                with torch.cuda.stream(side):
                    fn()
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=side):
                    fn()
                graphs.append(g)
            res = [event_pairs(f, args.launches) for f in (ca.launch, cb.launch, graphs[0].replay, graphs[1].replay)]
            assert ca.status() == 0 and cb.status() == 0 and cc.status() == 0
            hb = algorithmic_bytes(Mw, K, bits, nshare)
            us = [m / NL for m, _ in res]
            cols = " | ".join(f"{m / NL:6.2f} ({b / NL:5.2f}) {hb / (m / NL) * 1e-3 / 8000:5.3f}" for m, b in res)
            line = f"{name:9s} {bits:4d} | {cols} | {us[1] / us[0]:7.3f}  {us[1] / us[2]:7.3f}  {us[1] / us[3]:7.3f}"
            print(line, flush=True)
            lines.append(line)
            del graphs
            for c in (ca, cb, cc):
                c.free()
            for ws in plain_sets + perm_sets:
                for w in ws:
                    w.free()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stream", action="store_true")
    ap.add_argument("--nl", type=int, default=96)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--bits", default="2,4")
    ap.add_argument("--shapes", default="o,qkv,gate_up,down")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_actorder.py measures on a GPU"
    if args.stream:
        return stream_part(args)
    wr = tmac_amd.TMACGeMMWrapper(act_group_size=AGS)
    lines = ["# tools/bench_actorder.py: us per call in a replayed hipGraph, best of 5 replays of 3 passes over 8 rotating weight sets; fp16 activations and outputs",
             f"# device: {torch.cuda.get_device_name(0)}; group size {GS}; random g_idx with exactly {GS} members per group",
             "# (a) plain handle, pre-gathered x | (b) permuted handle | (c) torch index_select + plain handle",
             "shape     bits   N  |   (a) us    (b) us    (c) us  | (b)/(a)  (b)/(c)"]
    reg = ["# registration, host-clock ms, tensors on the device: plain (tmac_hip_register_weights_gptq_dev) | through the permutation (.._perm_dev)",
           "shape     bits  Mw     K      |  plain first  median3  |  perm first  median3  | perm / plain (median)"]
    for name in args.shapes.split(","):
        Mw, K, nshare = SHAPES[name]
        for bits in (int(b) for b in args.bits.split(",")):
            cfg = KCfg.make(Mw, K, bits, convert.default_bm(bits, Mw), 16, GS, AGS, True)
            kperm = tmac_amd.KPerm(random_g_idx(K + bits, K), GS)
            perm = torch.from_numpy(kperm.perm().astype(np.int64)).to(dev)
            plain_sets, perm_sets = [], []
            for s in range(NSETS):
                ts = [synthetic(1000 * s + 10 * i + bits, Mw, K, bits) for i in range(nshare)]
                plain_sets.append([tmac_amd.Weights.from_gptq(*t, cfg, True, F16) for t in ts])
                perm_sets.append([tmac_amd.Weights.from_gptq(*t, cfg, True, F16, g_idx=kperm) for t in ts])
                if s == 0:
                    pf, pm = register_ms(ts[0], cfg, None)
                    gf, gm = register_ms(ts[0], cfg, kperm)
                    reg.append(f"{name:9s} {bits:4d}  {Mw:5d}  {K:5d}  |  {pf:10.2f}  {pm:8.2f}  |  {gf:9.2f}  {gm:8.2f}  | {gm / pm:6.2f}")
                del ts
            for N in (1, 4, 64):
                outs = [torch.empty((N, Mw), dtype=torch.float16, device=dev) for _ in range(nshare)]
                x = torch.randn((N, K), device=dev).half()
                xg, scratch = x.index_select(1, perm).contiguous(), torch.empty((N, K), dtype=torch.float16, device=dev)

                def plain(ws):
                    return lambda st: wr.fused(ws, xg, outs, N, stream=st)

                def permuted(ws):
                    return lambda st: wr.fused(ws, x, outs, N, stream=st)

                def torch_then_plain(ws):
                    def f(st):
                        torch.index_select(x, 1, perm, out=scratch)
                        wr.fused(ws, scratch, outs, N, stream=st)
                    return f

                ta = timeit([plain(ws) for ws in plain_sets])
                tb = timeit([permuted(ws) for ws in perm_sets])
                tc = timeit([torch_then_plain(ws) for ws in plain_sets])
                line = f"{name:9s} {bits:4d} {N:3d}  | {ta:8.2f}  {tb:8.2f}  {tc:8.2f}  | {tb / ta:7.3f}  {tb / tc:7.3f}"
                print(line, flush=True)
                lines.append(line)
            for ws in plain_sets + perm_sets:
                for w in ws:
                    w.free()
    lines += reg
    print("\n".join(reg))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
