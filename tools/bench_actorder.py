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
usage: bench_actorder.py [--out FILE] [--bits 2,4] [--shapes o,qkv,gate_up,down]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--bits", default="2,4")
    ap.add_argument("--shapes", default="o,qkv,gate_up,down")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_actorder.py measures on a GPU"
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
