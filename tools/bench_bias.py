"""Biased handles (y = W x + b inside the store) against the plain call and against what a caller could do before them: llama-2-7B shapes,
W2 and W4, fp16 activations and outputs, N = 1, 4 and 64 activation rows, hipGraph replay over 8 rotating distinct weight sets
(tools/bench_actorder.py's method).  us per call of
  (a) the plain handle under ANOTHER build of the library (--parent-lib: the parent commit's libtmac_hip.so), timed first and again last:
      the difference between the two is the session's spread, the margin of the comparison below;
  (b) the biased handle under the tree's library: k_gemv_quad's / k_gemm_planes' bias instantiations;
  (c) the plain call under the tree's library followed by a torch in-place add of the bias on the output, inside the graph: what a caller
      can do without the feature.
One GPU session: the driver starts one child process per column group (a | b, c | a), one after the other; a child loads one library.
Expectation: (b) <= (c) everywhere, and (b) <= mean (a) + spread.  A cell that misses is marked MISS, not routed around.
--lib FILE: another build of the tree's library for (b) and (c) (an A/B of two kernel variants in one method).
usage: bench_bias.py --parent-lib FILE [--lib FILE] [--out FILE] [--bits 2,4] [--shapes o,qkv,gate_up,down] [--ns 1,4,64] [--note TEXT]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"o": (4096, 4096, 1), "qkv": (4096, 4096, 3), "gate_up": (11008, 4096, 2), "down": (4096, 11008, 1)}     # (Mw, K, matrices per call)
GS, AGS, NSETS = 128, 64, 8


def child(args):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import tmac_amd
    from tmac_amd import F16, KCfg, convert
    dev = torch.device("cuda")
    assert torch.cuda.is_available(), "bench_bias.py measures on a GPU"
    biased = args.phase == "bc"

    def synthetic(seed, Mw, K, bits):
        rng = np.random.default_rng(seed)
        qw = rng.integers(-2 ** 31, 2 ** 31, size=(K * bits // 32, Mw), dtype=np.int64).astype(np.int32)
        qz = rng.integers(-2 ** 31, 2 ** 31, size=(K // GS, Mw * bits // 32), dtype=np.int64).astype(np.int32)
        sc = (np.abs(rng.standard_normal((K // GS, Mw))) * 0.02 + 0.005).astype(np.float16)
        return tuple(torch.from_numpy(a).to(dev) for a in (qw, sc, qz))

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

    wr = tmac_amd.TMACGeMMWrapper(act_group_size=AGS)
    res = {"device": torch.cuda.get_device_name(0), "lib": tmac_amd.lib_path(), "cells": {}}
    for name in args.shapes.split(","):
        Mw, K, nshare = SHAPES[name]
        for bits in (int(b) for b in args.bits.split(",")):
            cfg = KCfg.make(Mw, K, bits, convert.default_bm(bits, Mw), 16, GS, AGS, True)
            gen = torch.Generator(device=dev); gen.manual_seed(K + bits)
            bias = [(torch.randn(Mw, device=dev, generator=gen)).half() for _ in range(nshare)]
            plain_sets, bias_sets = [], []
            for s in range(NSETS):
                ts = [synthetic(1000 * s + 10 * i + bits, Mw, K, bits) for i in range(nshare)]
                plain_sets.append([tmac_amd.Weights.from_gptq(*t, cfg, True, F16) for t in ts])
                if biased:
                    bias_sets.append([tmac_amd.Weights.from_gptq(*t, cfg, True, F16, bias=b) for t, b in zip(ts, bias)])
                del ts
            for N in (int(n) for n in args.ns.split(",")):
                outs = [torch.empty((N, Mw), dtype=torch.float16, device=dev) for _ in range(nshare)]
                x = torch.randn((N, K), device=dev).half()

                def call(ws):
                    return lambda st: wr.fused(ws, x, outs, N, stream=st)

                def plain_then_add(ws):
                    def f(st):
                        wr.fused(ws, x, outs, N, stream=st)
                        for o, b in zip(outs, bias):
                            o.add_(b)
                    return f

                cell = {}
                if biased:
                    cell["b"] = timeit([call(ws) for ws in bias_sets])
                    cell["c"] = timeit([plain_then_add(ws) for ws in plain_sets])
                else:
                    cell["a"] = timeit([call(ws) for ws in plain_sets])
                res["cells"][f"{name} {bits} {N}"] = cell
                print(f"# {args.phase} {name} W{bits} N={N}: " + "  ".join(f"({k}) {v:.2f}" for k, v in cell.items()), file=sys.stderr, flush=True)
            for ws in plain_sets + bias_sets:
                for w in ws:
                    w.free()
    print("RESULT " + json.dumps(res), flush=True)
    return 0


def run_child(args, phase, lib):
    env = dict(os.environ)
    if lib:
        env["TMAC_HIP_LIB"] = os.path.abspath(lib)
    else:
        env.pop("TMAC_HIP_LIB", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--phase", phase, "--bits", args.bits, "--shapes", args.shapes, "--ns", args.ns], env=env, check=True,
                         stdout=subprocess.PIPE, text=True, timeout=args.timeout).stdout
    line = [x for x in out.splitlines() if x.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phase", default="", help="(internal) a | bc: the measuring child process")
    ap.add_argument("--parent-lib", default="", help="libtmac_hip.so of the parent commit (column a)")
    ap.add_argument("--out", default="")
    ap.add_argument("--bits", default="2,4")
    ap.add_argument("--shapes", default="o,qkv,gate_up,down")
    ap.add_argument("--ns", default="1,4,64", help="activation rows")
    ap.add_argument("--lib", default="", help="another build of the tree's library for columns (b) and (c)")
    ap.add_argument("--note", default="", help="a line for the file's head (which variant this build is)")
    ap.add_argument("--timeout", type=int, default=400, help="seconds per child process")
    args = ap.parse_args()
    if args.phase:
        return child(args)
    assert args.parent_lib and os.path.exists(args.parent_lib), "--parent-lib: the parent commit's libtmac_hip.so"
    a1 = run_child(args, "a", args.parent_lib)
    bc = run_child(args, "bc", args.lib)
    a2 = run_child(args, "a", args.parent_lib)
    lines = ["# tools/bench_bias.py: us per call in a replayed hipGraph, best of 5 replays of 3 passes over 8 rotating weight sets; fp16 activations and outputs",
             f"# device: {bc['device']}; group size {GS}; one GPU session, three processes in this order: (a) first | (b), (c) | (a) last",
             "# (a) plain handle, the parent's library (first / last run; spread = their difference) | (b) biased handle | (c) plain call + torch in-place add of the bias",
             "# expectation: (b) <= (c), and (b) <= mean (a) + spread; a cell that misses is marked"]
    if args.note:
        lines.append("# " + args.note)
    lines.append("shape     bits   N  | (a) first  (a) last   spread |   (b) us    (c) us  | (b)/(a)  (b)/(c) | verdict")
    misses = 0
    for key, cell in bc["cells"].items():
        name, bits, N = key.split()
        f, l = a1["cells"][key]["a"], a2["cells"][key]["a"]
        spread, mean = abs(f - l), 0.5 * (f + l)
        b, c = cell["b"], cell["c"]
        bad = [w for w, miss in (("(b) > (c)", b > c), ("(b) > (a) + spread", b > mean + spread)) if miss]
        misses += bool(bad)
        line = f"{name:9s} {int(bits):4d} {int(N):3d}  | {f:9.2f}  {l:8.2f}  {spread:7.2f} | {b:8.2f}  {c:8.2f}  | {b / mean:7.3f}  {b / c:7.3f} | {'MISS: ' + ', '.join(bad) if bad else 'ok'}"
        print(line, flush=True)
        lines.append(line)
    lines.append(f"# cells that miss: {misses} of {len(bc['cells'])}")
    print(lines[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
