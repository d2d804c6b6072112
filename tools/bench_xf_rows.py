"""The element-wise operators of a decoder layer for N > 1 rows (llama-2-7B shapes, N = 4, 32, 256, hipGraph replay over rotating distinct
weight sets): us per call of
  (a) the plain fused call on a pre-transformed fp32 block (no operator; the block (b) builds, so (b) - (a) is the operator alone);
  (b) the same operators in torch into a buffer, followed by the plain call;
  (c) tmac_hip_qgemm_fused_xf_rows_dev: the operator inside the LUT build.
q/k/v and gate/up sit behind residual add + RMSNorm (residual_out written), down behind silu(gate) * up.  A library without the entry
point ($TMAC_HIP_LIB naming an older build) prints "-" for (c).  usage: bench_xf_rows.py [bits]"""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tmac_amd
from tmac_amd import KCfg, F16
L = tmac_amd.lib()
dev = torch.device("cuda")
BITS = int(sys.argv[1]) if len(sys.argv) > 1 else 2
BM = {1: 64, 2: 128, 3: 192, 4: 256}[BITS]
HAVE_XF = hasattr(L, "tmac_hip_qgemm_fused_xf_rows_dev") and L.tmac_hip_qgemm_fused_xf_rows_dev.argtypes is not None
NSETS, EPS = 8, 1e-5
wr = tmac_amd.TMACGeMMWrapper(act_group_size=64)


def timeit(fns, rounds=3):
    """fns: one closure per weight set; a graph of `rounds` passes over all of them"""
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


print(f"bits = {BITS}  us per call, {NSETS} weight sets in rotation: (a) plain | (b) torch operator + plain | (c) fused_xf_rows | (c) / (b)")
for name, Mw, K, nshare, kind in [("qkv", 4096, 4096, 3, "norm"), ("gate_up", 11008, 4096, 2, "norm"), ("down", 4096, 11008, 1, "glu")]:
    sets = []
    for _ in range(NSETS):
        ws = []
        for _ in range(nshare):
            A = torch.randint(0, 256, (Mw * BITS // BM, K // 4, BM // 2), dtype=torch.uint8, device=dev)
            S = (torch.randn((Mw * BITS // BM, K // 128, BM // BITS // 8, 2, 8), device=dev) * 0.01).half().contiguous()
            ws.append(tmac_amd.Weights(A, S, Mw, K, BITS, KCfg.make(Mw, K, BITS, BM), scales_dtype=F16, dev_dtype=F16, on_device=True))
        sets.append(ws)
    for N in (4, 32, 256):
        outs = [torch.empty((N, Mw), dtype=torch.float16, device=dev) for _ in range(nshare)]
        x, x2 = torch.randn((N, K), device=dev).half(), torch.randn((N, K), device=dev).half()
        res, gam = torch.randn((N, K), device=dev), 1.0 + 0.1 * torch.randn(K, device=dev)
        rout, xb = torch.empty((N, K), device=dev), torch.empty((N, K), device=dev)

        def torch_op():
            if kind == "norm":
                torch.add(x.float(), res, out=rout)
                torch.mul(rout * torch.rsqrt(rout.pow(2).mean(dim=1, keepdim=True) + EPS), gam, out=xb)
            else:
                torch.mul(torch.nn.functional.silu(x.float()), x2.float(), out=xb)

        def plain(ws):
            return lambda st: wr.fused(ws, xb, outs, N, stream=st)

        def torch_then_plain(ws):
            def f(st):
                torch_op()
                wr.fused(ws, xb, outs, N, stream=st)
            return f

        def xf(ws):
            if kind == "norm":
                return lambda st: wr.fused_xf_rows(ws, x, outs, "norm", N, residual=res, gamma=gam, eps=EPS, residual_out=rout, stream=st)
            return lambda st: wr.fused_xf_rows(ws, x, outs, "glu", N, in2=x2, stream=st)

        ta = timeit([plain(ws) for ws in sets])
        tb = timeit([torch_then_plain(ws) for ws in sets])
        tc = timeit([xf(ws) for ws in sets]) if HAVE_XF else None
        print(f"{name:8s} {kind:4s} N={N:3d}  (a) {ta:8.2f}   (b) {tb:8.2f}   (c) " + (f"{tc:8.2f}   (c)/(b) {tc / tb:.3f}" if tc is not None else "     -"), flush=True)
    for ws in sets:
        for w in ws:
            w.free()
