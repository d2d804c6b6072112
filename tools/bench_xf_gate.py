"""The gate of TMAC_XF_GLU / TMAC_XF_GLU_NORM, measured (random weights on the device, hipGraph replay over 8 distinct weight sets in rotation,
best of 5 replays, us per call):
  gate   BitNet b1.58 2B-4T `down` (2560 x 6912, W2, unified scale) at N = 1 and N = 4:
           (a) the plain call on a ready vector;
           (b) relu(gate)^2 * up and the RMSNorm as torch kernels into a buffer, then the plain call;
           (c) one "glu_norm:relu2" call (tmac_hip_qgemm_fused_xf_dev / _xf_rows_dev).
         Needs a library with the gate.
  silu   the SiLU figures that must not move, for A/B runs of two builds ($TMAC_HIP_LIB names the other one; the Python layer is this
         tree's in both): llama-2-7B W2 `down` (4096 x 11008) plain and "glu" (tools/bench_xf.py's row), BitNet-3B `down` (3200 x 8640) plain
         and "glu_norm" (tools/bench_xf_glunorm.py's row), N = 1.
usage: bench_xf_gate.py gate | silu"""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tmac_amd
from tmac_amd import KCfg, F16, F32
dev = torch.device("cuda")
BITS, BM, EPS, NSETS = 2, 128, 1e-5, 8
wr = tmac_amd.TMACGeMMWrapper(act_group_size=64)


def unified(Mw, K):
    A = torch.randint(0, 256, (Mw * BITS // BM, K // 4, BM // 2), dtype=torch.uint8, device=dev)
    S = torch.full((1,), 0.01, device=dev, dtype=torch.float32)
    return tmac_amd.Weights(A, S, Mw, K, BITS, KCfg.make(Mw, K, BITS, BM, 16, 128, K, False, 1), scales_dtype=F32, dev_dtype=F32, on_device=True)


def per_group(Mw, K):
    A = torch.randint(0, 256, (Mw * BITS // BM, K // 4, BM // 2), dtype=torch.uint8, device=dev)
    S = (torch.randn((Mw * BITS // BM, K // 128, BM // BITS // 8, 2, 8), device=dev) * 0.01).half().contiguous()
    return tmac_amd.Weights(A, S, Mw, K, BITS, KCfg.make(Mw, K, BITS, BM), scales_dtype=F16, dev_dtype=F16, on_device=True)


def timeit(fns, rounds=3):
    """fns: closures taking a stream; a graph of `rounds` passes over all of them"""
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


def gate():
    Mw, K = 2560, 6912
    sets = [unified(Mw, K) for _ in range(NSETS)]
    for N in (1, 4):
        out = torch.empty((N, Mw), dtype=torch.float16, device=dev)
        x, x2 = torch.randn((N, K), device=dev).half(), torch.randn((N, K), device=dev).half()
        gam, xb = 1.0 + 0.1 * torch.randn(K, device=dev), torch.empty((N, K), device=dev)

        def torch_then_plain(w):
            def f(st):
                g = torch.relu(x.float()).square() * x2.float()
                torch.mul(g * torch.rsqrt(g.pow(2).mean(dim=1, keepdim=True) + EPS), gam, out=xb)
                wr.fused([w], xb, [out], N, stream=st)
            return f

        def one_call(w):
            if N == 1:
                return lambda st: wr.fused_xf([w], x, [out], "glu_norm:relu2", in2=x2, gamma=gam, eps=EPS, stream=st)
            return lambda st: wr.fused_xf_rows([w], x, [out], "glu_norm:relu2", N, in2=x2, gamma=gam, eps=EPS, stream=st)
        ta = timeit([(lambda st, w=w: wr.fused([w], x, [out], N, stream=st)) for w in sets])
        tb = timeit([torch_then_plain(w) for w in sets])
        tc = timeit([one_call(w) for w in sets])
        print(f"BitNet-2B-4T down {Mw} x {K}, N = {N}, us per call: (a) plain {ta:6.2f}   (b) torch relu^2 * up + RMSNorm + plain {tb:6.2f}   "
              f"(c) glu_norm:relu2 call {tc:6.2f}   (c)/(b) {tc / tb:.3f}   (c)-(a) {tc - ta:5.2f}", flush=True)
    for w in sets:
        w.free()


def silu():
    for name, make, Mw, K, kind in (("llama-2-7B down", per_group, 4096, 11008, "glu"), ("BitNet-3B down", unified, 3200, 8640, "glu_norm")):
        sets = [make(Mw, K) for _ in range(NSETS)]
        out = torch.empty(Mw, dtype=torch.float16, device=dev)
        x, x2 = torch.randn(K, device=dev).half(), torch.randn(K, device=dev).half()
        gam = 1.0 + 0.1 * torch.randn(K, device=dev)
        ops = dict(in2=x2, gamma=gam, eps=EPS) if kind == "glu_norm" else dict(in2=x2)
        ta = timeit([(lambda st, w=w: wr.fused([w], x, [out], 1, stream=st)) for w in sets])
        tc = timeit([(lambda st, w=w: wr.fused_xf([w], x, [out], kind, stream=st, **ops)) for w in sets])
        print(f"{name} {Mw} x {K}, N = 1, us per call: (a) plain {ta:6.2f}   (c) {kind} call {tc:6.2f}", flush=True)
        for w in sets:
            w.free()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "gate"
    {"gate": gate, "silu": silu}[mode]()
