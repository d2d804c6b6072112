"""What TMAC_XF_GLU_NORM buys on BitNet shapes (unified scales, one act group per row; random weights on the device, hipGraph replay, best
of 5, us per call):
  1. BitNet-3B `down` (3200 x 8640) at N = 1 over rotating distinct weight sets:
       (a) the plain fused call on a ready vector;
       (b) silu(gate) * up and the RMSNorm as torch kernels into a buffer, then the plain call;
       (c) one tmac_hip_qgemm_fused_xf_dev call of kind GLU_NORM.
  2. the segment o -> NORM -> gate/up -> GLU_NORM -> down -> NORM -> q/k/v at H, F = 640, 1728 (tests/test_gpu_xf_glunorm.py):
       (d) one chain launch of the recording; (e) the same four calls one by one (fused + three fused_xf).
usage: bench_xf_glunorm.py"""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tmac_amd
from tmac_amd import KCfg, F32
dev = torch.device("cuda")
BITS, BM, EPS, NSETS = 2, 128, 1e-5, 8
wr = tmac_amd.TMACGeMMWrapper(act_group_size=64)


def weights(Mw, K):
    A = torch.randint(0, 256, (Mw * BITS // BM, K // 4, BM // 2), dtype=torch.uint8, device=dev)
    S = torch.full((1,), 0.01, device=dev, dtype=torch.float32)
    return tmac_amd.Weights(A, S, Mw, K, BITS, KCfg.make(Mw, K, BITS, BM, 16, 128, K, False, 1), scales_dtype=F32, dev_dtype=F32, on_device=True)


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


# ---- 1. BitNet-3B down
Mw, K = 3200, 8640
sets = [weights(Mw, K) for _ in range(NSETS)]
out = torch.empty(Mw, dtype=torch.float16, device=dev)
x, x2 = torch.randn(K, device=dev).half(), torch.randn(K, device=dev).half()
gam, xb = 1.0 + 0.1 * torch.randn(K, device=dev), torch.empty(K, device=dev)


def torch_then_plain(w):
    def f(st):
        g = torch.nn.functional.silu(x.float()) * x2.float()
        torch.mul(g * torch.rsqrt(g.pow(2).mean() + EPS), gam, out=xb)
        wr.fused([w], xb, [out], 1, stream=st)
    return f


ta = timeit([(lambda st, w=w: wr.fused([w], x, [out], 1, stream=st)) for w in sets])
tb = timeit([torch_then_plain(w) for w in sets])
tc = timeit([(lambda st, w=w: wr.fused_xf([w], x, [out], "glu_norm", in2=x2, gamma=gam, eps=EPS, stream=st)) for w in sets])
print(f"BitNet-3B down {Mw} x {K}, N = 1, us per call: (a) plain {ta:6.2f}   (b) torch GLU + RMSNorm + plain {tb:6.2f}   (c) GLU_NORM call {tc:6.2f}   "
      f"(c)/(b) {tc / tb:.3f}", flush=True)
for w in sets:
    w.free()

# ---- 2. the BitNet-shaped segment
H, F = 640, 1728
wo, wg, wu, wd, wq, wk, wv = weights(H, H), weights(F, H), weights(F, H), weights(H, F), weights(H, H), weights(H, H), weights(H, H)
f16 = lambda n: torch.zeros(n, dtype=torch.float16, device=dev)
attn = torch.randn(H, device=dev).half()
o, gate, up, down, q, k, v = f16(H), f16(F), f16(F), f16(H), f16(H), f16(H), f16(H)
h0, h1, h2 = torch.randn(H, device=dev), torch.zeros(H, device=dev), torch.zeros(H, device=dev)
g1, g2, g3 = (1.0 + 0.1 * torch.randn(n, device=dev) for n in (H, H, F))
with wr.record_chain() as rec:
    wr.fused([wo], attn, [o], 1)
    wr.chain_xform("norm", residual=h0, gamma=g2, eps=EPS, keep=True)
    wr.fused([wg, wu], o, [gate, up], 1)
    wr.chain_xform("glu_norm", in2=up, gamma=g3, eps=EPS)
    wr.fused([wd], gate, [down], 1)
    wr.chain_xform("norm", residual=wr.CARRY, gamma=g1, eps=EPS, residual_out=h2)
    wr.fused([wq, wk, wv], down, [q, k, v], 1)
chain = rec.chain


def one_by_one(st):
    wr.fused([wo], attn, [o], 1, stream=st)
    wr.fused_xf([wg, wu], o, [gate, up], "norm", residual=h0, gamma=g2, eps=EPS, residual_out=h1, stream=st)
    wr.fused_xf([wd], gate, [down], "glu_norm", in2=up, gamma=g3, eps=EPS, stream=st)
    wr.fused_xf([wq, wk, wv], down, [q, k, v], "norm", residual=h1, gamma=g1, eps=EPS, residual_out=h2, stream=st)


td = timeit([lambda st: chain.launch(stream=st)])
assert chain.status() == 0
te = timeit([one_by_one])
print(f"BitNet-shaped segment H = {H}, F = {F} (4 calls, 8 matrices), us per segment: (d) one chain launch {td:6.2f}   (e) call by call {te:6.2f}   "
      f"(d)/(e) {td / te:.3f}", flush=True)
chain.free()
