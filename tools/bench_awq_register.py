"""AutoAWQ tensors -> registered handle: the host route against the device route, the AWQ pack kernels beside the GPTQ W4 pack of the
same matrix and a plain copy, and the route a caller could assemble in torch.  tools/bench_register.py's method.

llama-2-7B shapes (o, qkv, gate/up, down), W4, group size 128, fp16 scales, seeded synthetic codes packed both ways (convert.pack_awq; GPTQ
v2 words of the same codes).  Per shape:
  (a) host route, SECONDS on the host clock, one run: convert.unpack_awq + weights.preprocess_weights (numpy, one thread) +
      tmac_hip_register_weights (upload of the blob + re-tile), ended by a device synchronise;
  (b) device route, MILLISECONDS on the host clock: upload of the three packed tensors from pageable memory + Weights.from_awq (pack +
      re-tile; it synchronises); first run and the median of the following three;
  (c) the pack kernels alone (tmac_hip_pack_awq_dev into preallocated buffers) under DEVICE EVENTS, microseconds per call, alternating
      pass by pass with tmac_hip_pack_gptq_dev at W4 on the same matrix -- the same bytes in and out -- and with a device-to-device
      hipMemcpyAsync of those bytes.  All three walk pools of distinct buffer sets larger than the 256 MiB Infinity Cache and are warmed;
      the alternation runs until each has filled a timed window of at least 0.3 s.  The GPTQ pack is also timed alone in front of the
      alternation and again behind it: the difference of the two is the session's spread.  Expectation: AWQ <= GPTQ + spread; a shape
      that misses is marked MISS and stands as measured;
  (d) the alternative in torch on the device, ms, median of three, tensors ALREADY on the device: shifts and masks to codes, scales and
      zeros, then Weights.from_codes -- beside Weights.from_awq on the same device tensors ((b) without its upload).
The one hard condition is (b) < (a) at every shape; the tool exits 1 when it does not hold.
usage: bench_awq_register.py [--out FILE] [--shapes o,qkv,gate_up,down] [--skip-host]"""
import argparse
import ctypes as C
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tmac_amd  # noqa: E402
from tmac_amd import F16, KCfg, convert, weights, wrapper  # noqa: E402
from bench_register import AGS, GS, POOL_BYTES, SHAPES, WINDOW_S, hip_runtime, median3  # noqa: E402


def synthetic(seed, Mw, K):
    """the same random codes, zero points and fp16 scales as AWQ GEMM tensors and as GPTQ (v2) W4 tensors"""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 16, size=(Mw, K), dtype=np.uint8)
    z = rng.integers(0, 16, size=(Mw, K // GS), dtype=np.uint8)
    sc = (np.abs(rng.standard_normal((Mw, K // GS))) * 0.02 + 0.005).astype(np.float16)
    sh = (np.arange(8, dtype=np.uint32) * np.uint32(4))

    def gptq_words(a):          # uint8 [R][C] -> int32 [R][C / 8]: eight consecutive columns per word, lowest field first
        return (a.reshape(a.shape[0], -1, 8).astype(np.uint32) << sh).sum(axis=-1, dtype=np.uint32).view(np.int32)

    gptq = (np.ascontiguousarray(gptq_words(w).T), np.ascontiguousarray(sc.T), np.ascontiguousarray(gptq_words(z.T)))
    return convert.pack_awq(w, sc, z), gptq


def host_route(qw, sc, qz, Mw, K, cfg):
    t0 = time.perf_counter()
    w, s, z, b, g = convert.unpack_awq(qw, sc, qz)
    t1 = time.perf_counter()
    A, S = weights.preprocess_weights(w, s, z, bits=4, bm=cfg.bm, kfactor=cfg.kfactor)
    t2 = time.perf_counter()
    h = tmac_amd.Weights(A, S, Mw, K, 4, cfg, scales_dtype=F16, dev_dtype=F16)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    h.free()
    return t1 - t0, t2 - t1, t3 - t2


def device_route(qw, sc, qz, cfg):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h = tmac_amd.Weights.from_awq(qw, sc, qz, cfg, F16)          # numpy in: uploaded first; the call synchronises
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    h.free()
    return (t1 - t0) * 1e3


def torch_route(dq, ds, dz, cfg):
    """what a caller without the AWQ entry points could do on the device: unpack with shifts and masks, then the codes form"""
    sh = torch.tensor([4 * i for i in convert.AWQ_INV], dtype=torch.int32, device="cuda")
    K, SG = int(dq.shape[0]), int(dz.shape[0])
    w = ((dq.unsqueeze(-1) >> sh) & 15).to(torch.uint8).reshape(K, -1).t().contiguous()
    z = ((dz.unsqueeze(-1) >> sh) & 15).reshape(SG, -1).t()
    s = ds.t().contiguous()
    zeros = ((z.to(s.dtype) - 8) * s).contiguous()
    return tmac_amd.Weights.from_codes(w, s, zeros, 4, cfg, F16)


def packs_vs_copy(hip, awq, gptq, Mw, K, cfg):
    """(bytes per call, {name: us per call}, GPTQ alone first us, GPTQ alone last us, passes)"""
    a_bytes, s_bytes = wrapper.ref_blob_bytes(Mw, K, 4, cfg, F16)
    in_bytes = sum(a.nbytes for a in awq)
    assert in_bytes == sum(a.nbytes for a in gptq)
    moved = in_bytes + a_bytes + s_bytes
    nsets = max(2, math.ceil(POOL_BYTES / moved))
    outs = [(torch.empty(a_bytes, dtype=torch.uint8, device="cuda"), torch.empty(s_bytes, dtype=torch.uint8, device="cuda")) for _ in range(nsets)]
    ins = {}
    for name, trip in (("awq", awq), ("gptq", gptq)):
        d = [torch.from_numpy(a).cuda() for a in trip]
        ins[name] = [tuple(t.clone() for t in d) for _ in range(nsets)]
    half = (moved // 2 + 15) // 16 * 16
    src = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(nsets)]
    dst = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(nsets)]
    st = torch.cuda.current_stream().cuda_stream
    L = tmac_amd.lib()

    def awq_pass():
        for (q, s, z), (A, S) in zip(ins["awq"], outs):
            tmac_amd.binding.check(L.tmac_hip_pack_awq_dev(q.data_ptr(), s.data_ptr(), z.data_ptr(), F16, Mw, K, C.byref(cfg), A.data_ptr(), S.data_ptr(),
                                                           F16, st))

    def gptq_pass():
        for (q, s, z), (A, S) in zip(ins["gptq"], outs):
            tmac_amd.binding.check(L.tmac_hip_pack_gptq_dev(q.data_ptr(), s.data_ptr(), z.data_ptr(), F16, 1, Mw, K, 4, C.byref(cfg), A.data_ptr(),
                                                            S.data_ptr(), F16, st))

    def copy_pass():
        for a, b in zip(src, dst):
            rc = hip.hipMemcpyAsync(C.c_void_p(b.data_ptr()), C.c_void_p(a.data_ptr()), C.c_size_t(half), 3, C.c_void_p(st))     # 3: device to device
            if rc:
                raise RuntimeError(f"hipMemcpyAsync: {rc}")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    def alone(fn):
        t, n = 0.0, 0
        while n < 3 or t < WINDOW_S / 3:
            t += timed(fn)
            n += 1
        return t / (n * nsets) * 1e6

    awq_pass(); gptq_pass(); copy_pass(); torch.cuda.synchronize()       # warm: code objects, first touch of every buffer
    first = alone(gptq_pass)
    t = {"awq": 0.0, "gptq": 0.0, "copy": 0.0}
    passes = 0
    while passes < 3 or min(t.values()) < WINDOW_S:
        t["gptq"] += timed(gptq_pass)
        t["awq"] += timed(awq_pass)
        t["copy"] += timed(copy_pass)
        passes += 1
    last = alone(gptq_pass)
    return moved, {k: v / (passes * nsets) * 1e6 for k, v in t.items()}, first, last, passes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--shapes", default="o,qkv,gate_up,down")
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()
    hip = hip_runtime()
    lines = ["# tools/bench_awq_register.py: AutoAWQ GEMM tensors -> handle, llama-2-7B shapes, W4, group size 128, fp16 scales.",
             f"# device: {torch.cuda.get_device_name(0)}",
             "# (a) host route s (unpack + preprocess + register) | (b) device route ms (first, median of 3) | (c) pack kernels alone, us per call by device",
             "#     events: GPTQ W4 alone first / last (spread = their difference), then AWQ, GPTQ, d2d copy alternating | (d) on device tensors, ms: from_awq, torch unpack + from_codes",
             "shape    Mw     K     | (a) unpack  preproc  register  total_s | (b) first_ms  median_ms | (c) MiB  gptq_first  gptq_last  spread |  awq_us  gptq_us  copy_us  awq/gptq | verdict | (d) from_awq_ms  torch_ms"]
    bad = False
    for name in args.shapes.split(","):
        Mw, K = SHAPES[name]
        cfg = KCfg.make(Mw, K, 4, convert.default_bm(4, Mw), 16, GS, AGS, True)
        awq, gptq = synthetic(Mw + K, Mw, K)
        ta = (float("nan"),) * 3 if args.skip_host else host_route(*awq, Mw, K, cfg)
        tb = [device_route(*awq, cfg) for _ in range(4)]
        moved, us, first, last, passes = packs_vs_copy(hip, awq, gptq, Mw, K, cfg)
        dev = [torch.from_numpy(a).cuda() for a in awq]
        td = median3(lambda: torch_route(*dev, cfg), free=True)
        tdev = median3(lambda: tmac_amd.Weights.from_awq(*dev, cfg, F16), free=True)
        spread = abs(first - last)
        verdict = "ok" if us["awq"] <= us["gptq"] + spread else "MISS: awq > gptq + spread"
        if not args.skip_host and not tb[0] * 1e-3 < sum(ta):
            bad = True
        line = (f"{name:8s} {Mw:5d}  {K:5d} | {ta[0]:9.3f}  {ta[1]:7.3f}  {ta[2]:8.3f}  {sum(ta):7.3f} | {tb[0]:12.3f}  {float(np.median(tb[1:])):9.3f} | "
                f"{moved / 2 ** 20:7.1f}  {first:10.2f}  {last:9.2f}  {spread:6.2f} | {us['awq']:7.2f}  {us['gptq']:7.2f}  {us['copy']:7.2f}  "
                f"{us['awq'] / us['gptq']:8.3f} | {verdict} | {tdev:11.3f}  {td:8.3f}")
        print(line, flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
