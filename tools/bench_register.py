"""GPTQ tensors -> registered handle: the host route against the device route, and the pack kernels against a plain copy.

llama-2-7B shapes (o, qkv, gate/up, down), W2 and W4, group size 128, seeded synthetic GPTQ tensors (fp16 scales).  Per shape:
  (a) host route, SECONDS on the host clock, one run: convert.unpack_gptq + weights.preprocess_weights (numpy, one thread) +
      tmac_hip_register_weights (upload of the blob + re-tile), ended by a device synchronise;
  (b) device route, MILLISECONDS on the host clock: upload of the three packed tensors from pageable memory +
      tmac_hip_register_weights_gptq_dev (pack + re-tile; it synchronises); first run and the median of the following three;
  (c) the pack kernels alone (tmac_hip_pack_gptq_dev into preallocated buffers) under DEVICE EVENTS, as bytes read + written over time,
      beside a device-to-device hipMemcpyAsync that moves the same number of bytes (it copies half of them: read + written are equal).
      Both walk a pool of distinct buffer sets larger than the 256 MiB Infinity Cache, are warmed, and alternate pass by pass in one run
      until each has filled a timed window of at least 0.3 s.
No rate is required of (c): the file states the kernels' share of the copy's rate.  The one hard condition is (b) < (a) at every shape;
the tool exits 1 when it does not hold.
--bitnet: BitNet-3B master weights (fp16 / bf16, on the device) -> handle instead: see bitnet() below.
--bitnet-packed: packed ternary BitNet weights (four weight rows per byte) -> handle, and the two pack kernels beside the codes kernel
and a copy: see bitnet_packed() below.
--dense: unquantised fp16 matrices of the same llama-2-7B shapes -> W2 / W4 handles by per-group round to nearest: see dense() below.
usage: bench_register.py [--out FILE] [--shapes o,qkv,gate_up,down] [--bits 2,4] [--skip-host] | --bitnet [--out FILE] | --bitnet-packed [--out FILE]
       | --dense [--out FILE] [--shapes ...] [--bits 2,4] [--skip-host]"""
import argparse
import ctypes as C
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tmac_amd  # noqa: E402
from tmac_amd import F16, F32, KCfg, convert, weights, wrapper  # noqa: E402

SHAPES = {"o": (4096, 4096), "qkv": (12288, 4096), "gate_up": (11008, 4096), "down": (4096, 11008)}     # (Mw, K)
GS, AGS, POOL_BYTES, WINDOW_S = 128, 64, 640 << 20, 0.3


def synthetic(seed, Mw, K, bits):
    """GPTQ tensors with every field random: qweight int32 [K*bits/32][Mw], scales fp16 [K/gs][Mw], qzeros int32 [K/gs][Mw*bits/32]"""
    rng = np.random.default_rng(seed)
    qw = rng.integers(-2 ** 31, 2 ** 31, size=(K * bits // 32, Mw), dtype=np.int64).astype(np.int32)
    qz = rng.integers(-2 ** 31, 2 ** 31, size=(K // GS, Mw * bits // 32), dtype=np.int64).astype(np.int32)
    sc = (np.abs(rng.standard_normal((K // GS, Mw))) * 0.02 + 0.005).astype(np.float16)
    return qw, sc, qz


def hip_runtime():
    """the HIP runtime this process already has (torch's): one more runtime in the process would be a second device context"""
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                return C.CDLL(line.split()[-1])
    raise RuntimeError("no libamdhip64 mapped")


def host_route(qw, sc, qz, Mw, K, bits, cfg):
    t0 = time.perf_counter()
    w, s, z, b, g = convert.unpack_gptq(qw, sc, qz, gptq_v2=True)
    t1 = time.perf_counter()
    A, S = weights.preprocess_weights(w, s, z, bits=bits, bm=cfg.bm, kfactor=cfg.kfactor)
    t2 = time.perf_counter()
    h = tmac_amd.Weights(A, S, Mw, K, bits, cfg, scales_dtype=F16, dev_dtype=F16)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    h.free()
    return t1 - t0, t2 - t1, t3 - t2


def device_route(qw, sc, qz, cfg):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h = tmac_amd.Weights.from_gptq(qw, sc, qz, cfg, True, F16)          # numpy in: uploaded first; the call synchronises
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    h.free()
    return (t1 - t0) * 1e3


def pack_vs_copy(hip, qw, sc, qz, Mw, K, bits, cfg):
    """(bytes per call, pack GB/s, copy GB/s, calls timed, pack window s, copy window s)"""
    a_bytes, s_bytes = wrapper.ref_blob_bytes(Mw, K, bits, cfg, F16)
    in_bytes = qw.nbytes + sc.nbytes + qz.nbytes
    moved = in_bytes + a_bytes + s_bytes
    nsets = max(2, math.ceil(POOL_BYTES / moved))
    dq, ds, dz = (torch.from_numpy(a).cuda() for a in (qw, sc, qz))
    sets = [(dq.clone(), ds.clone(), dz.clone(), torch.empty(a_bytes, dtype=torch.uint8, device="cuda"),
             torch.empty(s_bytes, dtype=torch.uint8, device="cuda")) for _ in range(nsets)]
    half = (moved // 2 + 15) // 16 * 16
    src = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(nsets)]
    dst = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(nsets)]
    st = torch.cuda.current_stream().cuda_stream
    L = tmac_amd.lib()

    def pack_pass():
        for q, s, z, A, S in sets:
            tmac_amd.binding.check(L.tmac_hip_pack_gptq_dev(q.data_ptr(), s.data_ptr(), z.data_ptr(), F16, 1, Mw, K, bits, C.byref(cfg),
                                                            A.data_ptr(), S.data_ptr(), F16, st))

    def copy_pass():
        for a, b in zip(src, dst):
            rc = hip.hipMemcpyAsync(C.c_void_p(b.data_ptr()), C.c_void_p(a.data_ptr()), C.c_size_t(half), 3, C.c_void_p(st))     # 3: device to device
            if rc:
                raise RuntimeError(f"hipMemcpyAsync: {rc}")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    pack_pass(); copy_pass(); torch.cuda.synchronize()       # warm: code objects, first touch of every buffer
    tp = tc = 0.0
    passes = 0
    while passes < 3 or tp < WINDOW_S or tc < WINDOW_S:
        tp += timed(pack_pass)
        tc += timed(copy_pass)
        passes += 1
    calls = passes * nsets
    return moved, moved * calls / tp / 1e9, 2 * half * calls / tc / 1e9, calls, tp, tc


BITNET_SHAPES = {"attn": (3200, 3200), "gate_up": (8640, 3200), "down": (3200, 8640)}      # BitNet-3B (hf-bitnet-3b), (Mw, K)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def median3(fn, free=False):
    """median of three runs after one warm-up, host-clock ms with a device synchronise on either side"""
    ts = []
    for i in range(4):
        t, r = wall_ms(fn)
        if free:
            r.free()
        if i:
            ts.append(t)
    return float(np.median(ts))


def bitnet(out):
    """BitNet-3B master weights -> handle, fp16 and bf16 masters ON THE DEVICE, median of three (host clock, ms):
      (a) host route: download + convert.bitnet_absmean_quant + weights.preprocess_weights + tmac_hip_register_weights;
      (b) Weights.from_bitnet (reduction + quantising pack + re-tile);
      (c) Weights.from_codes on pre-made levels on the device (the existing device pack; (b) reads 2 - 4 times its input bytes, twice);
    and (b) taken apart: the reduction alone (wrapper.absmean), the quantising pack alone (wrapper.pack_bitnet with the scale handed in),
    the codes pack alone (wrapper.pack_codes).  No threshold: the ratios are recorded."""
    lines = ["# tools/bench_register.py --bitnet: BitNet-3B master weights on the device -> handle; host-clock ms, median of three after a warm-up.",
             f"# device: {torch.cuda.get_device_name(0)}; unified scale (m_groups = 1), act_group_size = K, fp32 device scales",
             "shape    src   Mw     K     | (a) host_ms | (b) from_bitnet_ms | (c) from_codes_ms | (b)/(a)  (b)/(c) | absmean_ms  pack_given_scale_ms  pack_codes_ms"]
    for name, (Mw, K) in BITNET_SHAPES.items():
        cfg = KCfg.make(Mw, K, 2, convert.default_bm(2, Mw), 16, 128, K, False, 1)
        w32 = (np.random.default_rng(Mw + K).standard_normal((Mw, K)) * 0.02).astype(np.float32)
        for src, dt in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
            wd = torch.from_numpy(w32).cuda().to(dt)
            torch.cuda.synchronize()

            def host():
                st = wd.view(torch.int16).cpu().numpy()
                st = st.view(np.float16) if dt == torch.float16 else st.view(np.uint16)
                lv, s = convert.bitnet_absmean_quant(st)
                A, S = weights.preprocess_weights(lv, s, None, bits=2, bm=cfg.bm, kfactor=cfg.kfactor)
                return tmac_amd.Weights(A, S, Mw, K, 2, cfg, scales_dtype=F32, dev_dtype=F32)
            ta, h = wall_ms(host)                                    # seconds-class: one run
            h.free()
            tb = median3(lambda: tmac_amd.Weights.from_bitnet(wd, cfg), free=True)
            s_dev = wrapper.absmean(wd)
            lv, _ = convert.bitnet_absmean_quant(wd.view(torch.int16).cpu().numpy().view(np.float16 if dt == torch.float16 else np.uint16),
                                                 scale=s_dev.cpu().numpy())
            lvd = torch.from_numpy(lv).cuda()
            tc = median3(lambda: tmac_amd.Weights.from_codes(lvd, s_dev, None, 2, cfg, F32), free=True)
            t_mean = median3(lambda: wrapper.absmean(wd))
            t_pack = median3(lambda: wrapper.pack_bitnet(wd, cfg, scale=s_dev))
            t_codes = median3(lambda: wrapper.pack_codes(lvd, s_dev, None, 2, cfg, F32))
            line = (f"{name:8s} {src:5s} {Mw:5d}  {K:5d} | {ta:11.1f} | {tb:18.3f} | {tc:17.3f} | {tb / ta:7.4f}  {tb / tc:7.2f} | "
                    f"{t_mean:10.3f}  {t_pack:19.3f}  {t_codes:13.3f}")
            print(line, flush=True)
            lines.append(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


def dense(out, shapes, bits_list, skip_host):
    """Unquantised llama-2-7B matrices -> W2 / W4 handles with per-group scales (group size 128, zero points, fp16 device scales), fp16
    masters ON THE DEVICE.  Host clock with a device synchronise on either side, ms, median of ten after a warm-up, one process:
      (a) Weights.from_dense (k_rtn_params + k_pack_rtn_weights + the scales kernel + re-tile);
      (b) Weights.from_codes on codes, scales and zeros already on the device (the existing device pack: reads Mw K code bytes);
      (d) hipMemcpyAsync device-to-device of the masters' bytes: what reading them once and writing as much costs;
    and (c) the host route, ONE run (it takes seconds): download + convert.rtn_quant + weights.preprocess_weights +
    tmac_hip_register_weights.  (a) reads the masters twice (2 x 2 Mw K bytes) where (b) reads Mw K bytes once: the expectation is (a)
    near (b) plus one or two (d), orders of magnitude below (c).  No threshold: the figures are recorded."""
    hip = hip_runtime()
    st = torch.cuda.current_stream().cuda_stream

    def median10(fn, free=False):
        ts = []
        for i in range(11):
            t, r = wall_ms(fn)
            if free:
                r.free()
            if i:
                ts.append(t)
        return float(np.median(ts))

    lines = ["# tools/bench_register.py --dense: fp16 matrices on the device -> W2 / W4 handles, per-group round to nearest.  Host-clock ms with a",
             "# device synchronise on either side, median of ten after a warm-up; (c) one run.  (a) from_dense  (b) from_codes on device codes",
             f"# (c) host route  (d) D2D copy of the masters' bytes.  device: {torch.cuda.get_device_name(0)}; group size {GS}, zero points, fp16 scales",
             "shape     bits  Mw     K      | (a) dense_ms  (b) codes_ms  (d) copy_ms  (c) host_ms | (a)-(b) in (d)  (a)/(b)  (c)/(a)"]
    for name in shapes:
        Mw, K = SHAPES[name]
        w32 = (np.random.default_rng(Mw + K).standard_normal((Mw, K)) * 0.02).astype(np.float32)
        wd = torch.from_numpy(w32).cuda().half()
        dst = torch.empty_like(wd)
        nbytes = wd.numel() * 2

        def copy():
            rc = hip.hipMemcpyAsync(C.c_void_p(dst.data_ptr()), C.c_void_p(wd.data_ptr()), C.c_size_t(nbytes), 3, C.c_void_p(st))     # 3: device to device
            if rc:
                raise RuntimeError(f"hipMemcpyAsync: {rc}")
        td = median10(copy)
        for bits in bits_list:
            cfg = KCfg.make(Mw, K, bits, convert.default_bm(bits, Mw), 16, GS, AGS, True)
            ta = median10(lambda: tmac_amd.Weights.from_dense(wd, bits, GS, True, cfg, F16, AGS), free=True)
            stored = wd.cpu().numpy()
            codes, sc, zr = convert.rtn_quant(stored, bits, GS, True, True)
            cd, sd, zd = torch.from_numpy(codes).cuda(), torch.from_numpy(sc).cuda(), torch.from_numpy(zr).cuda()
            tb = median10(lambda: tmac_amd.Weights.from_codes(cd, sd, zd, bits, cfg, F16, AGS), free=True)
            if skip_host:
                tc = float("nan")
            else:
                def host():
                    c, s, z = convert.rtn_quant(wd.cpu().numpy(), bits, GS, True, True)
                    A, S = weights.preprocess_weights(c, s, z, bits=bits, bm=cfg.bm, kfactor=cfg.kfactor)
                    return tmac_amd.Weights(A, S, Mw, K, bits, cfg, scales_dtype=F32, dev_dtype=F16)
                tc, h = wall_ms(host)
                h.free()
            line = (f"{name:9s} {bits:4d}  {Mw:5d}  {K:5d}  | {ta:12.3f}  {tb:12.3f}  {td:11.3f}  {tc:11.1f} | {(ta - tb) / td:14.2f}  {ta / tb:7.2f}  "
                    f"{tc / ta:7.0f}")
            print(line, flush=True)
            lines.append(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


# bitnet-b1.58-2B-4T (q/o, k/v, gate/up, down) and the 3B preset, (Mw, K): Mw / 4 is a multiple of 16 at every one of them
BITNET_PACKED_SHAPES = {"2b4t_qo": (2560, 2560), "2b4t_kv": (640, 2560), "2b4t_gate_up": (6912, 2560), "2b4t_down": (2560, 6912),
                        "3b_attn": (3200, 3200), "3b_gate_up": (8640, 3200), "3b_down": (3200, 8640)}
SPREAD = 0.05       # run-to-run spread, the margin of the verdicts below


def alternate(contenders):
    """{name: pass function} -> {name: seconds per pass}: all warmed, then alternated pass by pass under device events until every one has
    filled a timed window of WINDOW_S"""
    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3
    for fn in contenders.values():
        fn()
    torch.cuda.synchronize()
    t = {n: 0.0 for n in contenders}
    passes = 0
    while passes < 3 or min(t.values()) < WINDOW_S:
        for n, fn in contenders.items():
            t[n] += timed(fn)
        passes += 1
    return {n: v / passes for n, v in t.items()}


def bitnet_packed(out):
    """Packed ternary BitNet weights (uint8 [Mw/4][K]) -> handle, every matrix shape of bitnet-b1.58-2B-4T and of the 3B preset.
      host clock, ms, median of three after a warm-up, inputs in pageable HOST memory (the upload is inside every figure):
        (a) Weights.from_bitnet_packed;  (b) Weights.from_codes on the unpacked levels (4 x the bytes);  (c) Weights.from_bitnet on fp16
        masters (8 x the bytes, and the reduction);
      device events, us per call of the pack entry point (the weight kernel + the one-block copy of the scale, no counter), alternated
      pass by pass over pools of distinct buffer sets larger than the 256 MiB Infinity Cache:
        x4: k_pack_ternary_weights_x4;  gen: k_pack_ternary_weights forced;  codes: k_pack_codes_weights<2> on the same matrix's levels;
        copy: hipMemcpyAsync device-to-device of the blob's bytes.
    Expectation (not a threshold of this tool: the verdict is written down): x4 <= codes and x4 <= gen, within SPREAD."""
    hip = hip_runtime()
    L = tmac_amd.lib()
    st = torch.cuda.current_stream().cuda_stream
    lines = ["# tools/bench_register.py --bitnet-packed: packed ternary weights -> handle.  Left: host-clock ms, median of three after a warm-up, upload",
             "# from pageable host memory included.  Right: device events, us per pack call, contenders alternated pass by pass, pool per contender",
             f"# >= {POOL_BYTES >> 20} MiB, window >= {WINDOW_S} s each.  device: {torch.cuda.get_device_name(0)}; m_groups = 1, act_group_size = K",
             "shape         Mw     K     | (a) packed_ms  (b) codes_ms  (c) masters_ms  (a)/(b)  (a)/(c) | x4_us   gen_us  codes_us  copy_us | x4/codes  x4/gen  x4/copy"]
    worst_codes = worst_gen = 0.0
    for name, (Mw, K) in BITNET_PACKED_SHAPES.items():
        cfg = KCfg.make(Mw, K, 2, convert.default_bm(2, Mw), 16, 128, K, False, 1)
        rng = np.random.default_rng(Mw + K)
        lv = rng.integers(1, 4, size=(Mw, K), dtype=np.uint8)
        packed = convert.pack_bitnet_packed(lv)
        s = np.array([0.0371], np.float32)
        masters = ((lv.astype(np.float32) - 2.0) * s[0]).astype(np.float16)
        ta = median3(lambda: tmac_amd.Weights.from_bitnet_packed(packed, s, cfg), free=True)
        tb = median3(lambda: tmac_amd.Weights.from_codes(lv, s, None, 2, cfg, F32), free=True)
        tc = median3(lambda: tmac_amd.Weights.from_bitnet(masters, cfg), free=True)
        # the kernels alone
        a_bytes, s_bytes = wrapper.ref_blob_bytes(Mw, K, 2, cfg, F32)
        pd, cd, sd = torch.from_numpy(packed).cuda(), torch.from_numpy(lv).cuda(), torch.from_numpy(np.concatenate([s, np.zeros(3, np.float32)])).cuda()

        def pool(src, per_set):
            return [(src.clone(), torch.empty(a_bytes, dtype=torch.uint8, device="cuda"), torch.empty(16, dtype=torch.uint8, device="cuda"))
                    for _ in range(max(2, math.ceil(POOL_BYTES / per_set)))]
        tern, codes = pool(pd, packed.nbytes + a_bytes), pool(cd, lv.nbytes + a_bytes)
        ncopy = max(2, math.ceil(POOL_BYTES / (2 * a_bytes)))
        csrc = [torch.empty(a_bytes, dtype=torch.uint8, device="cuda") for _ in range(ncopy)]
        cdst = [torch.empty(a_bytes, dtype=torch.uint8, device="cuda") for _ in range(ncopy)]

        def tern_pass(general):
            def run():
                tmac_amd.binding.check(L.tmac_hip_debug_pack_ternary_kernel(general))
                for p, A, S in tern:
                    tmac_amd.binding.check(L.tmac_hip_pack_ternary_dev(p.data_ptr(), sd.data_ptr(), Mw, K, C.byref(cfg), A.data_ptr(), S.data_ptr(), F32, None, st))
                tmac_amd.binding.check(L.tmac_hip_debug_pack_ternary_kernel(0))
            return run

        def codes_pass():
            for c, A, S in codes:
                tmac_amd.binding.check(L.tmac_hip_pack_codes_dev(c.data_ptr(), sd.data_ptr(), None, F32, Mw, K, 2, C.byref(cfg), A.data_ptr(), S.data_ptr(), F32, st))

        def copy_pass():
            for a, b in zip(csrc, cdst):
                rc = hip.hipMemcpyAsync(C.c_void_p(b.data_ptr()), C.c_void_p(a.data_ptr()), C.c_size_t(a_bytes), 3, C.c_void_p(st))     # 3: device to device
                if rc:
                    raise RuntimeError(f"hipMemcpyAsync: {rc}")
        t = alternate({"x4": tern_pass(0), "gen": tern_pass(1), "codes": codes_pass, "copy": copy_pass})
        x4, gen, cod, cpy = (t["x4"] / len(tern) * 1e6, t["gen"] / len(tern) * 1e6, t["codes"] / len(codes) * 1e6, t["copy"] / ncopy * 1e6)
        # what was timed is the same work: the blob of the last ternary pass is the codes kernel's (the suite holds both forms to it)
        assert torch.equal(tern[0][1], codes[0][1]) and torch.equal(tern[-1][1], codes[-1][1])
        worst_codes, worst_gen = max(worst_codes, x4 / cod), max(worst_gen, x4 / gen)
        line = (f"{name:13s} {Mw:5d}  {K:5d} | {ta:13.3f}  {tb:12.3f}  {tc:14.3f}  {ta / tb:7.2f}  {ta / tc:7.2f} | {x4:6.1f}  {gen:7.1f}  {cod:8.1f}  {cpy:7.1f} | "
                f"{x4 / cod:8.2f}  {x4 / gen:6.2f}  {x4 / cpy:7.2f}")
        print(line, flush=True)
        lines.append(line)
        del tern, codes, csrc, cdst
        torch.cuda.empty_cache()
    lines.append(f"# read-once no slower than the codes kernel within {SPREAD:.0%} at every shape: " + ("yes" if worst_codes <= 1 + SPREAD else "NO")
                 + f" (worst x4/codes {worst_codes:.2f})")
    lines.append(f"# read-once no slower than the general form within {SPREAD:.0%} at every shape: " + ("yes" if worst_gen <= 1 + SPREAD else "NO")
                 + f" (worst x4/gen {worst_gen:.2f})")
    print("\n".join(lines[-2:]))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--bitnet-packed", action="store_true", help="packed ternary BitNet weights instead: from_bitnet_packed, from_codes, from_bitnet, the kernels alone")
    ap.add_argument("--bitnet", action="store_true", help="the BitNet-3B master-weight shapes instead: host route, from_bitnet, from_codes")
    ap.add_argument("--dense", action="store_true", help="unquantised fp16 llama-2-7B matrices instead: from_dense, from_codes, the host route, a copy")
    ap.add_argument("--shapes", default="o,qkv,gate_up,down")
    ap.add_argument("--bits", default="2,4")
    ap.add_argument("--skip-host", action="store_true", help="leave (a) out (it takes seconds per shape)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_register.py measures on a GPU"
    if args.bitnet:
        return bitnet(args.out)
    if args.bitnet_packed:
        return bitnet_packed(args.out)
    if args.dense:
        return dense(args.out, args.shapes.split(","), [int(b) for b in args.bits.split(",")], args.skip_host)
    hip = hip_runtime()
    lines = ["# tools/bench_register.py: GPTQ tensors -> handle.  (a) host seconds, one run; (b) host-clock ms around upload + device-side",
             "# registration; (c) pack kernels alone, device events, bytes read + written per second, beside hipMemcpyAsync D2D of the same bytes.",
             f"# device: {torch.cuda.get_device_name(0)}; group size {GS}; fp16 scales; pool per contender >= {POOL_BYTES >> 20} MiB; window >= {WINDOW_S} s",
             "shape     bits  Mw     K      | (a) unpack_s  preprocess_s  register_s  total_s | (b) first_ms  median3_ms  (a)/(b) | "
             "(c) MB/call  calls  pack_GB/s  copy_GB/s  pack/copy"]
    ok = True
    for name in args.shapes.split(","):
        Mw, K = SHAPES[name]
        for bits in (int(b) for b in args.bits.split(",")):
            cfg = KCfg.make(Mw, K, bits, convert.default_bm(bits, Mw), 16, GS, AGS, True)
            qw, sc, qz = synthetic(1000 * bits + Mw % 997, Mw, K, bits)
            dev = [device_route(qw, sc, qz, cfg) for _ in range(4)]
            first, med = dev[0], float(np.median(dev[1:]))
            if args.skip_host:
                a_txt, ratio = "      -             -           -        -", "      -"
            else:
                tu, tpp, tr = host_route(qw, sc, qz, Mw, K, bits, cfg)
                total = tu + tpp + tr
                a_txt = f"{tu:9.3f}  {tpp:12.3f}  {tr:10.3f}  {total:7.3f}"
                ratio = f"{total * 1e3 / med:7.0f}"
                ok &= max(first, med) < total * 1e3
            moved, pg, cg, calls, tp, tc = pack_vs_copy(hip, qw, sc, qz, Mw, K, bits, cfg)
            line = (f"{name:9s} {bits:4d}  {Mw:5d}  {K:5d}  |    {a_txt} |    {first:9.2f}  {med:10.2f}  {ratio} |    "
                    f"{moved / 1e6:8.2f}  {calls:5d}  {pg:9.0f}  {cg:9.0f}  {pg / cg:9.2f}")
            print(line, flush=True)
            lines.append(line)
    lines.append("# (b) < (a) at every shape: " + ("yes" if ok else "NO"))
    print(lines[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
