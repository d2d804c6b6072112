"""Inputs and host references shared by the packing tests (test_pack_cpu.py, test_gpu_pack.py): seeded GPTQ tensors and plain codes,
and the blob the host route makes of them (convert.unpack_gptq + weights.preprocess_weights, which tests/test_convert.py and
tests/test_oracle_vs_ref.py tie to the reference)."""
import numpy as np

from tmac_amd import convert, weights


def pack_fields(v, bits):
    """uint8 [..., 32/bits] -> int32 [...], little-end-first bit fields (the inverse of the GPTQ unpack)"""
    sh = np.arange(0, 32, bits, dtype=np.uint64)
    return (v.astype(np.uint64) << sh).sum(axis=-1).astype(np.uint32).view(np.int32)


def hard_scales(rng, shape, dtype, hard=True):
    """positive scales whose products with a small integer ROUND: fp16 -- every one of the 11 mantissa bits in use, exponents around
    2^-6; fp32 -- random mantissas.  hard: rows 0 and 1 of group 0 are 60000 -- times 2 and more that overflows fp16."""
    if dtype == np.float16:
        m = (rng.integers(1024, 2048, size=shape) | 1).astype(np.float64)          # odd: the last mantissa bit is set
        s = (m / 1024.0 * 2.0 ** rng.integers(-9, -3, size=shape)).astype(np.float16)
        if hard:
            s[0, 0] = s[1, 0] = np.float16(60000.0)
    else:
        s = (np.abs(rng.standard_normal(shape)) * 0.02 + 0.005).astype(np.float32)
    return s


def make_gptq(seed, Mw, K, bits, gs, scales_dtype=np.float16, hard=True):
    """(qweight int32 [K*bits/32][Mw], scales [K/gs][Mw], qzeros int32 [K/gs][Mw*bits/32]).  hard: the zero fields under the two 60000
    scales are the lowest and the highest code, so that for 2 and 4 bits a zero overflows fp16 whether the tensors are read as v1 or v2
    (a 1-bit multiplier is -1, 0 or 1: nothing overflows there); hard=False: tensors a GEMV can be computed from"""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 2 ** bits, size=(Mw, K), dtype=np.uint8)
    z = rng.integers(0, 2 ** bits, size=(Mw, K // gs), dtype=np.uint8)
    if hard:
        z[0, 0], z[1, 0] = 0, 2 ** bits - 1
    sc = hard_scales(rng, (Mw, K // gs), np.dtype(scales_dtype).type, hard)
    per = 32 // bits
    qweight = np.ascontiguousarray(pack_fields(w.T.reshape(K // per, per, Mw).transpose(0, 2, 1), bits))
    qzeros = np.ascontiguousarray(pack_fields(z.T.reshape(K // gs, Mw // per, per), bits))
    return qweight, np.ascontiguousarray(sc.T), qzeros


def make_codes(seed, Mw, K, bits, gs, dtype=np.float32, junk_high_bits=True):
    """(codes uint8 [Mw][K], scales [Mw][K/gs], zeros [Mw][K/gs]); the codes carry random bits above `bits`, which a packer ignores"""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 256 if junk_high_bits else 2 ** bits, size=(Mw, K), dtype=np.uint8)
    sc = hard_scales(rng, (Mw, K // gs), np.dtype(dtype).type, hard=False)
    zr = (sc.astype(np.float32) * rng.integers(-(2 ** (bits - 1)), 2 ** (bits - 1), size=sc.shape)).astype(dtype)
    return codes, sc, zr


def host_blob_gptq(qweight, scales, qzeros, gptq_v2, bm, kfactor, zero_point=True):
    """(A uint8, S in the scales' dtype) by the host route; also (w, sc, zr, bits, gs) of the unpacking"""
    with np.errstate(over="ignore"):
        w, sc, zr, bits, gs = convert.unpack_gptq(qweight, scales, qzeros, gptq_v2=gptq_v2)
    A, S = weights.preprocess_weights(w, sc, zr if zero_point else None, bits=bits, bm=bm, kfactor=kfactor)
    return A, S, (w, sc, zr, bits, gs)


def host_blob_codes(codes, sc, zr, bits, bm, kfactor):
    return weights.preprocess_weights(codes, sc, zr, bits=bits, bm=bm, kfactor=kfactor)


def raw_bits(a):
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


# ---- synthetic checkpoints ----------------------------------------------------------------------------------------------------------
ST_DTYPES = {np.dtype(np.int32): "I32", np.dtype(np.float16): "F16", np.dtype(np.float32): "F32"}


def write_safetensors(path, tensors, dtype_names=None):
    """{name: numpy array} -> a .safetensors file (8-byte little-endian header length, JSON header with dtype / shape / data_offsets
    relative to the end of the header, then the bytes).  dtype_names: {name: str} overrides the recorded dtype (a BF16 tensor is two bytes
    per element like F16: the test writes fp16 bytes under that name).  Returns {name: (begin, end)} counted from the start of the file."""
    import json
    import struct
    hdr, pos, blobs = {"__metadata__": {"format": "pt"}}, 0, []
    for name, a in tensors.items():
        raw = np.ascontiguousarray(a).tobytes()
        hdr[name] = {"dtype": (dtype_names or {}).get(name, ST_DTYPES[a.dtype]), "shape": list(a.shape), "data_offsets": [pos, pos + len(raw)]}
        pos += len(raw)
        blobs.append(raw)
    text = json.dumps(hdr).encode()
    text += b" " * (-len(text) % 8)
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(text)) + text + b"".join(blobs))
    return {k: (8 + len(text) + v["data_offsets"][0], 8 + len(text) + v["data_offsets"][1]) for k, v in hdr.items() if k != "__metadata__"}


def write_gptq_checkpoint(d, layers, quantizer="gptqmodel:1.2.3", sym=False, desc_act=False, quant_method="gptq", drop=(), dtype_names=None):
    """A two-part GPTQ checkpoint in directory d.  layers: [(name, seed, Mw, K, bits, gs)], dealt to the parts in turn; every part also
    holds a tensor that is no GPTQ triple.  drop: tensor names left out.  Returns ({tensor name: array}, {tensor name: (file, begin, end)})."""
    import json
    import os
    parts = [dict(), dict()]
    tensors = {}
    for i, (name, seed, Mw, K, bits, gs) in enumerate(layers):
        qw, sc, qz = make_gptq(seed, Mw, K, bits, gs, np.float16, hard=False)
        for suffix, a in ((".qweight", qw), (".scales", sc), (".qzeros", qz), (".g_idx", np.arange(K, dtype=np.int32) // gs)):
            if name + suffix not in drop:
                parts[i % 2][name + suffix] = a
                tensors[name + suffix] = a
    parts[0]["model.norm.weight"] = np.ones(8, np.float16)
    parts[1]["lm_head.weight"] = np.ones((4, 8), np.float16)
    where = {}
    for i, p in enumerate(parts):
        fn = os.path.join(d, "model-{:05d}-of-00002.safetensors".format(i + 1))
        for k, (b, e) in write_safetensors(fn, p, dtype_names).items():
            where[k] = (fn, b, e)
    bits = layers[0][4]
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump({"model_type": "llama", "quantization_config": {"bits": bits, "group_size": layers[0][5], "sym": sym, "desc_act": desc_act,
                                                                   "quant_method": quant_method, "meta": {"quantizer": quantizer}}}, f)
    return tensors, where
