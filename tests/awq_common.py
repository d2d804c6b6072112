"""Inputs and host references shared by the AWQ tests (test_awq_*_cpu.py, test_checkpoint_awq_cpu.py, test_gpu_awq_pack.py): seeded
AutoAWQ GEMM tensors, the blob the host route makes of them (convert.unpack_awq + weights.preprocess_weights) and a synthetic two-part
checkpoint."""
import json
import os

import numpy as np

import pack_common as pc
from tmac_amd import convert, weights

# name -> (Mw, K, bm, kfactor, gs, ags): the smallest shapes that cross every boundary of the pack kernel's tiles
#   A  word loads (Mw / 8 = 9 words per row); an 8-row tail in the second 64-row tile; 80 tables = one tile + a tail of 16; five scale groups
#   B  16-byte loads (Mw / 8 = 12: three quads per row), a 32-row tail, the same K tail
#   C  four 64-row tiles -- a whole wide tile -- and two tiles of tables, group size 128
SHAPES = {"A": (72, 320, 96, 8, 64, 32), "B": (96, 320, 128, 16, 64, 64), "C": (256, 512, 256, 16, 128, 64)}


def make_awq(seed, Mw, K, gs, scales_dtype=np.float16, hard=True):
    """(qweight int32 [K][Mw/8], scales [K/gs][Mw], qzeros int32 [K/gs][Mw/8]) and the (w, z) they were packed from.  hard: as
    pack_common.make_gptq -- two scales of 60000 under the lowest and the highest zero code, so a zero overflows fp16"""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 16, size=(Mw, K), dtype=np.uint8)
    z = rng.integers(0, 16, size=(Mw, K // gs), dtype=np.uint8)
    if hard:
        z[0, 0], z[1, 0] = 0, 15
    sc = pc.hard_scales(rng, (Mw, K // gs), np.dtype(scales_dtype).type, hard)
    return convert.pack_awq(w, sc, z), (w, z)


def host_blob(qweight, scales, qzeros, bm, kfactor, zero_point=True):
    """(A uint8, S in the scales' dtype) by the host route; also (w, sc, zr, bits, gs) of the unpacking"""
    with np.errstate(over="ignore"):
        w, sc, zr, bits, gs = convert.unpack_awq(qweight, scales, qzeros)
    A, S = weights.preprocess_weights(w, sc, zr if zero_point else None, bits=bits, bm=bm, kfactor=kfactor)
    return A, S, (w, sc, zr, bits, gs)


def write_awq_checkpoint(d, layers, config=None, drop=(), dtype_names=None, replace=None, biases=()):
    """A two-part AWQ checkpoint in directory d.  layers: [(name, seed, Mw, K, gs)], dealt to the parts in turn; part 0 also holds a norm,
    part 1 a dense lm_head and a dense (not converted) gate.  config: overrides of the quantization_config; drop: tensor names left out;
    replace: {tensor name: array} written instead; biases: layer names that get a fp16 .bias.  Returns {tensor name: array}."""
    parts = [dict(), dict()]
    tensors = {}
    for i, (name, seed, Mw, K, gs) in enumerate(layers):
        (qw, sc, qz), _ = make_awq(seed, Mw, K, gs, np.float16, hard=False)
        named = [(".qweight", qw), (".scales", sc), (".qzeros", qz)]
        if name in biases:
            named.append((".bias", np.random.default_rng(seed + 1000).standard_normal(Mw).astype(np.float16)))
        for suffix, a in named:
            a = (replace or {}).get(name + suffix, a)
            if name + suffix not in drop:
                parts[i % 2][name + suffix] = a
                tensors[name + suffix] = a
    parts[0]["model.norm.weight"] = np.ones(8, np.float16)
    parts[1]["lm_head.weight"] = np.ones((4, 8), np.float16)
    parts[1]["model.layers.0.mlp.gate.weight"] = np.ones((4, 8), np.float16)
    for i, p in enumerate(parts):
        pc.write_safetensors(os.path.join(d, "model-{:05d}-of-00002.safetensors".format(i + 1)), p, dtype_names)
    qc = {"quant_method": "awq", "version": "gemm", "bits": 4, "group_size": layers[0][4], "zero_point": True,
          "modules_to_not_convert": ["mlp.gate"]}
    qc.update(config or {})
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump({"model_type": "qwen2", "quantization_config": qc}, f)
    return tensors
