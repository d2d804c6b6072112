"""Inputs and references shared by the packed ternary BitNet tests (test_bitnet_packed_cpu.py, test_checkpoint_bitnet_packed_cpu.py,
test_gpu_bitnet_packed.py): seeded level matrices with their packed bytes, matrices with a known number of invalid fields, weight_scale
in its three storage forms, and a synthetic checkpoint directory.

The packed bytes come from ``convert.pack_bitnet_packed``, which test_bitnet_packed_cpu.py holds to the bytes of the format's authors
(tests/golden/bitnet/bitnet_packed_ref.npz).
"""
import json
import os

import numpy as np

import bitnet_common as bc
import pack_common as pc
from tmac_amd import convert

pc.ST_DTYPES.setdefault(np.dtype(np.uint8), "U8")       # write_safetensors names a dtype through this table

KF = 16
# (Mw, K, bm, m_groups), R4 = Mw / 4:
#   (128, 256, 128, 1)   R4 = 32: the read-once kernel, the row tail inside a 64-row packed tile, one table tile
#   (160, 3200, 320, 1)  R4 = 40, no multiple of 16: the general kernel is the only route; BitNet's ragged K (12.5 table tiles)
#   (320, 320, 320, 1)   R4 = 80: read-once with a second, short packed-row tile (64 + 16) and a short table tile (64 + 16)
#   (256, 1024, 128, 2)  two scales; the fields cross the scale blocks
#   (640, 2560, 128, 1)  a k/v projection of bitnet-b1.58-2B-4T
SHAPES = [(128, 256, 128, 1), (160, 3200, 320, 1), (320, 320, 320, 1), (256, 1024, 128, 2), (640, 2560, 128, 1)]
LINEAR_CLASSES = ("autobitlinear", "bitlinear")


def reads_once(Mw):
    return (Mw // 4) % 16 == 0


def levels(seed, Mw, K):
    """(levels uint8 [Mw][K] in {1, 2, 3}, their packed bytes uint8 [Mw/4][K])"""
    lv = np.random.default_rng(seed).integers(1, 4, size=(Mw, K), dtype=np.uint8)
    return lv, convert.pack_bitnet_packed(lv)


def scales(m_groups):
    """fp32 [m_groups] unified scales, none of them a power of two"""
    return (np.float32(0.0371) * (1.0 + np.arange(m_groups, dtype=np.float32))).astype(np.float32)


def with_invalid(seed, Mw, K, n):
    """(packed bytes with exactly n fields of value 3, the levels they must give): the 3s are dealt over all four fields and over the
    whole matrix -- rows and columns drawn from everywhere, so that with 64 x 256-value tiles several workgroups meet some"""
    rng = np.random.default_rng(seed)
    lv, packed = levels(seed, Mw, K)
    R4 = Mw // 4
    flat = rng.choice(Mw * K, size=n, replace=False)
    flat[:4] = [f * R4 * K + (f * 7) % K for f in range(4)]              # every field at least once (row f R4, distinct columns)
    flat = np.unique(flat)
    o, k = flat // K, flat % K
    packed = packed.copy()
    np.bitwise_or.at(packed, (o % R4, k), (3 << (2 * (o // R4))).astype(np.uint8))      # (.at: two fields of one byte may both be hit)
    lv = lv.copy()
    lv[o, k] = 3
    return packed, lv, int(flat.size)


def scale_forms(value):
    """{name: (stored one-element array as the checkpoint holds it, its exact float32 value)}; uint16 = bf16 bit patterns"""
    v = np.float32(value)
    h = np.array([v], np.float16)
    b = bc.f32_to_bf16_bits(np.array([v], np.float32))
    return {"f32": (np.array([v], np.float32), v), "f16": (h, np.float32(h[0])), "bf16": (b, convert.bf16_bits_to_f32(b)[0])}


# ---- a synthetic checkpoint of packed ternary weights -------------------------------------------------------------------------------
# (name, seed, Mw, K, scale form, scale shape, weight_scale value): dealt to the two parts in turn
CKPT_LAYERS = [("model.layers.0.self_attn.q_proj", 61, 128, 256, "bf16", (1,), 1.6875), ("model.layers.0.mlp.down_proj", 62, 256, 128, "f16", (), 0.73),
               ("model.layers.1.mlp.gate_proj", 63, 160, 320, "f32", (1,), 2.3)]


def write_packed_checkpoint(d, layers=CKPT_LAYERS, quantization_config="default", linear_class="autobitlinear", extra=None, drop=(), dtype_names=None):
    """A two-part packed BitNet checkpoint in directory d, with an embedding, norms and a bf16 lm_head that are no layers.
    quantization_config: the dict written to config.json ("default": quant_method bitnet, offline, the given linear_class -- None leaves
    the field out).  extra: {tensor name: array} added to the first part; drop: tensor names left out.
    Returns ({layer name: (levels, packed, stored scale, its float32 value)}, {tensor name: (file, begin, end)})."""
    parts, out, names = [dict(), dict()], {}, dict(dtype_names or {})
    parts[0]["model.embed_tokens.weight"] = np.ones((16, 8), np.float16)
    names.setdefault("model.embed_tokens.weight", "BF16")
    parts[0]["model.layers.0.input_layernorm.weight"] = np.ones(8, np.float16)
    for i, (name, seed, Mw, K, form, shape, value) in enumerate(layers):
        lv, packed = levels(seed, Mw, K)
        stored, v = scale_forms(value)[form]
        out[name] = (lv, packed, stored, v)
        parts[i % 2][name + ".weight"] = packed
        # (the writer knows no 16-bit integer: bf16 words travel as fp16 bytes under the name BF16)
        parts[i % 2][name + ".weight_scale"] = (stored.view(np.float16) if form == "bf16" else stored).reshape(shape)
        if form == "bf16":
            names.setdefault(name + ".weight_scale", "BF16")
    parts[1]["model.norm.weight"] = np.ones(8, np.float16)
    parts[1]["lm_head.weight"] = np.ones((4, 8), np.float16)
    names.setdefault("lm_head.weight", "BF16")
    parts[0].update(extra or {})
    for k in extra or {}:                                   # an extra tensor is named after its own dtype unless the caller says otherwise
        if k not in (dtype_names or {}):
            names.pop(k, None)
    for p in parts:
        for k in drop:
            p.pop(k, None)
    where = {}
    for i, p in enumerate(parts):
        fn = os.path.join(d, "model-{:05d}-of-00002.safetensors".format(i + 1))
        for k, (b, e) in pc.write_safetensors(fn, p, names).items():
            where[k] = (fn, b, e)
    if quantization_config == "default":
        quantization_config = {"quant_method": "bitnet", "quantization_mode": "offline", "modules_to_not_convert": ["lm_head"], "use_rms_norm": False,
                               "rms_norm_eps": 1e-6}
        if linear_class is not None:
            quantization_config["linear_class"] = linear_class
    cfg = {"model_type": "bitnet", "weight_bits": 1, "input_bits": 8}
    if quantization_config is not None:
        cfg["quantization_config"] = quantization_config
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(cfg, f)
    return out, where
