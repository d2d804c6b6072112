"""Inputs and references shared by the BitNet master-weight tests (test_bitnet_quant_cpu.py, test_pack_dense_cpu.py,
test_checkpoint_bitnet_cpu.py, test_gpu_bitnet_pack.py): seeded master weights in the three source dtypes, the hand-written table of
rounding ties, and a synthetic checkpoint directory.

A master matrix travels in its STORAGE form: float32, float16, or uint16 holding bf16 bit patterns (numpy has no bfloat16) -- what
``convert.bitnet_absmean_quant`` and ``Weights.from_bitnet`` take.  ``as_f32`` gives the values, exactly.
"""
import json
import os

import numpy as np

import pack_common as pc
from tmac_amd import convert

SRCS = ("f32", "f16", "bf16")
SRC_CODE = {"f32": 0, "f16": 1, "bf16": 2}          # tmac_src_dtype_t
ST_NAME = {"f32": "F32", "f16": "F16", "bf16": "BF16"}


def f32_to_bf16_bits(x):
    """float32 -> the nearest bf16's bits (ties to even); NaN stays NaN"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7FC0), r).astype(np.uint16)


def storage(w, src):
    """float32 values -> the storage form of `src` (rounded to it)"""
    w = np.ascontiguousarray(w, np.float32)
    return w if src == "f32" else w.astype(np.float16) if src == "f16" else f32_to_bf16_bits(w)


def as_f32(stored):
    return convert.bf16_bits_to_f32(stored) if stored.dtype == np.uint16 else stored.astype(np.float32)


def masters(seed, Mw, K, src, m_groups=1, clear_of_ties=False):
    """Master weights like a trained layer's -- N(0, 0.02), each row block at its own magnitude -- in the storage form of `src`.
    clear_of_ties: no |w| / mean|w| of its block within 1e-3 of 0.5 or 1.5 (draw, then push the offenders away), so that float32 and
    float64 arithmetic must give the same levels."""
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((Mw, K)) * 0.02).astype(np.float32)
    w *= (1.0 + np.arange(m_groups, dtype=np.float32))[np.repeat(np.arange(m_groups), Mw // m_groups)][:, None]
    for _ in range(64):
        st = storage(w, src)
        if not clear_of_ties:
            return st
        v = as_f32(st).astype(np.float64).reshape(m_groups, -1)
        r = np.abs(v) / np.abs(v).mean(axis=1)[:, None]
        bad = ((np.abs(r - 0.5) < 2e-3) | (np.abs(r - 1.5) < 2e-3)).reshape(Mw, K)      # pushed to 2e-3, asserted at 1e-3 by the test
        if not bad.any():
            return st
        w = as_f32(st)
        w[bad] *= np.float32(1.03)
    raise AssertionError("could not clear the matrix of ties")


def tie_table(src):
    """(masters in storage form [13], the levels they must get at scale 1.0): halves go to even, so +-0.5 -> 0 and +-1.5 -> +-2 -> +-1
    after the clamp; the neighbours of 0.5 in the dtype fall to either side; -0.0 is 0; infinities clamp; NaN is 0."""
    if src == "f32":
        up, dn = np.nextafter(np.float32(0.5), np.float32(np.inf)), np.nextafter(np.float32(0.5), np.float32(-np.inf))
    elif src == "f16":
        up, dn = np.nextafter(np.float16(0.5), np.float16(np.inf)), np.nextafter(np.float16(0.5), np.float16(-np.inf))
    else:
        up, dn = convert.bf16_bits_to_f32(np.array([0x3F01, 0x3EFF], np.uint16))        # 0.5 is 0x3F00
    rows = [(0.5, 2), (-0.5, 2), (1.5, 3), (-1.5, 1), (2.5, 3), (-2.5, 1), (float(up), 3), (float(dn), 2), (-0.0, 2), (np.inf, 3), (-np.inf, 1),
            (np.nan, 2), (0.25, 2)]
    vals = np.array([v for v, _ in rows], np.float32)
    st = storage(vals, src)
    assert np.array_equal(as_f32(st)[:11], vals[:11]) and np.signbit(as_f32(st)[8]), "every table value is exact in the dtype"
    return st, np.array([lv for _, lv in rows], np.uint8)


def tie_matrix(src, Mw, K):
    """the table tiled into [Mw][K], shifted by one per row so that every value meets every position of a table of four"""
    st, lv = tie_table(src)
    idx = (np.arange(K)[None, :] + np.arange(Mw)[:, None]) % st.size
    return np.ascontiguousarray(st[idx]), np.ascontiguousarray(lv[idx])


def restated_levels(stored, m_groups=1, eps=1e-5):
    """the rule in float64, five lines: the yardstick of convert.bitnet_absmean_quant on matrices clear of ties"""
    w = as_f32(stored).astype(np.float64).reshape(m_groups, -1)
    s = np.maximum(np.abs(w).mean(axis=1), eps)
    t = np.clip(np.round(w / s[:, None]), -1, 1)
    return (t + 2).astype(np.uint8).reshape(stored.shape), s


def host_blob(stored, bm, kfactor, m_groups=1, eps=1e-5, scale=None):
    """(A uint8, S float32, levels) by the host route: the numpy rule, then weights.preprocess_weights"""
    lv, s = convert.bitnet_absmean_quant(stored, m_groups, eps, scale)
    A, S = pc.host_blob_codes(lv, s, None, 2, bm, kfactor)
    return A, S, lv


# ---- a synthetic checkpoint of master weights ---------------------------------------------------------------------------------------
# (name, seed, Mw, K, src): dealt to the two parts in turn
CKPT_LAYERS = [("model.layers.0.self_attn.q_proj", 51, 128, 256, "f16"), ("model.layers.0.mlp.down_proj", 52, 256, 128, "bf16"),
               ("model.layers.1.mlp.gate_proj", 53, 128, 320, "f32")]


def write_bitnet_checkpoint(d, layers=CKPT_LAYERS, weight_bits=1, extra=None, dtype_names=None):
    """A two-part BitNet checkpoint of master weights in directory d, with an embedding (2-D) and norm vectors that are no layers.
    extra: {tensor name: array} added to the first part.  Returns ({tensor name: storage array}, {tensor name: (file, begin, end)})."""
    parts, tensors, names = [dict(), dict()], {}, dict(dtype_names or {})
    parts[0]["model.embed_tokens.weight"] = np.ones((16, 8), np.float16)
    parts[0]["model.layers.0.input_layernorm.weight"] = np.ones(8, np.float16)
    for i, (name, seed, Mw, K, src) in enumerate(layers):
        st = masters(seed, Mw, K, src)
        tensors[name + ".weight"] = st
        # (the writer knows no 16-bit integer: bf16 words travel as fp16 bytes under the name BF16)
        parts[i % 2][name + ".weight"] = st.view(np.float16) if src == "bf16" else st
        if src == "bf16":
            names.setdefault(name + ".weight", "BF16")
    parts[1]["model.norm.weight"] = np.ones(8, np.float16)
    parts[1]["lm_head.weight"] = np.ones((4, 8), np.float16)
    parts[0].update(extra or {})
    where = {}
    for i, p in enumerate(parts):
        fn = os.path.join(d, "model-{:05d}-of-00002.safetensors".format(i + 1))
        for k, (b, e) in pc.write_safetensors(fn, p, names).items():
            where[k] = (fn, b, e)
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump({"model_type": "bitnet", "weight_bits": weight_bits, "input_bits": 8}, f)
    return tensors, where
