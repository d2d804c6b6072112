"""Inputs and references shared by the round-to-nearest tests (test_rtn_quant_cpu.py, test_pack_rtn_cpu.py, test_checkpoint_dense_cpu.py,
test_gpu_rtn_pack.py): seeded dense matrices in the three source dtypes, a float64 restatement of the rule, the hand-built table of
rounding ties, the edge groups, and a synthetic unquantised checkpoint.

A matrix travels in its STORAGE form, as in bitnet_common: float32, float16, or uint16 holding bf16 bit patterns.
"""
import json
import os

import numpy as np

import bitnet_common as bc
import pack_common as pc
from tmac_amd import convert

SRCS = bc.SRCS
SRC_CODE = bc.SRC_CODE
storage, as_f32 = bc.storage, bc.as_f32


def masters(seed, Mw, K, src):
    """weights like a trained layer's -- N(0, 0.02) with a few outliers, every row at its own magnitude and offset, so that groups are
    not centred on 0 -- in the storage form of `src`"""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal((Mw, K)) * 0.02
    w[rng.random((Mw, K)) < 0.002] *= 6.0
    w = w * (0.5 + rng.random((Mw, 1)) * 2.0) + (rng.random((Mw, 1)) - 0.5) * 0.01
    return storage(w.astype(np.float32), src)


def restated(stored, bits, gs, zero_point):
    """The rule in float64, as GPTQ's Quantizer states it: (real-valued quotient w / scale + zq BEFORE rounding [Mw][K], scale [Mw][SG],
    real-valued -lo / scale [Mw][SG]).  Finite masters only."""
    w = as_f32(stored).astype(np.float64)
    Mw, K = w.shape
    g = w.reshape(Mw, K // gs, gs)
    lo, hi = np.minimum(g.min(axis=2), 0.0), np.maximum(g.max(axis=2), 0.0)
    maxq = 2 ** bits - 1
    if not zero_point:
        hi = np.maximum(np.abs(lo), hi)
        lo = -hi
    flat = (lo == 0) & (hi == 0)
    lo, hi = np.where(flat, -1.0, lo), np.where(flat, 1.0, hi)
    s = (hi - lo) / maxq
    z = -lo / s if zero_point else np.full(s.shape, 2.0 ** (bits - 1))
    return g / s[:, :, None], s, z


def half(k):
    """round half to even of an exact k + 0.5 or integer: Python's round, an implementation numpy's rint does not share"""
    return float(round(k))


def tie_groups(bits, zero_point, gs=64):
    """[(group float32 [gs], scale, zq, codes uint8 [gs])]: groups whose scale is a power of two, 2^e, so that every w / scale -- and,
    with zero points, -lo / scale -- is exactly an integer or an integer and a half.  The expected values are written down with Python's
    round (halves to even) and a clamp; every value is a small dyadic rational, exact in fp32, fp16 and bf16."""
    maxq = 2 ** bits - 1
    out = []
    for e in (-3, 0, 2):
        s = 2.0 ** e
        if zero_point:
            shifts = [a + 0.5 for a in range(0, maxq)] + [0.0, float(maxq), float(maxq // 2)]
        else:
            shifts = [maxq / 2.0]                                  # lo = -hi, hi = maxq / 2 * scale
        for a in shifts:
            lo, hi = -a * s, (maxq - a) * s
            zq = half(a) if zero_point else float(2 ** (bits - 1))
            # every multiple of scale / 2 inside [lo, hi], ends included: the integers and all the ties
            q = np.arange(int(round(-2 * a)), int(round(2 * (maxq - a))) + 1) / 2.0
            vals = np.concatenate([[lo, hi], q * s])
            assert vals.size <= gs and vals.min() == lo and vals.max() == hi
            grp = np.zeros(gs, np.float32)
            grp[:vals.size] = vals
            codes = np.array([min(max(half(float(v) / s) + zq, 0.0), float(maxq)) for v in grp], np.uint8)
            out.append((grp, np.float32(s), np.float32(zq), codes))
    return out


def tie_matrix(bits, zero_point, Mw, K, gs=64):
    """the tie groups dealt round-robin over a [Mw][K] matrix, each group rotated by its index so that every value meets every position of
    a table of four: (float32 matrix, scales [Mw][SG], zq [Mw][SG], codes [Mw][K])"""
    groups = tie_groups(bits, zero_point, gs)
    SG = K // gs
    w = np.zeros((Mw, SG, gs), np.float32)
    sc, zq, cd = np.zeros((Mw, SG), np.float32), np.zeros((Mw, SG), np.float32), np.zeros((Mw, SG, gs), np.uint8)
    for i in range(Mw * SG):
        grp, s, z, codes = groups[i % len(groups)]
        o, sg = divmod(i, SG)
        w[o, sg], sc[o, sg], zq[o, sg], cd[o, sg] = np.roll(grp, i), s, z, np.roll(codes, i)
    return w.reshape(Mw, K), sc, zq, cd.reshape(Mw, K)


def edge_matrix(src, Mw, K, gs=64):
    """A matrix of edge groups, in the storage form of `src`, dealt round-robin: all zero; all positive; all negative; one non-zero
    value; -0.0 alone; the largest finite values of the dtype at both ends (fp32: hi - lo overflows, the group is invalid; fp16: a scale
    beyond fp16's range where the scale is rounded to it); fp16 subnormals -- multiples of 2^-24 -- with a scale that is one too; a
    range so small that the fp32 scale is subnormal (fp32 and bf16 only: the all-zero group's parameters)."""
    rng = np.random.default_rng(5)
    groups = [np.zeros(gs), np.abs(rng.standard_normal(gs)) + 0.1, -np.abs(rng.standard_normal(gs)) - 0.1, np.eye(1, gs, 7)[0] * 0.3,
              np.full(gs, -0.0), rng.integers(0, 1024, gs) * 2.0 ** -24, rng.integers(-512, 512, gs) * 2.0 ** -24]
    big = {"f32": 3.0e38, "f16": 65504.0, "bf16": 3.0e38}[src]
    ends = np.zeros(gs)
    ends[3], ends[9] = -big, big
    groups.append(ends)
    if src != "f16":
        groups.append(rng.standard_normal(gs) * 1e-39)
    SG = K // gs
    w = np.zeros((Mw, SG, gs), np.float32)
    for i in range(Mw * SG):
        o, sg = divmod(i, SG)
        w[o, sg] = np.roll(groups[i % len(groups)], i).astype(np.float32)
    return storage(w.reshape(Mw, K), src)


def host_blob(stored, bits, gs, zero_point, scale_f16, bm, kfactor, out_dtype=np.float32):
    """(A uint8, S, codes, scales, zeros) by the host route: the numpy rule, then weights.preprocess_weights"""
    codes, sc, zr = convert.rtn_quant(stored, bits, gs, zero_point, scale_f16)
    with np.errstate(over="ignore"):
        A, S = pc.host_blob_codes(codes, sc.astype(out_dtype), None if zr is None else zr.astype(out_dtype), bits, bm, kfactor)
    return A, S, codes, sc, zr


# ---- a synthetic unquantised checkpoint -----------------------------------------------------------------------------------------------
# (name, seed, Mw, K, src): dealt to the two parts in turn
CKPT_LAYERS = [("model.layers.0.self_attn.q_proj", 61, 128, 256, "f16"), ("model.layers.0.mlp.down_proj", 62, 256, 128, "bf16"),
               ("model.layers.1.mlp.gate_proj", 63, 128, 384, "f32")]


def write_dense_checkpoint(d, layers=CKPT_LAYERS, config=None, extra=None, dtype_names=None):
    """A two-part unquantised checkpoint in directory d, with an embedding (2-D), norm vectors and a head that are no layers.  config:
    the contents of config.json (None: an ordinary model's; False: no file).  extra: {tensor name: array} added to the first part.
    Returns ({tensor name: storage array}, {tensor name: (file, begin, end)})."""
    parts, tensors, names = [dict(), dict()], {}, dict(dtype_names or {})
    parts[0]["model.embed_tokens.weight"] = np.ones((16, 8), np.float16)
    parts[0]["model.layers.0.input_layernorm.weight"] = np.ones(8, np.float16)
    for i, (name, seed, Mw, K, src) in enumerate(layers):
        st = masters(seed, Mw, K, src)
        tensors[name + ".weight"] = st
        parts[i % 2][name + ".weight"] = st.view(np.float16) if src == "bf16" else st       # bf16 words travel as fp16 bytes under the name BF16
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
    if config is not False:
        with open(os.path.join(d, "config.json"), "w") as f:
            json.dump(config if config is not None else {"model_type": "llama", "torch_dtype": "float16"}, f)
    return tensors, where
