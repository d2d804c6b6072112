"""Checkpoint-side data formats of the T-MAC hot path: what sits on either side of
``tmac_hip_register_weights``.

* GPTQ (v1 / v2) packed tensors -> biased uint weights, scales, T-MAC zeros      (``python/t_mac/model_utils.py:95-129``)
* AutoAWQ (GEMM version, 4 bits) packed tensors -> the same four things (``unpack_awq``; the format is restated above it: nothing of
  AutoAWQ is needed)
* ``kcfg.ini`` emission for a set of (bits, M, K, N, m_groups) kernels           (``deploy/compile.py:153-165``; the
  file the converter and the runtime must share because bm / kfactor are baked into the weight bytes)
* the per-tensor blob a T-MAC GGUF stores: ``[permuted weight bytes][fp32 scales]`` (``model_utils.py:243-271``), and
  its inverse split for registration on the GPU

Nothing here touches a GPU: numpy in, numpy out.  Results are identical to the reference's functions (tests compare
them against the reference's Python, which imports without TVM).  One exception, named for it: ``preprocess_for_t_mac_gpu``
produces the same blob from the packed GPTQ tensors on the GPU; the numpy functions are its reference.
"""
import configparser
import os
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from .weights import preprocess_weights

# (bits, M = weight rows, K, N, m_groups) per preset, as the reference ships them (model_utils.py:20-89)
PRESET_KERNELS: Dict[str, List[List[int]]] = {
    "llama-2-7b-4bit": [[4, 4096, 4096, 1, -1], [4, 11008, 4096, 1, -1], [4, 4096, 11008, 1, -1]],
    "llama-2-7b-2bit": [[2, 4096, 4096, 1, -1], [2, 11008, 4096, 1, -1], [2, 4096, 11008, 1, -1]],
    "llama-2-13b-2bit": [[2, 5120, 5120, 1, -1], [2, 13824, 5120, 1, -1], [2, 5120, 13824, 1, -1]],
    "llama-3-8b-2bit": [[2, 4096, 4096, 1, -1], [2, 14336, 4096, 1, -1], [2, 4096, 14336, 1, -1], [2, 1024, 4096, 1, -1]],
    "llama-3-8b-4bit": [[4, 4096, 4096, 1, -1], [4, 14336, 4096, 1, -1], [4, 4096, 14336, 1, -1], [4, 1024, 4096, 1, -1]],
    "hf-bitnet-3b": [[2, 3200, 8640, 1, 1], [2, 8640, 3200, 1, 1], [2, 3200, 3200, 1, 1]],
    "hf-bitnet-large-intn": [[2, 1536, 4096, 1, 1], [2, 4096, 1536, 1, 1], [2, 1536, 1536, 1, 1]],
    "hf-bitnet-large-tq": [[2, 1536, 4096, 1, -1], [2, 4096, 1536, 1, -1], [2, 1536, 1536, 1, -1]],
    "ms-bitnet-3b": [[2, 3200, 800, 1, 1], [2, 3200, 3200, 1, 1], [2, 3200, 10240, 1, 1], [2, 10240, 3200, 1, 1], [2, 800, 3200, 1, 1]],
    "phi-3-mini-2bit": [[2, 3072, 3072, 1, -1], [2, 9216, 3072, 1, -1], [2, 3072, 8192, 1, -1], [2, 16384, 3072, 1, -1]],
    "trilm-3.9b": [[2, 3072, 3072, 1, -1], [2, 3072, 9216, 1, -1], [2, 9216, 3072, 1, -1], [2, 768, 3072, 1, -1]],
    "test": [],
    "gptq-auto": [],            # shapes read from the checkpoint (extract_kernel_shapes)
}


def get_preset_models() -> List[str]:
    return list(PRESET_KERNELS.keys())


def _safetensors_shapes(path: str) -> Dict[str, Tuple[str, Tuple[int, ...]]]:
    """{tensor name: (dtype, shape)} from a .safetensors file's header alone (8-byte little-endian length + JSON): a 7B checkpoint's kernel
    shapes are known after reading a few hundred KB, no tensor is loaded (the reference reads every scales / qzeros / qweight tensor)"""
    import json
    import struct
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.read(8)
        if len(head) != 8:
            raise RuntimeError("{}: not a safetensors file (shorter than its header length field)".format(path))
        (n,) = struct.unpack("<Q", head)
        if n == 0 or n > size - 8:
            raise RuntimeError("{}: corrupt safetensors header (length {} in a file of {} bytes)".format(path, n, size))
        try:
            hdr = json.loads(f.read(n))
            return {k: (v["dtype"], tuple(int(d) for d in v["shape"])) for k, v in hdr.items() if k != "__metadata__"}
        except (ValueError, KeyError, TypeError) as e:
            raise RuntimeError("{}: corrupt safetensors header ({})".format(path, e))


def extract_kernel_shapes(model_arch: Optional[str] = "gptq-auto", model_dir: Optional[str] = None) -> List[List[int]]:
    """The kernels a model needs, [bits, M, K, N, m_groups] each (``model_utils.py:206-216``): a preset's list, or -- "gptq-auto" -- the distinct
    (bits, M, K) of the GPTQ-packed linear layers found in the checkpoint's ``model*.safetensors`` parts, in order of first appearance.
    One group size per model, as the reference requires (``model_utils.py:170-198``); ``checkpoint_group_size`` returns it."""
    if model_arch not in PRESET_KERNELS:
        raise KeyError("Unsupported model_arch: {}".format(model_arch))
    if model_arch != "gptq-auto":
        return [list(k) for k in PRESET_KERNELS[model_arch]]
    return _scan_checkpoint(model_dir)[0]


def checkpoint_group_size(model_dir: str) -> int:
    return _scan_checkpoint(model_dir)[1]


def _scan_checkpoint(model_dir: Optional[str]) -> Tuple[List[List[int]], int]:
    if model_dir is None:
        raise ValueError("gptq-auto needs the checkpoint directory")
    parts = sorted(f for f in os.listdir(model_dir) if f.startswith("model") and f.endswith(".safetensors"))
    if not parts:
        raise RuntimeError("Models in {} not in GPTQ safetensors format (torch .bin checkpoints: convert them to safetensors first)".format(model_dir))
    shapes: Dict[str, Tuple[int, ...]] = {}
    order: List[str] = []
    for part in parts:
        for name, (_, shp) in _safetensors_shapes(os.path.join(model_dir, part)).items():
            shapes[name] = shp
            if name.endswith(".qweight"):
                order.append(name)
    ks: List[List[int]] = []
    gs_all = None
    for name in order:
        qw, sc, qz = shapes[name], shapes.get(name[:-8] + ".scales"), shapes.get(name[:-8] + ".qzeros")
        if sc is None or qz is None:
            raise RuntimeError("{}: scales / qzeros missing".format(name))
        if len(qw) != 2 or len(sc) != 2 or len(qz) != 2 or qz[1] <= 0 or sc[0] <= 0 or sc[1] < qz[1]:
            raise RuntimeError("{}: qweight {} / scales {} / qzeros {} are not GPTQ-packed shapes".format(name, qw, sc, qz))
        bits = 32 // (sc[1] // qz[1])                      # parse_gptq on shapes alone
        if bits not in (1, 2, 3, 4, 8):
            raise RuntimeError("{}: {} values per packed word".format(name, sc[1] // qz[1]))
        K, M = qw[0] * (32 // bits), qw[1]
        gs = K // sc[0]
        if [bits, M, K, 1, -1] not in ks:
            ks.append([bits, M, K, 1, -1])
        if gs_all is None:
            gs_all = gs
        elif gs_all != gs:
            raise RuntimeError("Different group_sizes unsupported")
    if not ks:
        raise RuntimeError("Models in {} not in GPTQ format".format(model_dir))
    return ks, int(gs_all)


def get_quantization_config(model_dir: str, allow_desc_act: bool = False) -> dict:
    """what the pipeline reads from a checkpoint's config.json (``model_utils.py:219-240``): GPTQ fields of ``quantization_config`` and
    BitNet's ``weight_bits``; act-order checkpoints (desc_act) are refused as the reference refuses them -- unless ``allow_desc_act``:
    the device-side registration takes them (``checkpoint.load_gptq_dir(..., act_order=True)``), and the result then says ``desc_act``"""
    import json
    with open(os.path.join(model_dir, "config.json"), "r", encoding="utf-8") as f:
        hp = json.load(f)
    qc = hp.get("quantization_config", {})
    if qc.get("desc_act", False) and not allow_desc_act:
        raise AssertionError("desc_act=True currently unsupported by T-MAC")
    extra = {"desc_act": bool(qc.get("desc_act", False))} if allow_desc_act else {}
    return {**extra, "quantizer": qc.get("meta", {}).get("quantizer", ""), "group_size": qc.get("group_size", 0), "bits": qc.get("bits", 0),
            "sym": qc.get("sym", False), "quant_method": qc.get("quant_method", ""), "weight_bits": hp.get("weight_bits", 0)}


def parse_gptq(qweight: np.ndarray, scales: np.ndarray, qzeros: np.ndarray) -> Tuple[int, int, int, int]:
    """(K, M, bits, group_size) from the packed tensor shapes: qweight int32 [K*bits/32][M], scales [K/gs][M],
    qzeros int32 [K/gs][M*bits/32]."""
    bits = 32 // (scales.shape[1] // qzeros.shape[1])
    K = qweight.shape[0] * (32 // bits)
    M = qweight.shape[1]
    return K, M, bits, K // scales.shape[0]


def _unpack_fields(x: np.ndarray, bits: int) -> np.ndarray:
    """int32 [...] -> [..., 32/bits] little-end-first bit fields"""
    shifts = np.arange(0, 32, bits, dtype=np.uint32)
    return ((x.astype(np.uint32)[..., None] >> shifts) & np.uint32((1 << bits) - 1)).astype(np.uint8)


def unpack_gptq(qweight: np.ndarray, scales: np.ndarray, qzeros: np.ndarray, gptq_v2: bool = True):
    """GPTQ tensors -> (w uint8 [M][K] in [0, 2^bits), scales [M][K/gs], zeros [M][K/gs], bits, group_size) with the
    zeros already in T-MAC's convention ``(z - 2^(bits-1)) * scale`` (``weights.py:29-31``); AutoGPTQ v1 stores z - 1."""
    if qweight.dtype != np.int32 or qzeros.dtype != np.int32:
        raise TypeError("qweight and qzeros must be int32")
    K, M, bits, gs = parse_gptq(qweight, scales, qzeros)
    # qweight[kp][m] packs rows kp*(32/bits) .. +32/bits-1 of column m
    w = _unpack_fields(qweight, bits).transpose(1, 0, 2).reshape(M, K)
    sc = np.ascontiguousarray(scales.T)
    z = _unpack_fields(qzeros, bits).reshape(K // gs, M).T.astype(sc.dtype)
    if not gptq_v2:
        z = z + 1
    return np.ascontiguousarray(w), sc, (z - (2 ** (bits - 1))) * sc, bits, gs


# AutoAWQ, WQLinear_GEMM (quantization_config.version "gemm"), 4 bits: eight fields per int32 word, packed along the OUTPUT axis.
# Field i (bits 4i .. 4i+3) of qweight[k][c] holds the code of weight row 8c + AWQ_ORDER[i] at column k; row 8c + j sits in field
# AWQ_INV[j].  qzeros the same.  Known answer: the word 0x76543210 gives rows 8c .. 8c+7 the codes 0, 4, 1, 5, 2, 6, 3, 7.
AWQ_ORDER = (0, 2, 4, 6, 1, 3, 5, 7)
AWQ_INV = (0, 4, 1, 5, 2, 6, 3, 7)


def parse_awq(qweight, scales, qzeros) -> Tuple[int, int, int, int]:
    """(K, M, bits = 4, group_size) from the AWQ tensor shapes: qweight int32 [K][M/8], scales [K/gs][M], qzeros int32 [K/gs][M/8]"""
    K, M = int(qweight.shape[0]), int(scales.shape[1])
    if len(qweight.shape) != 2 or len(scales.shape) != 2 or int(qweight.shape[1]) * 8 != M or int(scales.shape[0]) <= 0 or K % int(scales.shape[0]) or \
            (qzeros is not None and tuple(int(d) for d in qzeros.shape) != (int(scales.shape[0]), M // 8)):
        raise ValueError("qweight {} / scales {} / qzeros {} are not AWQ (GEMM, 4-bit) shapes: [K][M/8], [K/gs][M], [K/gs][M/8]".format(
            tuple(qweight.shape), tuple(scales.shape), None if qzeros is None else tuple(qzeros.shape)))
    return K, M, 4, K // int(scales.shape[0])


def _unpack_awq_fields(x: np.ndarray) -> np.ndarray:
    """int32 [R][C] -> uint8 [R][8 C]: column 8c + j is field AWQ_INV[j] of word c"""
    f = _unpack_fields(x, 4)                                      # [R][C][8], field order
    return np.ascontiguousarray(f[..., list(AWQ_INV)]).reshape(x.shape[0], -1)


def unpack_awq(qweight: np.ndarray, scales: np.ndarray, qzeros: np.ndarray):
    """AutoAWQ GEMM tensors -> (w uint8 [M][K] in [0, 16), scales [M][K/gs], zeros [M][K/gs], 4, group_size): what ``unpack_gptq`` returns.
    AWQ dequantises ``(q - z) * s`` with the stored z as it is, so the codes are T-MAC's and the zeros are ``(z - 8) * scale`` in the
    scales' dtype (``weights.py:29-31``).  The host reference of ``tmac_hip_pack_awq_dev`` / ``Weights.from_awq``, never the route."""
    if qzeros is None:
        raise ValueError("qzeros is None: AWQ without zero points (symmetric AWQ) is not served")
    if qweight.dtype != np.int32 or qzeros.dtype != np.int32:
        raise TypeError("qweight and qzeros must be int32")
    K, M, bits, gs = parse_awq(qweight, scales, qzeros)
    w = _unpack_awq_fields(qweight).T                             # [K][M] -> [M][K]
    sc = np.ascontiguousarray(scales.T)
    z = _unpack_awq_fields(qzeros).T.astype(sc.dtype)
    return np.ascontiguousarray(w), sc, (z - 8) * sc, bits, gs


def pack_awq(w: np.ndarray, scales: np.ndarray, z: np.ndarray):
    """The inverse of ``unpack_awq`` (tests, fixtures, the benchmark tool): codes uint8 [M][K] in [0, 16), scales [M][K/gs] and the
    integer zero points z uint8 [M][K/gs] in [0, 16) -- ``unpack_awq``'s zeros are ``(z - 8) * scales`` -- -> (qweight int32 [K][M/8],
    scales [K/gs][M], qzeros int32 [K/gs][M/8])."""
    w, z = np.asarray(w), np.asarray(z)
    if w.ndim != 2 or w.shape[0] % 8 or z.ndim != 2 or z.shape[0] != w.shape[0] or tuple(scales.shape) != tuple(z.shape) or max(int(w.max()), int(z.max())) > 15:
        raise ValueError("w is [M][K] and z [M][K/gs], both in [0, 16), M a multiple of 8; scales is [M][K/gs]")

    def fields(a):                                                # uint8 [M][C] -> int32 [C][M/8]
        f = a.T.reshape(a.shape[1], a.shape[0] // 8, 8)[..., list(AWQ_ORDER)].astype(np.uint32)      # field i takes row 8c + ORDER[i]
        return (f << (np.arange(8, dtype=np.uint32) * np.uint32(4))).sum(axis=-1, dtype=np.uint32).view(np.int32)

    return np.ascontiguousarray(fields(w)), np.ascontiguousarray(np.asarray(scales).T), np.ascontiguousarray(fields(z))


def bf16_bits_to_f32(bits: np.ndarray) -> np.ndarray:
    """uint16 bf16 bit patterns -> float32, exactly (the bits shifted left by 16; numpy has no bfloat16)"""
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def bitnet_absmean_quant(w: np.ndarray, m_groups: int = 1, eps: float = 1e-5, scale=None) -> Tuple[np.ndarray, np.ndarray]:
    """BitNet b1.58 master weights [Mw][K] -> (levels uint8 [Mw][K] in {1, 2, 3}, scales float32 [m_groups]) by the absmean rule of the
    paper and of the checkpoint authors' modelling code (``1 / mean|W|.clamp(min=1e-5)``, round, clamp to [-1, 1]): the host reference
    of ``tmac_hip_pack_absmean_dev`` (include/tmac_hip.h states the rule operation by operation).  ``w``: float32, float16, or uint16
    holding bf16 bit patterns.  One scale per block of Mw / m_groups rows: ``max(float32(mean |w|), eps)`` with the mean in float64, or
    ``scale`` (a float or [m_groups] values) as it is.  The element-wise part is float32: ``rint(w * (1 / s))`` -- halves to even --
    clamped to [-1, 1], a NaN product 0; level = that + 2, so ``w_real = (level - 2) * s``."""
    w = np.asarray(w)
    if w.dtype == np.uint16:
        w = bf16_bits_to_f32(w)
    elif w.dtype not in (np.float32, np.float16):
        raise TypeError("w must be float32, float16 or uint16 (bf16 bit patterns)")
    if w.ndim != 2 or m_groups < 1 or w.shape[0] % m_groups:
        raise ValueError("w is [Mw][K] with Mw a multiple of m_groups >= 1")
    Mw, K = w.shape
    eps = np.float32(eps)
    if not np.isfinite(eps) or not eps > 0:
        raise ValueError("eps must be finite and > 0")
    if scale is None:
        with np.errstate(invalid="ignore", over="ignore"):
            gamma = np.abs(w.astype(np.float64)).reshape(m_groups, -1).sum(axis=1) / float(Mw // m_groups * K)
            s = np.fmax(gamma.astype(np.float32), eps)               # fmaxf: a NaN mean gives eps
    else:
        s = np.broadcast_to(np.asarray(scale, np.float32).reshape(-1), (m_groups,)).copy()
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        inv = np.float32(1.0) / s                                    # float32 / float32, correctly rounded
        q = w.astype(np.float32).reshape(m_groups, -1) * inv[:, None]
        t = np.where(np.isnan(q), np.float32(0.0), np.clip(np.rint(q), np.float32(-1.0), np.float32(1.0)))
    return (t.astype(np.int8) + 2).astype(np.uint8).reshape(Mw, K), s.astype(np.float32)


def _masters_f32(w: np.ndarray) -> np.ndarray:
    """master weights in their storage form (float32, float16, uint16 = bf16 bit patterns) -> float32, exactly"""
    w = np.asarray(w)
    if w.dtype == np.uint16:
        return bf16_bits_to_f32(w)
    if w.dtype not in (np.float32, np.float16):
        raise TypeError("w must be float32, float16 or uint16 (bf16 bit patterns)")
    return w.astype(np.float32)


def rtn_params(w: np.ndarray, bits: int, group_size: int, zero_point: bool = True, scale_f16: bool = False):
    """The parameters of ``rtn_quant``: (scales float32 [Mw][K/gs], zq float32 [Mw][K/gs] -- the zero CODE, an integer value --, invalid:
    bool [Mw][K/gs]).  The host reference of ``tmac_hip_rtn_params_dev``; include/tmac_hip.h states the rule operation by operation.  An
    invalid group -- a master that is not finite, or a scale that is 0 or not finite (``scale_f16``: after its rounding to float16) --
    carries the parameters of the all-zero group."""
    w = _masters_f32(w)
    if w.ndim != 2 or not 1 <= bits <= 4 or group_size <= 0 or group_size % 4 or w.shape[1] % group_size:
        raise ValueError("w is [Mw][K], bits 1 to 4, group_size a positive multiple of 4 that divides K")
    Mw, K = w.shape
    g = w.reshape(Mw, K // group_size, group_size)
    f32 = np.float32
    maxq, one = f32(2 ** bits - 1), f32(1.0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        finite = np.isfinite(g).all(axis=2)
        lo = np.where(finite, np.fmin(np.fmin.reduce(g, axis=2), f32(0.0)), f32(0.0))       # fmin / fmax: a NaN is dropped
        hi = np.where(finite, np.fmax(np.fmax.reduce(g, axis=2), f32(0.0)), f32(0.0))
        if not zero_point:
            hi = np.fmax(np.abs(lo), hi)
            lo = -hi
        flat = (lo == 0) & (hi == 0)
        lo, hi = np.where(flat, -one, lo), np.where(flat, one, hi)
        s = ((hi - lo) / maxq).astype(f32)
        tiny = s < np.finfo(f32).tiny
        lo, hi, s = np.where(tiny, -one, lo), np.where(tiny, one, hi), np.where(tiny, f32(2.0) / maxq, s).astype(f32)
        if scale_f16:
            s = s.astype(np.float16).astype(f32)
        ok = finite & (s != 0) & np.isfinite(s)
        s0 = f32(2.0) / maxq
        if scale_f16:
            s0 = f32(np.float16(s0))
        lo, s = np.where(ok, lo, -one).astype(f32), np.where(ok, s, s0).astype(f32)
        zq = (np.rint((-lo) / s) + f32(0.0)).astype(f32) if zero_point else np.full(s.shape, 2 ** (bits - 1), f32)
    return s, zq, ~ok


def rtn_quant(w: np.ndarray, bits: int, group_size: int, zero_point: bool = True, scale_f16: bool = False):
    """Dense master weights [Mw][K] (float32, float16, or uint16 holding bf16 bit patterns) -> (codes uint8 [Mw][K] in [0, 2^bits),
    scales float32 [Mw][K/gs], zeros float32 [Mw][K/gs] in T-MAC's convention -- what ``Weights.from_codes`` takes; zeros None without
    zero points) by per-group round to nearest: GPTQ's quantiser without the error search (``Quantizer.find_params`` with ``mse=False``,
    then ``quantize``).  The host reference of ``tmac_hip_pack_rtn_dev`` and ``Weights.from_dense``, never the route.  Everything is
    float32, one correctly rounded operation per step, in the device's order: ``scale = (hi - lo) / maxq`` from the group's minimum and
    maximum (each taken with 0; symmetric about 0 without zero points), ``zq = rint(-lo / scale)`` (2^(bits-1) without zero points),
    ``code = clip(rint(w / scale) + zq, 0, maxq)``, ``zero = (zq - 2^(bits-1)) * scale``, so ``w_real = (code - zq) * scale``.
    ``scale_f16``: the scale is rounded to float16 BEFORE zq and the codes are derived (a handle that stores fp16 scales).  Invalid groups
    (``rtn_params``) get the all-zero group's parameters; ``rtn_invalid`` counts them."""
    s, zq, _ = rtn_params(w, bits, group_size, zero_point, scale_f16)
    w = _masters_f32(w)
    Mw, K = w.shape
    f32 = np.float32
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        q = np.rint(w.reshape(Mw, -1, group_size) / s[:, :, None]) + zq[:, :, None]
        codes = np.fmin(np.fmax(q, f32(0.0)), f32(2 ** bits - 1)).astype(np.uint8).reshape(Mw, K)       # fmax: a NaN gives 0
        zeros = ((zq - f32(2 ** (bits - 1))) * s).astype(f32) if zero_point else None
    return codes, s, zeros


def rtn_invalid(w: np.ndarray, bits: int, group_size: int, zero_point: bool = True, scale_f16: bool = False) -> int:
    """how many (row, group) pairs ``rtn_params`` calls invalid: what ``Weights.from_dense`` refuses, naming this count"""
    return int(np.count_nonzero(rtn_params(w, bits, group_size, zero_point, scale_f16)[2]))


def unpack_bitnet_packed(packed: np.ndarray) -> Tuple[np.ndarray, int]:
    """Packed ternary weights of the Hugging Face BitNet quantiser (``transformers.integrations.bitnet.pack_weights``), uint8 [Mw/4][K]
    -> (levels uint8 [Mw][K], invalid): the host reference of ``tmac_hip_pack_ternary_dev``, never the route.  With R4 = Mw / 4, weight
    row o is field o // R4 (bits 2 (o // R4) and up) of packed row o % R4; the field holds v = t + 1, the level is t + 2 = v + 1 in
    {1, 2, 3} (``w_real = (level - 2) * s``).  A field of 3 has no level: it becomes level 3 and is counted in ``invalid``."""
    packed = np.asarray(packed)
    if packed.dtype != np.uint8 or packed.ndim != 2:
        raise TypeError("packed must be uint8 [Mw/4][K]")
    v = np.concatenate([(packed >> np.uint8(2 * i)) & np.uint8(3) for i in range(4)], axis=0)
    return np.minimum(v + np.uint8(1), np.uint8(3)).astype(np.uint8), int(np.count_nonzero(v == 3))


def pack_bitnet_packed(levels: np.ndarray) -> np.ndarray:
    """the inverse: levels uint8 [Mw][K] in {1, 2, 3}, Mw a multiple of 4 -> packed uint8 [Mw/4][K] (fixtures and tests)"""
    levels = np.asarray(levels)
    if levels.dtype != np.uint8 or levels.ndim != 2 or levels.shape[0] % 4 or levels.size == 0 or levels.min() < 1 or levels.max() > 3:
        raise ValueError("levels must be uint8 [Mw][K] in {1, 2, 3} with Mw a multiple of 4")
    R4 = levels.shape[0] // 4
    v = (levels - np.uint8(1)).reshape(4, R4, levels.shape[1])
    return (v[0] | (v[1] << np.uint8(2)) | (v[2] << np.uint8(4)) | (v[3] << np.uint8(6))).astype(np.uint8)


BITNET_LINEAR_CLASSES = ("bitlinear", "autobitlinear")


def bitnet_packed_scale(weight_scale, linear_class: str = "bitlinear") -> np.float32:
    """The unified scale s (``w_real = (level - 2) * s``) a packed BitNet checkpoint's one-element ``weight_scale`` stands for.
    ``weight_scale``: a float, or a one-element array in float32, float16 or uint16 (bf16 bit patterns); its conversion to float32 is
    exact.  ``linear_class`` is ``quantization_config.linear_class``: "autobitlinear" (bitnet-b1.58-2B-4T) computes
    ``y = (x . levels) * weight_scale``, so s = float32(weight_scale); "bitlinear" (the default of ``BitNetQuantConfig``) computes
    ``y = (x . levels) / weight_scale``, so s = float32(1) / float32(weight_scale), one correctly rounded float32 division."""
    if linear_class not in BITNET_LINEAR_CLASSES:
        raise ValueError("linear_class must be one of {}, not {!r}".format(BITNET_LINEAR_CLASSES, linear_class))
    a = np.asarray(weight_scale)
    if a.size != 1:
        raise ValueError("weight_scale holds {} values: one expected".format(a.size))
    a = a.reshape(1)
    if a.dtype == np.uint16:
        ws = bf16_bits_to_f32(a)[0]
    elif a.dtype in (np.float32, np.float16) or a.dtype.kind in "fiu":
        ws = a.astype(np.float32)[0]
    else:
        raise TypeError("weight_scale must be a float, or float32 / float16 / uint16 (bf16 bit patterns), not {}".format(a.dtype))
    with np.errstate(divide="ignore"):
        return np.float32(ws) if linear_class == "autobitlinear" else np.float32(1.0) / np.float32(ws)


def kernel_name(M_bits: int, K: int, N: int, bits: int) -> str:
    return f"qgemm_lut_t1_int8_m{M_bits}_k{K}_n{N}_b{bits}"


def default_bm(bits: int, Mw: int) -> int:
    """a legal M-tile for shapes without a tuned entry: the largest of the reference's knob space that tiles M
    (``qgemm.py:98-116``); the GPU kernels do not care, the value only fixes the blob layout"""
    for bm in (256, 128, 512, 1024, 320, 640) if bits != 3 else (192, 384, 576, 768):
        if (Mw * bits) % bm == 0 and bm % bits == 0 and (bm // bits) % 8 == 0:
            return bm
    raise ValueError(f"no legal bm for Mw={Mw}, bits={bits}")


def write_kcfg(path: str, kernels: Iterable[Sequence[int]], group_size: int = 128, act_group_size: int = 64,
               zero_point: bool = True, bm: Optional[Dict[Tuple[int, int, int], int]] = None, kfactor: int = 16) -> None:
    """Emit the kcfg.ini the reference's ``deploy/compile.py`` writes next to its kernels: one section per kernel,
    fields bm, simd_n_in, simd_n_out, kfactor, group_size, lut_scales_size, scales_size, n_tile_num."""
    cf = configparser.ConfigParser()
    for bits, Mw, K, N, m_groups in kernels:
        b = (bm or {}).get((bits, Mw, K), default_bm(bits, Mw))
        ags = K if act_group_size == -1 else act_group_size
        zp = zero_point and m_groups == -1
        scales_size = m_groups if m_groups != -1 else Mw * K // group_size * (2 if zp else 1)
        cf[kernel_name(Mw * bits, K, N, bits)] = {
            "bm": str(b), "simd_n_in": "16", "simd_n_out": "8", "kfactor": str(kfactor),
            "group_size": str(group_size), "lut_scales_size": str(N * K // ags),
            "scales_size": str(scales_size), "n_tile_num": str(Mw * bits // b),
        }
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        cf.write(f)


def read_kcfg_entry(path: str, Mw: int, K: int, bits: int) -> Dict[str, int]:
    """the section for (M*bits, K) as ``preprocess_for_t_mac`` looks it up (first match on the m / k name fields)"""
    cf = configparser.ConfigParser()
    cf.read(path)
    for sec in cf.sections():
        f = sec.split("_")
        if f[-4] == f"m{Mw * bits}" and f[-3] == f"k{K}":
            return {k: int(v) for k, v in cf[sec].items()}
    raise KeyError(f"GEMM of shape ({Mw}, {K}) is not in {path}")


def preprocess_for_t_mac(kcfg_file: str, w: np.ndarray, scales: np.ndarray, zeros: Optional[np.ndarray] = None,
                         bits: int = 2) -> np.ndarray:
    """uint weights [M][K] (+ scales, zeros) -> the byte blob a T-MAC GGUF tensor holds: the permuted weight bytes
    followed by the fp32 scales (``model_utils.py:243-271``)."""
    M, K = w.shape
    e = read_kcfg_entry(kcfg_file, M, K, bits)
    A, S = preprocess_weights(w, scales, zeros, bits=bits, g=4, bm=e["bm"], kfactor=e["kfactor"],
                              simd_n_in=e["simd_n_in"], simd_n_out=e["simd_n_out"])
    return np.concatenate([A.reshape(-1), np.ascontiguousarray(S.astype(np.float32)).view(np.uint8).reshape(-1)])


def preprocess_for_t_mac_gpu(kcfg_file: str, qweight, scales, qzeros, gptq_v2: bool = True) -> np.ndarray:
    """``preprocess_for_t_mac(kcfg_file, w, scales, zeros, bits)`` on the tensors ``unpack_gptq(qweight, scales, qzeros, gptq_v2)`` gives,
    byte for byte, with the unpacking and the permutation done on the GPU (``tmac_hip_pack_gptq_dev``): the converter's route to the blob
    of a T-MAC GGUF tensor.  The one function of this module that needs a GPU; the numpy functions above stay the CPU reference.  A kcfg
    section without zero points (scales_size = M * K / group_size) drops the zeros, as passing ``zeros=None`` does there."""
    from . import wrapper
    from .binding import KCfg, F32
    K, Mw, bits, gs = parse_gptq(qweight, scales, qzeros)
    e = read_kcfg_entry(kcfg_file, Mw, K, bits)
    zp = e["scales_size"] >= 2 * Mw * (K // e["group_size"])
    cfg = KCfg.make(Mw, K, bits, e["bm"], e["kfactor"], e["group_size"], 64, zp)
    A, S = wrapper.pack_gptq(qweight, scales, qzeros if zp else None, cfg, gptq_v2, F32)
    return np.concatenate([A.cpu().numpy(), S.cpu().numpy().view(np.uint8)])


def preprocess_awq_for_t_mac_gpu(kcfg_file: str, qweight, scales, qzeros) -> np.ndarray:
    """``preprocess_for_t_mac(kcfg_file, w, scales, zeros, 4)`` on the tensors ``unpack_awq(qweight, scales, qzeros)`` gives, byte for byte,
    with the unpacking and the permutation done on the GPU (``tmac_hip_pack_awq_dev``): the twin of ``preprocess_for_t_mac_gpu`` for AutoAWQ
    GEMM checkpoints.  A kcfg section without zero points drops the zeros, as there."""
    from . import wrapper
    from .binding import KCfg, F32
    K, Mw, bits, gs = parse_awq(qweight, scales, qzeros)
    e = read_kcfg_entry(kcfg_file, Mw, K, bits)
    zp = e["scales_size"] >= 2 * Mw * (K // e["group_size"])
    cfg = KCfg.make(Mw, K, bits, e["bm"], e["kfactor"], e["group_size"], 64, zp)
    A, S = wrapper.pack_awq(qweight, scales, qzeros if zp else None, cfg, F32)
    return np.concatenate([A.cpu().numpy(), S.cpu().numpy().view(np.uint8)])


def split_blob(blob: np.ndarray, Mw: int, K: int, bits: int) -> Tuple[np.ndarray, np.ndarray]:
    """inverse of the concatenation: (weight bytes uint8 [Mw*K*bits/8], scales fp32 [...]) — the two pointers
    ``tmac_hip_register_weights`` takes"""
    nw = Mw * K * bits // 8
    b = np.ascontiguousarray(blob, dtype=np.uint8)
    return b[:nw], b[nw:].view(np.float32)
