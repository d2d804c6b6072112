"""GPTQ checkpoint directory -> registered weights, the blob packed on the GPU (``Weights.from_gptq``).

Two steps, split so that the first runs without a GPU:

* ``scan_gptq_dir``  reads the headers of the ``model*.safetensors`` parts (8-byte little-endian length + JSON, as
  ``convert._safetensors_shapes`` does, with the ``data_offsets``) and ``config.json``: which (qweight, scales, qzeros) triples exist,
  where their bytes lie, and whether the zeros are AutoGPTQ v1's (z - 1) or v2's.  No tensor is loaded.
* ``load_gptq_dir``  maps each part with ``np.memmap``, uploads the three packed tensors of a layer and registers them.  The
  ``safetensors`` package is not needed.

Refused, naming the tensor: act-order checkpoints (``desc_act``, as the reference refuses them) unless ``act_order=True`` is passed, a
``qweight`` without ``scales`` or ``qzeros``, tensors of another element type than I32 (qweight, qzeros) / F16 or F32 (scales).

``act_order=True``: each layer's ``.g_idx`` (int32 [K], required then) becomes the K permutation its handle carries (``wrapper.KPerm``);
one object per distinct content, so q/k/v and gate/up -- quantised against the same inputs -- share theirs and can be fused.  An identity
g_idx registers a plain handle.

A layer's ``<layer>.bias`` ([Mw], F32 / F16 / BF16) is found by the GPTQ and the dense scan (``GptqLayer.bias`` / ``DenseLayer.bias``) and
attached to the handle by their loaders (y = W x + b: the constructors' ``bias=``); a malformed one is refused, naming the tensor.  Where a handle
cannot take one -- act-order layers, BitNet's unified scales -- the loader raises, naming the layer, instead of dropping it.

BitNet b1.58 checkpoints of master weights take the same two steps: ``scan_bitnet_dir`` / ``load_bitnet_dir`` (``Weights.from_bitnet``:
the absmean rule and the packing on the GPU), and checkpoints of PACKED ternary weights (the Hugging Face BitNet quantiser, four weight
rows per byte) ``scan_bitnet_packed_dir`` / ``load_bitnet_packed_dir`` (``Weights.from_bitnet_packed``), both further down this file.
UNQUANTISED checkpoints (fp16 / bf16 / fp32 matrices) come last: ``scan_dense_dir`` / ``load_dense_dir`` (``Weights.from_dense``: per-group
round to nearest and the packing on the GPU).  AutoAWQ checkpoints (GEMM version, 4 bits: the Qwen2 ``*-AWQ`` releases) are at the end:
``scan_awq_dir`` / ``load_awq_dir`` (``Weights.from_awq``); ``load_gptq_dir`` refuses them, naming that loader.
"""
import json
import os
import re
import struct
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

from . import convert
from .binding import F16, F32

_NP = {"I32": np.int32, "F16": np.float16, "F32": np.float32, "BF16": np.uint16, "U8": np.uint8}      # BF16: its 16-bit words (numpy has no bfloat16)


class TensorRef(NamedTuple):
    """where one tensor of a safetensors file lies: bytes [begin, end) of ``path``, counted from the start of the file"""
    path: str
    dtype: str
    shape: Tuple[int, ...]
    begin: int
    end: int


class GptqLayer(NamedTuple):
    name: str               # the layer: "<name>.qweight" without its suffix
    qweight: TensorRef
    scales: TensorRef
    qzeros: TensorRef
    K: int
    Mw: int
    bits: int
    group_size: int
    g_idx: Optional[TensorRef] = None      # scan_gptq_dir(..., act_order=True) only
    bias: Optional[TensorRef] = None       # "<name>.bias", F32 / F16 / BF16 [Mw], where the layer has one (Qwen2's q/k/v, OPT, BLOOM, ...)


class GptqScan(NamedTuple):
    layers: List[GptqLayer]
    gptq_v2: bool
    zero_point: bool
    quantization_config: dict


def safetensors_index(path: str) -> Dict[str, TensorRef]:
    """{tensor name: TensorRef} from the header of a .safetensors file: ``convert._safetensors_shapes`` with the data offsets, made absolute
    (the header stores them relative to its own end)"""
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
            out = {}
            for k, v in hdr.items():
                if k == "__metadata__":
                    continue
                b, e = (int(x) for x in v["data_offsets"])
                if not 0 <= b <= e <= size - 8 - n:
                    raise ValueError("tensor {}: data_offsets [{}, {}) outside the file".format(k, b, e))
                out[k] = TensorRef(path, v["dtype"], tuple(int(d) for d in v["shape"]), 8 + n + b, 8 + n + e)
            return out
        except (ValueError, KeyError, TypeError) as e:
            raise RuntimeError("{}: corrupt safetensors header ({})".format(path, e))


def _bias_ref(index: Dict[str, TensorRef], base: str, Mw: int) -> Optional[TensorRef]:
    """``<base>.bias`` of a layer with Mw output rows, or None where the checkpoint has none.  Refused (RuntimeError naming the tensor):
    another element type than F32 / F16 / BF16, another shape than [Mw], byte ranges that do not match the shape."""
    ref = index.get(base + ".bias")
    if ref is None:
        return None
    if ref.dtype not in ("F32", "F16", "BF16"):
        raise RuntimeError("{}.bias has dtype {}: F32, F16 or BF16 expected".format(base, ref.dtype))
    if ref.shape != (Mw,):
        raise RuntimeError("{}.bias has shape {}: [{}] expected (one value per output row)".format(base, ref.shape, Mw))
    if (ref.end - ref.begin) != Mw * np.dtype(_NP[ref.dtype]).itemsize:
        raise RuntimeError("{}.bias: shape {} does not match its {} bytes".format(base, ref.shape, ref.end - ref.begin))
    return ref


def _refuse_bias(index: Dict[str, TensorRef], base: str, why: str) -> None:
    if base + ".bias" in index:
        raise RuntimeError("{} comes with {}.bias: {}".format(base, base, why))


def gptq_is_v2(qc: dict) -> bool:
    """AutoGPTQ (v1) stores z - 1 in qzeros, GPTQModel (v2) stores z: the reference's pipeline reads the difference off the checkpoint's
    ``quantization_config.meta.quantizer`` -- a GPTQModel checkpoint names "gptqmodel" there -- and a quant_method of "gptq_v2" says the
    same (deploy/compile.py:98 accepts both methods)."""
    q = qc.get("quantizer", "")
    q = " ".join(str(x) for x in q) if isinstance(q, (list, tuple)) else str(q)
    return "gptqmodel" in q.lower() or qc.get("quant_method", "") == "gptq_v2"


def scan_gptq_dir(model_dir: str, act_order: bool = False) -> GptqScan:
    """The GPTQ triples of a checkpoint directory, in order of first appearance, without loading a tensor.  act_order: desc_act
    checkpoints are accepted and every layer must come with its ``.g_idx``."""
    qc = convert.get_quantization_config(model_dir, allow_desc_act=act_order)           # refuses desc_act otherwise
    if str(qc.get("quant_method", "")).lower() == "awq":
        raise RuntimeError("Models in {} are AWQ checkpoints (config.json: quantization_config.quant_method is \"awq\"), not GPTQ: AWQ packs along the "
                           "output axis: use load_awq_dir".format(model_dir))
    parts = sorted(f for f in os.listdir(model_dir) if f.startswith("model") and f.endswith(".safetensors"))
    if not parts:
        raise RuntimeError("Models in {} not in GPTQ safetensors format (torch .bin checkpoints: convert them to safetensors first)".format(model_dir))
    index: Dict[str, TensorRef] = {}
    order: List[str] = []
    for part in parts:
        for name, ref in safetensors_index(os.path.join(model_dir, part)).items():
            index[name] = ref
            if name.endswith(".qweight"):
                order.append(name)
    layers = []
    for qname in order:
        base = qname[:-len(".qweight")]
        qw, sc, qz = index[qname], index.get(base + ".scales"), index.get(base + ".qzeros")
        if sc is None:
            raise RuntimeError("{}.scales is missing".format(base))
        if qz is None:
            raise RuntimeError("{}.qzeros is missing".format(base))
        for ref, suffix, ok in ((qw, ".qweight", ("I32",)), (qz, ".qzeros", ("I32",)), (sc, ".scales", ("F16", "F32"))):
            if ref.dtype not in ok:
                raise RuntimeError("{}{} has dtype {}: {} expected".format(base, suffix, ref.dtype, " or ".join(ok)))
            if len(ref.shape) != 2 or (ref.end - ref.begin) != int(np.prod(ref.shape)) * np.dtype(_NP[ref.dtype]).itemsize:
                raise RuntimeError("{}{}: shape {} does not match its {} bytes".format(base, suffix, ref.shape, ref.end - ref.begin))
        if qz.shape[1] <= 0 or sc.shape[0] <= 0 or sc.shape[1] < qz.shape[1] or sc.shape[0] != qz.shape[0] or sc.shape[1] != qw.shape[1]:
            raise RuntimeError("{}: qweight {} / scales {} / qzeros {} are not GPTQ-packed shapes".format(qname, qw.shape, sc.shape, qz.shape))
        bits = 32 // (sc.shape[1] // qz.shape[1])                      # convert.parse_gptq on shapes alone
        if bits not in (1, 2, 4):
            raise RuntimeError("{}: GPTQ-packed width {} is not served (1, 2, 4)".format(qname, bits))
        K, Mw = qw.shape[0] * (32 // bits), qw.shape[1]
        gi = None
        if act_order:
            gi = index.get(base + ".g_idx")
            if gi is None:
                raise RuntimeError("{}.g_idx is missing (act_order=True reads every layer's group indices)".format(base))
            if gi.dtype != "I32" or gi.shape != (K,) or (gi.end - gi.begin) != 4 * K:
                raise RuntimeError("{}.g_idx has dtype {} and shape {}: I32 [{}] expected".format(base, gi.dtype, gi.shape, K))
        layers.append(GptqLayer(base, qw, sc, qz, K, Mw, bits, K // sc.shape[0], gi, _bias_ref(index, base, Mw)))
    if not layers:
        raise RuntimeError("Models in {} not in GPTQ format".format(model_dir))
    return GptqScan(layers, gptq_is_v2(qc), not qc.get("sym", False), qc)


def read_tensor(ref: TensorRef) -> np.ndarray:
    """the tensor's bytes as a read-only numpy view of the mapped file"""
    return np.memmap(ref.path, dtype=_NP[ref.dtype], mode="r", offset=ref.begin, shape=ref.shape)


def load_gptq_dir(model_dir: str, wrapper, dev_dtype=F16, act_order: bool = False) -> Dict[str, "object"]:
    """{layer name: Weights} for every ``*.qweight`` triple of the checkpoint: the packed tensors are uploaded as they lie in the file
    and unpacked, permuted and re-tiled on the GPU (``wrapper.register_gptq``).  A symmetric checkpoint (``sym``) is registered without
    zero points, as the reference compiles its kernels (deploy/compile.py:103).  act_order: see the head of this file.  A layer's
    ``.bias`` ([Mw], F32 / F16 / BF16) is uploaded as it lies in the file and attached to the handle, which then computes y = W x + b;
    with act_order a layer that has one is refused, naming the layer (act-order handles take no bias yet)."""
    from .binding import KCfg
    from .wrapper import KPerm
    scan = scan_gptq_dir(model_dir, act_order)
    for L in scan.layers:       # (before anything is registered)
        if L.g_idx is not None and L.bias is not None:
            raise RuntimeError("{} comes with {}.bias: an act-order handle with a bias is not served yet (the bias would be dropped)".format(L.name, L.name))
    out = {}
    perms: Dict[Tuple[int, bytes], "object"] = {}      # one KPerm per distinct (group size, g_idx content)
    for L in scan.layers:
        cfg = KCfg.make(L.Mw, L.K, L.bits, convert.default_bm(L.bits, L.Mw), 16, L.group_size, wrapper._act_group_size, scan.zero_point)
        # np.array: a writable copy in memory (the map is read-only, and the upload wants one contiguous source)
        qz = np.array(read_tensor(L.qzeros)) if scan.zero_point else None
        kp = None
        if L.g_idx is not None:
            g = np.array(read_tensor(L.g_idx))
            key = (L.group_size, g.tobytes())
            if key not in perms:
                perms[key] = KPerm(g, L.group_size)
            kp = perms[key]
        bias = np.array(read_tensor(L.bias)) if L.bias is not None else None
        out[L.name] = wrapper.register_gptq(np.array(read_tensor(L.qweight)), np.array(read_tensor(L.scales)), qz, cfg, scan.gptq_v2, dev_dtype, g_idx=kp,
                                            bias=bias)
    return out


# ---- BitNet b1.58 checkpoints of master weights ------------------------------------------------------------------------------------------
class BitnetLayer(NamedTuple):
    name: str               # the layer: "<name>.weight" without its suffix
    weight: TensorRef       # F32, F16 or BF16 [Mw][K]
    Mw: int
    K: int


class BitnetScan(NamedTuple):
    layers: List[BitnetLayer]
    weight_bits: int


_BITNET_LAYER = re.compile(r"^model\.layers\..*_proj\.weight$")


def scan_bitnet_dir(model_dir: str) -> BitnetScan:
    """The linear layers of a BitNet b1.58 checkpoint of MASTER weights (``1bitLLM/bitnet_b1_58-3B``: fp16, bf16 or fp32 tensors, the
    ternary levels come from the absmean rule at load time), without loading a tensor.  ``config.json`` must carry a non-zero
    ``weight_bits`` (what ``convert.get_quantization_config`` reads); a layer is every tensor named ``model.layers.*_proj.weight`` in the
    ``model*.safetensors`` parts, in order of first appearance -- embeddings, norms and the head are not.  Refused (RuntimeError naming
    the tensor): another element type than F32 / F16 / BF16, a shape that is not 2-D, byte ranges that do not match the shape, and a
    layer with a sibling ``.weight_scale`` -- a pre-packed ternary checkpoint, another format."""
    qc = convert.get_quantization_config(model_dir)
    if not qc["weight_bits"]:
        raise RuntimeError("Models in {} not in BitNet format (config.json carries no weight_bits)".format(model_dir))
    parts = sorted(f for f in os.listdir(model_dir) if f.startswith("model") and f.endswith(".safetensors"))
    if not parts:
        raise RuntimeError("Models in {} not in safetensors format (torch .bin checkpoints: convert them to safetensors first)".format(model_dir))
    index: Dict[str, TensorRef] = {}
    order: List[str] = []
    for part in parts:
        for name, ref in safetensors_index(os.path.join(model_dir, part)).items():
            if name not in index and _BITNET_LAYER.match(name):
                order.append(name)
            index[name] = ref
    layers = []
    for wname in order:
        ref = index[wname]
        if wname + "_scale" in index:
            raise RuntimeError("{} comes with {}_scale: a pre-packed ternary checkpoint, not master weights".format(wname, wname))
        _refuse_bias(index, wname[:-len(".weight")], "unified-scale (BitNet) handles take no bias (it would be dropped)")
        if ref.dtype not in ("F32", "F16", "BF16"):
            raise RuntimeError("{} has dtype {}: F32, F16 or BF16 expected".format(wname, ref.dtype))
        if len(ref.shape) != 2:
            raise RuntimeError("{} has shape {}: a 2-D tensor expected".format(wname, ref.shape))
        if (ref.end - ref.begin) != int(np.prod(ref.shape)) * np.dtype(_NP[ref.dtype]).itemsize:
            raise RuntimeError("{}: shape {} does not match its {} bytes".format(wname, ref.shape, ref.end - ref.begin))
        layers.append(BitnetLayer(wname[:-len(".weight")], ref, ref.shape[0], ref.shape[1]))
    if not layers:
        raise RuntimeError("Models in {} hold no model.layers.*_proj.weight tensor".format(model_dir))
    return BitnetScan(layers, int(qc["weight_bits"]))


def load_bitnet_dir(model_dir: str, wrapper, dev_dtype=F32, eps: float = 1e-5) -> Dict[str, "object"]:
    """{layer name: Weights} for every layer ``scan_bitnet_dir`` finds: the master weights are uploaded as they lie in the file -- BF16
    as its 16-bit words, no conversion on the host -- and quantised (absmean, one scale per matrix) and packed on the GPU
    (``wrapper.register_bitnet``)."""
    scan = scan_bitnet_dir(model_dir)
    return {L.name: wrapper.register_bitnet(np.array(read_tensor(L.weight)), None, 1, eps, None, dev_dtype) for L in scan.layers}


# ---- BitNet b1.58 checkpoints of PACKED ternary weights (the Hugging Face BitNet quantiser, offline mode) ----------------------------------
class BitnetPackedLayer(NamedTuple):
    name: str               # the layer: "<name>.weight" without its suffix
    weight: TensorRef       # U8 [Mw / 4][K]: four weight rows per byte (convert.unpack_bitnet_packed)
    weight_scale: TensorRef # one element, BF16 / F16 / F32
    Mw: int                 # 4 * weight.shape[0]: the file does not record it
    K: int


class BitnetPackedScan(NamedTuple):
    layers: List[BitnetPackedLayer]
    linear_class: str       # "bitlinear" | "autobitlinear": whether a layer divides or multiplies by its weight_scale
    use_rms_norm: bool
    rms_norm_eps: float
    quantization_config: dict


def scan_bitnet_packed_dir(model_dir: str) -> BitnetPackedScan:
    """The linear layers of a PACKED ternary BitNet checkpoint (``quantization_config.quant_method == "bitnet"``, offline mode;
    ``microsoft/bitnet-b1.58-2B-4T``), without loading a tensor.  A layer is every tensor named ``*.weight`` with dtype U8 that has a
    sibling ``.weight_scale``, in order of first appearance in the ``model*.safetensors`` parts -- embeddings, norms, ``lm_head`` and
    whatever ``modules_to_not_convert`` names are floating tensors without a scale, so they are not layers.  ``linear_class`` defaults to
    "bitlinear" as ``BitNetQuantConfig`` does.  Refused (RuntimeError naming the tensor or the field): another ``quant_method``,
    ``quantization_mode == "online"`` (master weights: load_bitnet_dir), an unknown ``linear_class``, a U8 ``.weight`` without
    ``.weight_scale``, a scale that is not one element of BF16 / F16 / F32, a weight that is not 2-D, byte ranges that do not match the
    shape, and a directory without any layer."""
    with open(os.path.join(model_dir, "config.json"), "r", encoding="utf-8") as f:
        qc = json.load(f).get("quantization_config") or {}
    if qc.get("quant_method") != "bitnet":
        raise RuntimeError("Models in {} not in packed BitNet format (config.json: quantization_config.quant_method is {!r}, \"bitnet\" expected)".format(
            model_dir, qc.get("quant_method")))
    if qc.get("quantization_mode", "offline") == "online":
        raise RuntimeError("quantization_config.quantization_mode is \"online\": a checkpoint of master weights: load_bitnet_dir")
    linear_class = qc.get("linear_class", "bitlinear")
    if linear_class not in convert.BITNET_LINEAR_CLASSES:
        raise RuntimeError("quantization_config.linear_class is {!r}: \"bitlinear\" or \"autobitlinear\" expected".format(linear_class))
    parts = sorted(f for f in os.listdir(model_dir) if f.startswith("model") and f.endswith(".safetensors"))
    if not parts:
        raise RuntimeError("Models in {} not in safetensors format (torch .bin checkpoints: convert them to safetensors first)".format(model_dir))
    index: Dict[str, TensorRef] = {}
    order: List[str] = []
    for part in parts:
        for name, ref in safetensors_index(os.path.join(model_dir, part)).items():
            if name not in index and name.endswith(".weight") and ref.dtype == "U8":
                order.append(name)
            index[name] = ref
    layers = []
    for wname in order:
        ref, sc = index[wname], index.get(wname + "_scale")
        if sc is None:
            raise RuntimeError("{}_scale is missing ({} is U8: a packed ternary weight)".format(wname, wname))
        if sc.dtype not in ("BF16", "F16", "F32") or int(np.prod(sc.shape)) != 1 or len(sc.shape) > 1 or \
                (sc.end - sc.begin) != np.dtype(_NP[sc.dtype]).itemsize:
            raise RuntimeError("{}_scale has dtype {} and shape {}: one element of BF16, F16 or F32 expected".format(wname, sc.dtype, sc.shape))
        _refuse_bias(index, wname[:-len(".weight")], "unified-scale (BitNet) handles take no bias (it would be dropped)")
        if len(ref.shape) != 2:
            raise RuntimeError("{} has shape {}: a 2-D tensor expected".format(wname, ref.shape))
        if (ref.end - ref.begin) != int(np.prod(ref.shape)):
            raise RuntimeError("{}: shape {} does not match its {} bytes".format(wname, ref.shape, ref.end - ref.begin))
        layers.append(BitnetPackedLayer(wname[:-len(".weight")], ref, sc, 4 * ref.shape[0], ref.shape[1]))
    if not layers:
        raise RuntimeError("Models in {} hold no packed ternary layer (a U8 *.weight with a .weight_scale)".format(model_dir))
    return BitnetPackedScan(layers, linear_class, bool(qc.get("use_rms_norm", False)), float(qc.get("rms_norm_eps") or 1e-6), qc)


def load_bitnet_packed_dir(model_dir: str, wrapper, dev_dtype=F32) -> Dict[str, "object"]:
    """{layer name: Weights} for every layer ``scan_bitnet_packed_dir`` finds: the packed bytes are uploaded as they lie in the file and
    unpacked and re-tiled on the GPU (``wrapper.register_bitnet_packed``); the scale is a host scalar, read from the file and turned into
    the blob's scale by the checkpoint's ``linear_class`` (``convert.bitnet_packed_scale``).  Handles only: where the checkpoint sets
    ``use_rms_norm`` (the scan result says so, with ``rms_norm_eps``), a layer's ``<layer>.rms_norm.weight`` vector is the caller's to
    apply to the activations, for example through ``fused_xf(..., "norm", gamma=...)``.  A layer with a ``.bias`` is refused by the scan,
    naming the layer: unified-scale handles take none."""
    scan = scan_bitnet_packed_dir(model_dir)
    return {L.name: wrapper.register_bitnet_packed(np.array(read_tensor(L.weight)), np.array(read_tensor(L.weight_scale._replace(shape=(1,)))), None,
                                                   scan.linear_class, dev_dtype) for L in scan.layers}


# ---- unquantised checkpoints: dense fp16 / bf16 / fp32 matrices, quantised at load time (round to nearest) ----------------------------------
class DenseLayer(NamedTuple):
    name: str               # the layer: "<name>.weight" without its suffix
    weight: TensorRef       # F32, F16 or BF16 [Mw][K]
    Mw: int
    K: int
    bias: Optional[TensorRef] = None       # "<name>.bias", F32 / F16 / BF16 [Mw], where the layer has one


class DenseScan(NamedTuple):
    layers: List[DenseLayer]


def scan_dense_dir(model_dir: str) -> DenseScan:
    """The linear layers of an UNQUANTISED checkpoint (an ordinary fp16 / bf16 / fp32 model: llama-3, Mistral, a fine-tune, a merged
    LoRA), without loading a tensor: every tensor named ``model.layers.*_proj.weight`` in the ``model*.safetensors`` parts, in order of
    first appearance -- embeddings, norms and the head are not.  Refused (RuntimeError naming the config key): a ``config.json`` with a
    ``quantization_config`` -- the refusal names the loader of that format, ``load_gptq_dir`` for GPTQ methods, ``load_bitnet_packed_dir``
    / ``load_bitnet_dir`` for "bitnet" -- or with a non-zero ``weight_bits`` (BitNet master weights: ``load_bitnet_dir``).  Refused naming
    the tensor: another element type than F32 / F16 / BF16, a shape that is not 2-D, byte ranges that do not match the shape, a sibling
    ``.weight_scale``.  A directory without ``config.json`` is an unquantised one."""
    path = os.path.join(model_dir, "config.json")
    hp = {}
    if os.path.exists(path):
        with open(path, "r", encoding="utf-8") as f:
            hp = json.load(f)
    qc = hp.get("quantization_config")
    if qc:
        method = qc.get("quant_method", "")
        if method == "bitnet":
            use = "load_bitnet_dir" if qc.get("quantization_mode", "offline") == "online" else "load_bitnet_packed_dir"
        elif str(method).lower() == "awq":
            use = "load_awq_dir"
        elif str(method).startswith("gptq") or "bits" in qc:
            use = "load_gptq_dir"
        else:
            use = None
        raise RuntimeError("config.json carries a quantization_config (quant_method {!r}): a quantised checkpoint, not dense weights{}".format(
            method, ": use {}".format(use) if use else ""))
    if hp.get("weight_bits", 0):
        raise RuntimeError("config.json carries weight_bits = {}: BitNet master weights take the absmean rule: use load_bitnet_dir".format(hp["weight_bits"]))
    parts = sorted(f for f in os.listdir(model_dir) if f.startswith("model") and f.endswith(".safetensors"))
    if not parts:
        raise RuntimeError("Models in {} not in safetensors format (torch .bin checkpoints: convert them to safetensors first)".format(model_dir))
    index: Dict[str, TensorRef] = {}
    order: List[str] = []
    for part in parts:
        for name, ref in safetensors_index(os.path.join(model_dir, part)).items():
            if name not in index and _BITNET_LAYER.match(name):
                order.append(name)
            index[name] = ref
    layers = []
    for wname in order:
        ref = index[wname]
        if wname + "_scale" in index:
            raise RuntimeError("{} comes with {}_scale: a pre-packed ternary checkpoint, not dense weights".format(wname, wname))
        if ref.dtype not in ("F32", "F16", "BF16"):
            raise RuntimeError("{} has dtype {}: F32, F16 or BF16 expected".format(wname, ref.dtype))
        if len(ref.shape) != 2:
            raise RuntimeError("{} has shape {}: a 2-D tensor expected".format(wname, ref.shape))
        if (ref.end - ref.begin) != int(np.prod(ref.shape)) * np.dtype(_NP[ref.dtype]).itemsize:
            raise RuntimeError("{}: shape {} does not match its {} bytes".format(wname, ref.shape, ref.end - ref.begin))
        layers.append(DenseLayer(wname[:-len(".weight")], ref, ref.shape[0], ref.shape[1], _bias_ref(index, wname[:-len(".weight")], ref.shape[0])))
    if not layers:
        raise RuntimeError("Models in {} hold no model.layers.*_proj.weight tensor".format(model_dir))
    return DenseScan(layers)


def load_dense_dir(model_dir: str, wrapper, bits: int, group_size: int = 128, zero_point: bool = True, dev_dtype=F16) -> Dict[str, "object"]:
    """{layer name: Weights} for every layer ``scan_dense_dir`` finds: the matrix is uploaded as it lies in the file -- BF16 as its 16-bit
    words, no conversion on the host, one upload per tensor -- and quantised to ``bits`` (1 to 4) with per-group scales by round to nearest
    and packed on the GPU (``wrapper.register_dense``).  A layer's ``.bias`` is attached to its handle (y = W x + b)."""
    scan = scan_dense_dir(model_dir)
    return {L.name: wrapper.register_dense(np.array(read_tensor(L.weight)), bits, group_size, zero_point, None, dev_dtype,
                                           bias=np.array(read_tensor(L.bias)) if L.bias is not None else None) for L in scan.layers}


# ---- AutoAWQ checkpoints (WQLinear_GEMM, 4 bits): the official Qwen2 / Qwen2.5 *-AWQ releases and their like ----------------------------------
class AwqLayer(NamedTuple):
    name: str               # the layer: "<name>.qweight" without its suffix
    qweight: TensorRef      # I32 [K][Mw / 8]: eight weight rows per word along the output axis (convert.unpack_awq)
    scales: TensorRef       # F16 / F32 [K / gs][Mw]
    qzeros: TensorRef       # I32 [K / gs][Mw / 8]
    K: int
    Mw: int
    group_size: int
    bias: Optional[TensorRef] = None       # "<name>.bias", F32 / F16 / BF16 [Mw], where the layer has one (Qwen2's q/k/v)


class AwqScan(NamedTuple):
    layers: List[AwqLayer]
    skipped: List[str]      # dense layers the quantiser left alone (lm_head, modules_to_not_convert): "<name>.weight" without a .qweight
    quantization_config: dict


_AWQ_NOT_SERVED = ("gemv", "gemv_fast", "marlin")


def scan_awq_dir(model_dir: str) -> AwqScan:
    """The (qweight, scales, qzeros) triples of an AutoAWQ checkpoint directory, in order of first appearance, without loading a tensor.
    ``config.json`` is read directly.  Refused (RuntimeError naming the field or the tensor): a ``quant_method`` other than "awq"; a
    ``version`` other than "gemm" (case-insensitive; "gemv", "gemv_fast" and "marlin" lay the words out differently and are not served);
    ``bits`` other than 4; ``zero_point: false`` (symmetric AWQ); a ``qweight`` without ``scales`` or ``qzeros``; another element type
    than I32 (qweight, qzeros) / F16 or F32 (scales); shapes that are not [K][Mw/8], [K/gs][Mw], [K/gs][Mw/8] or byte ranges that do not
    match them; a ``group_size`` that disagrees with the shapes (-1: one group per row, K).  Dense layers -- ``lm_head``, the entries of
    ``modules_to_not_convert`` -- have a ``.weight`` and no ``.qweight``: they are no layers here, ``skipped`` names those of them that are
    2-D.  A layer's ``.bias`` is found as the GPTQ scan finds it."""
    with open(os.path.join(model_dir, "config.json"), "r", encoding="utf-8") as f:
        qc = json.load(f).get("quantization_config") or {}
    if str(qc.get("quant_method", "")).lower() != "awq":
        raise RuntimeError("Models in {} not in AWQ format (config.json: quantization_config.quant_method is {!r}, \"awq\" expected)".format(
            model_dir, qc.get("quant_method")))
    version = str(qc.get("version", "gemm")).lower()
    if version != "gemm":
        raise RuntimeError("quantization_config.version is {!r}: the \"gemm\" layout (WQLinear_GEMM) is served; {} are not".format(
            qc.get("version"), ", ".join(_AWQ_NOT_SERVED)))
    if int(qc.get("bits", 4)) != 4:
        raise RuntimeError("quantization_config.bits is {}: AWQ is served at 4 bits".format(qc.get("bits")))
    if not qc.get("zero_point", True):
        raise RuntimeError("quantization_config.zero_point is false: symmetric AWQ is not served")
    parts = sorted(f for f in os.listdir(model_dir) if f.startswith("model") and f.endswith(".safetensors"))
    if not parts:
        raise RuntimeError("Models in {} not in AWQ safetensors format (torch .bin checkpoints: convert them to safetensors first)".format(model_dir))
    index: Dict[str, TensorRef] = {}
    order: List[str] = []
    for part in parts:
        for name, ref in safetensors_index(os.path.join(model_dir, part)).items():
            if name not in index and name.endswith(".qweight"):
                order.append(name)
            index[name] = ref
    gs_cfg = int(qc.get("group_size", 128))
    layers = []
    for qname in order:
        base = qname[:-len(".qweight")]
        qw, sc, qz = index[qname], index.get(base + ".scales"), index.get(base + ".qzeros")
        if sc is None:
            raise RuntimeError("{}.scales is missing".format(base))
        if qz is None:
            raise RuntimeError("{}.qzeros is missing".format(base))
        for ref, suffix, ok in ((qw, ".qweight", ("I32",)), (qz, ".qzeros", ("I32",)), (sc, ".scales", ("F16", "F32"))):
            if ref.dtype not in ok:
                raise RuntimeError("{}{} has dtype {}: {} expected".format(base, suffix, ref.dtype, " or ".join(ok)))
            if len(ref.shape) != 2 or (ref.end - ref.begin) != int(np.prod(ref.shape)) * np.dtype(_NP[ref.dtype]).itemsize:
                raise RuntimeError("{}{}: shape {} does not match its {} bytes".format(base, suffix, ref.shape, ref.end - ref.begin))
        K, Mw = qw.shape[0], sc.shape[1]
        if K <= 0 or Mw <= 0 or qw.shape[1] * 8 != Mw or sc.shape[0] <= 0 or K % sc.shape[0] or qz.shape != (sc.shape[0], qw.shape[1]):
            raise RuntimeError("{}: qweight {} / scales {} / qzeros {} are not AWQ GEMM shapes ([K][Mw/8], [K/gs][Mw], [K/gs][Mw/8])".format(
                qname, qw.shape, sc.shape, qz.shape))
        gs = K // sc.shape[0]
        if gs != (K if gs_cfg == -1 else gs_cfg):
            raise RuntimeError("{}.scales has {} groups of {} for K={}: quantization_config.group_size is {}".format(base, sc.shape[0], gs, K, gs_cfg))
        layers.append(AwqLayer(base, qw, sc, qz, K, Mw, gs, _bias_ref(index, base, Mw)))
    if not layers:
        raise RuntimeError("Models in {} hold no AWQ layer (a *.qweight with .scales and .qzeros)".format(model_dir))
    quantised = {L.name for L in layers}
    skipped = [n[:-len(".weight")] for n, ref in index.items() if n.endswith(".weight") and len(ref.shape) == 2 and n[:-len(".weight")] not in quantised]
    return AwqScan(layers, skipped, qc)


def load_awq_dir(model_dir: str, wrapper, dev_dtype=F16) -> Dict[str, "object"]:
    """{layer name: Weights} for every layer ``scan_awq_dir`` finds: the three packed tensors are uploaded as they lie in the file and
    unpacked, permuted and re-tiled on the GPU (``wrapper.register_awq``).  A layer's ``.bias`` is uploaded as it lies in the file and
    attached to the handle (y = W x + b).  The dense layers the scan skipped are the caller's."""
    from .binding import KCfg
    scan = scan_awq_dir(model_dir)
    out = {}
    for L in scan.layers:
        cfg = KCfg.make(L.Mw, L.K, 4, convert.default_bm(4, L.Mw), 16, L.group_size, wrapper._act_group_size, True)
        bias = np.array(read_tensor(L.bias)) if L.bias is not None else None
        out[L.name] = wrapper.register_awq(np.array(read_tensor(L.qweight)), np.array(read_tensor(L.scales)), np.array(read_tensor(L.qzeros)), cfg,
                                           dev_dtype, bias=bias)
    return out
