"""Python mirror of ``TMAC::TMACGeMMWrapper`` (include/t-mac/tmac_gemm_wrapper.h:79-347) on the GPU.

Same method names and argument meaning as the reference's C++ wrapper — ``set_workspace``,
``get_kcfg``, ``llama_cpp_init`` (preprocessor), ``llama_cpp_compute`` (qgemm_lut) — with device
pointers instead of host pointers, and weights registered once (:class:`Weights`) instead of passed
as raw tile pointers on every call.  All compute goes through libtmac_hip.so's C-ABI.

PyTorch is used only as the owner of device memory / streams when the caller passes tensors; raw
integer device pointers work as well.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import binding as B
from .binding import KCfg, F16, F32, check, check_count


def _ptr(x) -> int:
    """device pointer of a torch tensor / raw int; host pointer of a numpy array"""
    if x is None:
        return 0
    if isinstance(x, int):
        return x
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    return x.data_ptr()


def _stream(stream=None) -> int:
    if stream is not None:
        return stream if isinstance(stream, int) else stream.cuda_stream
    try:
        import torch
        if torch.cuda.is_available():
            return torch.cuda.current_stream().cuda_stream
    except Exception:
        pass
    return 0


def _dtype_code(t) -> int:
    import torch
    if t.dtype == torch.float16:
        return F16
    if t.dtype == torch.float32:
        return F32
    raise TypeError(f"unsupported dtype {t.dtype}")


def _on_device(x, what: str, np_dtypes):
    """a contiguous torch CUDA tensor of ``x``: a CUDA tensor as it is, a numpy array or CPU tensor uploaded first.  ``np_dtypes``: the
    element types the argument may have (a TypeError names the argument otherwise)."""
    import torch
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    name = str(x.dtype).replace("torch.", "")
    if name not in np_dtypes:
        raise TypeError(f"{what} must be {' or '.join(np_dtypes)}, not {name}")
    return x.cuda().contiguous()


def _float_code(t, what: str) -> int:
    name = str(t.dtype).replace("torch.", "")
    if name == "float16":
        return F16
    if name == "float32":
        return F32
    raise TypeError(f"{what} must be float16 or float32, not {name}")


def _gptq_args(qweight, scales, qzeros, cfg, act_group_size):
    """device tensors, shape and configuration of a GPTQ triple (qzeros None: no zero points, which needs a cfg -- the width is read off
    the qzeros shape otherwise)"""
    from . import convert
    qw = _on_device(qweight, "qweight", ("int32",))
    sc = _on_device(scales, "scales", ("float16", "float32"))
    qz = _on_device(qzeros, "qzeros", ("int32",)) if qzeros is not None else None
    if qw.dim() != 2 or sc.dim() != 2 or (qz is not None and qz.dim() != 2):
        raise ValueError("qweight, scales and qzeros are 2-D: [K*bits/32][M], [K/gs][M], [K/gs][M*bits/32]")
    if cfg is None:
        if qz is None:
            raise ValueError("without qzeros the width cannot be read off the shapes: pass a cfg (and its bits)")
        K, Mw, bits, gs = convert.parse_gptq(qw, sc, qz)
        cfg = KCfg.make(Mw, K, bits, convert.default_bm(bits, Mw), 16, gs, act_group_size, True)
    else:
        Mw, gs = int(qw.shape[1]), cfg.group_size
        K = int(sc.shape[0]) * gs
        bits = int(qw.shape[0]) * 32 // K
    return qw, sc, qz, Mw, K, bits, cfg


def _codes_args(codes, scales, zeros, bits, cfg, act_group_size):
    from . import convert
    cd = _on_device(codes, "codes", ("uint8",))
    sc = _on_device(scales, "scales", ("float16", "float32"))
    zr = _on_device(zeros, "zeros", ("float16", "float32")) if zeros is not None else None
    if zr is not None and zr.dtype != sc.dtype:
        raise TypeError("scales and zeros share one dtype")
    Mw, K = int(cd.shape[0]), int(cd.shape[1])
    if cfg is None:
        if sc.dim() != 2:
            raise ValueError("unified scales (m_groups >= 1) need a cfg")
        cfg = KCfg.make(Mw, K, bits, convert.default_bm(bits, Mw), 16, K // int(sc.shape[1]), act_group_size, zr is not None)
    return cd, sc, zr, Mw, K, cfg


def ref_blob_bytes(Mw: int, K: int, bits: int, cfg: KCfg, ref_dtype=F32):
    """(bytes of A_ref, bytes of scales_ref) of the reference blob of this shape (tmac_hip_ref_blob_bytes; host only)"""
    a, s = C.c_size_t(0), C.c_size_t(0)
    check(B.lib().tmac_hip_ref_blob_bytes(Mw, K, bits, C.byref(cfg), ref_dtype, C.byref(a), C.byref(s)))
    return a.value, s.value


def _blob_buffers(Mw, K, bits, cfg, ref_dtype):
    import torch
    a, s = ref_blob_bytes(Mw, K, bits, cfg, ref_dtype)
    esz = 2 if ref_dtype == F16 else 4
    return (torch.empty(a, dtype=torch.uint8, device="cuda"),
            torch.empty(s // esz, dtype=torch.float16 if ref_dtype == F16 else torch.float32, device="cuda"))


class KPerm:
    """The K permutation of an act-order (``desc_act``) GPTQ matrix (tmac_hip_kperm): ``perm = stable_argsort(g_idx)``.  Built from a CUDA
    int32 tensor or a numpy array (uploaded first) of K group indices; refused (TMACHipError) unless every group has exactly
    ``group_size`` members.  ``identity``: g_idx == k // group_size, what every non-act-order exporter writes.  Handles registered through
    it keep the native object alive; two objects of equal content count as the same permutation."""

    def __init__(self, g_idx, group_size: int, stream=None):
        g = _on_device(g_idx, "g_idx", ("int32",))
        if g.dim() != 1:
            raise ValueError("g_idx is 1-D: [K]")
        self._h = C.c_void_p()
        check(B.lib().tmac_hip_kperm_from_gidx_dev(_ptr(g), int(g.shape[0]), int(group_size), C.byref(self._h), _stream(stream)))
        k, ident, pid = C.c_int(0), C.c_int(0), C.c_uint64(0)
        check(B.lib().tmac_hip_kperm_info(self._h, C.byref(k), C.byref(ident), C.byref(pid)))
        self.K, self.group_size, self.identity, self.id = k.value, int(group_size), bool(ident.value), pid.value

    @property
    def handle(self):
        return self._h

    def perm(self) -> np.ndarray:
        """int32 [K]: position k' of the permuted matrix holds source column (and activation) perm[k']"""
        out = np.empty(self.K, np.int32)
        check(B.lib().tmac_hip_kperm_read(self._h, out.ctypes.data))
        return out

    def free(self):
        if self._h:
            B.lib().tmac_hip_kperm_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _kperm(g_idx, group_size: int, stream=None) -> Optional[KPerm]:
    """``g_idx`` of the registration / packing calls -> a KPerm, or None where there is nothing to permute (None, or an identity)"""
    if g_idx is None:
        return None
    kp = g_idx if isinstance(g_idx, KPerm) else KPerm(g_idx, group_size, stream)
    return None if kp.identity else kp


def pack_gptq(qweight, scales, qzeros, cfg: Optional[KCfg] = None, gptq_v2: bool = True, ref_dtype=F32, act_group_size: int = 64, stream=None,
              g_idx=None):
    """GPTQ tensors -> the reference blob, on the GPU (tmac_hip_pack_gptq_dev): (A_ref uint8, scales_ref) as flat CUDA tensors, exactly
    ``weights.preprocess_weights(*convert.unpack_gptq(...))``.  Asynchronous on the stream.  (numpy inputs are uploaded on torch's current
    stream and released in its order: leave ``stream`` at its default with them.)  ``g_idx`` (act-order; a KPerm or the tensor): the blob
    of the matrix with its columns in group order, ``w[:, perm]`` (tmac_hip_pack_gptq_perm_dev)."""
    qw, sc, qz, Mw, K, bits, cfg = _gptq_args(qweight, scales, qzeros, cfg, act_group_size)
    A, S = _blob_buffers(Mw, K, bits, cfg, ref_dtype)
    kp = _kperm(g_idx, cfg.group_size, stream)
    if kp is not None:
        check(B.lib().tmac_hip_pack_gptq_perm_dev(_ptr(qw), _ptr(sc), _ptr(qz), _float_code(sc, "scales"), int(bool(gptq_v2)), kp.handle, Mw, K, bits,
                                                  C.byref(cfg), _ptr(A), _ptr(S), ref_dtype, _stream(stream)))
        return A, S
    check(B.lib().tmac_hip_pack_gptq_dev(_ptr(qw), _ptr(sc), _ptr(qz), _float_code(sc, "scales"), int(bool(gptq_v2)), Mw, K, bits, C.byref(cfg),
                                         _ptr(A), _ptr(S), ref_dtype, _stream(stream)))
    return A, S


def _awq_args(qweight, scales, qzeros, cfg, act_group_size):
    """device tensors, shape and configuration of an AutoAWQ GEMM triple (qweight int32 [K][Mw/8], scales [K/gs][Mw], qzeros int32
    [K/gs][Mw/8] or None: no zero points, which needs a cfg saying so)"""
    from . import convert
    qw = _on_device(qweight, "qweight", ("int32",))
    sc = _on_device(scales, "scales", ("float16", "float32"))
    qz = _on_device(qzeros, "qzeros", ("int32",)) if qzeros is not None else None
    K, Mw, bits, gs = convert.parse_awq(qw, sc, qz)
    if cfg is None:
        cfg = KCfg.make(Mw, K, bits, convert.default_bm(bits, Mw), 16, gs, act_group_size, qz is not None)
    return qw, sc, qz, Mw, K, cfg


def pack_awq(qweight, scales, qzeros, cfg: Optional[KCfg] = None, ref_dtype=F32, act_group_size: int = 64, stream=None):
    """AutoAWQ GEMM tensors (4 bits) -> the reference blob, on the GPU (tmac_hip_pack_awq_dev): (A_ref uint8, scales_ref) as flat CUDA
    tensors, exactly ``weights.preprocess_weights(*convert.unpack_awq(...))``.  Asynchronous on the stream; numpy inputs as in
    ``pack_gptq``."""
    qw, sc, qz, Mw, K, cfg = _awq_args(qweight, scales, qzeros, cfg, act_group_size)
    A, S = _blob_buffers(Mw, K, 4, cfg, ref_dtype)
    check(B.lib().tmac_hip_pack_awq_dev(_ptr(qw), _ptr(sc), _ptr(qz), _float_code(sc, "scales"), Mw, K, C.byref(cfg), _ptr(A), _ptr(S), ref_dtype,
                                        _stream(stream)))
    return A, S


def pack_codes(codes, scales, zeros, bits: int, cfg: Optional[KCfg] = None, ref_dtype=F32, act_group_size: int = 64, stream=None, g_idx=None):
    """codes uint8 [Mw][K] + scales / zeros [Mw][K/gs] in T-MAC's convention -> the reference blob, on the GPU (tmac_hip_pack_codes_dev;
    with ``g_idx``: of ``codes[:, perm]``, tmac_hip_pack_codes_perm_dev)"""
    cd, sc, zr, Mw, K, cfg = _codes_args(codes, scales, zeros, bits, cfg, act_group_size)
    A, S = _blob_buffers(Mw, K, bits, cfg, ref_dtype)
    kp = _kperm(g_idx, cfg.group_size, stream)
    if kp is not None:
        check(B.lib().tmac_hip_pack_codes_perm_dev(_ptr(cd), _ptr(sc), _ptr(zr), _float_code(sc, "scales"), kp.handle, Mw, K, bits, C.byref(cfg),
                                                   _ptr(A), _ptr(S), ref_dtype, _stream(stream)))
        return A, S
    check(B.lib().tmac_hip_pack_codes_dev(_ptr(cd), _ptr(sc), _ptr(zr), _float_code(sc, "scales"), Mw, K, bits, C.byref(cfg), _ptr(A), _ptr(S),
                                          ref_dtype, _stream(stream)))
    return A, S


_SRC_CODES = {"float32": B.SRC_F32, "float16": B.SRC_F16, "bfloat16": B.SRC_BF16}


def _masters_on_device(weight):
    """(contiguous 2-D CUDA tensor, tmac_src_dtype_t) of BitNet master weights: a torch tensor in fp32, fp16 or bf16 (uploaded if it is
    not on the GPU), or a numpy array uploaded as it is -- float32, float16, or uint16 holding bf16 bit patterns (numpy has no bfloat16;
    what ``checkpoint.read_tensor`` gives for a BF16 tensor).  Nothing is converted on the host."""
    import torch
    if isinstance(weight, np.ndarray):
        if weight.dtype == np.uint16:
            weight = torch.from_numpy(np.ascontiguousarray(weight).view(np.int16)).view(torch.bfloat16)
        elif weight.dtype in (np.float32, np.float16):
            weight = torch.from_numpy(np.ascontiguousarray(weight))
        else:
            raise TypeError(f"weight must be float32, float16 or uint16 (bf16 bit patterns), not {weight.dtype}")
    name = str(weight.dtype).replace("torch.", "")
    if name not in _SRC_CODES:
        raise TypeError(f"weight must be float32, float16 or bfloat16, not {name}")
    if weight.dim() != 2:
        raise ValueError("weight is 2-D: [Mw][K]")
    return weight.cuda().contiguous(), _SRC_CODES[name]


def _bias_on_device(bias):
    """(contiguous 1-D CUDA tensor, tmac_src_dtype_t) of a layer's bias: a torch tensor in fp32, fp16 or bf16 (uploaded if it is not on
    the GPU), or a numpy array uploaded as it is -- float32, float16, or uint16 holding bf16 bit patterns.  Nothing is converted on the
    host."""
    import torch
    if isinstance(bias, np.ndarray):
        if bias.dtype == np.uint16:
            bias = torch.from_numpy(np.ascontiguousarray(bias).view(np.int16)).view(torch.bfloat16)
        elif bias.dtype in (np.float32, np.float16):
            bias = torch.from_numpy(np.ascontiguousarray(bias))
        else:
            raise TypeError(f"bias must be float32, float16 or uint16 (bf16 bit patterns), not {bias.dtype}")
    name = str(bias.dtype).replace("torch.", "")
    if name not in _SRC_CODES:
        raise TypeError(f"bias must be float32, float16 or bfloat16, not {name}")
    if bias.dim() != 1:
        raise ValueError("bias is 1-D: [Mw]")
    return bias.cuda().contiguous(), _SRC_CODES[name]


def _bitnet_args(weight, cfg, m_groups, eps, scale):
    """device tensors, shape and configuration of a BitNet matrix.  Without a cfg: the unified-scale configuration ``from_codes`` is handed
    for BitNet -- ``convert.default_bm``, kfactor 16, one activation group per row (act_group_size = K).  With one, its m_groups counts."""
    from . import convert
    w, src = _masters_on_device(weight)
    Mw, K = int(w.shape[0]), int(w.shape[1])
    if cfg is None:
        cfg = KCfg.make(Mw, K, 2, convert.default_bm(2, Mw), 16, 128, K, False, int(m_groups))
    sc = None
    if scale is not None:
        if isinstance(scale, (int, float)):
            scale = np.full(max(cfg.m_groups, 1), scale, np.float32)
        sc = _on_device(scale, "scale", ("float32",)).reshape(-1)
        if int(sc.shape[0]) != cfg.m_groups:
            raise ValueError(f"scale holds {int(sc.shape[0])} values: one per row block, m_groups = {cfg.m_groups}")
    return w, src, sc, float(eps), Mw, K, cfg


def absmean(weight, m_groups: int = 1, eps: float = 1e-5, stream=None):
    """The BitNet absmean scales of master weights [Mw][K] (fp32 / fp16 / bf16, see ``Weights.from_bitnet``): fp32 [m_groups] on the GPU,
    ``max(mean |w|, eps)`` per block of Mw / m_groups rows, the mean accumulated in fp64 (tmac_hip_absmean_dev)."""
    import torch
    w, src = _masters_on_device(weight)
    out = torch.empty(max(int(m_groups), 1), dtype=torch.float32, device="cuda")
    check(B.lib().tmac_hip_absmean_dev(_ptr(w), src, int(w.shape[0]), int(w.shape[1]), int(m_groups), float(eps), _ptr(out), _stream(stream)))
    return out


def pack_bitnet(weight, cfg: Optional[KCfg] = None, m_groups: int = 1, eps: float = 1e-5, scale=None, ref_dtype=F32, stream=None):
    """BitNet master weights -> the reference blob of their ternary levels, on the GPU (tmac_hip_pack_absmean_dev): (A_ref uint8,
    scales_ref) as ``pack_codes`` returns them, exactly ``weights.preprocess_weights(*convert.bitnet_absmean_quant(...))`` under the same
    scales.  ``scale`` (a float, or fp32 [m_groups]): the scales themselves instead of the absmean."""
    w, src, sc, eps, Mw, K, cfg = _bitnet_args(weight, cfg, m_groups, eps, scale)
    A, S = _blob_buffers(Mw, K, 2, cfg, ref_dtype)
    check(B.lib().tmac_hip_pack_absmean_dev(_ptr(w), src, _ptr(sc), eps, Mw, K, C.byref(cfg), _ptr(A), _ptr(S), ref_dtype, _stream(stream)))
    return A, S


def _bitnet_packed_args(packed, scale, cfg):
    """device tensors, shape and configuration of a packed ternary matrix (uint8 [Mw/4][K]: a torch CUDA tensor, or a numpy array
    uploaded as it is) and its scale(s): a float, or fp32 [m_groups].  Without a cfg: what ``from_bitnet`` builds, one scale."""
    from . import convert
    pk = _on_device(packed, "packed", ("uint8",))
    if pk.dim() != 2:
        raise ValueError("packed is 2-D: [Mw/4][K]")
    Mw, K = 4 * int(pk.shape[0]), int(pk.shape[1])
    if cfg is None:
        cfg = KCfg.make(Mw, K, 2, convert.default_bm(2, Mw), 16, 128, K, False, 1)
    if isinstance(scale, (int, float, np.floating)):
        scale = np.full(max(cfg.m_groups, 1), scale, np.float32)
    sc = _on_device(scale, "scale", ("float32",)).reshape(-1)
    if int(sc.shape[0]) != cfg.m_groups:
        raise ValueError(f"scale holds {int(sc.shape[0])} values: one per row block, m_groups = {cfg.m_groups}")
    return pk, sc, Mw, K, cfg


def _bitnet_weight_scale(weight_scale):
    """``weight_scale`` of a packed BitNet checkpoint as ``convert.bitnet_packed_scale`` takes it: a one-element torch tensor (bf16,
    fp16 or fp32) becomes the float32 it converts to exactly; floats and numpy arrays pass through"""
    if hasattr(weight_scale, "detach"):
        name = str(weight_scale.dtype).replace("torch.", "")
        if name not in ("bfloat16", "float16", "float32"):
            raise TypeError(f"weight_scale must be bfloat16, float16 or float32, not {name}")
        return weight_scale.detach().float().cpu().numpy()
    return weight_scale


def pack_ternary(packed, scale, cfg: Optional[KCfg] = None, ref_dtype=F32, stream=None, count_invalid: bool = False):
    """Packed ternary weights uint8 [Mw/4][K] (the Hugging Face BitNet quantiser's format; ``convert.unpack_bitnet_packed`` states it) +
    the unified scale(s) -> the reference blob, on the GPU (tmac_hip_pack_ternary_dev): (A_ref uint8, scales_ref) as ``pack_codes``
    returns them, exactly ``weights.preprocess_weights`` of the unpacked levels.  ``scale``: a float or fp32 [m_groups], the s of
    ``w_real = (level - 2) * s`` (``convert.bitnet_packed_scale`` of a checkpoint's ``weight_scale``).  ``count_invalid``: a third
    result, an int32 CUDA tensor of one element -- the number of fields of value 3 (they are packed as level 3).  Asynchronous."""
    import torch
    pk, sc, Mw, K, cfg = _bitnet_packed_args(packed, scale, cfg)
    A, S = _blob_buffers(Mw, K, 2, cfg, ref_dtype)
    n = torch.empty(4, dtype=torch.int32, device="cuda") if count_invalid else None      # 16 bytes: the call's alignment rule
    check(B.lib().tmac_hip_pack_ternary_dev(_ptr(pk), _ptr(sc), Mw, K, C.byref(cfg), _ptr(A), _ptr(S), ref_dtype, _ptr(n), _stream(stream)))
    return (A, S, n[:1]) if count_invalid else (A, S)


def _dense_args(weight, bits, group_size, zero_point, cfg, act_group_size):
    """device tensor, shape and configuration of an unquantised matrix (``_masters_on_device`` says what it may be).  Without a cfg:
    per-group scales of ``group_size``, ``convert.default_bm``, kfactor 16."""
    from . import convert
    w, src = _masters_on_device(weight)
    Mw, K = int(w.shape[0]), int(w.shape[1])
    if cfg is None:
        cfg = KCfg.make(Mw, K, int(bits), convert.default_bm(int(bits), Mw), 16, int(group_size), act_group_size, bool(zero_point))
    return w, src, Mw, K, cfg


def rtn_params(weight, bits: int, group_size: int, zero_point: bool = True, scale_f16: bool = False, stream=None, count_invalid: bool = False):
    """The round-to-nearest parameters of an unquantised matrix [Mw][K] (fp32 / fp16 / bf16, see ``Weights.from_dense``): (scales, zq),
    fp32 [Mw][K/group_size] CUDA tensors -- ``convert.rtn_params``'s, bit for bit (tmac_hip_rtn_params_dev).  ``count_invalid``: a third
    result, an int32 CUDA tensor of one element -- the number of groups that cannot be quantised.  Asynchronous."""
    import torch
    w, src = _masters_on_device(weight)
    Mw, K = int(w.shape[0]), int(w.shape[1])
    sg = K // int(group_size) if int(group_size) > 0 else 0
    sc = torch.empty((Mw, sg), dtype=torch.float32, device="cuda")
    zq = torch.empty((Mw, sg), dtype=torch.float32, device="cuda")
    n = torch.empty(4, dtype=torch.int32, device="cuda") if count_invalid else None      # 16 bytes: the call's alignment rule
    check(B.lib().tmac_hip_rtn_params_dev(_ptr(w), src, Mw, K, int(bits), int(group_size), int(bool(zero_point)), int(bool(scale_f16)), _ptr(sc), _ptr(zq),
                                          _ptr(n), _stream(stream)))
    return (sc, zq, n[:1]) if count_invalid else (sc, zq)


def pack_rtn(weight, bits: int, group_size: int = 128, zero_point: bool = True, cfg: Optional[KCfg] = None, ref_dtype=F32, act_group_size: int = 64,
             stream=None, count_invalid: bool = False):
    """An unquantised matrix -> the reference blob of its round-to-nearest codes, on the GPU (tmac_hip_pack_rtn_dev): (A_ref uint8,
    scales_ref) as ``pack_codes`` returns them, exactly ``weights.preprocess_weights(*convert.rtn_quant(weight, bits, group_size,
    zero_point, ref_dtype == F16))`` -- a blob of fp16 scales holds the scales that divided.  ``count_invalid``: as in ``rtn_params``."""
    import torch
    w, src, Mw, K, cfg = _dense_args(weight, bits, group_size, zero_point, cfg, act_group_size)
    A, S = _blob_buffers(Mw, K, int(bits), cfg, ref_dtype)
    n = torch.empty(4, dtype=torch.int32, device="cuda") if count_invalid else None
    check(B.lib().tmac_hip_pack_rtn_dev(_ptr(w), src, Mw, K, int(bits), C.byref(cfg), _ptr(A), _ptr(S), ref_dtype, _ptr(n), _stream(stream)))
    return (A, S, n[:1]) if count_invalid else (A, S)


class Weights:
    """One weight matrix resident on the GPU (tmac_hip_register_weights)."""

    @classmethod
    def _adopt(cls, handle, Mw, K, bits, cfg):
        self = cls.__new__(cls)
        self.Mw, self.K, self.bits, self.cfg = Mw, K, bits, cfg
        self._h, self._keep, self._caches = handle, None, []
        self.kperm = None
        return self

    @classmethod
    def from_gptq(cls, qweight, scales, qzeros, cfg: Optional[KCfg] = None, gptq_v2: bool = True, dev_dtype=F16, act_group_size: int = 64,
                  stream=None, g_idx=None, bias=None) -> "Weights":
        """Register straight from GPTQ tensors -- torch CUDA tensors, or numpy arrays that are uploaded first -- packed into the reference
        blob on the GPU (tmac_hip_register_weights_gptq_dev).  The handle is the one ``Weights(*blob)`` gives.  Without a ``cfg`` the
        shapes come from ``convert.parse_gptq`` and the M-tile from ``convert.default_bm``; ``qzeros=None`` (no zero points) needs one.
        ``g_idx`` (act-order checkpoints: a CUDA int32 tensor, a numpy array or a KPerm): the handle holds the matrix in group order and
        carries the permutation (``.kperm``), through which every fused call gathers its activations; an identity g_idx gives a plain
        handle (tmac_hip_register_weights_gptq_perm_dev).  ``bias`` ([Mw], fp32 / fp16 / bf16: a CUDA tensor or a numpy array): the
        handle computes y = W x + b (tmac_hip_weights_set_bias_dev); with a ``g_idx`` that permutes, the library's refusal is raised."""
        qw, sc, qz, Mw, K, bits, cfg = _gptq_args(qweight, scales, qzeros, cfg, act_group_size)
        h = C.c_void_p()
        ref = _float_code(sc, "scales")        # the blob in the scales' own dtype: nothing is rounded on the way
        kp = _kperm(g_idx, cfg.group_size, stream)
        if kp is not None:
            check(B.lib().tmac_hip_register_weights_gptq_perm_dev(C.byref(h), _ptr(qw), _ptr(sc), _ptr(qz), ref, int(bool(gptq_v2)), kp.handle, Mw, K,
                                                                  bits, C.byref(cfg), ref, dev_dtype, _stream(stream)))
        else:
            check(B.lib().tmac_hip_register_weights_gptq_dev(C.byref(h), _ptr(qw), _ptr(sc), _ptr(qz), ref, int(bool(gptq_v2)), Mw, K, bits,
                                                             C.byref(cfg), ref, dev_dtype, _stream(stream)))
        self = cls._adopt(h, Mw, K, bits, cfg)
        self.kperm = kp
        return self._with_bias(bias, stream)

    @classmethod
    def from_awq(cls, qweight, scales, qzeros, cfg: Optional[KCfg] = None, dev_dtype=F16, act_group_size: int = 64, stream=None,
                 bias=None) -> "Weights":
        """Register straight from AutoAWQ GEMM tensors (``quantization_config.version == "gemm"``, 4 bits: qweight int32 [K][Mw/8], scales
        [K/gs][Mw], qzeros int32 [K/gs][Mw/8]) -- torch CUDA tensors, or numpy arrays uploaded as they are -- unpacked and packed into the
        reference blob on the GPU (tmac_hip_register_weights_awq_dev).  The handle is the one ``from_codes(*convert.unpack_awq(...)[:3], 4)``
        gives.  Without a ``cfg`` the shape is read off the tensors and the M-tile comes from ``convert.default_bm``.  ``bias``: as in
        ``from_gptq``."""
        qw, sc, qz, Mw, K, cfg = _awq_args(qweight, scales, qzeros, cfg, act_group_size)
        h = C.c_void_p()
        ref = _float_code(sc, "scales")        # the blob in the scales' own dtype: nothing is rounded on the way
        check(B.lib().tmac_hip_register_weights_awq_dev(C.byref(h), _ptr(qw), _ptr(sc), _ptr(qz), ref, Mw, K, C.byref(cfg), ref, dev_dtype,
                                                        _stream(stream)))
        return cls._adopt(h, Mw, K, 4, cfg)._with_bias(bias, stream)

    @classmethod
    def from_codes(cls, codes, scales, zeros, bits: int, cfg: Optional[KCfg] = None, dev_dtype=F16, act_group_size: int = 64,
                   stream=None, g_idx=None, bias=None) -> "Weights":
        """Register from unpacked codes uint8 [Mw][K] with scales / zeros [Mw][K/gs] already in T-MAC's convention (or [m_groups] unified
        scales with a ``cfg``), packed on the GPU (tmac_hip_register_weights_codes_dev).  The route for 3-bit weights.  ``g_idx``: as in
        ``from_gptq`` (codes in the checkpoint's column order, scales / zeros in group order).  ``bias``: as in ``from_gptq``."""
        cd, sc, zr, Mw, K, cfg = _codes_args(codes, scales, zeros, bits, cfg, act_group_size)
        h = C.c_void_p()
        ref = _float_code(sc, "scales")
        kp = _kperm(g_idx, cfg.group_size, stream)
        if kp is not None:
            check(B.lib().tmac_hip_register_weights_codes_perm_dev(C.byref(h), _ptr(cd), _ptr(sc), _ptr(zr), ref, kp.handle, Mw, K, bits, C.byref(cfg),
                                                                   ref, dev_dtype, _stream(stream)))
        else:
            check(B.lib().tmac_hip_register_weights_codes_dev(C.byref(h), _ptr(cd), _ptr(sc), _ptr(zr), ref, Mw, K, bits, C.byref(cfg), ref, dev_dtype,
                                                              _stream(stream)))
        self = cls._adopt(h, Mw, K, bits, cfg)
        self.kperm = kp
        return self._with_bias(bias, stream)

    @classmethod
    def from_bitnet(cls, weight, cfg: Optional[KCfg] = None, m_groups: int = 1, eps: float = 1e-5, scale=None, dev_dtype=F32,
                    stream=None) -> "Weights":
        """Register BitNet b1.58 master weights [Mw][K] -- a torch tensor in fp32, fp16 or bf16, or a numpy array uploaded as it is
        (float32, float16, uint16 = bf16 bit patterns): quantised to ternary levels by the absmean rule and packed on the GPU
        (tmac_hip_register_weights_absmean_dev; include/tmac_hip.h states the rule).  One scale per block of Mw / m_groups rows,
        ``max(mean |w|, eps)``, or ``scale`` (a float, or fp32 [m_groups]) as it is.  The handle is the one
        ``from_codes(levels, scales, None, 2, cfg)`` gives for ``convert.bitnet_absmean_quant``'s levels under the same scales.  Without a
        ``cfg``: ``convert.default_bm``, kfactor 16, act_group_size = K (one activation group per row, BitNet's)."""
        w, src, sc, eps, Mw, K, cfg = _bitnet_args(weight, cfg, m_groups, eps, scale)
        h = C.c_void_p()
        check(B.lib().tmac_hip_register_weights_absmean_dev(C.byref(h), _ptr(w), src, _ptr(sc), eps, Mw, K, C.byref(cfg), F32, dev_dtype,
                                                            _stream(stream)))
        return cls._adopt(h, Mw, K, 2, cfg)

    @classmethod
    def from_bitnet_packed(cls, packed, weight_scale, cfg: Optional[KCfg] = None, linear_class: str = "autobitlinear", dev_dtype=F32,
                           stream=None) -> "Weights":
        """Register a layer of a PACKED ternary BitNet checkpoint (``quant_method: "bitnet"``, offline mode; bitnet-b1.58-2B-4T):
        ``packed`` uint8 [Mw/4][K], four weight rows per byte -- a torch CUDA tensor, or a numpy array uploaded as it is -- unpacked and
        packed into the blob on the GPU (tmac_hip_register_weights_ternary_dev; no [Mw][K] tensor exists anywhere).  ``weight_scale``:
        the checkpoint's one-element tensor (bf16 / fp16 / fp32), a float, or a one-element numpy array (uint16 = bf16 bits);
        ``linear_class`` (``quantization_config.linear_class``) says whether the layer multiplies by it ("autobitlinear") or divides
        ("bitlinear"): ``convert.bitnet_packed_scale``.  The handle is the one ``from_codes(levels, [s], None, 2, cfg)`` gives for
        ``convert.unpack_bitnet_packed``'s levels.  A field of value 3 (no ternary level) is refused (TMACHipError naming the count).
        Without a ``cfg``: as ``from_bitnet``.  With a ``cfg`` of m_groups > 1 every row block gets the same scale."""
        from . import convert
        s = convert.bitnet_packed_scale(_bitnet_weight_scale(weight_scale), linear_class)
        pk, sc, Mw, K, cfg = _bitnet_packed_args(packed, float(s), cfg)
        h = C.c_void_p()
        check(B.lib().tmac_hip_register_weights_ternary_dev(C.byref(h), _ptr(pk), _ptr(sc), Mw, K, C.byref(cfg), F32, dev_dtype, _stream(stream)))
        return cls._adopt(h, Mw, K, 2, cfg)

    @classmethod
    def from_dense(cls, weight, bits: int, group_size: int = 128, zero_point: bool = True, cfg: Optional[KCfg] = None, dev_dtype=F16,
                   act_group_size: int = 64, stream=None, bias=None) -> "Weights":
        """Register an UNQUANTISED matrix [Mw][K] -- a torch tensor in fp32, fp16 or bf16, or a numpy array uploaded as it is (float32,
        float16, uint16 = bf16 bit patterns) -- as a W1 - W4 handle with per-group scales: quantised by per-group round to nearest
        (GPTQ's quantiser without the error search) and packed on the GPU (tmac_hip_register_weights_rtn_dev; include/tmac_hip.h states
        the rule).  The handle is the one ``from_codes(*convert.rtn_quant(weight, bits, group_size, zero_point, dev_dtype == F16), bits,
        cfg, dev_dtype)`` gives: with fp16 device scales the scale is rounded to fp16 before the codes are derived.  A group that cannot
        be quantised -- a master that is not finite, a scale that is 0 or not finite in the scales' dtype -- is refused (TMACHipError
        naming the count).  Without a ``cfg``: ``convert.default_bm``, kfactor 16; with one, its group_size and zero_point count.
        ``bias``: as in ``from_gptq``."""
        w, src, Mw, K, cfg = _dense_args(weight, bits, group_size, zero_point, cfg, act_group_size)
        h = C.c_void_p()
        check(B.lib().tmac_hip_register_weights_rtn_dev(C.byref(h), _ptr(w), src, Mw, K, int(bits), C.byref(cfg), F32, dev_dtype, _stream(stream)))
        return cls._adopt(h, Mw, K, int(bits), cfg)._with_bias(bias, stream)

    def __init__(self, A_ref, scales_ref, Mw: int, K: int, bits: int, cfg: KCfg, scales_dtype=F32, dev_dtype=F32,
                 on_device: bool = False, stream=None):
        self.Mw, self.K, self.bits, self.cfg = Mw, K, bits, cfg
        self._h = C.c_void_p()
        L = B.lib()
        fn = L.tmac_hip_register_weights_dev if on_device else L.tmac_hip_register_weights
        if not on_device:
            A_ref = np.ascontiguousarray(A_ref, np.uint8)
            scales_ref = np.ascontiguousarray(scales_ref, np.float16 if scales_dtype == F16 else np.float32)
        self._keep = (A_ref, scales_ref)
        check(fn(C.byref(self._h), _ptr(A_ref), _ptr(scales_ref), Mw, K, bits, C.byref(cfg), scales_dtype, dev_dtype,
                 _stream(stream)))
        self._keep = None
        self._caches = []          # fused-call caches holding this handle (TMACGeMMWrapper.fused)
        self.kperm = None          # the K permutation of an act-order matrix (from_gptq / from_codes with g_idx)

    @property
    def handle(self):
        return self._h

    def _set_bias(self, bias, stream=None) -> None:
        """y = W x + b from now on (tmac_hip_weights_set_bias_dev): ``bias`` is [Mw] in fp32, fp16 or bf16 -- a CUDA tensor, or a numpy
        array uploaded first (uint16 = bf16 bit patterns).  The handle keeps an fp32 copy of its own.  Once per handle, straight after
        registration; unified-scale and act-order handles are refused (TMACHipError)."""
        b, src = _bias_on_device(bias)
        if int(b.shape[0]) != self.Mw:
            raise ValueError(f"bias holds {int(b.shape[0])} values: one per output row, Mw = {self.Mw}")
        check(B.lib().tmac_hip_weights_set_bias_dev(self._h, _ptr(b), src, _stream(stream)))

    def _with_bias(self, bias, stream=None) -> "Weights":
        """the constructors' ``bias=``: set it, or free the new handle and raise what the library (or the shape check) raises"""
        if bias is not None:
            try:
                self._set_bias(bias, stream)
            except Exception:
                self.free()
                raise
        return self

    @property
    def has_bias(self) -> bool:
        has = C.c_int(0)
        check(B.lib().tmac_hip_weights_has_bias(self._h, C.byref(has)))
        return bool(has.value)

    def algorithmic_bytes(self) -> int:
        return int(B.lib().tmac_hip_weights_bytes(self._h))

    def free(self):
        if self._h:
            hv = self._h.value
            for cache in getattr(self, "_caches", []):     # no cached call may keep the freed native handle
                for key in [k for k in cache if hv in k[0]]:
                    del cache[key]
            self._caches = []
            B.lib().tmac_hip_free_weights(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Workspace:
    """QLUT / LUT_Scales / LUT_Biases on the device (TMACGeMMWrapper::set_workspace)."""

    def __init__(self, maxK: int, maxN: int = 1):
        self.maxK, self.maxN = maxK, maxN
        self._h = C.c_void_p()
        check(B.lib().tmac_hip_workspace_create(C.byref(self._h), maxK, maxN))

    @property
    def handle(self):
        return self._h

    def ptrs(self):
        q, ls, lb, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t()
        check(B.lib().tmac_hip_workspace_ptrs(self._h, C.byref(q), C.byref(n), C.byref(ls), C.byref(lb)))
        return q.value, n.value, ls.value, lb.value

    def read(self, K: int, N: int, act_group_size: int, stream=None):
        q = np.zeros((N, K // 4, 16), np.int8)
        ls = np.zeros((N, K // act_group_size), np.float32)
        lb = np.zeros((N, K // act_group_size), np.float32)
        check(B.lib().tmac_hip_workspace_read(self._h, q.ctypes.data, ls.ctypes.data, lb.ctypes.data, K, N,
                                              act_group_size, _stream(stream)))
        return q, ls, lb

    def read_gemm_image(self, K: int, N: int, act_group_size: int = 64, stream=None):
        """The LUT image k_gemm_planes streams, in plain layouts: half tables int8 [N][K/4][8], lut_scales, lut_biases,
        entry sums fp32 [N][K/act_group_size] (act_group_size 64, or K for the unified-scale flavour)."""
        G = K // act_group_size
        h = np.zeros((N, K // 4, 8), np.int8)
        ls = np.zeros((N, G), np.float32)
        lb = np.zeros((N, G), np.float32)
        hs = np.zeros((N, G), np.float32)
        check(B.lib().tmac_hip_debug_gemm_image_read(self._h, h.ctypes.data, ls.ctypes.data, lb.ctypes.data, hs.ctypes.data, N,
                                                     _stream(stream)))
        return h, ls, lb, hs

    def write(self, qlut: np.ndarray, lut_scales: np.ndarray, lut_biases: np.ndarray, act_group_size: int, stream=None):
        q = np.ascontiguousarray(qlut, np.int8)
        ls = np.ascontiguousarray(lut_scales, np.float32)
        lb = np.ascontiguousarray(lut_biases, np.float32)
        N, T, _ = q.shape
        check(B.lib().tmac_hip_workspace_write(self._h, q.ctypes.data, ls.ctypes.data, lb.ctypes.data, T * 4, N,
                                               act_group_size, _stream(stream)))

    def free(self):
        if self._h:
            B.lib().tmac_hip_workspace_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Comm:
    """The exchange step of the row-sharded multi-GPU path through the C-ABI (tmac_hip_comm_*: RCCL over xGMI, one process
    per GPU).  ``Comm.unique_id()`` on rank 0, hand the 128 bytes to every rank, ``Comm(id, rank, world)`` on each."""

    ID_BYTES = 128

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_char * Comm.ID_BYTES)()
        rc = B.lib().tmac_hip_comm_unique_id(buf)
        if rc:
            raise B.TMACHipError(rc, B.lib().tmac_hip_comm_last_error().decode())
        return bytes(buf)

    def __init__(self, uid: bytes, rank: int, world: int):
        self._h = C.c_void_p()
        self.rank, self.world = rank, world
        buf = (C.c_char * Comm.ID_BYTES).from_buffer_copy(uid)
        rc = B.lib().tmac_hip_comm_init(C.byref(self._h), buf, rank, world)
        if rc:
            raise B.TMACHipError(rc, B.lib().tmac_hip_comm_last_error().decode())

    BLOB_BYTES = 128

    @classmethod
    def ipc(cls, max_bytes_per_rank: int, rank: int, world: int) -> "Comm":
        """the same exchange step over IPC-mapped windows instead of RCCL (tmac_hip_comm_init_ipc): ``export()`` on every rank,
        all-gather the blobs over any transport, ``connect(blobs)``"""
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        self.rank, self.world = rank, world
        rc = B.lib().tmac_hip_comm_init_ipc(C.byref(self._h), max_bytes_per_rank, rank, world)
        if rc:
            raise B.TMACHipError(rc, B.lib().tmac_hip_comm_last_error().decode())
        return self

    def export(self) -> bytes:
        buf = C.create_string_buffer(self.BLOB_BYTES)
        rc = B.lib().tmac_hip_comm_export(self._h, buf)
        if rc:
            raise B.TMACHipError(rc, B.lib().tmac_hip_comm_last_error().decode())
        return buf.raw

    def connect(self, blobs) -> None:
        raw = b"".join(blobs) if not isinstance(blobs, (bytes, bytearray)) else bytes(blobs)
        rc = B.lib().tmac_hip_comm_connect(self._h, raw, len(raw) // self.BLOB_BYTES)
        if rc:
            raise B.TMACHipError(rc, B.lib().tmac_hip_comm_last_error().decode())

    def status(self) -> int:
        w = C.c_uint32(0)
        rc = B.lib().tmac_hip_comm_status(self._h, C.byref(w))
        if rc:
            raise B.TMACHipError(rc, B.lib().tmac_hip_comm_last_error().decode())
        return w.value

    def allgather(self, send, recv, nbytes_per_rank: int, stream=None) -> None:
        rc = B.lib().tmac_hip_comm_allgather(self._h, _ptr(send), _ptr(recv), nbytes_per_rank, _stream(stream))
        if rc:
            raise B.TMACHipError(rc, B.lib().tmac_hip_comm_last_error().decode())

    def destroy(self):
        if self._h:
            B.lib().tmac_hip_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class DecodeChain:
    """A recorded sequence of ``TMACGeMMWrapper.fused`` calls (N = 1) executed by ONE persistent kernel launch
    (tmac_hip_chain_*, include/tmac_hip.h).  Built by ``TMACGeMMWrapper.record_chain``.

    ``record_chain(independent=True)`` declares that no recorded call reads another's output: the chain is then a stream-mode one
    (``stream`` is True: k_lut_images + k_gemv_stream) or the recording fails -- it never becomes k_decode_chain.  Only such a
    recording notes calls on act-order handles (``register_weights_*_perm``): k_lut_images gathers x[perm] per call, and the chain
    keeps the permutations it reads alive, whatever becomes of the ``KPerm`` objects."""

    def __init__(self, handle, keep):
        self._h = handle
        self._keep = keep          # weights / tensors the chain points into
        n, g, b = C.c_int32(0), C.c_int32(0), C.c_size_t(0)
        check(B.lib().tmac_hip_chain_info(self._h, 0, C.byref(n), None, C.byref(g), C.byref(b)))
        self.nops, self.grid, self.weight_bytes = n.value, g.value, b.value
        self.threads = int(B.lib().tmac_hip_chain_threads())     # threads per workgroup of k_decode_chain (for A/B against k_gemv_quad)
        is_stream = getattr(B.lib(), "tmac_hip_chain_is_stream", None)
        # stream mode: no recorded call consumes another's output -- tables prebuilt by k_lut_images, lookups by k_gemv_stream (include/tmac_hip.h)
        mode = int(is_stream(self._h)) if is_stream is not None and getattr(is_stream, "argtypes", None) else 0
        self.stream = mode != 0
        self.quarter_walk = mode == 2      # k_gemv_stream's quarter-walk form: per-group-scale outputs to the oracle's tolerance, not bit-identical to stand-alone launches

    @property
    def handle(self):
        return self._h

    BLOB_BYTES = 128       # TMAC_HIP_CHAIN_BLOB_BYTES

    def export(self) -> bytes:
        """row-sharded chains: this rank's hand-off arena as an IPC blob; all-gather the blobs of all ranks (rank order, any
        transport) and hand them to :meth:`connect`"""
        buf = C.create_string_buffer(self.BLOB_BYTES)
        check(B.lib().tmac_hip_chain_export(self._h, buf))
        return buf.raw

    def connect(self, blobs) -> None:
        """blobs: the exported blobs of ALL ranks in rank order (list of bytes, or one bytes object)"""
        raw = b"".join(blobs) if not isinstance(blobs, (bytes, bytearray)) else bytes(blobs)
        world = len(raw) // self.BLOB_BYTES
        check(B.lib().tmac_hip_chain_connect(self._h, raw, world))

    def launch(self, stream=None) -> None:
        check(B.lib().tmac_hip_chain_launch(self._h, _stream(stream)))

    def status(self) -> int:
        """after a stream synchronisation: 0 if every in-kernel hand-off of the last launches completed"""
        w = C.c_uint32(0)
        check(B.lib().tmac_hip_chain_status(self._h, C.byref(w)))
        return w.value

    def wpq(self, op: int) -> int:
        w = C.c_int32(0)
        check(B.lib().tmac_hip_chain_info(self._h, op, None, C.byref(w), None, None))
        return w.value

    def tap_layout(self, op: int):
        """(offset, count) in ints of call `op` inside the tap buffer; op == nops: (size of the whole buffer, 0)"""
        off, cnt = C.c_size_t(0), C.c_size_t(0)
        check(B.lib().tmac_hip_chain_tap_layout(self._h, op, C.byref(off), C.byref(cnt)))
        return off.value, cnt.value

    def set_tap(self, dev_buffer) -> None:
        """parity tap (include/tmac_hip.h): an int32 device buffer of tap_layout(nops)[0] ints, or None"""
        check(B.lib().tmac_hip_chain_set_tap(self._h, _ptr(dev_buffer) if dev_buffer is not None else None))
        self._tap = dev_buffer

    def set_stamps(self, dev_buffer) -> None:
        check(B.lib().tmac_hip_chain_set_stamps(self._h, _ptr(dev_buffer)))
        self._stamps = dev_buffer

    def free(self):
        if self._h:
            B.lib().tmac_hip_chain_free(self._h)
            self._h = C.c_void_p()
        self._keep = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _ChainRecorder:
    def __init__(self, wrapper, independent=False):
        self.wr = wrapper
        self.independent = independent
        self.chain: Optional[DecodeChain] = None

    def __enter__(self):
        check(B.lib().tmac_hip_chain_begin_independent() if self.independent else B.lib().tmac_hip_chain_begin())
        self.wr._recording = []
        return self

    def __exit__(self, et, ev, tb):
        keep, self.wr._recording = self.wr._recording, None
        h = C.c_void_p()
        rc = B.lib().tmac_hip_chain_end(C.byref(h))
        if et is None:
            check(rc)
            self.chain = DecodeChain(h, keep)
        elif rc == 0 and h:
            B.lib().tmac_hip_chain_free(h)      # the block raised: the chain that was built anyway is not handed out
        return False


class TMACGeMMWrapper:
    """Mirror of the reference wrapper's no-TVM branch (tmac_gemm_wrapper.h:170-228).

    >>> wr = TMACGeMMWrapper(act_group_size=64, kcfg_file="kcfg.ini")
    >>> wr.set_workspace(maxK=11008, maxN=1)
    >>> w = wr.register_weights(A_ref, scales_ref, M=4096, K=11008, bits=2)
    >>> wr.llama_cpp_init(B_dev, M=4096, K=11008, N=1, bits=2)        # preprocessor -> workspace
    >>> wr.llama_cpp_compute(w, C_dev, N=1)                           # qgemm_lut
    """

    def __init__(self, n_threads: int = 1, act_group_size: int = 32, kcfg_file: str = "", library_file: str = ""):
        self._act_group_size = act_group_size
        self._ws: Optional[Workspace] = None
        L = B.lib()
        if kcfg_file:
            check(L.tmac_hip_load_kcfg(kcfg_file.encode()))

    def set_num_threads(self, n_threads: int) -> None:  # no-op without a TVM threadpool, as in the reference
        pass

    def set_workspace(self, maxK: int, maxN: int) -> None:
        self._ws = Workspace(maxK, maxN)

    @property
    def workspace(self) -> Workspace:
        if self._ws is None:
            raise RuntimeError("set_workspace() must be called first (tmac_gemm_wrapper.h:257-270)")
        return self._ws

    def get_kcfg(self, M: int, K: int, N: int, bits: int) -> KCfg:
        cfg = KCfg()
        check(B.lib().tmac_hip_get_kcfg(M, K, N, bits, C.byref(cfg)))
        return cfg

    def set_kcfg(self, M: int, K: int, N: int, bits: int, cfg: KCfg) -> None:
        check(B.lib().tmac_hip_set_kcfg(M, K, N, bits, C.byref(cfg)))

    def register_weights(self, A_ref, scales_ref, M: int, K: int, bits: int, cfg: Optional[KCfg] = None,
                         scales_dtype=F32, dev_dtype=F32, on_device=False, fast_aggregation: int = 0) -> Weights:
        """fast_aggregation: 0 exact (default) | 1 signed halving adds (the reference's ARM ``-fa`` build) | 2 its AVX2
        build; the lossy aggregation of python/t_mac/ops/qgemm.py:30,86 — a property of the registered weights here."""
        cfg = cfg or self.get_kcfg(M, K, 1, bits)
        if not fast_aggregation:
            return Weights(A_ref, scales_ref, M, K, bits, cfg, scales_dtype, dev_dtype, on_device)
        check(B.lib().tmac_hip_set_fast_aggregation(int(fast_aggregation)))
        try:
            return Weights(A_ref, scales_ref, M, K, bits, cfg, scales_dtype, dev_dtype, on_device)
        finally:
            B.lib().tmac_hip_set_fast_aggregation(0)

    def register_gptq(self, qweight, scales, qzeros, cfg: Optional[KCfg] = None, gptq_v2: bool = True, dev_dtype=F16, stream=None,
                      g_idx=None, bias=None) -> Weights:
        """``Weights.from_gptq`` with this wrapper's act_group_size: GPTQ tensors (CUDA tensors, or numpy arrays uploaded first) -> handle,
        the blob packed on the GPU.  ``g_idx``: an act-order checkpoint's group indices (tensor, array or KPerm); ``bias``: the layer's [Mw]"""
        return Weights.from_gptq(qweight, scales, qzeros, cfg, gptq_v2, dev_dtype, self._act_group_size, stream, g_idx, bias)

    def register_awq(self, qweight, scales, qzeros, cfg: Optional[KCfg] = None, dev_dtype=F16, stream=None, bias=None) -> Weights:
        """``Weights.from_awq`` with this wrapper's act_group_size: AutoAWQ GEMM tensors (CUDA tensors, or numpy arrays uploaded first) ->
        handle, the blob packed on the GPU"""
        return Weights.from_awq(qweight, scales, qzeros, cfg, dev_dtype, self._act_group_size, stream, bias)

    def register_codes(self, codes, scales, zeros, bits: int, cfg: Optional[KCfg] = None, dev_dtype=F16, stream=None, g_idx=None,
                       bias=None) -> Weights:
        """``Weights.from_codes`` with this wrapper's act_group_size"""
        return Weights.from_codes(codes, scales, zeros, bits, cfg, dev_dtype, self._act_group_size, stream, g_idx, bias)

    def register_bitnet(self, weight, cfg: Optional[KCfg] = None, m_groups: int = 1, eps: float = 1e-5, scale=None, dev_dtype=F32,
                        stream=None) -> Weights:
        """``Weights.from_bitnet``: BitNet master weights (fp32 / fp16 / bf16) -> handle, quantised and packed on the GPU.  (Unified
        scales have one activation group per row: the wrapper's act_group_size plays no part.)"""
        return Weights.from_bitnet(weight, cfg, m_groups, eps, scale, dev_dtype, stream)

    def register_bitnet_packed(self, packed, weight_scale, cfg: Optional[KCfg] = None, linear_class: str = "autobitlinear", dev_dtype=F32,
                               stream=None) -> Weights:
        """``Weights.from_bitnet_packed``: a layer of a packed ternary BitNet checkpoint (uint8 [Mw/4][K] + its weight_scale) -> handle"""
        return Weights.from_bitnet_packed(packed, weight_scale, cfg, linear_class, dev_dtype, stream)

    def register_dense(self, weight, bits: int, group_size: int = 128, zero_point: bool = True, cfg: Optional[KCfg] = None, dev_dtype=F16,
                       stream=None, bias=None) -> Weights:
        """``Weights.from_dense`` with this wrapper's act_group_size: an unquantised matrix (fp32 / fp16 / bf16) -> a W1 - W4 handle with
        per-group scales, quantised (round to nearest) and packed on the GPU"""
        return Weights.from_dense(weight, bits, group_size, zero_point, cfg, dev_dtype, self._act_group_size, stream, bias)

    def llama_cpp_init(self, B_dev, M: int, K: int, N: int, bits: int, act_group_size: Optional[int] = None,
                       act_dtype: Optional[int] = None, stream=None, kperm: Optional[KPerm] = None) -> None:
        """preprocessor_int8(M*bits, K, N, bits, B, lut_scales, lut_biases, qlut) on the device.  ``kperm``: the LUT of act-order weights
        (``Weights.kperm``), built from B[:, perm] (tmac_hip_preprocessor_perm_dev); llama_cpp_compute refuses a mismatch."""
        ags = act_group_size or self._act_group_size
        if act_dtype is None:
            act_dtype = _dtype_code(B_dev)
        if kperm is not None:
            check(B.lib().tmac_hip_preprocessor_perm_dev(self.workspace.handle, _ptr(B_dev), act_dtype, K, N, ags, kperm.handle, _stream(stream)))
            return
        check(B.lib().tmac_hip_preprocessor_dev(self.workspace.handle, _ptr(B_dev), act_dtype, K, N, ags, _stream(stream)))

    def llama_cpp_compute(self, weights: Weights, C_dev, N: int = 1, out_dtype: Optional[int] = None, stream=None) -> None:
        """qgemm_lut_int8 over ALL M-tiles of the registered matrix in one launch."""
        if out_dtype is None:
            out_dtype = _dtype_code(C_dev)
        check(B.lib().tmac_hip_qgemm_dev(weights.handle, self.workspace.handle, _ptr(C_dev), out_dtype, N, _stream(stream)))

    def fused(self, weights_list, B_dev, C_list, N: int = 1, act_dtype: Optional[int] = None,
              out_dtype: Optional[int] = None, stream=None) -> None:
        """llama_cpp_init + llama_cpp_compute in ONE launch for up to 4 matrices that share the activation
        rows B_dev (q/k/v, gate/up): tmac_hip_qgemm_fused_dev.  The LUT is built inside the kernel."""
        n = len(weights_list)
        if act_dtype is None:
            act_dtype = _dtype_code(B_dev)
        if out_dtype is None:
            out_dtype = _dtype_code(C_list[0])
        # keyed by the native handle VALUES (an id() can be reused once a Weights object is collected); the arrays
        # hold raw handles, so an entry is dropped when any of its weights is freed (see Weights.free / _forget)
        key = (tuple(w.handle.value for w in weights_list), tuple(_ptr(c) for c in C_list))
        cache = self.__dict__.setdefault("_fused_cache", {})
        if key not in cache:   # the ctypes pointer arrays are reused across calls (cheap host path)
            if len(cache) > 4096:
                cache.clear()
            wa = (C.c_void_p * n)(*[w.handle.value for w in weights_list])
            ca = (C.c_void_p * n)(*[_ptr(c) for c in C_list])
            cache[key] = (wa, ca)
            for w in weights_list:
                w._caches.append(cache)
        wa, ca = cache[key]
        rec = getattr(self, "_recording", None)
        if rec is not None:
            rec.append((list(weights_list), B_dev, list(C_list)))
        check(B.lib().tmac_hip_qgemm_fused_dev(wa, n, _ptr(B_dev), act_dtype, ca, out_dtype, N, _stream(stream)))

    def record_gather(self, send_dev, recv_dev, bytes_per_rank: int, rank: int, world: int) -> None:
        """while recording a chain: the exchange step ``recv = all-gather over the ranks of send`` (what ``Comm.allgather`` records
        by itself); inside the launch it becomes part of the hand-off"""
        rec = getattr(self, "_recording", None)
        if rec is not None:
            rec.append((send_dev, recv_dev))
        check(B.lib().tmac_hip_chain_record_gather(_ptr(send_dev), _ptr(recv_dev), bytes_per_rank, rank, world))

    CARRY = "carry"
    _XF_KINDS = {None: 0, "norm": 1, "glu": 2, "glu_norm": 4}      # TMAC_XF_* (3 is not a kind)
    _XF_GATES = {"silu": 0, "relu2": 0x100, "gelu": 0x200}         # TMAC_XF_GATE_*: bits 8..15 of the kind

    @staticmethod
    def _xf_kind(kind, none_ok: bool = True) -> int:
        """``tmac_hip_xform.kind`` of a kind string: "norm", "glu", "glu_norm", the last two optionally with a gate -- "glu:relu2",
        "glu_norm:gelu", ":silu" = the bare name -- or None (no transform).  An unknown gate name raises ValueError, an unknown kind
        KeyError; a gate on a kind that takes none ("norm:relu2") is left to the library, which refuses it.  An int is passed through
        (tests of the library's own refusals)."""
        if isinstance(kind, int):
            return kind
        kinds = TMACGeMMWrapper._XF_KINDS
        if kind is None:
            if not none_ok:
                raise KeyError(kind)
            return kinds[None]
        base, sep, gate = kind.partition(":")
        if sep and gate not in TMACGeMMWrapper._XF_GATES:
            raise ValueError(f"unknown gate {gate!r} in transform kind {kind!r}: one of {sorted(TMACGeMMWrapper._XF_GATES)}")
        if base not in kinds:
            raise KeyError(kind)
        return kinds[base] | (TMACGeMMWrapper._XF_GATES[gate] if sep else 0)

    @staticmethod
    def _xform(kind, in2, residual, gamma, eps, residual_out, keep, none_ok) -> "B.XForm":
        """the ``tmac_hip_xform`` of a transform given as the methods below take it (``residual`` may be ``CARRY``)"""
        xf = B.XForm()
        xf.kind = TMACGeMMWrapper._xf_kind(kind, none_ok=none_ok)
        xf.in2 = _ptr(in2) if in2 is not None else None
        xf.residual = 1 if residual is TMACGeMMWrapper.CARRY else (_ptr(residual) if residual is not None else None)
        xf.gamma = _ptr(gamma) if gamma is not None else None
        xf.eps = float(eps)
        xf.residual_out = _ptr(residual_out) if residual_out is not None else None
        xf.keep = 1 if keep else 0
        return xf

    def chain_xform(self, kind: str, in2=None, residual=None, gamma=None, eps: float = 1e-5, residual_out=None, keep: bool = False) -> None:
        """while recording a chain: a vector transform of the NEXT ``fused`` call's activations, applied inside its LUT build
        (tmac_hip_chain_xform).  kind "norm": t = in + residual (fp32 tensor, None, or ``TMACGeMMWrapper.CARRY`` = the t the latest
        kept NORM left in LDS); x = t * rsqrt(mean(t^2) + eps) * gamma (x = t without gamma); residual_out: t also goes to memory;
        keep: leave t for a later CARRY.  kind "glu": x = silu(in) * in2.  kind "glu_norm": g = silu(in) * in2, x = g * rsqrt(mean(g^2) +
        eps) * gamma (gamma required, no residual operand); recorded only where the gate/up call in front publishes g itself.
        Another gate in the place of silu rides in the string: "glu:relu2" (max(in, 0)^2 * in2), "glu:gelu" (tanh-approximated GELU),
        "glu_norm:relu2" (BitNet b1.58 2B-4T's FFN), "glu_norm:gelu"; ":silu" is the bare name."""
        xf = self._xform(kind, in2, residual, gamma, eps, residual_out, keep, none_ok=False)
        rec = getattr(self, "_recording", None)
        if rec is not None:
            rec.append((in2, residual, gamma, residual_out))      # kept alive with the chain
        check(B.lib().tmac_hip_chain_xform(C.byref(xf)))

    def fused_xf(self, weights_list, B_dev, C_list, kind, in2=None, residual=None, gamma=None, eps: float = 1e-5, residual_out=None,
                 act_dtype: Optional[int] = None, out_dtype: Optional[int] = None, stream=None) -> None:
        """``fused`` (N = 1) with a vector transform of the activations applied inside the kernel's LUT build
        (tmac_hip_qgemm_fused_xf_dev): kind "norm" / "glu" / "glu_norm" (the last two with an optional ":relu2" / ":gelu" gate) as in ``chain_xform``, or None (a plain ``fused`` call).  Outside a
        recording the call launches by itself -- residual ``CARRY`` is refused there, and residual_out must not overlap a vector the
        call reads; inside ``record_chain()`` it records the transform and the call."""
        n = len(weights_list)
        if act_dtype is None:
            act_dtype = _dtype_code(B_dev)
        if out_dtype is None:
            out_dtype = _dtype_code(C_list[0])
        xf = self._xform(kind, in2, residual, gamma, eps, residual_out, False, none_ok=True)
        wa = (C.c_void_p * n)(*[w.handle.value for w in weights_list])
        ca = (C.c_void_p * n)(*[_ptr(c) for c in C_list])
        rec = getattr(self, "_recording", None)
        if rec is not None:      # kept alive with the chain
            rec.append((list(weights_list), B_dev, list(C_list), in2, residual, gamma, residual_out))
        check(B.lib().tmac_hip_qgemm_fused_xf_dev(wa, n, _ptr(B_dev), act_dtype, C.byref(xf) if kind is not None else None, ca, out_dtype,
                                                  _stream(stream)))

    def fused_xf_rows(self, weights_list, B_dev, C_list, kind, N, in2=None, residual=None, gamma=None, eps: float = 1e-5, residual_out=None,
                      act_dtype: Optional[int] = None, out_dtype: Optional[int] = None, stream=None) -> None:
        """``fused_xf`` for N activation rows (tmac_hip_qgemm_fused_xf_rows_dev): B_dev and in2 [N][K], residual and residual_out fp32
        [N][K], gamma fp32 [K] shared by the rows, C_list[i] [N][Mw_i].  N = 1 is ``fused_xf`` itself, kind None is ``fused`` itself;
        for N >= 2 the transform is applied inside the LUT build of the route ``fused`` would take.  Not recordable for N >= 2."""
        n = len(weights_list)
        if act_dtype is None:
            act_dtype = _dtype_code(B_dev)
        if out_dtype is None:
            out_dtype = _dtype_code(C_list[0])
        xf = self._xform(kind, in2, residual, gamma, eps, residual_out, False, none_ok=True)
        wa = (C.c_void_p * n)(*[w.handle.value for w in weights_list])
        ca = (C.c_void_p * n)(*[_ptr(c) for c in C_list])
        rec = getattr(self, "_recording", None)
        if rec is not None and N == 1:      # kept alive with the chain
            rec.append((list(weights_list), B_dev, list(C_list), in2, residual, gamma, residual_out))
        check(B.lib().tmac_hip_qgemm_fused_xf_rows_dev(wa, n, _ptr(B_dev), act_dtype, C.byref(xf) if kind is not None else None, ca, out_dtype,
                                                       N, _stream(stream)))

    def xf_rows_tap(self, B_dev, x_out, kind, K, N, in2=None, residual=None, gamma=None, eps: float = 1e-5, residual_out=None,
                    act_dtype: Optional[int] = None, stream=None) -> None:
        """the fp32 x [N][K] that the LUT builds of ``fused_xf_rows`` consume, into ``x_out`` (tmac_hip_debug_xf_rows); residual_out is
        written as the call writes it.  Synchronises the stream."""
        if act_dtype is None:
            act_dtype = _dtype_code(B_dev)
        xf = self._xform(kind, in2, residual, gamma, eps, residual_out, False, none_ok=True)
        check(B.lib().tmac_hip_debug_xf_rows(_ptr(B_dev), act_dtype, C.byref(xf), K, N, _ptr(x_out), _stream(stream)))

    def record_chain(self, independent: bool = False) -> "_ChainRecorder":
        """``with wr.record_chain() as rec: <the token's wr.fused(...) calls>`` — the calls are noted instead of launched;
        afterwards ``rec.chain.launch()`` executes all of them in ONE persistent kernel launch (tmac_hip_chain_*).
        ``independent=True`` (tmac_hip_chain_begin_independent): the calls are declared to carry no data flow -- the chain is a
        stream-mode one or the block's exit raises (TMAC_HIP_E_ARG naming the offending call); transforms are refused inside, and
        calls on act-order handles are noted."""
        return _ChainRecorder(self, independent)

    def autotune(self, weights_list, act_dtype=F16, out_dtype=F16):
        """Measure the launch configurations of the fused decode kernel on these matrices (the list ``fused`` will be
        called with) and keep the fastest: ``tmac_hip_autotune_fused``.  Returns dict(ft, wpq, us, heuristic_us);
        ft == 0 means the built-in heuristic was kept."""
        n = len(weights_list)
        wa = (C.c_void_p * n)(*[w.handle.value for w in weights_list])
        ft, wpq, us, hus = C.c_int(0), C.c_int(0), C.c_float(0), C.c_float(0)
        check(B.lib().tmac_hip_autotune_fused(wa, n, act_dtype, out_dtype, C.byref(ft), C.byref(wpq), C.byref(us), C.byref(hus)))
        return dict(ft=ft.value, wpq=wpq.value, us=us.value, heuristic_us=hus.value)

    @staticmethod
    def tune_save(path: str) -> int:
        return check_count(B.lib().tmac_hip_tune_save(path.encode()))

    @staticmethod
    def tune_load(path: str) -> int:
        return check_count(B.lib().tmac_hip_tune_load(path.encode()))

    def fused_partial_sums(self, weights: Weights, B_dev, N: int = 1, act_dtype: Optional[int] = None, stream=None):
        """Parity tap of the fused kernel: (int32 PS as partial_sums(), fp32 C [N][Mw]); the in-kernel LUT
        scales/biases are left in ``self.last_fused_lut``."""
        if act_dtype is None:
            act_dtype = _dtype_code(B_dev)
        s_final = weights.cfg.m_groups >= 1 and weights.cfg.act_group_size == weights.K
        G = 1 if s_final else weights.K // weights.cfg.act_group_size
        ps = np.zeros((N, weights.Mw * weights.bits, G), np.int32)
        c = np.zeros((N, weights.Mw), np.float32)
        lut = np.zeros((N, 2, weights.K // weights.cfg.act_group_size), np.float32)
        check(B.lib().tmac_hip_qgemm_fused_partial_sums(weights.handle, _ptr(B_dev), act_dtype, ps.ctypes.data,
                                                        c.ctypes.data, lut.ctypes.data, N, _stream(stream)))
        self.last_fused_lut = lut   # [N][0] = LUT scales, [N][1] = LUT biases built inside the kernel
        return ps, c

    def comb_sums(self, weights: Weights, N: int, stream=None) -> np.ndarray:
        """Parity tap of the plane-combined GEMM (k_gemm_planes): int32 [N][Mw][K/64], sum_p 2^p PS_p."""
        G = 1 if weights.cfg.m_groups >= 1 else weights.K // 64
        out = np.zeros((N, weights.Mw, G), np.int32)
        check(B.lib().tmac_hip_debug_gemm_comb_sums(weights.handle, self.workspace.handle, out.ctypes.data, N, _stream(stream)))
        return out

    def rows_comb_sums(self, weights: Weights, N: int, stream=None) -> np.ndarray:
        """Parity tap of the rows kernel (k_gemv_rows): int32 [N][Mw][K/64], sum_p 2^p PS_p; unified scales: [N][Mw][bits] plane totals."""
        G = weights.bits if weights.cfg.m_groups >= 1 else weights.K // 64
        out = np.zeros((N, weights.Mw, G), np.int32)
        check(B.lib().tmac_hip_debug_rows_comb_sums(weights.handle, self.workspace.handle, out.ctypes.data, N, _stream(stream)))
        return out

    def partial_sums(self, weights: Weights, N: int = 1, stream=None) -> np.ndarray:
        """Parity tap: int32 [N][M][K/ags] (or [N][M] for the unified-scale path), M-space row order."""
        s_final = weights.cfg.m_groups >= 1 and weights.cfg.act_group_size == weights.K
        G = 1 if s_final else weights.K // weights.cfg.act_group_size
        out = np.zeros((N, weights.Mw * weights.bits, G), np.int32)
        check(B.lib().tmac_hip_qgemm_partial_sums(weights.handle, self.workspace.handle, out.ctypes.data, N, _stream(stream)))
        return out
