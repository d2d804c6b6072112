"""What the vector-transform GPU tests share (test_gpu_xf*.py, test_gpu_chain_xform.py, test_gpu_chain_gate.py, test_gpu_sequences.py and
the transform part of test_gpu_footprint.py): one registered matrix with its oracle, the numpy references of the transforms, and the small
device helpers.  A plain module like footprint.py: no test, no fixture.
"""
import numpy as np

from oracle import oracle as orc

KF = 16


def rel_err(c, ref):
    return float(np.abs(c.astype(np.float64) - ref.astype(np.float64)).max() / max(np.abs(ref).max(), 1e-30))


def pick_bm(Mw, bits):
    """the largest bm of the usual ones that tiles M = Mw * bits (registration: bm % 32, (bm / bits) % 8, M % bm)"""
    return next(b for b in {1: (128, 32), 2: (128, 32), 3: (192, 96), 4: (256, 128, 32)}[bits] if (Mw * bits) % b == 0)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.float().cpu().numpy()


def poison(shape, dtype):
    """a device tensor of NaNs; shape: an int or a tuple"""
    import torch
    return torch.full(shape if isinstance(shape, tuple) else (shape,), float("nan"), dtype=dtype, device="cuda")


class Mat:
    """one matrix with scales sized so that its outputs are O(1) for O(1) inputs.  m_groups >= 1: unified scales, one act group per row.
    Per-group scales: zero points unless zp=False, act groups of `ags` (32: kfactor 8), device scales fp16 unless dev_dtype says otherwise,
    fa: the fast-aggregation mode the weights are registered under."""

    def __init__(self, tm, wr, seed, Mw, K, bits=2, gs=128, zp=True, m_groups=-1, ags=64, fa=0, dev_dtype=None):
        self.Mw, self.K, self.bits, self.gs, self.mg, self.zp = Mw, K, bits, gs, m_groups, zp and m_groups < 1
        self.ags = K if m_groups >= 1 else ags
        self.bm = pick_bm(Mw, bits)
        c = 1.0 / np.sqrt(2.5 * K)
        kf = KF if self.ags != 32 else 8
        if m_groups >= 1:
            case = orc.make_case(seed, Mw, K, bits=bits, ags=K, m_groups=m_groups, zero_point=False)
            self.S = (case["sc"] * c).astype(np.float32)
            cfg = tm.KCfg.make(Mw, K, bits, self.bm, kf, gs, K, False, m_groups)
            self.A = orc.preprocess_weights(case["w"], bits, self.bm, kf)
            self.w = wr.register_weights(self.A, self.S, Mw, K, bits, cfg, scales_dtype=tm.F32, dev_dtype=tm.F32)
            return
        case = orc.make_case(seed, Mw, K, bits=bits, gs=gs, ags=self.ags, zero_point=self.zp, fp16_values=True)
        sc = (case["sc"] * c).astype(np.float16).astype(np.float32)
        zr = None
        if self.zp:
            lvl = (2 ** bits - 1) / 2.0 - 2 ** (bits - 1)
            zr = (case["zr"] * c + lvl * sc).astype(np.float16).astype(np.float32)
        self.A = orc.preprocess_weights(case["w"], bits, self.bm, kf)
        self.S = orc.preprocess_scales(sc, zr, bits, self.bm)
        cfg = tm.KCfg.make(Mw, K, bits, self.bm, kf, gs, self.ags, self.zp, -1)
        self.w = wr.register_weights(self.A, self.S, Mw, K, bits, cfg, scales_dtype=tm.F32, dev_dtype=tm.F16 if dev_dtype is None else dev_dtype,
                                     fast_aggregation=fa)

    def oracle(self, x):
        """fp32 outputs of the oracle on fp32 activations: [Mw] for a vector x [K], [N][Mw] for rows x [N][K]"""
        X = np.ascontiguousarray(x if x.ndim == 2 else x[None, :], np.float32)
        N = X.shape[0]
        q, ls, lb = orc.preprocessor(X, self.ags)
        if self.mg >= 1:
            out = orc.qgemm_scale_final(self.A, q, self.S, ls[:, 0], lb[:, 0], self.Mw, self.K, N, self.bits, self.bm, KF, self.mg)[0]
        else:
            out = orc.qgemm_float(self.A, q, self.S, ls, lb, self.Mw, self.K, N, self.bits, self.bm, KF, self.gs, self.ags, self.zp)
        return out if x.ndim == 2 else out[0]


# ---- the transforms in numpy, float32 (the mean square in float64, rounded once) ----
def np_norm(t, gamma, eps):
    """RMSNorm over the last axis: a vector [K], or rows [N][K] one by one (gamma [K] shared)"""
    t = t.astype(np.float32)
    rs = np.float32(1.0) / np.sqrt((t.astype(np.float64) ** 2).mean(axis=-1, keepdims=True).astype(np.float32) + np.float32(eps))
    return (t * rs).astype(np.float32) * gamma.astype(np.float32)


def np_glu(a, b):
    a = a.astype(np.float32); b = b.astype(np.float32)
    return (a / (np.float32(1.0) + np.exp(-a))).astype(np.float32) * b


def np_relu2(a, b):
    a = a.astype(np.float32); b = b.astype(np.float32)
    return (np.maximum(a, 0) ** 2 * b).astype(np.float32)


def np_gelu(a, b):
    a = a.astype(np.float32); b = b.astype(np.float32)
    return (np.float32(0.5) * a * (np.float32(1) + np.tanh(np.float32(0.7978845608) * (a + np.float32(0.044715) * a ** 3))) * b).astype(np.float32)


NP_GATE = {"relu2": np_relu2, "gelu": np_gelu}


def np_gated(kind, a, b, gamma, eps=1e-5, handed_over_f16=False):
    """the vector (or rows) a call of kind "glu:<gate>" / "glu_norm:<gate>" builds its tables from; handed_over_f16: the product went
    through a chain's fp16 hand-off first"""
    base, gate = kind.split(":")
    g = NP_GATE[gate](a, b)
    if handed_over_f16:
        g = g.astype(np.float16).astype(np.float32)
    return np_norm(g, gamma, eps) if base == "glu_norm" else g
