"""Shared by tests/test_gpu_hostptr_purity.py and its child-process script tests/hostptr_purity_child.py: the host-pointer ABI
(preprocessor_int8 / qgemm_lut_int8, include/tmac_hip.h layer 1) driven tile by tile through ctypes, and the oracle's result for
the bytes that are in the caller's buffers at the moment of the call.

Bars (tests/test_gpu_hostptr.py, tests/test_gpu_parity.py): QLUT, lut_scales and lut_biases from preprocessor_int8 bit-exact;
outputs max|diff| / max|ref| <= 2e-5.  A staleness test first asserts, on the CPU, that the oracle's outputs for the old and the
new bytes differ by more than 2e-3 max|C| (100 x the bar) in at least half the rows of every tile it calls, so that a stale tile
cannot pass under the tolerance."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from oracle import oracle as orc

BAR = 2e-5
APART = 2e-3


def vp(a):
    return C.c_void_p(a.ctypes.data)


@dataclass(frozen=True)
class Cfg:
    """one kcfg section: Mw output rows in tiles of bm / bits rows; ss > 0 = unified scale with scales_size = ss (else per-group scales)"""
    Mw: int
    K: int
    bits: int
    bm: int
    kf: int = 16
    gs: int = 128
    ags: int = 64
    zp: bool = True
    ss: int = 0
    N: int = 1

    @property
    def rpt(self):
        return self.bm // self.bits

    @property
    def ntile(self):
        return self.Mw // self.rpt

    def section(self):
        scales = self.ss if self.ss else self.Mw * (self.K // self.gs) * (2 if self.zp else 1)
        return (f"[qgemm_lut_t1_int8_m{self.Mw * self.bits}_k{self.K}_n{self.N}_b{self.bits}]\nbm = {self.bm}\nsimd_n_in = 16\nsimd_n_out = 8\n"
                f"kfactor = {self.kf}\ngroup_size = {self.gs}\nlut_scales_size = {self.N * self.K // self.ags}\nscales_size = {scales}\n"
                f"n_tile_num = {self.ntile}\n\n")

    def with_n(self, n):
        return Cfg(self.Mw, self.K, self.bits, self.bm, self.kf, self.gs, self.ags, self.zp, self.ss, n)


def load_kcfg(L, path, cfgs):
    """the sections of `cfgs` become the whole kcfg table"""
    with open(path, "w") as f:
        f.write("".join(dict.fromkeys(c.section() for c in cfgs)))
    assert L.tmac_hip_load_kcfg_ex(str(path).encode(), 1) == 0, L.tmac_hip_last_error()


class Matrix:
    """weights and scales in the reference layout, tile after tile, in arrays of the caller's that are edited in place"""

    def __init__(self, cfg, seed, scale_values=None):
        self.cfg = cfg
        self.A = np.zeros((cfg.ntile, cfg.K // 4, cfg.bm // 2), np.uint8)
        if cfg.ss:
            self.S = np.zeros(cfg.ss, np.float32)
        else:
            self.S = np.zeros((cfg.ntile, cfg.K // cfg.gs, cfg.rpt * (2 if cfg.zp else 1)), np.float32)
        self.fill(seed, scale_values)

    def fill(self, seed, scale_values=None):
        """another matrix copied over the same arrays"""
        c = self.cfg
        case = orc.make_case(seed, c.Mw, c.K, bits=c.bits, gs=c.gs, ags=c.ags, zero_point=c.zp, m_groups=c.ss if c.ss else -1)
        self.A[...] = orc.preprocess_weights(case["w"], c.bits, c.bm, c.kf)
        if c.ss:
            self.S[...] = case["sc"] if scale_values is None else np.asarray(scale_values, np.float32)
        else:
            self.S[...] = orc.preprocess_scales(case["sc"], case["zr"] if c.zp else None, c.bits, c.bm)

    def scales_of(self, t):
        """the scale pointer a caller passes with tile t (unified scale: Scales + m / m_group_size, qgemm.py:147-150)"""
        c = self.cfg
        return self.S[t * c.ss // c.ntile:] if c.ss else self.S[t]

    def expect(self, lut, n=1):
        """the oracle's [n][Mw] for the bytes that A, S and the LUT buffers hold now"""
        c = self.cfg
        q, ls, lb = lut.q[:n], lut.ls[:n], lut.lb[:n]
        if not c.ss:
            return orc.qgemm_float(self.A, q, self.S, ls, lb, c.Mw, c.K, n, c.bits, c.bm, c.kf, c.gs, c.ags, c.zp)
        if c.ags == c.K:
            return orc.qgemm_scale_final(self.A, q, self.S, ls[:, 0], lb[:, 0], c.Mw, c.K, n, c.bits, c.bm, c.kf, c.ss)[0]
        tpg = c.ntile // c.ss          # one weight scale per row block, per-group LUT scales: the oracle takes one block at a time
        return np.concatenate([orc.qgemm_float(self.A[g * tpg:(g + 1) * tpg], q, self.S[g:g + 1], ls, lb, c.Mw // c.ss, c.K, n, c.bits, c.bm,
                                               c.kf, c.gs, c.ags, False, one_scale=True) for g in range(c.ss)], axis=1)


class Lut:
    """ONE set of caller-owned LUT buffers (QLUT, LUT_Scales, LUT_Biases) for up to n activation rows"""

    def __init__(self, K, ags, n=1):
        self.K, self.ags, self.n = K, ags, n
        self.q = np.zeros((n, K // 4, 16), np.int8)
        self.ls = np.zeros((n, K // ags), np.float32)
        self.lb = np.zeros((n, K // ags), np.float32)

    def write(self, B):
        """caller-built: the oracle's LUT of B written into the buffers in place; the library's preprocessor is not called"""
        q, ls, lb = orc.preprocessor(np.atleast_2d(B), self.ags)
        n = q.shape[0]
        self.q[:n], self.ls[:n], self.lb[:n] = q, ls, lb

    def preprocess(self, L, B, m, bits):
        """preprocessor_int8 into the buffers, bit-exact against the oracle"""
        B = np.ascontiguousarray(np.atleast_2d(B), np.float32)
        n = B.shape[0]
        assert L.preprocessor_int8(m, self.K, n, bits, vp(B), vp(self.ls), vp(self.lb), vp(self.q)) == 0, L.tmac_hip_last_error()
        q, ls, lb = orc.preprocessor(B, self.ags)
        assert np.array_equal(self.q[:n], q), "QLUT"
        assert np.array_equal(self.ls[:n].view(np.uint32), ls.view(np.uint32)), "lut_scales"
        assert np.array_equal(self.lb[:n].view(np.uint32), lb.view(np.uint32)), "lut_biases"

    def snapshot(self):
        return self.q.copy(), self.ls.copy(), self.lb.copy()


def gemv(L, mat, lut, tile_order, n=1):
    """the tile calls of one GEMV in the order given; [n][Mw], NaN where no tile was called"""
    c = mat.cfg
    out = np.full((n, c.Mw), np.nan, np.float32)
    for t in tile_order:
        ct = np.zeros((n, c.rpt), np.float32)         # the C tile is [n][bm / bits]
        rc = L.qgemm_lut_int8(c.bm, c.K, n, c.bits, vp(mat.A[t]), vp(lut.q), vp(mat.scales_of(t)), vp(lut.ls), vp(lut.lb), vp(ct))
        assert rc == 0, L.tmac_hip_last_error()
        out[:, t * c.rpt:(t + 1) * c.rpt] = ct
    return out


def rows_of(cfg, tiles):
    return np.concatenate([np.arange(t * cfg.rpt, (t + 1) * cfg.rpt) for t in tiles])


def rel_err(c, ref):
    return float(np.abs(c.astype(np.float64) - ref.astype(np.float64)).max() / max(np.abs(ref).max(), 1e-30))


def check(L, mat, lut, tile_order, n=1, tag=""):
    """one GEMV against the oracle's result for the bytes in the buffers now, every activation row on its own"""
    want = mat.expect(lut, n)
    got = gemv(L, mat, lut, tile_order, n)
    idx = rows_of(mat.cfg, tile_order)
    for i in range(n):
        err = rel_err(got[i, idx], want[i, idx])
        assert err <= BAR, (tag, "row", i, err)
    return want


def assert_apart(cfg, old, new, tiles, tag=""):
    """premise of a staleness test: the old result cannot pass for the new one in any tile that is called"""
    lim = APART * float(np.abs(new).max())
    for t in tiles:
        r = rows_of(cfg, [t])
        far = np.abs(old[:, r].astype(np.float64) - new[:, r].astype(np.float64)) > lim
        assert (far.sum(axis=1) * 2 >= cfg.rpt).all(), (tag, "tile", t, far.sum(axis=1), cfg.rpt)


def acts(seed, K, n=1):
    """activations on a 1/64 grid: every sum of 64 of them is exact in fp32, whatever the order"""
    return (np.round(np.random.default_rng(seed).standard_normal((n, K)) * 64) / 64).astype(np.float32)
