"""Weight group size 64 on the persistent decode paths: k_decode_chain, stream mode (k_lut_images + k_gemv_stream, both forms) and the
deferred queue's batching.

A lane of a (row quad, 64-unit step) item owns four units = two act groups of 64.  With scale groups of 64 those are two scale groups,
and the kernels run the instantiations whose fragment carries a second scale word (G2, tmac_chain_core.h).  Bars, the project's own:

  * the integers of every call, written by the persistent launch itself (tmac_hip_chain_set_tap): array_equal to the oracle;
  * fp outputs <= 1e-3 of max|C| against orc.qgemm_float(..., gs = 64, ags = 64, zp) on the vector the call consumed;
  * k_decode_chain and the (row quad x 64 units) stream form: BIT-IDENTICAL to the same call launched on its own through
    tmac_hip_qgemm_fused_dev with tmac_hip_debug_quad_config(tmac_hip_chain_threads(), waves per quad of the call) -- k_gemv_quad has
    served group size 64 all along (tests/test_gpu_parity.py);
  * the quarter-walk stream form (another order of a row's fp32 partial sums): <= 1e-4 (fp32 outputs) / 2e-3 (fp16) of that launch,
    the bound of tests/test_gpu_chain.py's Model.check.

Scales are orc.make_case's: |N(0, 1)| per (row, group), neighbouring groups unrelated -- a kernel that applies one group's scale to
both act groups of a lane misses 1e-3 by orders of magnitude (test_premise_neighbouring_groups_differ pins that on the oracle).

Row counts.  A registered matrix has Mw * bits divisible by its tile height bm, a multiple of 32 with (bm / bits) % 8 == 0: 1- and
3-bit matrices have multiples of 32 rows, 2-bit ones multiples of 16, 4-bit ones multiples of 8.  A 20-row matrix therefore cannot
be registered at any width; the row counts below are the smallest that can: [16] / [32, 16] / [64, 32, 32] at 2 and 4 bits, [32] /
[64, 32] / [64, 32, 32] at 1 and 3 bits, and [24] (six quads, no multiple of 16 rows) at 4 bits, which takes the quarter-walk form
away as 20 rows would.  Where no such row count exists (1 to 3 bits) the (row quad x 64 units) form is taken with TMAC_STREAM_QW=0,
as tests/test_gpu_stream.py does: every (bits, zero points, scale dtype) and every K runs in both forms.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
import footprint as fp

pytestmark = pytest.mark.gpu

KF, AGS = 16, 64
BM_CANDIDATES = {1: (64, 32), 2: (128, 64, 32), 3: (192, 96), 4: (256, 128, 64, 32)}


def bm_for(bits, Mw):
    """the tallest tile of the usual ones that a matrix of Mw rows is made of"""
    for bm in BM_CANDIDATES[bits]:
        if (Mw * bits) % bm == 0:
            return bm
    raise ValueError(f"{Mw} rows of {bits}-bit weights cannot be tiled")


@pytest.fixture(scope="module")
def tm():
    import torch
    import tmac_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert tmac_amd.lib().tmac_hip_device_count() > 0
    return tmac_amd


@pytest.fixture(autouse=True)
def _short_spin(tm):
    # after conftest's per-test reset: a broken hand-off fails in ~0.2 s, not 2 s
    tm.binding.check(tm.lib().tmac_hip_debug_chain_config(0, 1 << 17))


def rel_err(c, ref):
    return float(np.abs(c.astype(np.float64) - ref.astype(np.float64)).max() / max(np.abs(ref).max(), 1e-30))


def bits_of(a):
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


class Model:
    """tests/test_gpu_chain.py's Model with the group size a property of the op: ops = [(K, [Mw, ...], src, gs)], src = None (a vector
    in memory) or (op, matrix) of an earlier op; per-group scales, act groups of 64.  xf = {op: dict(kind="norm", residual=, gamma=) |
    dict(kind="glu", in2=(op, matrix))}: a vector transform in front of that op (tmac_hip_chain_xform)."""

    def __init__(self, tm, ops, bits=2, zp=True, dev_f16=True, out_f16=True, seed=0, weights_fn=None, x_fn=None, out_alloc=None,
                 ext_alloc=None, xf=None, glu_in_producer=False):
        self.tm, self.ops, self.bits, self.zp, self.out_f16, self.xf = tm, ops, bits, zp, out_f16, xf or {}
        # a GLU whose two vectors are the gate / up outputs of ONE earlier call is computed by that call's publishing wave (the default;
        # TMAC_CHAIN_GLU_EPILOGUE=0: inside the reader's LUT build): the hand-off image then carries silu(gate) * up as fp16, so the vector
        # the reader's tables are built from is the fp32 product ROUNDED TO FP16 (tmac_chain.h, ChainOp::epi) -- a plain call on that vector
        self.glu_in_producer = glu_in_producer
        self.wr = tm.TMACGeMMWrapper(act_group_size=AGS)
        rng = np.random.default_rng(seed)
        self.host, self.ws, self.x_host = [], [], {}
        for i, (K, rows, src, gs) in enumerate(ops):
            hs, ws = [], []
            for m, Mw in enumerate(rows):
                bm = bm_for(bits, Mw)
                case = orc.make_case(1000 * seed + 10 * i + m, Mw, K, bits=bits, gs=gs, ags=AGS, zero_point=zp, fp16_values=True)
                w_given = weights_fn(i, m, Mw, K, bits) if weights_fn is not None else None
                if w_given is not None:
                    case["w"] = np.ascontiguousarray(w_given, np.uint8)
                # (test_gpu_chain.Model's sizing: chained activations stay O(1); the groups' scales keep make_case's spread)
                c = 1.0 / np.sqrt(2.5 * K)
                case["sc"] = (case["sc"] * c).astype(np.float16).astype(np.float32)
                if zp:
                    lvl = (2 ** bits - 1) / 2.0 - 2 ** (bits - 1)
                    case["zr"] = (case["zr"] * c + lvl * case["sc"]).astype(np.float16).astype(np.float32)
                else:
                    case["sc"] = (case["sc"] * (4.0 / np.sqrt(K))).astype(np.float16).astype(np.float32)
                A = orc.preprocess_weights(case["w"], bits, bm, KF)
                S = orc.preprocess_scales(case["sc"], case["zr"] if zp else None, bits, bm)
                cfg = tm.KCfg.make(Mw, K, bits, bm, KF, gs, AGS, zp, -1)
                ws.append(self.wr.register_weights(A, S, Mw, K, bits, cfg, scales_dtype=tm.F32, dev_dtype=tm.F16 if dev_f16 else tm.F32))
                hs.append((A, S, bm, case))
            self.host.append(hs); self.ws.append(ws)
            if src is None:
                x = rng.standard_normal(K).astype(np.float16).astype(np.float32)
                x_given = x_fn(i, K) if x_fn is not None else None
                self.x_host[i] = x if x_given is None else np.ascontiguousarray(x_given, np.float32)
        self.allocate(out_alloc, ext_alloc)

    def allocate(self, out_alloc=None, ext_alloc=None):
        import torch
        odt = torch.float16 if self.out_f16 else torch.float32
        self.outs, self.x_ext = [], {}
        for i, (K, rows, src, gs) in enumerate(self.ops):
            self.outs.append([torch.zeros(Mw, dtype=odt, device="cuda") if out_alloc is None else out_alloc(i, m, Mw, odt) for m, Mw in enumerate(rows)])
            if src is None:
                self.x_ext[i] = torch.from_numpy(self.x_host[i]).cuda().half() if ext_alloc is None else ext_alloc(i, self.x_host[i], torch.float16)

    def x_of(self, i, outs=None):
        src = self.ops[i][2]
        return self.x_ext[i] if src is None else (outs or self.outs)[src[0]][src[1]]

    def _xf_args(self, i, outs=None):
        x = dict(self.xf[i])
        kind = x.pop("kind")
        if "in2" in x:
            x["in2"] = (outs or self.outs)[x["in2"][0]][x["in2"][1]]
        return kind, x

    def issue(self, only=None):
        for i in range(len(self.ops)):
            if only is not None and i not in only:
                continue
            if i in self.xf:
                kind, kw = self._xf_args(i)
                self.wr.chain_xform(kind, **kw)
            self.wr.fused(self.ws[i], self.x_of(i), self.outs[i], 1, act_dtype=self.tm.F16)

    def record(self, only=None):
        with self.wr.record_chain() as rec:
            self.issue(only)
        return rec.chain

    def oracle_outputs(self, i, x):
        """the oracle's fp32 outputs of op i on the fp32 vector x its tables are built from"""
        K, rows, _, gs = self.ops[i]
        q, ls, lb = orc.preprocessor(x[None, :].astype(np.float32), AGS)
        return [orc.qgemm_float(A, q, S, ls, lb, Mw, K, 1, self.bits, bm, KF, gs, AGS, self.zp)[0] for (A, S, bm, _), Mw in zip(self.host[i], rows)]

    def transformed(self, i, got):
        """numpy fp32: the vector op i's tables are built from (tests/test_gpu_chain_xform.py's formulas)"""
        x = self.x_of(i, got).float().cpu().numpy()
        if i not in self.xf:
            return x
        kind, kw = self._xf_args(i, got)
        if kind == "glu":
            a, b = x, kw["in2"].float().cpu().numpy()
            y = ((a / (np.float32(1.0) + np.exp(-a))).astype(np.float32) * b).astype(np.float32)
            return y.astype(np.float16).astype(np.float32) if self.glu_in_producer else y
        t = x + kw["residual"].cpu().numpy() if kw.get("residual") is not None else x
        if kw.get("gamma") is None:
            return t
        rs = np.float32(1.0) / np.sqrt(np.float32((t.astype(np.float64) ** 2).mean()) + np.float32(kw.get("eps", 1e-5)))
        return (t * rs).astype(np.float32) * kw["gamma"].cpu().numpy()

    def check(self, chain, report=None):
        """after chain.launch(): every op against its stand-alone launch and against the oracle (the module docstring's bars)"""
        import torch
        L = self.tm.lib()
        torch.cuda.synchronize()
        assert chain.status() == 0, "a hand-off inside the chain timed out"
        got = [[o.clone() for o in os_] for os_ in self.outs]
        for i, (K, rows, src, gs) in enumerate(self.ops):
            x = self.x_of(i, got)
            assert bool(torch.isfinite(x.float()).all()) and float(x.float().abs().max()) > 0, f"op {i}: degenerate activations"
            # (the transformed stand-alone kernel exists for four launch configurations of its own and is compared to a tolerance: it picks)
            if not chain.quarter_walk and i not in self.xf:
                L.tmac_hip_debug_quad_config(chain.threads, chain.wpq(i))
            ref = [torch.empty_like(o) for o in got[i]]
            try:
                if i in self.xf and self.xf[i]["kind"] == "glu" and self.glu_in_producer:
                    # the stand-alone equivalent of the producer's form: a plain call on fp16(silu(gate) * up), the product in fp32
                    g32, u32 = x.float(), self._xf_args(i, got)[1]["in2"].float()
                    x16 = (g32 / (1.0 + torch.exp(-g32)) * u32).half()
                    self.wr.fused(self.ws[i], x16, ref, 1, act_dtype=self.tm.F16)
                elif i in self.xf:
                    kind, kw = self._xf_args(i, got)
                    self.wr.fused_xf(self.ws[i], x, ref, kind, **kw)
                else:
                    self.wr.fused(self.ws[i], x, ref, 1, act_dtype=self.tm.F16)
                torch.cuda.synchronize()
            finally:
                L.tmac_hip_debug_quad_config(0, 0)
            want = self.oracle_outputs(i, self.transformed(i, got))
            for m in range(len(rows)):
                a, b = got[i][m].cpu().numpy(), ref[m].cpu().numpy()
                e_alone, e_orc = rel_err(a.astype(np.float32), b.astype(np.float32)), rel_err(a.astype(np.float32), want[m])
                if report is not None:
                    report.append((i, m, e_alone, e_orc))
                print(f"op {i} matrix {m} K {K} gs {gs}: vs stand-alone {e_alone:.3e}, vs oracle {e_orc:.3e}")
                if i in self.xf:
                    # a transform is specified to a tolerance (tests/test_gpu_chain_xform.py: the mean square is summed in another order,
                    # exp differs in the last bit, and either can move a table entry by one step): 2e-3 against both.  Both references
                    # see the vector in the precision the chain's form of the transform has (fp32, or fp16 for a GLU in the producer)
                    assert e_alone <= 2e-3, f"op {i} matrix {m}: chain vs tmac_hip_qgemm_fused_xf_dev"
                    assert e_orc <= 2e-3, f"op {i} matrix {m} vs oracle"
                    continue
                if chain.quarter_walk:
                    assert e_alone <= (1e-4 if a.dtype == np.float32 else 2e-3), f"op {i} matrix {m}: quarter-walk stream vs stand-alone launch"
                else:
                    assert np.array_equal(bits_of(a), bits_of(b)), f"op {i} matrix {m}: persistent launch != stand-alone launch"
                assert e_orc <= 1e-3, f"op {i} matrix {m} vs oracle"
        return got

    def check_tap(self, chain):
        """the integers of every call as they enter the float part, written by the persistent launch itself: comb[row][act group] =
        sum_p 2^p PS_p -- array_equal to the oracle on the vector the call consumed"""
        import torch
        total, _ = chain.tap_layout(len(self.ops))
        buf = torch.full((total,), -(2 ** 31), dtype=torch.int32, device="cuda")
        chain.set_tap(buf)
        try:
            chain.launch()
            torch.cuda.synchronize()
            assert chain.status() == 0
        finally:
            chain.set_tap(None)
        tap = buf.cpu().numpy()
        got = [[o.clone() for o in os_] for os_ in self.outs]
        for i, (K, rows, src, gs) in enumerate(self.ops):
            q, _, _ = orc.preprocessor(self.transformed(i, got)[None, :], AGS)
            off, cnt = chain.tap_layout(i)
            per_row = K // 64
            assert cnt == sum(rows) * per_row
            r0 = 0
            for m, Mw in enumerate(rows):
                A, _, bm, _ = self.host[i][m]
                PS = orc.partial_sums(A, q[0], Mw, K, self.bits, bm, KF, AGS)
                o = np.arange(Mw)
                want = sum(PS[(o // 8) * 8 * self.bits + p * 8 + (o % 8)].astype(np.int64) << p for p in range(self.bits))
                g = tap[off + r0 * per_row: off + (r0 + Mw) * per_row].reshape(Mw, per_row)
                assert np.array_equal(g.astype(np.int64), want), f"op {i} matrix {m}: integer tap of the persistent kernel != oracle"
                r0 += Mw

    def free(self):
        for ws in self.ws:
            for w in ws:
                w.free()


# -------------------------------------------------------------------------------------------------
# the premise of every fp bar below

def test_premise_neighbouring_groups_differ():
    """orc.make_case's scales: a kernel that served BOTH act groups of a lane with the first one's scale group computes the oracle's
    result for scales whose odd groups are replaced by their even neighbour's.  That result must be far from the true one: > 1e-2 of
    max|C|, ten times the bar the kernels are held to."""
    for bits, zp in ((2, True), (4, False), (1, True)):
        Mw, K = 64, 2112
        bm = bm_for(bits, Mw)
        case = orc.make_case(77 + bits, Mw, K, bits=bits, gs=64, ags=AGS, zero_point=zp, fp16_values=True)
        A = orc.preprocess_weights(case["w"], bits, bm, KF)
        q, ls, lb = orc.preprocessor(case["B"], AGS)

        def out(sc, zr):
            return orc.qgemm_float(A, q, orc.preprocess_scales(sc, zr, bits, bm), ls, lb, Mw, K, 1, bits, bm, KF, 64, AGS, zp)[0]
        true = out(case["sc"], case["zr"])
        sc2 = case["sc"].copy(); sc2[:, 1::2] = sc2[:, 0:-1:2]
        zr2 = None
        if zp:
            zr2 = case["zr"].copy(); zr2[:, 1::2] = zr2[:, 0:-1:2]
        wrong = out(sc2, zr2)
        d = float(np.abs(wrong - true).max() / np.abs(true).max())
        print(f"W{bits} zp={zp}: one scale group for both act groups is off by {d:.3f} of max|C|")
        assert d > 1e-2


# -------------------------------------------------------------------------------------------------
# 1. stream mode, every issue path

def rows_sets(bits):
    return ([16], [32, 16], [64, 32, 32]) if bits in (2, 4) else ([32], [64, 32], [64, 32, 32])


def stream_ops(bits, Ks, odd_rows=False):
    """independent calls: every K of Ks with every row set (K = 64: one group, both words clamp to group 0; 192: three groups, one ragged
    step, the last lane group's second word clamps; 2112: 33 groups, a full step + a ragged one; 4096: two full steps, the pointer-stepped
    path only); multi-matrix calls cross the per-matrix scale pointer, and the last quad of the last matrix is where an unclamped second
    word would leave the scale buffer.  odd_rows (4-bit): a 24-row call, which takes the quarter-walk form away."""
    ops = [(K, list(rows), None, 64) for K in Ks for rows in rows_sets(bits)]
    if odd_rows:
        ops += [(K, [24], None, 64) for K in Ks]
    return ops


def predicted_form(ops, bits, qw_env):
    """plan_stream's rule (tmac_chain_host.cpp): the quarter-walk form (2) needs whole groups of 16 rows in every matrix; 1- / 2-bit
    recordings then always take it, 3- / 4-bit ones when it saves more than 15 % of the items; TMAC_STREAM_QW=0 keeps form 1"""
    if qw_env == 0 or any(Mw % 16 for _, rows, _, _ in ops for Mw in rows):
        return 1
    it64 = sum(sum(Mw // 4 for Mw in rows) * ((K // 32 + 63) // 64) for K, rows, _, _ in ops)
    it16 = sum(sum(Mw // 4 for Mw in rows) // 4 * ((K // 32 + 15) // 16) for K, rows, _, _ in ops)
    return 1 if bits >= 3 and it16 > 0.85 * it64 else 2


SMALL_K, BIG_K = (64, 192, 2112), (4096,)
# Every (bits, zero points, fp16 device scales) triple with all four K, once per form: as recorded -- the three ragged K make the quarter
# walk pay at every width -- and in the (row quad x 64 units) form, forced by a 24-row call at 4 bits and by TMAC_STREAM_QW=0 below that.
# Then K = 4096 on its own, where the rule keeps 3- / 4-bit recordings in form 1 without being told to.  36 cases; the output dtype alternates.
TRIPLES = [(b, z, h) for b in (1, 2, 3, 4) for z in (True, False) for h in (True, False)]
STREAM_CASES = []
for n, (b, z, h) in enumerate(TRIPLES):
    STREAM_CASES.append((b, z, h, n % 2 == 0, "both", "auto"))
    STREAM_CASES.append((b, z, h, n % 2 == 1, "both", "odd" if b == 4 else "qw0"))
STREAM_CASES += [(3, True, True, True, "big", "auto"), (4, True, False, False, "big", "auto"), (3, False, False, True, "big", "auto"),
                 (4, False, True, False, "big", "auto")]


@pytest.mark.parametrize("bits,zp,dev_f16,out_f16,ks,how", STREAM_CASES)
def test_stream_every_issue_path(tm, monkeypatch, bits, zp, dev_f16, out_f16, ks, how):
    Ks = {"small": SMALL_K, "big": BIG_K, "both": SMALL_K + BIG_K}[ks]
    if how == "qw0":
        monkeypatch.setenv("TMAC_STREAM_QW", "0")
    ops = stream_ops(bits, Ks, odd_rows=how == "odd")
    m = Model(tm, ops, bits=bits, zp=zp, dev_f16=dev_f16, out_f16=out_f16, seed=3 + bits)
    chain = m.record()
    mode = int(tm.lib().tmac_hip_chain_is_stream(chain.handle))
    assert mode == predicted_form(ops, bits, 0 if how == "qw0" else -1), mode
    chain.launch()
    m.check(chain)
    m.check_tap(chain)
    chain.free(); m.free()


# -------------------------------------------------------------------------------------------------
# 2. the decode chain

CHAIN_OPS = [(256, [512], None, 64), (512, [256, 256], (0, 0), 64), (256, [64], (1, 1), 64)]


@pytest.mark.parametrize("bits", [2, 4])
def test_decode_chain(tm, bits):
    """three dependent calls, zero points, fp16 hand-offs: every call against its stand-alone launch (bits) and the oracle, the kernel's
    own integers array_equal"""
    m = Model(tm, CHAIN_OPS, bits=bits, zp=True, seed=20 + bits)
    chain = m.record()
    assert not chain.stream and chain.nops == 3
    for rep in range(2):          # the second launch: the generation tag advances
        chain.launch()
        m.check(chain)
    m.check_tap(chain)
    chain.free(); m.free()


@pytest.mark.parametrize("glu_in_producer", [1, 0])
@pytest.mark.parametrize("bits", [2, 4])
def test_decode_chain_with_transforms(tm, monkeypatch, bits, glu_in_producer):
    """a decoder segment in small: x -> [512]; + residual, RMSNorm -> gate / up [256, 256]; silu(gate) * up -> [64].  The NORM and the GLU
    run inside the consumers' LUT builds (XF instance of the G2 kernel); the GLU also in the producer's epilogue (row quads dealt in
    gate / up pairs: the default).  Each transformed call against tmac_hip_qgemm_fused_xf_dev on the same inputs and against the oracle on
    the numpy transform -- for the GLU in the producer, whose product is handed over as fp16, against the plain call and the oracle on the
    product rounded to fp16 (the K = 256 call is off by 1.4e-3 / 2.1e-3 of max|C| from the references fed the unrounded product, measured:
    all 256 elements move by up to half an fp16 ulp and table entries flip by a step)."""
    import torch
    monkeypatch.setenv("TMAC_CHAIN_GLU_EPILOGUE", str(glu_in_producer))
    rng = np.random.default_rng(9)
    res = torch.from_numpy(rng.standard_normal(512).astype(np.float32)).cuda()
    gam = torch.from_numpy((1.0 + 0.1 * rng.standard_normal(512)).astype(np.float32)).cuda()
    ops = [(256, [512], None, 64), (512, [256, 256], (0, 0), 64), (256, [64], (1, 0), 64)]
    m = Model(tm, ops, bits=bits, zp=True, seed=30 + bits, glu_in_producer=bool(glu_in_producer),
              xf={1: dict(kind="norm", residual=res, gamma=gam, eps=1e-5), 2: dict(kind="glu", in2=(1, 1))})
    chain = m.record()
    assert not chain.stream
    for rep in range(2):
        chain.launch()
        m.check(chain)
    chain.free(); m.free()


# -------------------------------------------------------------------------------------------------
# 3. mixed group sizes in one recording

@pytest.mark.parametrize("bits,form", [(2, "auto"), (2, "qw0"), (4, "auto")])
def test_mixed_group_sizes_stream(tm, monkeypatch, bits, form):
    """calls of group size 64 and 128 in one stream launch: all meet the bars, and the outputs of the gs = 128 calls are bit-identical to
    the same calls recorded WITHOUT the gs = 64 ones (a launch of the instantiations of before).  TMAC_STREAM_NCLS=1: every row range
    visits every call in both recordings, so a call's waves per quad -- the order of its fp32 partial sums -- cannot depend on what else
    was recorded."""
    import torch
    monkeypatch.setenv("TMAC_STREAM_NCLS", "1")
    if form == "qw0":
        monkeypatch.setenv("TMAC_STREAM_QW", "0")
    ops = [(2176, [64, 32], None, 128), (192, [32, 16], None, 64), (4096, [64], None, 128), (2112, [64, 32, 32], None, 64),
           (256, [32], None, 128), (4096, [32], None, 64)]
    m = Model(tm, ops, bits=bits, zp=True, seed=40 + bits)
    big = [i for i, o in enumerate(ops) if o[3] == 128]
    mixed = m.record()
    assert mixed.stream
    mixed.launch()
    got = m.check(mixed)
    m.check_tap(mixed)
    for os_ in m.outs:
        for o in os_:
            o.zero_()
    plain = m.record(only=big)
    assert plain.stream and plain.quarter_walk == mixed.quarter_walk and [plain.wpq(k) for k in range(len(big))] == [mixed.wpq(i) for i in big]
    plain.launch(); torch.cuda.synchronize()
    for i in big:
        for a, b in zip(got[i], m.outs[i]):
            assert torch.equal(a, b), f"call {i} (gs = 128): its output depends on a gs = 64 call in the same launch"
    mixed.free(); plain.free(); m.free()


@pytest.mark.parametrize("bits", [2, 4])
def test_mixed_group_sizes_chain(tm, monkeypatch, bits):
    """a dependent chain whose middle call has group size 64: every call meets the bars; the gs = 128 call in front of it is
    bit-identical to the same call recorded alone (k_decode_chain without G2), the one behind it to a recording of its own fed the
    vector the mixed chain produced"""
    import torch
    ops = [(256, [512], None, 128), (512, [256, 256], (0, 0), 64), (256, [128], (1, 0), 128)]
    m = Model(tm, ops, bits=bits, zp=True, seed=50 + bits)
    mixed = m.record()
    assert not mixed.stream
    mixed.launch()
    got = m.check(mixed)
    m.check_tap(mixed)
    # the same gs = 128 calls in recordings without a gs = 64 call (a lone call would be a stream: TMAC_CHAIN_STREAM=0 keeps k_decode_chain)
    monkeypatch.setenv("TMAC_CHAIN_STREAM", "0")
    for i in (0, 2):
        x = m.x_of(i, got)
        o = [torch.zeros_like(t) for t in got[i]]
        with m.wr.record_chain() as rec:
            m.wr.fused(m.ws[i], x, o, 1, act_dtype=tm.F16)
        c = rec.chain
        assert not c.stream and c.wpq(0) == mixed.wpq(i)
        c.launch(); torch.cuda.synchronize()
        assert c.status() == 0
        for a, b in zip(got[i], o):
            assert torch.equal(a, b), f"call {i} (gs = 128): its output depends on the gs = 64 call in the same launch"
        c.free()
    mixed.free(); m.free()


# -------------------------------------------------------------------------------------------------
# 4. deferred queue, 5. acceptance where there was refusal

def defer_stats(tm):
    st = [C.c_uint64(0) for _ in range(4)]
    tm.binding.check(tm.lib().tmac_hip_defer_stats(*[C.byref(x) for x in st]))
    return [int(x.value) for x in st]      # flushes, cache hits, stream launches, single calls


def test_deferred_queue_batches_gs64_calls(tm):
    """four independent gs = 64 calls queued: ONE stream launch at the flush, no call launched singly; the second flush of the same
    batch hits the cache of recordings; outputs against the in-order launches (2e-3: the batch may run the quarter-walk form, fp16
    outputs) and the oracle (1e-3)"""
    import torch
    L = tm.lib()
    ops = [(2112, [64, 32], None, 64), (192, [32], None, 64), (4096, [64], None, 64), (1024, [128, 64], None, 64)]
    m = Model(tm, ops, seed=61)
    m.issue(); torch.cuda.synchronize()
    want = [[o.clone() for o in os_] for os_ in m.outs]
    before = defer_stats(tm)
    tm.binding.check(L.tmac_hip_defer(1))
    try:
        for rep in range(2):
            for os_ in m.outs:
                for o in os_:
                    o.zero_()
            m.issue()
            tm.binding.check(L.tmac_hip_flush(None))
            torch.cuda.synchronize()
            flushes, hits, streams, singles = [a - b for a, b in zip(defer_stats(tm), before)]
            assert (flushes, hits, streams, singles) == (rep + 1, rep, rep + 1, 0), (flushes, hits, streams, singles)
            for i, (K, rows, src, gs) in enumerate(ops):
                ref = m.oracle_outputs(i, m.x_host[i])
                for k in range(len(rows)):
                    g = m.outs[i][k].float().cpu().numpy()
                    assert rel_err(g, want[i][k].float().cpu().numpy()) <= 2e-3
                    assert rel_err(g, ref[k]) <= 1e-3
    finally:
        tm.binding.check(L.tmac_hip_defer(0))
    m.free()


@pytest.mark.parametrize("bits", [1, 2, 3, 4])
def test_recording_a_gs64_call_is_accepted(tm, monkeypatch, bits):
    """tmac_hip_chain_end used to refuse group size 64 ("group >= 128"); it returns a chain now, in stream mode (a lone call) and as
    k_decode_chain"""
    m = Model(tm, [(192, [64, 32], None, 64)], bits=bits, seed=70 + bits)
    c = m.record()
    assert c.stream and c.nops == 1
    c.launch(); m.check(c)
    c.free()
    monkeypatch.setenv("TMAC_CHAIN_STREAM", "0")
    c = m.record()
    assert not c.stream
    c.launch(); m.check(c)
    c.free(); m.free()


# -------------------------------------------------------------------------------------------------
# 6. saturating inputs

SAT_WEIGHTS = ["kblocks", "max", "rows", "planes"]       # kblocks: the extreme levels alternate per 64 elements = per scale group


def sat_names(i, m=0):
    return SAT_WEIGHTS[(i + m) % 4], ("spike", "const")[i % 2]       # spike: every table entry +-127


def assert_saturates(m):
    """the oracle alone: the tables and the integers of every call fed from memory are at their limits (orc.assert_saturates), and
    the outputs stay inside fp16"""
    outs = []
    for i, (K, rows, src, gs) in enumerate(m.ops):
        x = m.x_host[i] if src is None else outs[src[0]][src[1]]
        o = [c.astype(np.float16).astype(np.float32) for c in m.oracle_outputs(i, x)]
        for c in o:
            assert np.isfinite(c).all() and 0 < np.abs(c).max() < 65504, f"op {i}: the model leaves fp16"
        outs.append(o)
        if src is None:
            q, _, _ = orc.preprocessor(x[None, :], AGS)
            A, _, bm, _ = m.host[i][0]
            orc.assert_saturates(*sat_names(i), q[0], orc.partial_sums(A, q[0], rows[0], K, m.bits, bm, KF, AGS), AGS, K)


@pytest.mark.parametrize("bits", [2, 4])
@pytest.mark.parametrize("kind", ["stream", "chain"])
def test_saturating_inputs(tm, bits, kind):
    if kind == "stream":
        ops = [(2112, [64, 32], None, 64), (192, [32, 16], None, 64), (4096, [64], None, 64), (64, [16], None, 64)]
    else:
        ops = [(256, [512], None, 64), (512, [256, 256], (0, 0), 64), (256, [64], (1, 1), 64)]
    m = Model(tm, ops, bits=bits, zp=True, seed=80 + bits, weights_fn=lambda i, k, Mw, K, b: orc.hard_weights(sat_names(i, k)[0], Mw, K, b),
              x_fn=lambda i, K: orc.hard_acts(sat_names(i)[1], K))
    assert_saturates(m)
    chain = m.record()
    assert chain.stream == (kind == "stream")
    chain.launch()
    m.check(chain)
    m.check_tap(chain)
    chain.free(); m.free()


# -------------------------------------------------------------------------------------------------
# 7. footprint

@pytest.mark.parametrize("kind", ["stream", "chain"])
def test_footprint(tm, kind):
    """guard bands around the activations and every output, both placements, both guard patterns (tests/footprint.py): no byte outside
    an output changes, and poisoning the guards changes no result"""
    import torch
    if kind == "stream":
        ops = [(2112, [32, 16], None, 64), (192, [32, 16], None, 64)]
    else:
        ops = [(256, [512], None, 64), (512, [256, 256], (0, 0), 64), (256, [64], (1, 1), 64)]
    m = Model(tm, ops, bits=2, zp=True, seed=90)

    def call(alloc):
        m.allocate(out_alloc=lambda i, k, Mw, dt: alloc.out((1, Mw), dt, name=f"C{i}_{k}").view(Mw),
                   ext_alloc=lambda i, x, dt: alloc.inp(x, dt, name=f"B{i}"))
        chain = m.record()
        assert chain.stream == (kind == "stream")
        alloc.arm()
        chain.launch()
        torch.cuda.synchronize()
        assert chain.status() == 0
        call.chains.append(chain)
    call.chains = []

    def check_want(want):
        outs, prev = {}, []
        for i, (K, rows, src, gs) in enumerate(ops):
            x = m.x_host[i] if src is None else prev[src[0]][src[1]]
            ref = m.oracle_outputs(i, x)
            prev.append([want[f"C{i}_{k}"].reshape(-1).astype(np.float32) for k in range(len(rows))])
            for k in range(len(rows)):
                assert rel_err(prev[i][k], ref[k]) <= 1e-3, (i, k)

    fp.check_footprint(call, check_want=check_want)
    for c in call.chains:
        c.free()
    m.free()
