"""Biased linear layers on the GPU: y = W x + b inside k_gemv_quad's and k_gemm_planes' stores (tmac_hip_weights_set_bias_dev).

The yardstick of every compute case is the UNBIASED TWIN: the same handle registered twice from the same tensors, once with a bias.  Both
kernels have one writer per output element and the bias is one correctly rounded add in front of the store (the build has
-ffp-contract=off), so there is no tolerance:
    fp32 outputs:  torch.equal(biased, plain + bias_fp32)
    fp16 outputs:  torch.equal(biased, (plain_fp32 + bias_fp32).to(float16))        plain_fp32: the twin's call with fp32 outputs
The twin is held to the oracle at the project's 1e-3 of max |C|.  The bias is drawn with |b| between 0.25 and 1 times max |C| of the
oracle, so every output differs from the plain one -- asserted, an ignored bias cannot pass -- and b = 0 must give the plain output.

Shapes: Mw one and two M-tiles (128 / 192 per width); K 512, 1024 and 2304 (a ragged last 64-unit step); 2 and 4 bits everywhere, 1 and 3
bits at K = 1024; group sizes 64 and 128, with and without zero points, fp16 and fp32 device scales, fp32 / fp16 / bf16 bias sources dealt
in turn; fp16 and fp32 activations and outputs at every case.
"""
import ctypes as C
import os

import numpy as np
import pytest

import footprint as fp
import pack_common as pc
import rtn_common as rc
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
E_NOMATCH, E_ARG = -1, -4
KF, AGS = 16, 64
BM = {1: 128, 2: 128, 3: 192, 4: 128}
BI_CONFIGS = [(512, 1), (512, 2), (768, 3), (1024, 4)]                 # (threads, waves per quad) with a bias instantiation
R_PLANES, R_ONEHOT, R_QUAD, R_ROWS, R_ROW_LOOP = 0, 1, 2, 3, 7         # enum Route (tmac_hip_debug_route_stats)
BIAS_DTYPES = ("float32", "float16", "bfloat16")
FILL = 7.0


@pytest.fixture(scope="module")
def tm():
    import torch
    import tmac_amd
    assert torch.cuda.is_available()
    return tmac_amd


@pytest.fixture(autouse=True)
def knobs_back(tm):
    """Every test of this file sets debug knobs (launch configuration, GEMM kernel, rows kernel, variant) in line; whatever a test leaves
    set -- also when one of its assertions fails half-way -- is undone here, so that nothing it forced reaches the next test."""
    yield
    tm.lib().tmac_hip_defer(0)
    tm.binding.check(tm.lib().tmac_hip_reset_state())


@pytest.fixture(scope="module", autouse=True)
def free_pairs():
    """the shared matrices (_PAIRS) live as long as the module's tests and are freed behind the last one"""
    yield
    for p in _PAIRS.values():
        p.wp.free(); p.wb.free()
    _PAIRS.clear()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def acts(seed, N, K, dtype):
    x = np.random.default_rng(seed).standard_normal((N, K)).astype(np.float32)
    return dev(x).to(dtype)


def draw_bias(seed, Mw, max_c, dtype_name):
    """|b| in [0.25, 1] max |C|, random signs, as a CUDA tensor of the source dtype; and its exact fp32 value"""
    import torch
    rng = np.random.default_rng(seed)
    b = (rng.uniform(0.25, 1.0, Mw) * max_c * rng.choice([-1.0, 1.0], Mw)).astype(np.float32)
    src = dev(b).to(getattr(torch, dtype_name))
    return src, src.float()


_PAIRS = {}


class Pair:
    """One matrix registered twice from the same tensors (codes form: every width, with or without zero points): `wp` plain, `wb` with a
    bias, `wz` with b = 0; its oracle blob.  Made once per key and shared (nothing in it is modified)."""

    def __init__(self, tm, seed, Mw, K, bits, gs, zp, dd, bias_dtype):
        self.tm, self.Mw, self.K, self.bits, self.gs, self.zp, self.bm = tm, Mw, K, bits, gs, zp, BM[bits]
        self.cfg = tm.KCfg.make(Mw, K, bits, self.bm, KF, gs, AGS, zp)
        codes, sc, zr = pc.make_codes(seed, Mw, K, bits, gs, np.float16)
        self.src = (codes, sc, zr if zp else None)
        self.A, self.S = pc.host_blob_codes(codes, sc, zr if zp else None, bits, self.bm, KF)
        self.wr = tm.TMACGeMMWrapper(act_group_size=AGS)
        self.dd = dd
        self.wp = self.wr.register_codes(*self.src, bits, self.cfg, dd)
        x = np.random.default_rng(seed + 1).standard_normal((1, K)).astype(np.float32)
        self.max_c = float(np.abs(self.oracle(x)).max())
        self.bias_src, self.bias = draw_bias(seed + 2, Mw, self.max_c, bias_dtype)
        self.wb = self.wr.register_codes(*self.src, bits, self.cfg, dd, bias=self.bias_src)
        assert self.wb.has_bias and not self.wp.has_bias

    def oracle(self, x):
        q, ls, lb = orc.preprocessor(x, AGS)
        return orc.qgemm_float(self.A, q, self.S.astype(np.float32), ls, lb, self.Mw, self.K, x.shape[0], self.bits, self.bm, KF, self.gs, AGS, self.zp)

    def zero_biased(self):
        import torch
        return self.wr.register_codes(*self.src, self.bits, self.cfg, self.dd, bias=torch.zeros(self.Mw, dtype=torch.float32, device="cuda"))


def pair(tm, Mw, K, bits, gs, zp=True, dd=None, bias_dtype="float32"):
    dd = tm.F16 if dd is None else dd
    key = (Mw, K, bits, gs, zp, dd, bias_dtype)
    if key not in _PAIRS:
        _PAIRS[key] = Pair(tm, 500 + bits + K // 64 + Mw, *key)
    return _PAIRS[key]


def cases_of(tm, K):
    """every width the K takes at both Mw; group size, zero points, device scale dtype and bias source dtype dealt in turn"""
    out = []
    for bits in ((1, 2, 3, 4) if K == 1024 else (2, 4)):
        for i, Mw in enumerate((BM[bits], 2 * BM[bits])):
            j = 2 * bits + i + K // 512
            out.append(pair(tm, Mw, K, bits, (64, 128)[j % 2], zp=bool((j // 2) % 2), dd=(tm.F16, tm.F32)[(j // 4 + i) % 2], bias_dtype=BIAS_DTYPES[j % 3]))
    return out


def test_the_cases_cover_every_attribute(tm):
    ps = [p for K in (512, 1024, 2304) for p in cases_of(tm, K)]
    for attr, want in (("gs", {64, 128}), ("zp", {True, False}), ("dd", {tm.F16, tm.F32}), ("bits", {1, 2, 3, 4})):
        assert {getattr(p, attr) for p in ps} == want, attr
    assert {str(p.bias_src.dtype) for p in ps} == {"torch." + d for d in BIAS_DTYPES}


def run(wr, ws, x, N, out_dtype=None):
    import torch
    outs = [torch.full((N, w.Mw), FILL, dtype=out_dtype or torch.float32, device="cuda") for w in ws]
    wr.fused(ws, x, outs, N)
    torch.cuda.synchronize()
    return outs


def route_stats(tm):
    counts = (C.c_uint64 * 8)()
    tm.binding.check(tm.lib().tmac_hip_debug_route_stats(counts))
    return list(counts)


def route_delta(before, after):
    return {r: b - a for r, (a, b) in enumerate(zip(before, after)) if b != a}


def check_against_twin(biased, plain32, plain_same, bias32, what):
    """the bar of the file: biased == rn(plain_fp32 + b) in the output dtype, bit for bit; every output moved"""
    import torch
    want = (plain32 + bias32).to(biased.dtype)
    assert torch.equal(biased, want), (what, float((biased.float() - want.float()).abs().max()))
    assert bool((biased != plain_same).all()), (what, "an output equals the plain one: the bias was ignored there")


def check_oracle(p, plain32, x, what):
    ref = p.oracle(x.float().cpu().numpy())
    err = np.abs(plain32.cpu().numpy() - ref).max() / np.abs(ref).max()
    assert err < 1e-3, (what, err)


# ---- 1. N = 1: every covered launch configuration -------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (512, 1024, 2304))
def test_one_row_every_configuration(tm, K):
    import torch
    L = tm.lib()
    for p in cases_of(tm, K):
        wz = p.zero_biased()
        for adt in (torch.float16, torch.float32):
            x = acts(K + p.bits, 1, K, adt)
            for ft, wpq in [(0, 0)] + BI_CONFIGS:
                tm.binding.check(L.tmac_hip_debug_quad_config(ft, wpq))
                what = (p.bits, p.Mw, K, p.gs, p.zp, p.dd, str(p.bias_src.dtype), adt, ft, wpq)
                (c32,) = run(p.wr, [p.wp], x, 1)
                check_oracle(p, c32, x, what)
                for odt in (torch.float32, torch.float16):
                    before = route_stats(tm)
                    (cb,) = run(p.wr, [p.wb], x, 1, odt)
                    assert route_delta(before, route_stats(tm)) == {R_QUAD: 1}
                    (cp,) = run(p.wr, [p.wp], x, 1, odt)
                    check_against_twin(cb, c32, cp, p.bias, what + (odt,))
                    (cz,) = run(p.wr, [wz], x, 1, odt)
                    assert torch.equal(cz, cp), what + (odt, "b = 0")
            tm.binding.check(L.tmac_hip_debug_quad_config(0, 0))
        wz.free()
    # a forced configuration without a bias instantiation is refused, the output untouched
    tm.binding.check(L.tmac_hip_debug_quad_config(768, 1))
    out = torch.full((1, p.Mw), FILL, dtype=torch.float32, device="cuda")
    with pytest.raises(tm.TMACHipError) as e:
        p.wr.fused([p.wb], x, [out], 1)
    torch.cuda.synchronize()
    assert e.value.code == E_NOMATCH and "bias" in str(e.value) and bool((out == FILL).all())


# ---- 2. fused calls that mix biased and plain matrices ----------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,K,gs", [(2, 1024, 64), (4, 2304, 128), (3, 1024, 128)])
def test_three_matrices_biased_plain_biased(tm, bits, K, gs):
    import torch
    L = tm.lib()
    a, b, c = pair(tm, BM[bits], K, bits, gs), pair(tm, 2 * BM[bits], K, bits, gs, bias_dtype="float16"), pair(tm, BM[bits], K, bits, gs, bias_dtype="bfloat16")
    wr = a.wr
    seen = set()
    for N in (1, 5, 70):
        for adt, odt in ((torch.float16, torch.float16), (torch.float32, torch.float32)):
            x = acts(N + K, N, K, adt)
            p32 = run(wr, [a.wp, b.wp, c.wp], x, N)
            pod = run(wr, [a.wp, b.wp, c.wp], x, N, odt)
            before = route_stats(tm)
            got = run(wr, [a.wb, b.wp, c.wb], x, N, odt)
            seen |= set(route_delta(before, route_stats(tm)))
            check_against_twin(got[0], p32[0], pod[0], a.bias, (bits, K, N, odt, 0))
            assert torch.equal(got[1], pod[1]), "the plain matrix of a mixed call moved"
            check_against_twin(got[2], p32[2], pod[2], c.bias, (bits, K, N, odt, 2))
            for q, c32 in zip((a, b, c), p32):
                check_oracle(q, c32, x, (bits, K, N))
    assert seen == {R_QUAD, R_PLANES}
    del L


# ---- 3. N >= 2: the route of the plain call, asserted ------------------------------------------------------------------------------------
def plan_of(tm, ws, N):
    n = len(ws)
    wa = (C.c_void_p * n)(*[w.handle.value for w in ws])
    ca = (C.c_void_p * n)(*[0x1000] * n)
    route, lut = C.c_int32(-1), C.c_int32(-1)
    tm.binding.check(tm.lib().tmac_hip_debug_fused_plan(wa, n, ca, N, C.byref(route), C.byref(lut)))
    return route.value


@pytest.mark.parametrize("bits,K,gs,zp", [(2, 1024, 128, True), (4, 2304, 64, False), (1, 1024, 64, True), (3, 1024, 128, False)])
def test_several_rows_fused_entry_point(tm, bits, K, gs, zp):
    """N = 2, 5: k_gemv_quad with grid.y = N (every workgroup builds its row's LUT); N = 33, 70: k_gemm_planes (70: two token tiles), in the
    form the launcher picks and in both forced workgroup forms"""
    import torch
    L = tm.lib()
    p = pair(tm, 2 * BM[bits], K, bits, gs, zp=zp, dd=tm.F32 if bits == 4 else tm.F16, bias_dtype=BIAS_DTYPES[bits % 3])
    seen = set()
    for N in (2, 5, 33, 70):
        for form in ((0,) if N < 33 else (0, 2, 3)):
            tm.binding.check(L.tmac_hip_debug_gemm_kernel(form))
            for adt, odt in ((torch.float16, torch.float32), (torch.float32, torch.float16)):
                x = acts(N + K, N, K, adt)
                want_route = plan_of(tm, [p.wp], N)
                assert plan_of(tm, [p.wb], N) == want_route
                (c32,) = run(p.wr, [p.wp], x, N)
                (cp,) = run(p.wr, [p.wp], x, N, odt)
                before = route_stats(tm)
                (cb,) = run(p.wr, [p.wb], x, N, odt)
                assert route_delta(before, route_stats(tm)) == {want_route: 1}
                seen.add(want_route)
                check_against_twin(cb, c32, cp, p.bias, (bits, K, N, form, odt))
                check_oracle(p, c32, x, (bits, K, N, form))
        tm.binding.check(L.tmac_hip_debug_gemm_kernel(0))
    assert seen == {R_QUAD, R_PLANES}


@pytest.mark.parametrize("bits,K,gs", [(2, 1024, 64), (4, 512, 128)])
def test_row_loop_behind_a_half_table_image(tm, bits, K, gs):
    """Two matrices of different widths share a LUT but no kernel instantiation: from the GEMM crossover on the fused entry point builds the
    half-table image once and plans each matrix by itself -- k_gemv_quad with grid.y = N copying the image (LUTSRC 0)."""
    import torch
    other = 4 if bits == 2 else 2
    a, b = pair(tm, 2 * BM[bits], K, bits, gs), pair(tm, BM[other], K, other, gs, bias_dtype="float16")
    N = 33
    for odt in (torch.float32, torch.float16):
        x = acts(N + K, N, K, torch.float16)
        assert plan_of(tm, [a.wp, b.wp], N) == R_ROW_LOOP
        p32 = run(a.wr, [a.wp, b.wp], x, N)
        pod = run(a.wr, [a.wp, b.wp], x, N, odt)
        before = route_stats(tm)
        got = run(a.wr, [a.wb, b.wb], x, N, odt)
        assert route_delta(before, route_stats(tm)) == {R_ROW_LOOP: 1, R_QUAD: 2}
        check_against_twin(got[0], p32[0], pod[0], a.bias, (bits, K, odt, 0))
        check_against_twin(got[1], p32[1], pod[1], b.bias, (bits, K, odt, 1))
        check_oracle(a, p32[0], x, (bits, K))
    # from 64 rows on the row loop hands each matrix to k_gemm_onehot, which adds no bias: refused by name before anything is launched
    x = acts(70, 70, K, torch.float16)
    outs = [torch.full((70, w.Mw), FILL, dtype=torch.float32, device="cuda") for w in (a.wb, b.wb)]
    before = route_stats(tm)
    with pytest.raises(a.tm.TMACHipError) as e:
        a.wr.fused([a.wb, b.wb], x, outs, 70)
    torch.cuda.synchronize()
    assert e.value.code == E_NOMATCH and "k_gemm_onehot" in str(e.value) and route_stats(tm) == before
    assert all(bool((o == FILL).all()) for o in outs)


@pytest.mark.parametrize("bits,K,gs,zp", [(2, 2304, 64, True), (4, 1024, 128, False), (3, 1024, 64, True)])
def test_split_path(tm, bits, K, gs, zp):
    """preprocessor_dev + qgemm_dev: k_gemv_quad copying the workspace's image below the crossover, k_gemm_planes on its LUT image above"""
    import torch
    p = pair(tm, 2 * BM[bits], K, bits, gs, zp=zp, bias_dtype=BIAS_DTYPES[(bits + 1) % 3])
    wr = p.wr
    wr.set_workspace(K, 70)
    seen = set()
    for N in (1, 2, 5, 33, 70):
        for adt, odt in ((torch.float16, torch.float32), (torch.float32, torch.float16)):
            x = acts(N + K + 1, N, K, adt)
            wr.llama_cpp_init(x, p.Mw, K, N, bits)
            outs = {}
            for name, w, dt in (("p32", p.wp, torch.float32), ("pod", p.wp, odt), ("b", p.wb, odt)):
                outs[name] = torch.full((N, p.Mw), FILL, dtype=dt, device="cuda")
                before = route_stats(tm)
                wr.llama_cpp_compute(w, outs[name], N)
                torch.cuda.synchronize()
                delta = route_delta(before, route_stats(tm))
                outs[name + "_route"] = delta
            assert outs["b_route"] == outs["pod_route"] and list(outs["b_route"].values()) == [1]
            seen |= set(outs["b_route"])
            check_against_twin(outs["b"], outs["p32"], outs["pod"], p.bias, (bits, K, N, odt))
            check_oracle(p, outs["p32"], x, (bits, K, N))
    assert seen == {R_QUAD, R_PLANES}


def test_forced_configuration_on_the_copy_form(tm):
    """The copy form (split entry point, row loop) exists for (512,1) and (512,2): a forced configuration outside them is refused before
    the first launch -- no LUT build, no matrix in front of the refused one has run -- and a forced one inside is the twin's, bit for bit."""
    import torch
    L = tm.lib()
    bits, K, gs, N = 2, 1024, 64, 33
    a, b = pair(tm, 2 * BM[bits], K, bits, gs), pair(tm, BM[4], K, 4, gs, bias_dtype="float16")
    wr = a.wr
    x = acts(N + K, N, K, torch.float16)
    wr.set_workspace(K, N)
    for ft, wpq in ((768, 3), (1024, 4), (768, 1)):
        tm.binding.check(L.tmac_hip_debug_quad_config(ft, wpq))
        for ws in ([a.wb, b.wb], [a.wp, b.wb]):
            assert plan_of(tm, ws, N) == R_ROW_LOOP
            outs = [torch.full((N, w.Mw), FILL, dtype=torch.float32, device="cuda") for w in ws]
            before = route_stats(tm)
            with pytest.raises(tm.TMACHipError) as e:
                wr.fused(ws, x, outs, N)
            torch.cuda.synchronize()
            assert e.value.code == E_NOMATCH and "carries a bias" in str(e.value) and route_stats(tm) == before, (ft, wpq, str(e.value))
            assert all(bool((o == FILL).all()) for o in outs), (ft, wpq)
        tm.binding.check(L.tmac_hip_debug_quad_config(0, 0))
        wr.llama_cpp_init(x[:5].contiguous(), a.Mw, K, 5, bits)
        tm.binding.check(L.tmac_hip_debug_quad_config(ft, wpq))
        out = torch.full((5, a.Mw), FILL, dtype=torch.float32, device="cuda")
        before = route_stats(tm)
        with pytest.raises(tm.TMACHipError) as e:
            wr.llama_cpp_compute(a.wb, out, 5)
        torch.cuda.synchronize()
        assert e.value.code == E_NOMATCH and "carries a bias" in str(e.value) and route_stats(tm) == before and bool((out == FILL).all())
    for ft, wpq in ((512, 1), (512, 2)):
        tm.binding.check(L.tmac_hip_debug_quad_config(ft, wpq))
        p32 = run(wr, [a.wp, b.wp], x, N)
        got = run(wr, [a.wb, b.wb], x, N)
        check_against_twin(got[0], p32[0], p32[0], a.bias, (ft, wpq, 0))
        check_against_twin(got[1], p32[1], p32[1], b.bias, (ft, wpq, 1))


# ---- 4. transforms in front of a biased matrix ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,K,gs", [(2, 1024, 128), (4, 2304, 64)])
def test_transforms(tm, bits, K, gs):
    """NORM (with gamma and residual, residual_out compared; and bare) and the silu GLU at N = 1, 2, 5, 70: rn(unbiased transformed call +
    b), bit for bit"""
    import torch
    L = tm.lib()
    a, b = pair(tm, BM[bits], K, bits, gs), pair(tm, 2 * BM[bits], K, bits, gs, bias_dtype="bfloat16")
    wr = a.wr
    rng = np.random.default_rng(K + bits)
    for N in (1, 2, 5, 70):
        for adt, odt in ((torch.float16, torch.float16), (torch.float32, torch.float32)):
            x = acts(N + K + 3, N, K, adt)
            in2 = acts(N + K + 4, N, K, adt)
            res = dev(rng.standard_normal((N, K)).astype(np.float32))
            gamma = dev((1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32))
            for kind, kw in (("norm", dict(residual=res, gamma=gamma, ro=True)), ("norm", dict()), ("glu", dict(in2=in2))):
                def call(ws, dt):
                    outs = [torch.full((N, w.Mw), FILL, dtype=dt, device="cuda") for w in ws]
                    ro = torch.full((N, K), FILL, dtype=torch.float32, device="cuda") if kw.get("ro") else None
                    args = {k: v for k, v in kw.items() if k != "ro"}
                    before = route_stats(tm)
                    wr.fused_xf_rows(ws, x, outs, kind, N, residual_out=ro, **args)
                    torch.cuda.synchronize()
                    return outs, ro, route_delta(before, route_stats(tm))
                p32, ro_p, _ = call([a.wp, b.wp], torch.float32)
                pod, _, r_plain = call([a.wp, b.wp], odt)
                got, ro_b, r_bias = call([a.wb, b.wb], odt)
                assert r_bias == r_plain, (kind, N, r_bias, r_plain)
                what = (bits, K, N, kind, sorted(kw), odt)
                check_against_twin(got[0], p32[0], pod[0], a.bias, what)
                check_against_twin(got[1], p32[1], pod[1], b.bias, what)
                if ro_p is not None:
                    assert torch.equal(ro_b, ro_p) and not bool((ro_b == FILL).all())
    # at N = 1 the covered configurations, forced
    x, in2 = acts(K + 5, 1, K, torch.float16), acts(K + 6, 1, K, torch.float16)
    for ft, wpq in BI_CONFIGS:
        tm.binding.check(L.tmac_hip_debug_quad_config(ft, wpq))
        outs = {}
        for name, ws, dt in (("p32", [a.wp], torch.float32), ("b", [a.wb], torch.float32)):
            outs[name] = torch.full((1, a.Mw), FILL, dtype=dt, device="cuda")
            wr.fused_xf(ws, x, [outs[name]], "glu", in2=in2)
        torch.cuda.synchronize()
        check_against_twin(outs["b"], outs["p32"], outs["p32"], a.bias, (bits, K, "glu", ft, wpq))


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_set_bias_refusals(tm):
    import torch
    L = tm.lib()
    bits, Mw, K, gs = 2, 128, 512, 64
    p = pair(tm, Mw, K, bits, gs)
    wr = p.wr
    bias = torch.zeros(Mw + 8, dtype=torch.float32, device="cuda")

    def has(w):
        h = C.c_int(-1)
        tm.binding.check(L.tmac_hip_weights_has_bias(w.handle, C.byref(h)))
        return h.value

    def refused(w, ptr, dtype, code, *words):
        before = has(w)
        rc_ = L.tmac_hip_weights_set_bias_dev(w.handle, ptr, dtype, None)
        msg = L.tmac_hip_last_error().decode()
        assert rc_ == code and all(t in msg for t in words), (rc_, msg)
        assert has(w) == before

    fresh = wr.register_codes(*p.src, bits, p.cfg, tm.F16)
    refused(fresh, None, 0, E_ARG, "bias_dev")
    refused(fresh, bias.data_ptr() + 4, 0, E_ARG, "aligned")
    refused(fresh, bias.data_ptr(), 3, E_ARG, "dtype")
    refused(fresh, bias.data_ptr(), -1, E_ARG, "dtype")
    assert L.tmac_hip_weights_set_bias_dev(None, bias.data_ptr(), 0, None) == E_ARG
    assert has(fresh) == 0
    refused(p.wb, bias.data_ptr(), 0, E_ARG, "already has a bias")
    # unified scales
    ucfg = tm.KCfg.make(Mw, K, bits, BM[bits], KF, gs, K, False, 1)
    wu = wr.register_codes(p.src[0], np.ones(1, np.float32), None, bits, ucfg, tm.F32)
    refused(wu, bias.data_ptr(), 0, E_NOMATCH, "unified")
    # a K permutation: through the library's entry point and through the constructor's bias=
    g = np.ascontiguousarray((np.arange(K, dtype=np.int32) // gs)[::-1])
    wk = wr.register_codes(*p.src, bits, p.cfg, tm.F16, g_idx=g)
    refused(wk, bias.data_ptr(), 0, E_ARG, "K permutation", "not served yet")
    with pytest.raises(tm.TMACHipError) as e:
        wr.register_codes(*p.src, bits, p.cfg, tm.F16, g_idx=g, bias=bias[:Mw])
    assert e.value.code == E_ARG and "K permutation" in str(e.value)
    # an identity g_idx gives a plain handle: served
    wi = wr.register_codes(*p.src, bits, p.cfg, tm.F16, g_idx=np.arange(K, dtype=np.int32) // gs, bias=bias[:Mw])
    assert wi.has_bias
    # another layout, fast aggregation
    tm.binding.check(L.tmac_hip_set_variant(1))
    wl = wr.register_codes(*p.src, bits, p.cfg, tm.F16)
    tm.binding.check(L.tmac_hip_set_variant(0))
    refused(wl, bias.data_ptr(), 0, E_NOMATCH, "QUAD layout")
    wf = wr.register_weights(p.A, p.S.astype(np.float32), Mw, K, bits, p.cfg, tm.F32, tm.F16, fast_aggregation=1)
    refused(wf, bias.data_ptr(), 0, E_NOMATCH, "fast aggregation")
    # the shape check of the Python side
    with pytest.raises(ValueError):
        wr.register_codes(*p.src, bits, p.cfg, tm.F16, bias=bias)
    with pytest.raises(TypeError):
        wr.register_codes(*p.src, bits, p.cfg, tm.F16, bias=np.zeros(Mw, np.float64))
    assert has(fresh) == 0
    assert wr.register_codes(*p.src, bits, p.cfg, tm.F16, bias=np.zeros(Mw, np.float16)).has_bias


def test_call_refusals_leave_outputs_and_state_alone(tm):
    import torch
    L = tm.lib()
    bits, Mw, K, gs = 2, 256, 1024, 128
    p = pair(tm, Mw, K, bits, gs)
    wr = p.wr
    x1, x5, x70 = (acts(9 + n, n, K, torch.float16) for n in (1, 5, 70))
    in2 = {1: acts(31, 1, K, torch.float16), 5: acts(35, 5, K, torch.float16)}
    gamma = torch.ones(K, dtype=torch.float32, device="cuda")

    def refused(fn, N, code, *words):
        out = torch.full((N, Mw), FILL, dtype=torch.float32, device="cuda")
        before = route_stats(tm)
        with pytest.raises(tm.TMACHipError) as e:
            fn(out)
        torch.cuda.synchronize()
        assert e.value.code == code and all(t in str(e.value) for t in words), str(e.value)
        assert bool((out == FILL).all()) and route_stats(tm) == before

    # the tap
    with pytest.raises(tm.TMACHipError) as e:
        wr.fused_partial_sums(p.wb, x1)
    assert e.value.code == E_ARG and "bias" in str(e.value)
    # GLU_NORM and both non-silu gates, at N = 1 and N = 5: one rule
    for N, x in ((1, x1), (5, x5)):
        for kind in ("glu_norm", "glu:relu2", "glu:gelu", "glu_norm:relu2"):
            refused(lambda o: wr.fused_xf_rows([p.wb], x, [o], kind, N, in2=in2[N], gamma=gamma if "norm" in kind else None), N, E_NOMATCH, "bias")
    # forced rows kernel
    tm.binding.check(L.tmac_hip_debug_rows_kernel(2))
    refused(lambda o: wr.fused([p.wb], x5, [o], 5), 5, E_NOMATCH, "carries a bias", "k_gemv_rows")
    wr.set_workspace(K, 70)
    wr.llama_cpp_init(x5, Mw, K, 5, bits)
    refused(lambda o: wr.llama_cpp_compute(p.wb, o, 5), 5, E_NOMATCH, "carries a bias", "k_gemv_rows")
    tm.binding.check(L.tmac_hip_debug_rows_kernel(0))
    # k_gemm_onehot selected
    tm.binding.check(L.tmac_hip_debug_gemm_kernel(1))
    refused(lambda o: wr.fused([p.wb], x70, [o], 70), 70, E_NOMATCH, "carries a bias", "k_gemm_onehot")
    tm.binding.check(L.tmac_hip_debug_gemm_kernel(0))
    # the v_mqsad variant, the reference-layout variant
    for v in (7, 3):
        tm.binding.check(L.tmac_hip_set_variant(v))
        refused(lambda o: wr.fused([p.wb], x1, [o], 1), 1, E_NOMATCH, "carries a bias")
    tm.binding.check(L.tmac_hip_set_variant(0))
    # ... and with every knob back the handle computes what it computed
    (c32,) = run(wr, [p.wp], x1, 1)
    (cb,) = run(wr, [p.wb], x1, 1)
    check_against_twin(cb, c32, c32, p.bias, "after the refusals")


@pytest.mark.parametrize("independent", (False, True))
def test_recording_refuses_a_biased_call_and_stays_usable(tm, independent):
    import torch
    bits, Mw, K, gs = 2, 256, 1024, 128
    p = pair(tm, Mw, K, bits, gs)
    wr = p.wr
    x = acts(77, 1, K, torch.float16)[0].contiguous()
    x2 = acts(78, 1, K, torch.float16)[0].contiguous()
    o1, o2, ob = (torch.full((Mw,), FILL, dtype=torch.float16, device="cuda") for _ in range(3))
    with wr.record_chain(independent=independent) as rec:
        wr.fused([p.wp], x, [o1], 1)
        with pytest.raises(tm.TMACHipError) as e:
            wr.fused([p.wb], x, [ob], 1)
        assert e.value.code == E_ARG and "carries a bias" in str(e.value)
        with pytest.raises(tm.TMACHipError) as e:
            wr.fused([p.wp, p.wb], x, [o2, ob], 1)
        assert e.value.code == E_ARG and "carries a bias" in str(e.value)
        wr.fused([p.wp], x2, [o2], 1)
    assert rec.chain.nops == 2
    rec.chain.launch()
    torch.cuda.synchronize()
    assert rec.chain.status() == 0 and bool((ob == FILL).all())
    for o, xx in ((o1, x), (o2, x2)):
        ref = p.oracle(xx.float().cpu().numpy()[None, :])[0]
        assert np.abs(o.float().cpu().numpy() - ref).max() / np.abs(ref).max() < 1e-3
    rec.chain.free()


# ---- 6. deferred mode ------------------------------------------------------------------------------------------------------------------------
def test_a_queued_producer_is_ordered_in_front_of_the_biased_call(tm):
    import torch
    L = tm.lib()
    bits, K0, K, gs = 2, 512, 256, 64
    prod = pair(tm, K, K0, bits, gs)                       # K0 -> K rows
    cons = pair(tm, 2 * BM[bits], K, bits, gs, bias_dtype="float16")
    wr = cons.wr
    x = acts(5, 1, K0, torch.float16)
    mid = torch.full((1, K), 60000.0, dtype=torch.float16, device="cuda")        # what a consumer that runs first would read
    out = torch.full((1, cons.Mw), FILL, dtype=torch.float32, device="cuda")
    st = [C.c_uint64(0) for _ in range(4)]

    def stats():
        tm.binding.check(L.tmac_hip_defer_stats(*[C.byref(s) for s in st]))
        return tuple(int(s.value) for s in st)

    tm.binding.check(L.tmac_hip_defer(1))
    try:
        s0 = stats()
        wr.fused([prod.wp], x, [mid], 1)
        assert stats() == s0, "the producer was not queued"
        wr.fused([cons.wb], mid, [out], 1)
        s1 = stats()
        assert s1[0] == s0[0] + 1, "the biased call did not flush the queue it depends on"
        tm.binding.check(L.tmac_hip_flush(None))
        assert stats() == s1, "the biased call was queued"
        torch.cuda.synchronize()
    finally:
        L.tmac_hip_defer(0)
    assert not bool((mid == 60000.0).any())
    (again,) = run(wr, [cons.wb], mid, 1)
    (plain,) = run(wr, [cons.wp], mid, 1)
    assert torch.equal(out, again)
    check_against_twin(out, plain, plain, cons.bias, "deferred")


# ---- 7. footprint ------------------------------------------------------------------------------------------------------------------------------
def test_footprint_of_the_bias_and_both_outputs(tm):
    """Guard bands around the caller's bias and the outputs of an N = 1 call (k_gemv_quad) and an N = 70 call (k_gemm_planes) at two
    placements and two guard patterns: nothing outside the outputs is written, and no byte next to the bias reaches a result."""
    import torch
    bits, Mw, K, gs = 2, 192, 1024, 64                     # Mw: one and a half 128-row tiles, three 64-row tiles
    cfg = tm.KCfg.make(Mw, K, bits, 64, KF, gs, AGS, True)
    codes, sc, zr = pc.make_codes(901, Mw, K, bits, gs, np.float16)
    wr = tm.TMACGeMMWrapper(act_group_size=AGS)
    b = np.random.default_rng(902).uniform(0.5, 2.0, Mw).astype(np.float16)
    x1 = np.random.default_rng(903).standard_normal((1, K)).astype(np.float16)
    x70 = np.random.default_rng(904).standard_normal((70, K)).astype(np.float16)
    plain = wr.register_codes(codes, sc, zr, bits, cfg, tm.F16)
    want = {}
    for name, x, N in (("one", x1, 1), ("planes", x70, 70)):
        (c,) = run(wr, [plain], dev(x), N)
        want[name] = (c + dev(b).float()).cpu().numpy()
    routes = []

    def call(alloc):
        bias = alloc.inp(b, name="bias")
        a1, a70 = alloc.inp(x1, name="x1"), alloc.inp(x70, name="x70")
        o1, o70 = alloc.out((1, Mw), np.float32, "one"), alloc.out((70, Mw), np.float32, "planes")
        alloc.arm()
        w = wr.register_codes(codes, sc, zr, bits, cfg, tm.F16, bias=bias)
        before = route_stats(tm)
        wr.fused([w], a1, [o1], 1)
        wr.fused([w], a70, [o70], 70)
        torch.cuda.synchronize()
        routes.append(route_delta(before, route_stats(tm)))
        w.free()

    def check_want(got):
        for name in want:
            assert np.array_equal(got[name].view(np.uint32), want[name].view(np.uint32)), name

    fp.check_footprint(call, check_want=check_want)
    assert all(r == {R_QUAD: 1, R_PLANES: 1} for r in routes), routes


def test_the_callers_bias_buffer_is_free_after_the_call(tm):
    import torch
    p = pair(tm, 256, 1024, 2, 128)
    buf = p.bias_src.float().clone()
    w = p.wr.register_codes(*p.src, p.bits, p.cfg, p.dd, bias=buf)
    torch.cuda.synchronize()
    buf.fill_(float("nan"))
    torch.cuda.synchronize()
    for N in (1, 70):
        x = acts(N, N, p.K, torch.float16)
        (c32,) = run(p.wr, [p.wp], x, N)
        (cb,) = run(p.wr, [w], x, N)
        check_against_twin(cb, c32, c32, p.bias, ("overwritten", N))
    w.free()


# ---- 8. call sequences ---------------------------------------------------------------------------------------------------------------------------
def test_plain_calls_around_a_biased_call_keep_their_bits(tm):
    import torch
    p = pair(tm, 256, 1024, 2, 128)
    q = pair(tm, 256, 2304, 4, 64, zp=False)
    for pr in (p, q):
        for N in (1, 5, 70):
            x = acts(N + 40, N, pr.K, torch.float16)
            (alone,) = run(pr.wr, [pr.wp], x, N)
            (alone_b,) = run(pr.wr, [pr.wb], x, N)
            o = [torch.full((N, pr.Mw), FILL, dtype=torch.float32, device="cuda") for _ in range(4)]
            pr.wr.fused([pr.wp], x, [o[0]], N)
            pr.wr.fused([pr.wb], x, [o[1]], N)
            pr.wr.fused([pr.wp], x, [o[2]], N)
            pr.wr.fused([pr.wb], x, [o[3]], N)
            torch.cuda.synchronize()
            assert torch.equal(o[0], alone) and torch.equal(o[2], alone), (pr.bits, N)
            assert torch.equal(o[1], alone_b) and torch.equal(o[3], alone_b), (pr.bits, N)


# ---- 9. loaders ------------------------------------------------------------------------------------------------------------------------------------
def test_loaders_attach_the_bias(tm, tmp_path):
    import torch
    from tmac_amd import checkpoint
    wr = tm.TMACGeMMWrapper(act_group_size=AGS)
    # GPTQ: biases on two of three layers, fp16 and fp32
    d = str(tmp_path / "gptq")
    os.makedirs(d)
    layers = [("model.layers.0.self_attn.q_proj", 81, 128, 512, 2, 64), ("model.layers.0.self_attn.o_proj", 82, 256, 512, 2, 64),
              ("model.layers.0.mlp.down_proj", 83, 128, 1024, 2, 64)]
    tensors, _ = pc.write_gptq_checkpoint(d, layers)
    rng = np.random.default_rng(84)
    biases = {layers[0][0]: rng.standard_normal(128).astype(np.float16), layers[1][0]: rng.standard_normal(256).astype(np.float32)}
    pc.write_safetensors(os.path.join(d, "model-extra.safetensors"), {k + ".bias": v for k, v in biases.items()})
    got = checkpoint.load_gptq_dir(d, wr)
    for name, _, Mw, K, bits, gs in layers:
        assert got[name].has_bias == (name in biases)
        cfg = tm.KCfg.make(Mw, K, bits, tm.convert.default_bm(bits, Mw), 16, gs, AGS, True)
        twin = wr.register_gptq(tensors[name + ".qweight"], tensors[name + ".scales"], tensors[name + ".qzeros"], cfg, True, tm.F16, bias=biases.get(name))
        plain = wr.register_gptq(tensors[name + ".qweight"], tensors[name + ".scales"], tensors[name + ".qzeros"], cfg, True, tm.F16)
        x = acts(K, 1, K, torch.float16)
        (a,), (b,), (c,) = run(wr, [got[name]], x, 1), run(wr, [twin], x, 1), run(wr, [plain], x, 1)
        assert torch.equal(a, b)
        if name in biases:
            assert torch.equal(a, c + dev(biases[name]).float())
        else:
            assert torch.equal(a, c)
    # dense: a bf16 bias on one layer
    d = str(tmp_path / "dense")
    os.makedirs(d)
    name, _, Mw, K, _ = rc.CKPT_LAYERS[0]
    b32 = torch.from_numpy(rng.standard_normal(Mw).astype(np.float32)).to(torch.bfloat16)
    words = b32.view(torch.int16).numpy().view(np.uint16)
    tensors, _ = rc.write_dense_checkpoint(d, extra={name + ".bias": words.view(np.float16)}, dtype_names={name + ".bias": "BF16"})
    got = checkpoint.load_dense_dir(d, wr, 4, 128)
    assert [n for n, w in got.items() if w.has_bias] == [name]
    twin = wr.register_dense(tensors[name + ".weight"], 4, 128, True, None, tm.F16, bias=words)
    plain = wr.register_dense(tensors[name + ".weight"], 4, 128, True, None, tm.F16)
    x = acts(K + 1, 1, K, torch.float16)
    (a,), (b,), (c,) = run(wr, [got[name]], x, 1), run(wr, [twin], x, 1), run(wr, [plain], x, 1)
    assert torch.equal(a, b) and torch.equal(a, c + b32.cuda().float()) and not torch.equal(a, c)
