"""Act-order (desc_act / g_idx) GPTQ matrices on the GPU: the K permutation packed and gathered on the device.

An act-order matrix is a group-quantised matrix whose K axis is permuted: with perm = stable_argsort(g_idx), y = W x = W' x[perm], W' =
W[:, perm].  A handle registered with a g_idx holds W' and carries perm; every LUT build that serves it gathers.  The yardstick of every
compute case here is the PLAIN TWIN: a plain handle registered from the host blob of w[:, perm], run on x.index_select(perm).  The gather
changes which elements are loaded and nothing after them, so the two agree bit for bit (torch.equal) -- and the twin meets the project's
bar against the oracle (1e-3 of max |C|), which ties the pair to the reference.

Shapes: Mw one and two M-tiles; K 256 (less than a wave of pairs), 512 / 1024 (the sequence tests' shapes), 2304 (a ragged last 64-unit
step), 6144 (six tables per thread at 512 threads); group sizes 64 and 128; 2 and 4 bits everywhere, 1 and 3 bits at K = 1024; fp16 and
fp32 activations; permutations: random with exactly gs members per group, the reversal, group 0 made of the last gs columns.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import footprint as fp
import pack_common as pc
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
E_NOMATCH, E_ARG = -1, -4
KF, AGS = 16, 64
BM = {1: 128, 2: 128, 3: 192, 4: 128}                                  # the M-tile of the configuration; Mw = bm and 2 bm
GA_CONFIGS = [(512, 1), (512, 2), (768, 3), (1024, 4)]                 # (threads, waves per quad) with a gather instantiation
PERM_KINDS = ("random", "reversal", "last_first")
R_PLANES, R_QUAD, R_ROWS, R_ROW_LOOP = 0, 2, 3, 7                      # enum Route (tmac_hip_debug_route_stats)


@pytest.fixture(scope="module")
def tm():
    import torch
    import tmac_amd
    assert torch.cuda.is_available()
    return tmac_amd


def make_g_idx(kind, seed, K, gs):
    base = np.arange(K, dtype=np.int32) // gs
    if kind == "random":
        g = base.copy()
        np.random.default_rng(seed).shuffle(g)
        return g
    if kind == "reversal":
        return np.ascontiguousarray(base[::-1])
    return np.roll(base, -gs)                                           # the last gs columns are group 0


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_MATS = {}


class Mat:
    """One act-order matrix: the checkpoint tensors (GPTQ form for 1, 2, 4 bits, codes for 3), its g_idx and perm, the host blob of the
    gathered matrix, the permuted handle and the plain twin.  Made once per key and shared (nothing in it is modified)."""

    def __init__(self, tm, seed, Mw, K, bits, gs, kind, kperm=None, dev_dtype=None, g_idx=None):
        self.tm, self.Mw, self.K, self.bits, self.gs, self.bm = tm, Mw, K, bits, gs, BM[bits]
        self.cfg = tm.KCfg.make(Mw, K, bits, self.bm, KF, gs, AGS, True)
        self.g_idx = make_g_idx(kind, seed, K, gs) if g_idx is None else g_idx      # (g_idx: that of the KPerm handed in)
        self.perm = np.argsort(self.g_idx, kind="stable").astype(np.int32)
        self.gptq = bits != 3
        if self.gptq:
            self.src = pc.make_gptq(seed, Mw, K, bits, gs, np.float16, hard=False)
            _, _, (w, sc, zr, b, g) = pc.host_blob_gptq(*self.src, True, self.bm, KF)
            assert (b, g) == (bits, gs)
        else:
            w, sc, zr = pc.make_codes(seed, Mw, K, bits, gs, np.float16)
            self.src = (w, sc, zr)
        self.A, self.S = pc.host_blob_codes(np.ascontiguousarray(w[:, self.perm]), sc, zr, bits, self.bm, KF)      # the gathered matrix
        self.A_plain, self.S_plain = pc.host_blob_codes(w, sc, zr, bits, self.bm, KF)                              # columns as they come
        wr = tm.TMACGeMMWrapper(act_group_size=AGS)
        dd = tm.F16 if dev_dtype is None else dev_dtype
        self.kperm = kperm if kperm is not None else tm.KPerm(self.g_idx, gs)
        if self.gptq:
            self.wp = wr.register_gptq(*self.src, self.cfg, True, dd, g_idx=self.kperm)
        else:
            self.wp = wr.register_codes(*self.src, bits, self.cfg, dd, g_idx=self.kperm)
        self.wt = wr.register_weights(self.A, self.S.astype(np.float32), Mw, K, bits, self.cfg, tm.F32, dd)
        self.dperm = dev(self.perm.astype(np.int64))

    def oracle(self, xg):
        """fp32 [N][Mw] of the gathered matrix on the gathered rows xg (fp32 numpy)"""
        q, ls, lb = orc.preprocessor(xg, AGS)
        return orc.qgemm_float(self.A, q, self.S.astype(np.float32), ls, lb, self.Mw, self.K, xg.shape[0], self.bits, self.bm, KF, self.gs, AGS, True)


def mat(tm, seed, Mw, K, bits, gs, kind):
    key = (seed, Mw, K, bits, gs, kind)
    if key not in _MATS:
        _MATS[key] = Mat(tm, *key)
    return _MATS[key]


def acts(seed, N, K, dtype):
    import torch
    x = np.random.default_rng(seed).standard_normal((N, K)).astype(np.float32)
    return dev(x).to(dtype)


def gathered(m, x):
    return x.index_select(1, m.dperm).contiguous()


def run(wr, ws, x, N, out_dtype=None):
    import torch
    outs = [torch.full((N, w.Mw), 7.0, dtype=out_dtype or torch.float32, device="cuda") for w in ws]
    wr.fused(ws, x, outs, N)
    torch.cuda.synchronize()
    return outs


def route_stats(tm):
    counts = (C.c_uint64 * 8)()
    tm.binding.check(tm.lib().tmac_hip_debug_route_stats(counts))
    return list(counts)


def route_delta(before, after):
    return {r: b - a for r, (a, b) in enumerate(zip(before, after)) if b != a}


def cases_of(K):
    """(bits, Mw, gs, perm kind) at this K: every width the K takes, both Mw, group sizes and permutations dealt in turn"""
    out = []
    for bits in ((1, 2, 3, 4) if K == 1024 else (2, 4)):
        for i, Mw in enumerate((BM[bits], 2 * BM[bits])):
            out.append((bits, Mw, (64, 128)[(i + bits) % 2], PERM_KINDS[(i + bits + K // 256) % 3]))
    return out


# ---- 1. the pack --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (256, 1024, 2304))
def test_pack_through_the_permutation_is_the_host_blob_of_the_gathered_matrix(tm, K):
    from tmac_amd import wrapper
    for bits, Mw, gs, kind in cases_of(K):
        m = mat(tm, 100 + bits, Mw, K, bits, gs, kind)
        if m.gptq:
            gA, gS = wrapper.pack_gptq(*m.src, m.cfg, True, tm.F16, g_idx=m.kperm)
            pA, pS = wrapper.pack_gptq(*m.src, m.cfg, True, tm.F16)
        else:
            gA, gS = wrapper.pack_codes(*m.src, bits, m.cfg, tm.F16, g_idx=m.kperm)
            pA, pS = wrapper.pack_codes(*m.src, bits, m.cfg, tm.F16)
        assert np.array_equal(gA.cpu().numpy(), m.A.reshape(-1)), (bits, Mw, gs, kind)
        assert not np.array_equal(m.A, m.A_plain) and np.array_equal(pA.cpu().numpy(), m.A_plain.reshape(-1))
        # scales and zeros do not pass through the permutation: bit for bit the plain pack's
        assert np.array_equal(pc.raw_bits(gS.cpu().numpy()), pc.raw_bits(pS.cpu().numpy()))
        assert np.array_equal(pc.raw_bits(gS.cpu().numpy()), pc.raw_bits(m.S.astype(np.float16)))
        assert np.array_equal(m.kperm.perm(), m.perm) and not m.kperm.identity and m.kperm.K == K


def test_pack_refusals(tm):
    import torch
    from tmac_amd import wrapper
    bits, Mw, K, gs = 2, 128, 512, 64
    m = mat(tm, 102, Mw, K, bits, gs, "random")
    L = tm.lib()
    ab, sb = wrapper.ref_blob_bytes(Mw, K, bits, m.cfg, tm.F16)
    bufA = torch.full((ab,), 0xFF, dtype=torch.uint8, device="cuda")
    bufS = torch.full((sb,), 0xFF, dtype=torch.uint8, device="cuda")
    qw, sc, qz = (dev(a) for a in m.src)
    other_K = tm.KPerm(make_g_idx("random", 1, 2 * K, gs), gs)
    other_gs = tm.KPerm(make_g_idx("reversal", 1, K, 128), 128)
    h = C.c_void_p()
    for kp, names in ((other_K, ["K=1024", "K=512"]), (other_gs, ["group_size=128", "group_size=64"])):
        rc = L.tmac_hip_pack_gptq_perm_dev(qw.data_ptr(), sc.data_ptr(), qz.data_ptr(), tm.F16, 1, kp.handle, Mw, K, bits, C.byref(m.cfg),
                                           bufA.data_ptr(), bufS.data_ptr(), tm.F16, None)
        msg = L.tmac_hip_last_error().decode()
        assert rc == E_ARG and all(n in msg for n in names), (rc, msg)
        rc = L.tmac_hip_register_weights_gptq_perm_dev(C.byref(h), qw.data_ptr(), sc.data_ptr(), qz.data_ptr(), tm.F16, 1, kp.handle, Mw, K, bits,
                                                       C.byref(m.cfg), tm.F16, tm.F16, None)
        assert rc == E_ARG and not h
    # the plain twin's own rules come first: a misaligned qweight is refused as there
    rc = L.tmac_hip_pack_gptq_perm_dev(qw.data_ptr() + 8, sc.data_ptr(), qz.data_ptr(), tm.F16, 1, m.kperm.handle, Mw, K, bits, C.byref(m.cfg),
                                       bufA.data_ptr(), bufS.data_ptr(), tm.F16, None)
    assert rc == E_ARG and "qweight" in L.tmac_hip_last_error().decode()
    # unified scales take no permutation
    ucfg = tm.KCfg.make(Mw, K, bits, BM[bits], KF, gs, K, False, 1)
    codes = torch.zeros((Mw, K), dtype=torch.uint8, device="cuda")
    s1 = torch.ones(4, dtype=torch.float32, device="cuda")
    rc = L.tmac_hip_register_weights_codes_perm_dev(C.byref(h), codes.data_ptr(), s1.data_ptr(), None, tm.F32, m.kperm.handle, Mw, K, bits,
                                                    C.byref(ucfg), tm.F32, tm.F32, None)
    assert rc == E_ARG and "unified" in L.tmac_hip_last_error().decode() and not h
    # the object itself: a group with the wrong number of members, a value outside the groups, K % group_size, a misaligned pointer
    g = make_g_idx("random", 2, K, gs)
    bad = g.copy(); bad[np.nonzero(g == 3)[0][0]] = 5
    for arr, gsz, names in ((bad, gs, ["group 3 has 63 members"]), (np.where(g == 0, K // gs, g).astype(np.int32), gs, ["outside [0, 8)"]), (g, 96, ["K=512", "96"])):
        with pytest.raises(tm.TMACHipError) as e:
            tm.KPerm(arr, gsz)
        assert e.value.code == E_ARG and all(n in str(e.value) for n in names), str(e.value)
    gd = dev(np.concatenate([g, g]))
    rc = L.tmac_hip_kperm_from_gidx_dev(gd.data_ptr() + 4, K, gs, C.byref(h), None)
    assert rc == E_ARG and "aligned" in L.tmac_hip_last_error().decode() and not h
    rc = L.tmac_hip_kperm_from_gidx_dev(None, K, gs, C.byref(h), None)
    assert rc == E_ARG and not h
    torch.cuda.synchronize()
    assert bool((bufA == 0xFF).all()) and bool((bufS == 0xFF).all()), "a refused pack wrote its outputs"


# ---- 2. N = 1: the gather instantiations of k_gemv_quad -----------------------------------------------------------------------------
@pytest.mark.parametrize("K", (256, 512, 1024, 2304, 6144))
def test_one_row_is_the_plain_twin_bit_for_bit(tm, K):
    import torch
    wr = tm.TMACGeMMWrapper(act_group_size=AGS)
    L = tm.lib()
    for bits, Mw, gs, kind in cases_of(K):
        m = mat(tm, 100 + bits, Mw, K, bits, gs, kind)
        for dt in (torch.float16, torch.float32):
            x = acts(K + bits, 1, K, dt)
            xg = gathered(m, x)
            ref = m.oracle(xg.float().cpu().numpy())
            for ft, wpq in [(0, 0)] + GA_CONFIGS:
                tm.binding.check(L.tmac_hip_debug_quad_config(ft, wpq))
                before = route_stats(tm)
                (cp,) = run(wr, [m.wp], x, 1)
                assert route_delta(before, route_stats(tm)) == {R_QUAD: 1}
                (ct,) = run(wr, [m.wt], xg, 1)
                assert torch.equal(cp, ct), (bits, Mw, gs, kind, dt, ft, wpq, float((cp - ct).abs().max()))
                err = np.abs(ct.cpu().numpy() - ref).max() / np.abs(ref).max()
                assert err < 1e-3, (bits, Mw, gs, kind, dt, ft, wpq, err)
            tm.binding.check(L.tmac_hip_debug_quad_config(0, 0))
        # the permutation is not a no-op: the permuted handle on the gathered vector is something else
        (cw,) = run(wr, [m.wp], xg, 1)
        assert not torch.equal(cw, ct)
    # a forced configuration without a gather instantiation is refused, as a transformed call's is
    tm.binding.check(L.tmac_hip_debug_quad_config(768, 1))
    with pytest.raises(tm.TMACHipError) as e:
        run(wr, [m.wp], x, 1)
    assert e.value.code == E_NOMATCH and "gather" in str(e.value)


# ---- 3. N >= 2 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,bits,gs,kind", [(1024, 2, 128, "random"), (2304, 4, 64, "last_first"), (512, 4, 128, "reversal")])
def test_several_rows_are_the_plain_twin_bit_for_bit(tm, K, bits, gs, kind):
    """N = 2, 5 take the row loop behind ONE gathered half-table build (k_gemv_quad copies the image), N = 13 and 70 k_gemm_planes behind the
    gathered LUT image (the GEMM threshold is set to 12 so that both are GEMM calls at every shape), and with tmac_hip_debug_rows_kernel(2)
    N = 2, 5 take k_gemv_rows behind the gathered half-table build.  The row loop of the permuted call and the twin's k_gemv_quad launch
    with grid.y = N are compared under one forced configuration, (512, 2), as in the one-row case: the waves per quad shape the sums."""
    import torch
    wr = tm.TMACGeMMWrapper(act_group_size=AGS)
    L = tm.lib()
    m = mat(tm, 100 + bits, 2 * BM[bits], K, bits, gs, kind)
    for dt in (torch.float16, torch.float32):
        for N, rows_forced in ((2, False), (5, False), (13, False), (70, False), (2, True), (5, True)):
            tm.binding.check(L.tmac_hip_reset_state())
            tm.binding.check(L.tmac_hip_set_gemm_min_n(12))
            if rows_forced:
                tm.binding.check(L.tmac_hip_debug_rows_kernel(2))
            elif N < 12:
                tm.binding.check(L.tmac_hip_debug_quad_config(512, 2))
            x = acts(N + K, N, K, dt)
            xg = gathered(m, x)
            before = route_stats(tm)
            (cp,) = run(wr, [m.wp], x, N)
            got = route_delta(before, route_stats(tm))
            want = {R_ROWS: 1} if rows_forced else {R_ROW_LOOP: 1, R_QUAD: 1} if N < 12 else {R_PLANES: 1}
            assert got == want, (N, rows_forced, got)
            (ct,) = run(wr, [m.wt], xg, N)
            for n in range(N):
                assert torch.equal(cp[n], ct[n]), (N, rows_forced, dt, n, float((cp[n] - ct[n]).abs().max()))
            ref = m.oracle(xg.float().cpu().numpy())
            assert np.abs(ct.cpu().numpy() - ref).max() < 1e-3 * np.abs(ref).max()


# ---- 4. fused q/k/v-style calls -----------------------------------------------------------------------------------------------------
def test_fused_calls_share_the_permutation_or_are_refused(tm):
    import torch
    wr = tm.TMACGeMMWrapper(act_group_size=AGS)
    bits, K, gs = 2, 1024, 128
    q = mat(tm, 200, 128, K, bits, gs, "random")
    # three matrices on ONE KPerm object, and three on distinct objects of equal content
    shared = [q] + [Mat(tm, 201 + i, Mw, K, bits, gs, "random", kperm=q.kperm, g_idx=q.g_idx) for i, Mw in enumerate((256, 128))]
    own = []
    for i, Mw in enumerate((128, 256, 128)):
        kp = tm.KPerm(q.g_idx.copy(), gs)
        assert kp.handle.value != q.kperm.handle.value and kp.id == q.kperm.id
        own.append(Mat(tm, 204 + i, Mw, K, bits, gs, "random", kperm=kp, g_idx=q.g_idx))
    for mats in (shared, own):
        for N in (1, 5):
            x = acts(7 + N, N, K, torch.float16)
            xg = gathered(q, x)
            cps = run(wr, [mm.wp for mm in mats], x, N, torch.float16)
            cts = run(wr, [mm.wt for mm in mats], xg, N, torch.float16)
            for cp, ct, mm in zip(cps, cts, mats):
                assert torch.equal(cp, ct), (N, float((cp.float() - ct.float()).abs().max()))
                ref = mm.oracle(xg.float().cpu().numpy())
                assert np.abs(cp.float().cpu().numpy() - ref).max() < 2e-3 * np.abs(ref).max()
    # a mix of permutations, and a mix of permuted and plain: refused, outputs untouched
    other = mat(tm, 210, 128, K, bits, gs, "reversal")
    x = acts(9, 1, K, torch.float16)
    for ws in ([q.wp, other.wp], [q.wp, q.wt], [q.wt, q.wp, other.wp]):
        for N in (1, 5):
            outs = [torch.full((N, w.Mw), 7.0, dtype=torch.float32, device="cuda") for w in ws]
            with pytest.raises(tm.TMACHipError) as e:
                wr.fused(ws, acts(9, N, K, torch.float16), outs, N)
            assert e.value.code == E_ARG and "must share the K permutation" in str(e.value)
            torch.cuda.synchronize()
            assert all(bool((o == 7.0).all()) for o in outs)


# ---- 5. the split path --------------------------------------------------------------------------------------------------------------
def test_split_path(tm):
    import torch
    bits, K, gs = 2, 1024, 64
    m = mat(tm, 102, 256, K, bits, gs, "random")
    wr = tm.TMACGeMMWrapper(act_group_size=AGS)
    wr.set_workspace(K, 16)
    for N in (1, 5, 13):
        x = acts(30 + N, N, K, torch.float16)
        xg = gathered(m, x)
        sp, st = (torch.full((N, m.Mw), 7.0, dtype=torch.float32, device="cuda") for _ in range(2))
        wr.llama_cpp_init(x, m.Mw, K, N, bits, kperm=m.kperm)
        wr.llama_cpp_compute(m.wp, sp, N)
        # ... and the plain handle on the permuted workspace is refused
        with pytest.raises(tm.TMACHipError) as e:
            wr.llama_cpp_compute(m.wt, st, N)
        assert e.value.code == E_ARG and "K permutation" in str(e.value)
        torch.cuda.synchronize()
        assert bool((st == 7.0).all())
        wr.llama_cpp_init(xg, m.Mw, K, N, bits)
        wr.llama_cpp_compute(m.wt, st, N)
        # ... and the permuted handle on the plain workspace
        scratch = torch.full((N, m.Mw), 7.0, dtype=torch.float32, device="cuda")
        with pytest.raises(tm.TMACHipError) as e:
            wr.llama_cpp_compute(m.wp, scratch, N)
        assert e.value.code == E_ARG and "K permutation" in str(e.value)
        torch.cuda.synchronize()
        assert bool((scratch == 7.0).all())
        assert torch.equal(sp, st), (N, float((sp - st).abs().max()))
        (fp_,) = run(wr, [m.wp], x, N)
        (ft_,) = run(wr, [m.wt], xg, N)
        if torch.equal(st, ft_):          # where the plain split and fused paths agree bit for bit, so do the permuted ones
            assert torch.equal(sp, fp_), N
        ref = m.oracle(xg.float().cpu().numpy())
        assert np.abs(sp.cpu().numpy() - ref).max() < 1e-3 * np.abs(ref).max()
    # an identity permutation is the plain build: a plain handle runs on it
    ident = tm.KPerm(np.arange(K, dtype=np.int32) // gs, gs)
    assert ident.identity
    wr.llama_cpp_init(xg, m.Mw, K, N, bits, kperm=ident)
    wr.llama_cpp_compute(m.wt, scratch, N)
    torch.cuda.synchronize()
    assert torch.equal(scratch, st)


# ---- 6. recording and deferral ------------------------------------------------------------------------------------------------------
def defer_stats(tm):
    st = [C.c_uint64(0) for _ in range(4)]
    tm.binding.check(tm.lib().tmac_hip_defer_stats(*[C.byref(x) for x in st]))
    return tuple(int(x.value) for x in st)          # flushes, cache hits, stream launches, single calls


def test_a_recording_refuses_a_permuted_handle_and_stays_usable(tm):
    import torch
    bits, K, gs = 2, 1024, 128
    m = mat(tm, 200, 128, K, bits, gs, "random")
    wr = tm.TMACGeMMWrapper(act_group_size=AGS)
    x0, x1 = acts(1, 1, K, torch.float16)[0], acts(2, 1, K, torch.float16)[0]
    o0, o1, op = (torch.full((m.Mw,), 7.0, dtype=torch.float16, device="cuda") for _ in range(3))
    with wr.record_chain() as rec:
        wr.fused([m.wt], x0, [o0], 1)
        with pytest.raises(tm.TMACHipError) as e:
            wr.fused([m.wp], x0, [op], 1)
        assert e.value.code == E_ARG and "recorded" in str(e.value) and "K permutation" in str(e.value)
        wr.fused([m.wt], x1, [o1], 1)
    assert rec.chain.nops == 2
    rec.chain.launch(); torch.cuda.synchronize()
    assert rec.chain.status() == 0 and bool((op == 7.0).all())
    r0, r1 = (torch.zeros(m.Mw, dtype=torch.float16, device="cuda") for _ in range(2))
    wr.fused([m.wt], x0, [r0], 1); wr.fused([m.wt], x1, [r1], 1)
    torch.cuda.synchronize()
    for o, r in ((o0, r0), (o1, r1)):
        assert float((o.float() - r.float()).abs().max()) <= 2e-3 * float(r.float().abs().max())
    rec.chain.free()


def test_deferred_mode_orders_a_permuted_call_behind_the_queue(tm):
    import torch
    bits, K, gs = 2, 1024, 128
    m = mat(tm, 200, 128, K, bits, gs, "random")
    wr = tm.TMACGeMMWrapper(act_group_size=AGS)
    xs = [acts(40 + i, 1, K, torch.float32) for i in range(3)]
    want = [run(wr, [m.wt], xs[0], 1)[0], run(wr, [m.wp], xs[1], 1)[0], run(wr, [m.wt], xs[2], 1)[0]]
    outs = [torch.full((1, m.Mw), 7.0, dtype=torch.float32, device="cuda") for _ in range(3)]
    tm.binding.check(tm.lib().tmac_hip_defer(1))
    wr.fused([m.wt], xs[0], [outs[0]], 1)
    before = defer_stats(tm)
    wr.fused([m.wp], xs[1], [outs[1]], 1)                  # behind the queue, stand-alone
    after = defer_stats(tm)
    assert after[0] == before[0] + 1, (before, after)
    wr.fused([m.wt], xs[2], [outs[2]], 1)
    tm.binding.check(tm.lib().tmac_hip_flush(None))
    tm.binding.check(tm.lib().tmac_hip_defer(0))
    torch.cuda.synchronize()
    for o, r in zip(outs, want):
        assert torch.equal(o, r)


# ---- 7. transforms and taps on a permuted handle ------------------------------------------------------------------------------------
def test_transforms_and_taps_are_refused(tm):
    import torch
    bits, K, gs = 2, 1024, 128
    m = mat(tm, 200, 128, K, bits, gs, "random")
    wr = tm.TMACGeMMWrapper(act_group_size=AGS)
    gamma = torch.ones(K, dtype=torch.float32, device="cuda")
    for N in (1, 3):
        x = acts(50, N, K, torch.float16)
        out = torch.full((N, m.Mw), 7.0, dtype=torch.float32, device="cuda")
        with pytest.raises(tm.TMACHipError) as e:
            if N == 1:
                wr.fused_xf([m.wp], x, [out], "norm", gamma=gamma)
            else:
                wr.fused_xf_rows([m.wp], x, [out], "norm", N, gamma=gamma)
        assert e.value.code == E_ARG and "vector transform" in str(e.value) and "K permutation" in str(e.value)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())
    with pytest.raises(tm.TMACHipError) as e:
        wr.fused_partial_sums(m.wp, acts(51, 1, K, torch.float16), 1)
    assert e.value.code == E_ARG and "tap" in str(e.value)
    # the plain twin takes all three
    wr.fused_xf([m.wt], acts(50, 1, K, torch.float16), [torch.zeros((1, m.Mw), dtype=torch.float32, device="cuda")], "norm", gamma=gamma)
    wr.fused_partial_sums(m.wt, acts(51, 1, K, torch.float16), 1)
    torch.cuda.synchronize()


# ---- 8. footprint -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (1, 5))
def test_footprint(tm, N):
    """guard bands around B, g_idx, qweight and both pack outputs (and the scales, zeros and the result), at two placements: no byte
    outside an output changes, and what lies in the guards changes no result"""
    import torch
    from tmac_amd import wrapper
    bits, Mw, K, gs = 2, 128, 2304, 128
    m = mat(tm, 102, Mw, K, bits, gs, "last_first")
    ab, sb = wrapper.ref_blob_bytes(Mw, K, bits, m.cfg, tm.F16)
    x = np.random.default_rng(60).standard_normal((N, K)).astype(np.float16)
    L = tm.lib()

    def call(alloc):
        tq, ts, tz = alloc.inp(m.src[0], name="qweight"), alloc.inp(m.src[1], name="scales"), alloc.inp(m.src[2], name="qzeros")
        tg, tb = alloc.inp(m.g_idx, name="g_idx"), alloc.inp(x, name="B")
        oA, oS = alloc.out(ab, np.uint8, "A_ref", tile=False), alloc.out(sb // 2, np.float16, "scales_ref", tile=False)
        oC = alloc.out((N, Mw), np.float32, "C")
        alloc.arm()
        kp, h = C.c_void_p(), C.c_void_p()
        tm.binding.check(L.tmac_hip_kperm_from_gidx_dev(tg.data_ptr(), K, gs, C.byref(kp), None))
        tm.binding.check(L.tmac_hip_pack_gptq_perm_dev(tq.data_ptr(), ts.data_ptr(), tz.data_ptr(), tm.F16, 1, kp, Mw, K, bits, C.byref(m.cfg),
                                                       oA.data_ptr(), oS.data_ptr(), tm.F16, None))
        tm.binding.check(L.tmac_hip_register_weights_gptq_perm_dev(C.byref(h), tq.data_ptr(), ts.data_ptr(), tz.data_ptr(), tm.F16, 1, kp, Mw, K, bits,
                                                                   C.byref(m.cfg), tm.F16, tm.F16, None))
        tm.binding.check(L.tmac_hip_kperm_free(kp))              # the handle keeps the permutation alive
        wa, ca = (C.c_void_p * 1)(h.value), (C.c_void_p * 1)(oC.data_ptr())
        tm.binding.check(L.tmac_hip_qgemm_fused_dev(wa, 1, tb.data_ptr(), tm.F16, ca, tm.F32, N, None))
        torch.cuda.synchronize()
        tm.binding.check(L.tmac_hip_free_weights(h))

    def check_want(want):
        assert np.array_equal(want["A_ref"], m.A.reshape(-1))
        assert np.array_equal(pc.raw_bits(want["scales_ref"]), pc.raw_bits(m.S.astype(np.float16)))
        ref = m.oracle(x[:, m.perm].astype(np.float32))
        assert np.abs(want["C"] - ref).max() < 1e-3 * np.abs(ref).max()

    fp.check_footprint(call, check_want=check_want)


def test_misaligned_activations_are_refused(tm):
    import torch
    bits, K, gs = 2, 1024, 128
    m = mat(tm, 200, 128, K, bits, gs, "random")
    wr = tm.TMACGeMMWrapper(act_group_size=AGS)
    buf = torch.zeros(K + 8, dtype=torch.float16, device="cuda")
    out = torch.full((1, m.Mw), 7.0, dtype=torch.float32, device="cuda")
    with pytest.raises(tm.TMACHipError) as e:
        wr.fused([m.wp], buf[4:4 + K], [out], 1)
    assert e.value.code == E_ARG and "B_dev" in str(e.value) and "aligned" in str(e.value)
    wr.set_workspace(K, 1)
    with pytest.raises(tm.TMACHipError) as e:
        wr.llama_cpp_init(buf[4:4 + K], m.Mw, K, 1, bits, kperm=m.kperm)
    assert e.value.code == E_ARG and "B_dev" in str(e.value)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---- 9. Python ----------------------------------------------------------------------------------------------------------------------
def test_weights_from_gptq_with_g_idx(tm):
    import torch
    bits, Mw, K, gs = 4, 128, 512, 128
    m = mat(tm, 104, Mw, K, bits, gs, "reversal")
    wr = tm.TMACGeMMWrapper(act_group_size=AGS)
    x = acts(70, 1, K, torch.float16)
    (want,) = run(wr, [m.wt], gathered(m, x), 1)
    from_numpy = tm.Weights.from_gptq(*m.src, m.cfg, True, tm.F16, g_idx=m.g_idx)
    from_torch = tm.Weights.from_gptq(*(dev(a) for a in m.src), m.cfg, True, tm.F16, g_idx=dev(m.g_idx))
    for w in (from_numpy, from_torch):
        assert w.kperm is not None and w.kperm.id == m.kperm.id and np.array_equal(w.kperm.perm(), m.perm)
        pid = C.c_uint64(0)
        tm.binding.check(tm.lib().tmac_hip_weights_kperm_id(w.handle, C.byref(pid)))
        assert pid.value == m.kperm.id
        assert torch.equal(run(wr, [w], x, 1)[0], want)
    # and all three fuse: equal content is the same permutation
    outs = run(wr, [m.wp, from_numpy, from_torch], x, 1)
    assert all(torch.equal(o, want) for o in outs)
    # an identity g_idx gives a plain handle
    plain = tm.Weights.from_gptq(*m.src, m.cfg, True, tm.F16, g_idx=np.arange(K, dtype=np.int32) // gs)
    assert plain.kperm is None
    pid = C.c_uint64(1)
    tm.binding.check(tm.lib().tmac_hip_weights_kperm_id(plain.handle, C.byref(pid)))
    assert pid.value == 0
    none = tm.Weights.from_gptq(*m.src, m.cfg, True, tm.F16)
    assert torch.equal(run(wr, [plain], x, 1)[0], run(wr, [none], x, 1)[0])
    for w in (from_numpy, from_torch, plain, none):
        w.free()


def write_act_order_checkpoint(d, layers, g_of):
    """pack_common.write_gptq_checkpoint's two-part layout with desc_act set and a non-trivial .g_idx per layer (g_of(name, K, gs))"""
    parts, tensors = [dict(), dict()], {}
    for i, (name, seed, Mw, K, bits, gs) in enumerate(layers):
        qw, sc, qz = pc.make_gptq(seed, Mw, K, bits, gs, np.float16, hard=False)
        for suffix, a in ((".qweight", qw), (".scales", sc), (".qzeros", qz), (".g_idx", g_of(name, K, gs))):
            parts[i % 2][name + suffix] = a
            tensors[name + suffix] = a
    parts[0]["model.norm.weight"] = np.ones(8, np.float16)
    for i, p in enumerate(parts):
        pc.write_safetensors(os.path.join(d, "model-{:05d}-of-00002.safetensors".format(i + 1)), p)
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump({"model_type": "llama", "quantization_config": {"bits": layers[0][4], "group_size": layers[0][5], "sym": False, "desc_act": True,
                                                                   "quant_method": "gptq", "meta": {"quantizer": "gptqmodel:1.2.3"}}}, f)
    return tensors


def test_load_gptq_dir_act_order(tm, tmp_path):
    import torch
    from tmac_amd import checkpoint, convert
    gs, bits, H = 128, 2, 512
    names = ["model.layers.0.self_attn.{}_proj".format(n) for n in "qkv"] + ["model.layers.0.mlp.down_proj", "model.layers.0.mlp.up_proj"]
    layers = [(names[0], 81, 128, H, bits, gs), (names[1], 82, 128, H, bits, gs), (names[2], 83, 256, H, bits, gs), (names[3], 84, 128, 1024, bits, gs),
              (names[4], 85, 128, H, bits, gs)]
    g_qkv, g_down = make_g_idx("random", 5, H, gs), make_g_idx("random", 6, 1024, gs)

    def g_of(name, K, g):
        return g_down if "down" in name else np.arange(K, dtype=np.int32) // g if "up_proj" in name else g_qkv

    tensors = write_act_order_checkpoint(str(tmp_path), layers, g_of)
    wr = tm.TMACGeMMWrapper(act_group_size=AGS)
    with pytest.raises(AssertionError, match="desc_act=True currently unsupported"):
        checkpoint.load_gptq_dir(str(tmp_path), wr)
    with pytest.raises(AssertionError, match="desc_act=True currently unsupported"):
        convert.get_quantization_config(str(tmp_path))
    assert convert.get_quantization_config(str(tmp_path), allow_desc_act=True)["desc_act"] is True
    loaded = checkpoint.load_gptq_dir(str(tmp_path), wr, act_order=True)
    assert sorted(loaded) == sorted(names)
    q, k, v, down, up = (loaded[n] for n in names)
    assert q.kperm is not None and q.kperm is k.kperm and q.kperm is v.kperm, "q/k/v share one KPerm"
    assert down.kperm is not None and down.kperm is not q.kperm and up.kperm is None
    x = acts(90, 1, H, torch.float16)
    outs = run(wr, [q, k, v], x, 1)
    perm = np.argsort(g_qkv, kind="stable")
    xg = x.float().cpu().numpy()[:, perm]
    for (name, seed, Mw, K, b, g), o in zip(layers[:3], outs):
        bm = convert.default_bm(b, Mw)
        _, _, (w, sc, zr, _, _) = pc.host_blob_gptq(tensors[name + ".qweight"], tensors[name + ".scales"], tensors[name + ".qzeros"], True, bm, KF)
        A, S = pc.host_blob_codes(np.ascontiguousarray(w[:, perm]), sc, zr, b, bm, KF)
        ql, ls, lb = orc.preprocessor(xg, AGS)
        ref = orc.qgemm_float(A, ql, S.astype(np.float32), ls, lb, Mw, K, 1, b, bm, KF, g, AGS, True)
        assert np.abs(o.cpu().numpy() - ref).max() <= 1e-3 * np.abs(ref).max()
    # a layer without its .g_idx is refused by name
    os.remove(os.path.join(str(tmp_path), "model-00002-of-00002.safetensors"))
    pc.write_safetensors(os.path.join(str(tmp_path), "model-00002-of-00002.safetensors"),
                         {n + s: tensors[n + s] for n in (names[1], names[3]) for s in (".qweight", ".scales", ".qzeros")})
    with pytest.raises(RuntimeError, match=r"k_proj\.g_idx is missing"):
        checkpoint.load_gptq_dir(str(tmp_path), wr, act_order=True)
    for w in loaded.values():
        w.free()
