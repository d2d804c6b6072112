"""Act-order handles in stream mode: a recording DECLARED INDEPENDENT when it begins (tmac_hip_chain_begin_independent,
record_chain(independent=True)) becomes k_lut_images + k_gemv_stream or fails, never k_decode_chain -- and therefore notes calls on handles
that carry a K permutation: k_lut_images gathers x[perm] per call, k_gemv_stream sees finished tables.

The bar is exact and has no tolerance of its own.  Two declared-independent recordings of the same shapes -- the permuted handles wp on x,
and the plain twins wt (registered from the host blob of w[:, perm], test_gpu_actorder.Mat) on x.index_select(perm) -- get the same plan
and the same k_gemv_stream: their outputs are torch.equal and so are their integer taps (tmac_hip_chain_set_tap), in both forms of
k_gemv_stream (the autouse fixture, as in test_gpu_stream.py).  The twin's recording is held to the oracle at the project's 1e-3 and its
tap to the oracle bit for bit, which ties the gather build to the reference through the twin.

Shapes are the smallest at which k_lut_images can go wrong: K = 256 (P = 32 pairs: most of the only 256-pair block is padding), 1024 (half
a block), 2304 (a ragged second block), 6144 (three full blocks); 128 rows (192 for 3 bits); group sizes 128 and 64 (the G2 instances of
k_gemv_stream); fp16 and fp32 activations; the three permutation kinds of test_gpu_actorder.
"""
import ctypes as C

import numpy as np
import pytest

import footprint as fp
from oracle import oracle as orc
from test_gpu_actorder import AGS, BM, KF, PERM_KINDS, Mat, acts, dev, mat, tm      # noqa: F401  (tm: fixture)

pytestmark = pytest.mark.gpu
E_NOMATCH, E_ARG = -1, -4


@pytest.fixture(autouse=True, params=["auto", "quad64"])
def _form(request, monkeypatch):
    """both forms of k_gemv_stream (test_gpu_stream.py): the default choice, and the (quad x 64 units) form forced"""
    if request.param == "quad64":
        monkeypatch.setenv("TMAC_STREAM_QW", "0")


def fresh(ws, dtype):
    import torch
    return [torch.full((w.Mw,), 7.0, dtype=dtype, device="cuda") for w in ws]


def record(wr, calls, out_dtype, independent=True):
    """calls: [(handles, activation vector)] -> (chain, outputs per call), every call recorded with N = 1"""
    outs = [fresh(ws, out_dtype) for ws, _ in calls]
    with wr.record_chain(independent=independent) as rec:
        for (ws, x), os_ in zip(calls, outs):
            wr.fused(ws, x, os_, 1)
    return rec.chain, outs


def launch(chain):
    import torch
    chain.launch()
    torch.cuda.synchronize()
    assert chain.status() == 0


def tapped(chain):
    """one more launch with the parity tap set: the integers k_gemv_stream accumulated, all calls"""
    import torch
    total, _ = chain.tap_layout(chain.nops)
    buf = torch.full((total,), -(2 ** 31), dtype=torch.int32, device="cuda")
    chain.set_tap(buf)
    try:
        launch(chain)
    finally:
        chain.set_tap(None)
    return buf


def oracle_tap(m, xg):
    """comb[row][act group] = sum_p 2^p PS_p of the gathered matrix on the gathered vector xg (fp32 numpy [K]): test_gpu_chain.check_tap"""
    q, _, _ = orc.preprocessor(xg[None, :], AGS)
    PS = orc.partial_sums(m.A, q[0], m.Mw, m.K, m.bits, m.bm, KF, AGS)
    o = np.arange(m.Mw)
    return sum(PS[(o // 8) * 8 * m.bits + p * 8 + (o % 8)].astype(np.int64) << p for p in range(m.bits))


def permuted_and_twin(calls):
    """calls: [(Mat or (Mat, ...) fused, x, permuted?)] -> the two recordings' call lists: permuted handles on x | plain twins on x[perm]
    (a call that is not permuted is the twin on the gathered vector in BOTH: a plain op of a mixed chain)"""
    a, b = [], []
    for ms, x, permuted in calls:
        ms = ms if isinstance(ms, tuple) else (ms,)
        xg = x.index_select(0, ms[0].dperm).contiguous()
        b.append(([mm.wt for mm in ms], xg))
        a.append(([mm.wp for mm in ms], x) if permuted else b[-1])
    return a, b


def check_pair(tm, wr, calls, out_dtype, oracle=True, launches=1, rewrite=None):
    """the module's bar on one set of calls; returns nothing.  launches > 1: rewrite(i) changes the activations in place between launches
    and every launch is compared again (the images are rebuilt per launch)."""
    import torch
    ca, cb = permuted_and_twin(calls)
    pa, oa = record(wr, ca, out_dtype)
    pb, ob = record(wr, cb, out_dtype)
    try:
        assert pa.stream and pb.stream and pa.quarter_walk == pb.quarter_walk and pa.nops == pb.nops == len(calls)
        for i in range(len(calls)):
            assert pa.wpq(i) == pb.wpq(i), "the two recordings have one plan"
        for it in range(launches):
            if it and rewrite is not None:
                rewrite(it)
                for (ms, x, _), (_, xg) in zip(calls, cb):      # the twin reads the gathered copy: gather it again, in place
                    ms = ms if isinstance(ms, tuple) else (ms,)
                    xg.copy_(x.index_select(0, ms[0].dperm))
            launch(pa); launch(pb)
            for i, (xa, xb) in enumerate(zip(oa, ob)):
                for k, (p, q) in enumerate(zip(xa, xb)):
                    assert torch.equal(p, q), (it, i, k, float((p.float() - q.float()).abs().max()))
        ta, tb = tapped(pa), tapped(pb)
        assert torch.equal(ta, tb), "the integers of the two launches differ"
        if oracle:
            tap = tb.cpu().numpy()
            for i, ((ms, _, _), (_, xg)) in enumerate(zip(calls, cb)):
                ms = ms if isinstance(ms, tuple) else (ms,)
                xn = xg.float().cpu().numpy()
                off, cnt = pb.tap_layout(i)
                r0, per_row = 0, ms[0].K // 64
                assert cnt == sum(mm.Mw for mm in ms) * per_row
                for k, mm in enumerate(ms):
                    ref = mm.oracle(xn[None, :])[0]
                    got = ob[i][k].float().cpu().numpy()
                    assert np.abs(got - ref).max() < 1e-3 * np.abs(ref).max(), (i, k)
                    g = tap[off + r0 * per_row: off + (r0 + mm.Mw) * per_row].reshape(mm.Mw, per_row)
                    assert np.array_equal(g.astype(np.int64), oracle_tap(mm, xn)), f"call {i} matrix {k}: the twin's integer tap != oracle"
                    r0 += mm.Mw
    finally:
        pa.free(); pb.free()


def matrix_cases(K):
    """(bits, rows, group size, permutation kind): 2 and 4 bits at both group sizes, 1 and 3 bits once (K = 1024); the kinds dealt in turn"""
    out = [(bits, 128, gs, PERM_KINDS[(2 * i + j + K // 256) % 3]) for i, bits in enumerate((2, 4)) for j, gs in enumerate((128, 64))]
    if K == 1024:
        out += [(3, 192, 128, "random"), (1, 128, 64, "reversal")]
    return out


# ---- 1. the equality matrix: a lone permuted call -----------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (256, 1024, 2304, 6144))
def test_a_lone_permuted_call_is_the_plain_twin_bit_for_bit(tm, K):
    import torch
    wr = tm.TMACGeMMWrapper(act_group_size=AGS)
    for bits, Mw, gs, kind in matrix_cases(K):
        m = mat(tm, 300 + bits, Mw, K, bits, gs, kind)
        for dt in (torch.float16, torch.float32):
            x = acts(K + bits + gs, 1, K, dt)[0].contiguous()
            check_pair(tm, wr, [(m, x, True)], torch.float32)
            # the permutation is not a no-op: the permuted handle on the gathered vector computes something else
        xg = x.index_select(0, m.dperm).contiguous()
        c1, o1 = record(wr, [([m.wp], x)], torch.float32)
        c2, o2 = record(wr, [([m.wp], xg)], torch.float32)
        launch(c1); launch(c2)
        assert not torch.equal(o1[0][0], o2[0][0])
        c1.free(); c2.free()


# ---- 2. recordings ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", (2, 4))
def test_plain_ops_and_two_permutations_in_one_chain(tm, bits):
    """five calls: permuted (permutation A, group size 128), plain, permuted (permutation B, another K, group size 64), plain, permuted (A
    again, through another object of equal content); fp16 and fp32 activations mixed, fp16 outputs"""
    import torch
    wr = tm.TMACGeMMWrapper(act_group_size=AGS)
    a = mat(tm, 310 + bits, 128, 1024, bits, 128, "random")
    b = mat(tm, 320 + bits, 128, 2304, bits, 64, "last_first")
    a2 = Mat(tm, 330 + bits, 256, 1024, bits, 128, "random", kperm=tm.KPerm(a.g_idx.copy(), 128), g_idx=a.g_idx)
    assert a2.kperm.handle.value != a.kperm.handle.value and a2.kperm.id == a.kperm.id
    xs = [acts(400 + i, 1, K, dt)[0].contiguous() for i, (K, dt) in enumerate(((1024, torch.float16), (1024, torch.float32), (2304, torch.float16),
                                                                               (2304, torch.float16), (1024, torch.float32)))]
    check_pair(tm, wr, [(a, xs[0], True), (a, xs[1], False), (b, xs[2], True), (b, xs[3], False), (a2, xs[4], True)], torch.float16)


def test_a_fused_triple_shares_one_permutation(tm):
    """q/k/v: three matrices on ONE KPerm object, then three on distinct objects of equal content, each as one call of the chain"""
    import torch
    wr = tm.TMACGeMMWrapper(act_group_size=AGS)
    bits, K, gs = 2, 1024, 128
    q = mat(tm, 340, 128, K, bits, gs, "random")
    shared = (q,) + tuple(Mat(tm, 341 + i, Mw, K, bits, gs, "random", kperm=q.kperm, g_idx=q.g_idx) for i, Mw in enumerate((256, 128)))
    own = tuple(Mat(tm, 344 + i, Mw, K, bits, gs, "random", kperm=tm.KPerm(q.g_idx.copy(), gs), g_idx=q.g_idx) for i, Mw in enumerate((128, 256, 128)))
    x0, x1 = (acts(410 + i, 1, K, torch.float16)[0].contiguous() for i in range(2))
    check_pair(tm, wr, [(shared, x0, True), (own, x1, True)], torch.float32)


def test_an_identity_g_idx_records_a_plain_op(tm):
    """a handle registered through an identity g_idx carries no permutation: the declared recording holds no permuted op (it launches the
    plain k_lut_images) and equals the plain recording of the handle registered without a g_idx, bit for bit"""
    import torch
    wr = tm.TMACGeMMWrapper(act_group_size=AGS)
    bits, Mw, K, gs = 2, 128, 1024, 128
    m = mat(tm, 340, Mw, K, bits, gs, "random")
    ident = tm.Weights.from_gptq(*m.src, m.cfg, True, tm.F16, g_idx=np.arange(K, dtype=np.int32) // gs)
    none = tm.Weights.from_gptq(*m.src, m.cfg, True, tm.F16)
    pid = C.c_uint64(1)
    tm.binding.check(tm.lib().tmac_hip_weights_kperm_id(ident.handle, C.byref(pid)))
    assert ident.kperm is None and pid.value == 0
    x = acts(420, 1, K, torch.float16)[0].contiguous()
    ci, oi = record(wr, [([ident], x)], torch.float32)
    cn, on = record(wr, [([none], x)], torch.float32, independent=False)
    launch(ci); launch(cn)
    assert ci.stream and cn.stream and torch.equal(oi[0][0], on[0][0])
    assert torch.equal(tapped(ci), tapped(cn))
    ci.free(); cn.free(); ident.free(); none.free()


def test_every_launch_rebuilds_the_images(tm):
    """one chain, three launches, x rewritten in between: every launch equals the twin's"""
    import torch
    wr = tm.TMACGeMMWrapper(act_group_size=AGS)
    m = mat(tm, 302, 128, 2304, 2, 64, PERM_KINDS[(1 + 2304 // 256) % 3])
    x = acts(430, 1, m.K, torch.float16)[0].contiguous()

    def rewrite(it):
        x.copy_(acts(430 + it, 1, m.K, torch.float16)[0])

    check_pair(tm, wr, [(m, x, True)], torch.float32, oracle=False, launches=3, rewrite=rewrite)


# ---- 3. the rules of the declaration ------------------------------------------------------------------------------------------------
def untouched(*ts):
    import torch
    torch.cuda.synchronize()
    return all(bool((t == 7.0).all()) for t in ts)


def test_data_flow_ends_a_declared_recording_with_both_ops_named(tm):
    import torch
    wr = tm.TMACGeMMWrapper(act_group_size=AGS)
    m = mat(tm, 350, 256, 256, 2, 128, "random")            # 256 rows of K = 256: its output is a vector it can read
    x = acts(440, 1, 256, torch.float16)[0].contiguous()
    o0, o1 = fresh([m.wt, m.wt], torch.float16)
    with pytest.raises(tm.TMACHipError) as e:
        with wr.record_chain(independent=True):
            wr.fused([m.wt], x, [o0], 1)
            wr.fused([m.wt], o0, [o1], 1)
    assert e.value.code == E_ARG and "op 1 reads an output of op 0" in str(e.value) and "declared independent" in str(e.value), str(e.value)
    assert untouched(o0, o1)
    # the recording is over: the thread launches calls again, and the undeclared recording of the same calls is k_decode_chain's
    wr.fused([m.wt], x, [o0], 1)
    torch.cuda.synchronize()
    assert not bool((o0 == 7.0).any())
    with wr.record_chain() as rec:
        wr.fused([m.wt], x, [o0], 1)
        wr.fused([m.wt], o0, [o1], 1)
    assert not rec.chain.stream
    rec.chain.free()


def test_transforms_and_exchange_steps_are_refused_at_once_and_the_recording_stays_usable(tm):
    import torch
    wr = tm.TMACGeMMWrapper(act_group_size=AGS)
    m = mat(tm, 340, 128, 1024, 2, 128, "random")
    x = acts(450, 1, m.K, torch.float16)[0].contiguous()
    gamma = torch.ones(m.K, dtype=torch.float32, device="cuda")
    (o0,), (o1,), (ox,) = (fresh([m.wt], torch.float16) for _ in range(3))
    send, recv = torch.zeros(128, dtype=torch.float16, device="cuda"), torch.zeros(128, dtype=torch.float16, device="cuda")
    with wr.record_chain(independent=True) as rec:
        wr.fused([m.wp], x, [o0], 1)
        with pytest.raises(tm.TMACHipError) as e:
            wr.fused_xf([m.wt], x, [ox], "norm", gamma=gamma)
        assert e.value.code == E_ARG and "declared independent" in str(e.value) and "transform" in str(e.value), str(e.value)
        with pytest.raises(tm.TMACHipError) as e:
            wr.record_gather(send, recv, 256, 0, 1)
        assert e.value.code == E_ARG and "declared independent" in str(e.value) and "exchange" in str(e.value), str(e.value)
        wr.fused([m.wt], x, [o1], 1)          # (no transform is left pending for this call)
    assert rec.chain.nops == 2 and rec.chain.stream
    launch(rec.chain)
    assert untouched(ox) and not bool((o0 == 7.0).any()) and not bool((o1 == 7.0).any())
    rec.chain.free()


def test_stream_mode_switched_off_fails_a_declared_recording(tm, monkeypatch):
    import torch
    wr = tm.TMACGeMMWrapper(act_group_size=AGS)
    m = mat(tm, 340, 128, 1024, 2, 128, "random")
    x = acts(460, 1, m.K, torch.float16)[0].contiguous()
    monkeypatch.setenv("TMAC_CHAIN_STREAM", "0")
    for w in (m.wp, m.wt):
        (o,) = fresh([w], torch.float16)
        with pytest.raises(tm.TMACHipError) as e:
            with wr.record_chain(independent=True):
                wr.fused([w], x, [o], 1)
        assert e.value.code == E_ARG and "TMAC_CHAIN_STREAM=0" in str(e.value) and "declared independent" in str(e.value), str(e.value)
        assert untouched(o)
    monkeypatch.delenv("TMAC_CHAIN_STREAM")
    c, _ = record(wr, [([m.wp], x)], torch.float16)       # the thread records again
    assert c.stream
    c.free()


def test_a_mix_of_permutations_in_one_fused_call_is_refused(tm):
    import torch
    wr = tm.TMACGeMMWrapper(act_group_size=AGS)
    q = mat(tm, 340, 128, 1024, 2, 128, "random")
    other = mat(tm, 351, 128, 1024, 2, 128, "reversal")
    x = acts(470, 1, 1024, torch.float16)[0].contiguous()
    (o,) = fresh([q.wp], torch.float16)
    with wr.record_chain(independent=True) as rec:
        for ws in ([q.wp, other.wp], [q.wp, q.wt], [q.wt, q.wp, other.wp]):
            outs = fresh(ws, torch.float16)
            with pytest.raises(tm.TMACHipError) as e:
                wr.fused(ws, x, outs, 1)
            assert e.value.code == E_ARG and "must share the K permutation" in str(e.value)
            assert untouched(*outs)
        wr.fused([q.wp], x, [o], 1)
    assert rec.chain.nops == 1
    rec.chain.free()


def test_a_plain_declared_recording_is_the_undeclared_one(tm):
    """no permuted op: the declaration changes nothing about what is launched -- outputs and integers bit for bit those of record_chain()"""
    import torch
    wr = tm.TMACGeMMWrapper(act_group_size=AGS)
    a, b = mat(tm, 340, 128, 1024, 2, 128, "random"), mat(tm, 302, 128, 2304, 2, 64, PERM_KINDS[(1 + 2304 // 256) % 3])
    calls = [([a.wt], acts(480, 1, a.K, torch.float16)[0].contiguous()), ([b.wt], acts(481, 1, b.K, torch.float32)[0].contiguous()),
             ([a.wt, a.wt], acts(482, 1, a.K, torch.float16)[0].contiguous())]
    cd, od = record(wr, calls, torch.float16)
    cu, ou = record(wr, calls, torch.float16, independent=False)
    assert cd.stream and cu.stream and cd.quarter_walk == cu.quarter_walk
    launch(cd); launch(cu)
    for xa, xb in zip(od, ou):
        for p, q in zip(xa, xb):
            assert torch.equal(p, q) and not bool((p == 7.0).any())
    assert torch.equal(tapped(cd), tapped(cu))
    cd.free(); cu.free()


def test_an_undeclared_recording_still_refuses_a_permuted_handle(tm):
    """(a restatement: test_gpu_actorder.py pins this refusal)"""
    import torch
    wr = tm.TMACGeMMWrapper(act_group_size=AGS)
    m = mat(tm, 340, 128, 1024, 2, 128, "random")
    x = acts(490, 1, m.K, torch.float16)[0].contiguous()
    (o,), (op,) = fresh([m.wt], torch.float16), fresh([m.wp], torch.float16)
    with wr.record_chain() as rec:
        wr.fused([m.wt], x, [o], 1)
        with pytest.raises(tm.TMACHipError) as e:
            wr.fused([m.wp], x, [op], 1)
        assert e.value.code == E_ARG and "recorded" in str(e.value) and "K permutation" in str(e.value)
    assert rec.chain.nops == 1 and untouched(op)
    rec.chain.free()


# ---- 4. lifetime --------------------------------------------------------------------------------------------------------------------
def test_the_chain_keeps_its_permutations_alive(tm):
    """after _end the caller's KPerm object is freed and the Python handle drops its reference to it, the weights stay: the launch reads
    the permutation the chain itself holds, and the result is the one from before"""
    import torch
    wr = tm.TMACGeMMWrapper(act_group_size=AGS)
    m = Mat(tm, 360, 128, 2304, 2, 128, "random")           # its own KPerm, shared with nothing
    x = acts(500, 1, m.K, torch.float16)[0].contiguous()
    chain, ((o,),) = record(wr, [([m.wp], x)], torch.float32)
    launch(chain)
    want = o.clone()
    assert not bool((want == 7.0).any())
    m.kperm.free()
    m.wp.kperm = None
    m.kperm = None
    # (allocations that would land where a released array was)
    junk = [torch.full((m.K,), 2 ** 30, dtype=torch.int32, device="cuda") for _ in range(8)]
    o.fill_(7.0)
    launch(chain)
    assert torch.equal(o, want)
    del junk
    chain.free()


# ---- 5. footprint -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (256, 2304))
def test_footprint(tm, K):
    """guard bands around x, g_idx (the permutation is built from it), the checkpoint tensors and both outputs of a chain of a permuted and
    a plain call, at two placements: nothing outside the outputs is written, and what lies in the guards changes no result"""
    import torch
    bits, Mw, gs = 2, 128, 128
    m = mat(tm, 370, Mw, K, bits, gs, "last_first")
    x = np.random.default_rng(61).standard_normal(K).astype(np.float16)
    L = tm.lib()

    def call(alloc):
        tq, ts, tz = alloc.inp(m.src[0], name="qweight"), alloc.inp(m.src[1], name="scales"), alloc.inp(m.src[2], name="qzeros")
        tg, tb = alloc.inp(m.g_idx, name="g_idx"), alloc.inp(x, name="B")
        oP, oT = alloc.out((1, Mw), np.float32, "C_permuted"), alloc.out((1, Mw), np.float32, "C_plain")
        alloc.arm()
        kp, hp, ht, ch = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        tm.binding.check(L.tmac_hip_kperm_from_gidx_dev(tg.data_ptr(), K, gs, C.byref(kp), None))
        tm.binding.check(L.tmac_hip_register_weights_gptq_perm_dev(C.byref(hp), tq.data_ptr(), ts.data_ptr(), tz.data_ptr(), tm.F16, 1, kp, Mw, K, bits,
                                                                   C.byref(m.cfg), tm.F16, tm.F16, None))
        tm.binding.check(L.tmac_hip_register_weights_gptq_dev(C.byref(ht), tq.data_ptr(), ts.data_ptr(), tz.data_ptr(), tm.F16, 1, Mw, K, bits,
                                                              C.byref(m.cfg), tm.F16, tm.F16, None))
        tm.binding.check(L.tmac_hip_kperm_free(kp))
        tm.binding.check(L.tmac_hip_chain_begin_independent())
        try:
            for h, o in ((hp, oP), (ht, oT)):
                wa, ca = (C.c_void_p * 1)(h.value), (C.c_void_p * 1)(o.data_ptr())
                tm.binding.check(L.tmac_hip_qgemm_fused_dev(wa, 1, tb.data_ptr(), tm.F16, ca, tm.F32, 1, None))
        except Exception:
            L.tmac_hip_chain_abort()
            raise
        tm.binding.check(L.tmac_hip_chain_end(C.byref(ch)))
        assert L.tmac_hip_chain_is_stream(ch) != 0
        tm.binding.check(L.tmac_hip_chain_launch(ch, None))
        torch.cuda.synchronize()
        tm.binding.check(L.tmac_hip_chain_free(ch))
        tm.binding.check(L.tmac_hip_free_weights(hp))
        tm.binding.check(L.tmac_hip_free_weights(ht))

    def check_want(want):
        ref = m.oracle(x[m.perm].astype(np.float32)[None, :])
        assert np.abs(want["C_permuted"] - ref).max() < 1e-3 * np.abs(ref).max()
        assert not np.array_equal(want["C_permuted"], want["C_plain"])

    fp.check_footprint(call, check_want=check_want)
