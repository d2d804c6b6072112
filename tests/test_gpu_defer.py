"""The deferred queue (tmac_hip_defer / tmac_hip_flush, tmac_amd/csrc/tmac_defer.cpp) against every entry point that can run ahead of it, and
through its error paths.  include/tmac_hip.h promises "results are those of launching the calls in order": here a producer (an N = 1 fused
call into `y`) is QUEUED and a second call that reads, or overwrites, what the producer writes or reads is issued through another entry point
-- the split path, the taps, a recorded chain, an N > 1 fused call, the calls that free what the queue names -- with no flush in between.

Every hazard scenario is checked three ways (the harness and the bounds of test_gpu_stream.py's deferred tests):
 (a) against the same calls issued in order with deferral off: 2e-3 max-norm on fp16 outputs (a batch may run k_gemv_stream's quarter-walk form);
 (b) against the oracle on the vectors the calls actually consumed: 1e-3;
 (c) against the WRONG answer: every output and intermediate vector is poisoned before each run, and the test first computes, with deferral
     off, what the calls give in the order a queue that is not consulted would run them (the second call on the poisoned / not yet written
     bytes, the producer afterwards).  That result must differ from the right one by at least 50 x the bound of (a): a condition on the
     inputs, asserted, so that a scenario which cannot tell the two orders apart fails instead of passing.
The flush must happen AT the second call (tmac_hip_defer_stats), not at the explicit flush that follows.

Error paths: no flush fails on a healthy GPU, so they are driven by tmac_hip_debug_defer_fail(n) -- the n-th launch attempt of the following
flushes returns TMAC_HIP_E_RUNTIME on the host side, before anything reaches the device.

Each test prints its figures (`DEFER <scenario>: ...`): the stale-vs-right margin of (c) and the observed errors of (a) and (b).
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_chain import AGS, BITS_BM, KF, Model, rel_err, tm, _short_spin      # noqa: F401  (fixtures)
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

BOUND_INORDER = 2e-3        # deferred batch vs in-order launches (test_gpu_stream.py: test_deferred_launches_equal_in_order_launches)
BOUND_ORACLE = 1e-3         # ... vs the oracle on the consumed vectors (same test)
MARGIN = 50 * BOUND_INORDER  # what the wrong order must differ by for a scenario to count
E_RUNTIME = -3              # TMAC_HIP_E_RUNTIME (include/tmac_hip.h)
POISON_IN = 1.0             # a queued output that was not written yet: a constant vector against N(0, 1)-like data
POISON_OUT = -3.0           # an output of the second call that was never written


def f32(t):
    return t.float().cpu().numpy()


def stats(tm):
    st = [C.c_uint64(0) for _ in range(4)]
    tm.binding.check(tm.lib().tmac_hip_defer_stats(*[C.byref(x) for x in st]))
    return tuple(int(x.value) for x in st)          # flushes, cache hits, stream launches, single calls


def report(name, margin, ea, eb):
    print(f"DEFER {name}: stale-vs-right margin {margin:.3g} (needs >= {MARGIN:.3g}); (a) vs in-order {ea:.3g} (<= {BOUND_INORDER:g}); "
          f"(b) vs oracle {eb:.3g} (<= {BOUND_ORACLE:g})")


def check_bits(a, b):
    assert a.shape == b.shape and np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


class Producer:
    """the queued call: y = W x, one N = 1 fused call (K0 -> rows); `into` places y inside a larger buffer (row of an [N][rows] matrix)"""

    def __init__(self, tm, K0=1024, rows=1024, seed=1, into=None):
        self.m = Model(tm, [(K0, [rows], None)], seed=seed)
        if into is not None:
            self.m.outs[0][0] = into
        self.x, self.y = self.m.x_ext[0], self.m.outs[0][0]
        self.x0 = self.x.clone()

    def __call__(self):
        self.m.issue()

    def oracle(self, x=None):
        return self.m.oracle_outputs(0, f32(self.x0) if x is None else x)[0]

    def free(self):
        self.m.free()


def drive(tm, name, producer, consumer, collect, oracle, hazard_keys, poison, restore=lambda: None, exact=None):
    """right order with deferral off; wrong order with deferral off; then the producer queued and the consumer issued with no flush between."""
    import torch
    L = tm.lib()

    def prepare():
        restore(); poison(); torch.cuda.synchronize()

    prepare(); producer(); consumer(); torch.cuda.synchronize()
    right = collect()
    prepare(); consumer(); producer(); torch.cuda.synchronize()      # what a queue that is not consulted gives
    stale = collect()
    margin = min(rel_err(stale[k], right[k]) for k in hazard_keys)
    assert margin >= MARGIN, f"{name}: the wrong order differs by {margin:.3g} only: the scenario cannot discriminate"
    prepare()
    tm.binding.check(L.tmac_hip_defer(1))
    try:
        s0 = stats(tm)
        producer()
        assert stats(tm) == s0, "the producer was not queued"
        consumer()
        s1 = stats(tm)
        assert s1[0] == s0[0] + 1, f"{name}: the queue was not flushed by the call that depends on it: {s0} -> {s1}"
        tm.binding.check(L.tmac_hip_flush(None))
        assert stats(tm) == s1, f"{name}: the explicit flush still found queued calls"
        torch.cuda.synchronize()
        got = collect()
    finally:
        L.tmac_hip_defer(0)
    ea = max(rel_err(got[k], right[k]) for k in right)
    want = oracle(got)
    eb = max(rel_err(got[k], want[k]) for k in want)
    report(name, margin, ea, eb)
    assert ea <= BOUND_INORDER, f"{name}: deferred run vs in-order launches"
    assert eb <= BOUND_ORACLE, f"{name}: deferred run vs the oracle"
    if exact is not None:
        exact(got, right, want)
    return got


def rows_oracle(m, i, X):
    """oracle outputs of op i of Model m, matrix 0, for every row of X [N][K] -> [N][Mw]"""
    return np.stack([m.oracle_outputs(i, X[n])[0] for n in range(X.shape[0])])


# ---- 1 / 8: RAW through the split path (tmac_hip_preprocessor_dev + tmac_hip_qgemm_dev) and through an N > 1 fused call ------------------
def _raw_rows(tm, name, N, split):
    import torch
    R, M1 = 1024, 512
    Y = torch.from_numpy(np.random.default_rng(70 + N).standard_normal((N, R)).astype(np.float32)).cuda().half()
    r = N // 2
    p = Producer(tm, rows=R, seed=11, into=Y[r])
    mc = Model(tm, [(R, [M1], None)], seed=12)
    w = mc.ws[0][0]
    out = torch.zeros((N, M1), dtype=torch.float16, device="cuda")
    if split:
        mc.wr.set_workspace(R, N)

    def consumer():
        if split:
            mc.wr.llama_cpp_init(Y, M1, R, N, mc.bits)
            mc.wr.llama_cpp_compute(w, out, N)
        else:
            mc.wr.fused([w], Y, [out], N)

    def poison():
        Y[r].fill_(POISON_IN); out.fill_(POISON_OUT)

    drive(tm, name, p, consumer, lambda: {"y": f32(Y), "c": f32(out)},
          lambda got: {"y": np.concatenate([got["y"][:r], p.oracle()[None], got["y"][r + 1:]]), "c": rows_oracle(mc, 0, got["y"])},
          ["c"], poison)
    p.free(); mc.free()


@pytest.mark.parametrize("N", [1, 5])
def test_split_path_reads_a_queued_output(tm, N):
    _raw_rows(tm, f"1 split path RAW N={N}", N, split=True)


def test_fused_n3_reads_a_queued_output(tm):
    _raw_rows(tm, "8 fused N=3 RAW", 3, split=False)


# ---- 2 / 3: tmac_hip_qgemm_dev writes what a queued call reads (WAR) or writes (WAW) --------------------------------------------------------
@pytest.mark.parametrize("hazard", ["war", "waw"])
def test_split_path_overwrites_a_queued_calls_buffer(tm, hazard):
    import torch
    K0, R, Kz = 1024, 512, 512
    p = Producer(tm, K0=K0, rows=R, seed=21)
    target = p.x if hazard == "war" else p.y                   # the buffer tmac_hip_qgemm_dev writes its C into
    mc = Model(tm, [(Kz, [target.numel()], None)], seed=22)
    z = mc.x_ext[0]
    mc.wr.set_workspace(Kz, 1)
    mc.wr.llama_cpp_init(z, target.numel(), Kz, 1, mc.bits)     # the LUT is in the workspace before anything is queued: only qgemm_dev follows
    torch.cuda.synchronize()

    def poison():
        p.y.fill_(POISON_IN)

    def oracle(got):
        c = mc.oracle_outputs(0, f32(z))[0]
        return {"y": p.oracle(), "x": c} if hazard == "war" else {"y": c}

    drive(tm, f"{'2 WAR' if hazard == 'war' else '3 WAW'} qgemm_dev into a queued call's {'input' if hazard == 'war' else 'output'}", p,
          lambda: mc.wr.llama_cpp_compute(mc.ws[0][0], target, 1),
          (lambda: {"y": f32(p.y), "x": f32(p.x)}) if hazard == "war" else (lambda: {"y": f32(p.y)}), oracle, ["y"], poison,
          restore=lambda: p.x.copy_(p.x0))
    p.free(); mc.free()


# ---- 4 / 5: the taps ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["fused_tap", "split_tap"])
def test_taps_read_a_queued_output(tm, which):
    """4: tmac_hip_qgemm_fused_partial_sums on a queued output (the tap branch of the fused entry point); 5: tmac_hip_qgemm_partial_sums after a
    llama_cpp_init that read one.  The integers and the LUT scales / biases: bit for bit against the oracle on the fresh y."""
    R, M1 = 1024, 256
    p = Producer(tm, rows=R, seed=31)
    mc = Model(tm, [(R, [M1], None)], seed=32)
    w, (A, S) = mc.ws[0][0], mc.host[0][0]
    mc.wr.set_workspace(R, 1)
    res = {}

    def consumer():
        if which == "fused_tap":
            ps, c = mc.wr.fused_partial_sums(w, p.y)
            res.update(ps=ps, c=c, lut=mc.wr.last_fused_lut.copy())
        else:
            mc.wr.llama_cpp_init(p.y, M1, R, 1, mc.bits)
            res.update(ps=mc.wr.partial_sums(w, 1))

    def poison():
        p.y.fill_(POISON_IN); res.clear()

    def collect():
        d = {"y": f32(p.y), "ps": res["ps"].astype(np.float64)}
        if which == "fused_tap":
            d["c"] = res["c"]; d["lut"] = res["lut"]
        return d

    def oracle(got):
        q, ls, lb = orc.preprocessor(got["y"][None, :], AGS)
        want = {"y": p.oracle(), "ps": orc.partial_sums(A, q[0], M1, R, mc.bits, BITS_BM[mc.bits], KF, AGS)[None].astype(np.float64)}
        if which == "fused_tap":
            want["c"] = rows_oracle(mc, 0, got["y"][None, :])
            want["lut"] = np.stack([ls, lb], axis=1)
        return want

    def exact(got, right, want):
        assert np.array_equal(got["ps"], want["ps"]), "integer partial sums on the fresh y != oracle"
        assert np.array_equal(got["ps"], right["ps"])
        if which == "fused_tap":
            check_bits(got["lut"][:, 0, :], want["lut"][:, 0, :])
            check_bits(got["lut"][:, 1, :], want["lut"][:, 1, :])

    drive(tm, "4 fused tap RAW" if which == "fused_tap" else "5 split tap RAW", p, consumer, collect, oracle, ["ps"] + (["c"] if which == "fused_tap" else []),
          poison, exact=exact)
    p.free(); mc.free()


# ---- 6 / 7: tmac_hip_chain_launch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["chain", "stream"])
def test_chain_launch_reads_a_queued_output(tm, form):
    R = 1024
    p = Producer(tm, rows=R, seed=41)
    ops = [(R, [256], None), (256, [128, 256], (0, 0))] if form == "chain" else [(R, [256], None), (R, [128, 512], None), (R, [1024], None)]
    mc = Model(tm, ops, seed=42)
    for i in mc.x_ext:
        mc.x_ext[i] = p.y
    chain = mc.record()
    assert chain.stream == (form == "stream")
    keys = [(i, k) for i in range(len(ops)) for k in range(len(ops[i][1]))]

    def poison():
        p.y.fill_(POISON_IN)
        for os_ in mc.outs:
            for o in os_:
                o.fill_(POISON_OUT)

    def oracle(got):
        want = {"y": p.oracle()}
        for i, (K, rows, src) in enumerate(ops):
            ref = mc.oracle_outputs(i, got["y"] if src is None else got[f"c{src[0]}.{src[1]}"])
            for k in range(len(rows)):
                want[f"c{i}.{k}"] = ref[k]
        return want

    drive(tm, f"6 chain_launch RAW ({form})", p, chain.launch, lambda: {"y": f32(p.y), **{f"c{i}.{k}": f32(mc.outs[i][k]) for i, k in keys}}, oracle,
          [f"c{i}.{k}" for i, k in keys], poison)
    assert chain.status() == 0
    chain.free(); p.free(); mc.free()


def test_chain_launch_overwrites_a_queued_calls_input(tm):
    K0 = 1024
    p = Producer(tm, K0=K0, rows=512, seed=51)
    ops = [(512, [256], None), (256, [K0], (0, 0))]
    mc = Model(tm, ops, seed=52)
    mc.outs[1][0] = p.x                                         # the chain's last call writes the vector the queued call reads
    chain = mc.record()

    def poison():
        p.y.fill_(POISON_IN); mc.outs[0][0].fill_(POISON_OUT)

    def oracle(got):
        return {"y": p.oracle(), "c0": mc.oracle_outputs(0, f32(mc.x_ext[0]))[0], "x": mc.oracle_outputs(1, got["c0"])[0]}

    drive(tm, "7 chain_launch WAR", p, chain.launch, lambda: {"y": f32(p.y), "c0": f32(mc.outs[0][0]), "x": f32(p.x)}, oracle, ["y"], poison,
          restore=lambda: p.x.copy_(p.x0))
    assert chain.status() == 0
    chain.free(); p.free(); mc.free()


# ---- 9 / 10: releasing what the queue names --------------------------------------------------------------------------------------------------
def _lifetime(tm, name, release):
    """the producer is queued, then `release(producer)` runs: the queued call must have been launched by it (flush counter), its output right
    after a synchronisation, and a following flush a no-op"""
    import torch
    L = tm.lib()
    p = Producer(tm, rows=512, seed=61)
    p(); torch.cuda.synchronize()
    right = f32(p.y)
    p.y.fill_(POISON_IN); torch.cuda.synchronize()
    margin = rel_err(f32(p.y), right)
    assert margin >= MARGIN
    want = p.oracle()
    tm.binding.check(L.tmac_hip_defer(1))
    try:
        s0 = stats(tm)
        p()
        assert stats(tm) == s0
        release(p)
        s1 = stats(tm)
        assert s1[0] == s0[0] + 1 and s1[3] == s0[3] + 1, f"{name}: the queued call was not launched by the releasing call: {s0} -> {s1}"
        torch.cuda.synchronize()
        got = f32(p.y)
        tm.binding.check(L.tmac_hip_flush(None))
        assert stats(tm) == s1, f"{name}: a flush after the release still found queued calls"
        torch.cuda.synchronize()
        assert np.array_equal(f32(p.y), got)
    finally:
        L.tmac_hip_defer(0)
    ea, eb = rel_err(got, right), rel_err(got, want)
    report(name, margin, ea, eb)
    assert ea <= BOUND_INORDER and eb <= BOUND_ORACLE
    p.free()


def test_freeing_a_queued_matrix_launches_the_queue_first(tm):
    _lifetime(tm, "9 free_weights of a queued matrix", lambda p: p.m.ws[0][0].free())


@pytest.mark.parametrize("what", ["chain_free", "cache_clear"])
def test_chain_free_and_cache_clear_with_a_non_empty_queue(tm, what):
    other = Model(tm, [(256, [128], None), (128, [64], (0, 0))], seed=62)
    chain = other.record()
    _lifetime(tm, f"10 {what} with a queued call", (lambda p: chain.free()) if what == "chain_free" else (lambda p: tm.binding.check(tm.lib().tmac_hip_cache_clear())))
    chain.free(); other.free()


# ---- error paths --------------------------------------------------------------------------------------------------------------------------------
class Calls:
    """independent N = 1 calls with poisoned outputs: in-order results first, then whatever the test does with the queue"""

    def __init__(self, tm, models):
        import torch
        self.tm, self.models = tm, models
        self.calls = [(m, i) for m in models for i in range(len(m.ops))]
        for m in models:
            m.issue()
        torch.cuda.synchronize()
        self.right = [[f32(o) for o in m.outs[i]] for m, i in self.calls]
        self.poison()

    def poison(self):
        import torch
        for m, i in self.calls:
            for o in m.outs[i]:
                o.fill_(POISON_OUT)
        torch.cuda.synchronize()

    def issue(self, j):
        m, i = self.calls[j]
        m.wr.fused(m.ws[i], m.x_of(i), m.outs[i], 1, act_dtype=m.act_dtype(i))

    def check_right(self, j, name):
        m, i = self.calls[j]
        want = m.oracle_outputs(i, f32(m.x_of(i)))
        for k, o in enumerate(m.outs[i]):
            g = f32(o)
            margin, ea, eb = rel_err(np.full_like(g, POISON_OUT), self.right[j][k]), rel_err(g, self.right[j][k]), rel_err(g, want[k])
            report(f"{name} call {j} matrix {k}", margin, ea, eb)
            assert margin >= MARGIN and ea <= BOUND_INORDER and eb <= BOUND_ORACLE, f"{name}: call {j} matrix {k}"

    def check_poison(self, j):
        m, i = self.calls[j]
        for o in m.outs[i]:
            assert bool((o == POISON_OUT).all()), f"call {j} was launched"

    def free(self):
        for m in self.models:
            m.free()


def raw_fused(tm, weights, x, outs):
    """tmac_hip_qgemm_fused_dev without the wrapper's exception: (return code, message)"""
    L = tm.lib()
    n = len(weights)
    wa = (C.c_void_p * n)(*[w.handle.value for w in weights])
    ca = (C.c_void_p * n)(*[o.data_ptr() if o is not None else None for o in outs])
    rc = L.tmac_hip_qgemm_fused_dev(wa, n, x.data_ptr(), tm.F16, ca, tm.F16, 1, None)
    return rc, L.tmac_hip_last_error().decode()


def test_invalid_calls_are_refused_when_they_are_queued(tm):
    """E1: matrices of different K in one call, and a null output pointer: the code and message of the non-deferred call, at once; the valid
    calls queued before and after are launched by ONE flush"""
    import torch
    L = tm.lib()
    c = Calls(tm, [Model(tm, [(1024, [256], None), (512, [128], None), (1024, [512], None)], seed=71)])
    m = c.models[0]
    bad = [([m.ws[0][0], m.ws[1][0]], m.x_ext[0], [m.outs[0][0], m.outs[1][0]]),            # K = 1024 and K = 512 fused
           ([m.ws[1][0]], m.x_ext[1], [None])]                                           # null output
    off = [raw_fused(tm, *b) for b in bad]
    torch.cuda.synchronize()
    assert all(rc != 0 for rc, _ in off)
    c.poison()
    tm.binding.check(L.tmac_hip_defer(1))
    try:
        s0 = stats(tm)
        c.issue(0)
        for j, (b, (rc_off, msg_off)) in enumerate(zip(bad, off)):
            rc, msg = raw_fused(tm, *b)
            assert (rc, msg) == (rc_off, msg_off), f"deferred: {rc} {msg!r}; not deferred: {rc_off} {msg_off!r}"
            c.issue(1 + j)
        assert stats(tm) == s0, "a refused call disturbed the queue"
        tm.binding.check(L.tmac_hip_flush(None))
        s1 = stats(tm)
        assert s1[0] == s0[0] + 1 and (s1[2] - s0[2], s1[3] - s0[3]) == (1, 0), (s0, s1)      # three valid calls of one configuration: one stream launch
        torch.cuda.synchronize()
    finally:
        L.tmac_hip_defer(0)
    for j in range(3):
        c.check_right(j, "E1 refusal at enqueue")
    c.free()


def test_a_failed_single_launch_does_not_take_the_rest_down(tm):
    """E2: four calls that flush one by one (two configurations of two calls), the second launch fails"""
    import torch
    L = tm.lib()
    ops = [(1024, [256], None), (512, [128, 256], None)]
    c = Calls(tm, [Model(tm, ops, bits=2, seed=72), Model(tm, ops, bits=4, seed=73)])
    tm.binding.check(L.tmac_hip_defer(1))
    try:
        s0 = stats(tm)
        for j in range(4):
            c.issue(j)
        tm.binding.check(L.tmac_hip_debug_defer_fail(2))
        rc = L.tmac_hip_flush(None)
        assert rc == E_RUNTIME, rc
        s1 = stats(tm)
        assert (s1[0] - s0[0], s1[2] - s0[2], s1[3] - s0[3]) == (1, 0, 4), (s0, s1)
        tm.binding.check(L.tmac_hip_flush(None))              # nothing left: no launch, no error
        assert stats(tm) == s1
        torch.cuda.synchronize()
    finally:
        L.tmac_hip_defer(0)
    for j in (0, 2, 3):
        c.check_right(j, "E2 failed single launch")
    c.check_poison(1)
    c.free()


def test_a_failed_stream_launch_falls_back_to_single_launches(tm):
    """E3: four calls of one configuration flush as one stream launch; it fails; the calls go out one by one and the flush has done its work"""
    import torch
    L = tm.lib()
    c = Calls(tm, [Model(tm, [(1024, [256], None), (512, [128, 256], None), (2688, [128], None), (1024, [1024], None)], seed=74)])
    tm.binding.check(L.tmac_hip_defer(1))
    try:
        s0 = stats(tm)
        for j in range(4):
            c.issue(j)
        tm.binding.check(L.tmac_hip_debug_defer_fail(1))
        tm.binding.check(L.tmac_hip_flush(None))
        s1 = stats(tm)
        assert (s1[0] - s0[0], s1[2] - s0[2], s1[3] - s0[3]) == (1, 1, 4), (s0, s1)
        torch.cuda.synchronize()
        for j in range(4):
            c.check_right(j, "E3 failed stream launch")
        # the same batch again, nothing injected: the cached recording, one stream launch
        c.poison()
        for j in range(4):
            c.issue(j)
        tm.binding.check(L.tmac_hip_flush(None))
        s2 = stats(tm)
        assert (s2[0] - s1[0], s2[1] - s1[1], s2[2] - s1[2], s2[3] - s1[3]) == (1, 1, 1, 0), (s1, s2)
        torch.cuda.synchronize()
        for j in range(4):
            c.check_right(j, "E3 the batch again")
    finally:
        L.tmac_hip_defer(0)
    c.free()


def test_a_failed_flush_fails_the_n3_call_behind_it(tm):
    """E4: the flush an N = 3 fused call triggers fails: the call returns the error and launches nothing"""
    import torch
    L = tm.lib()
    c = Calls(tm, [Model(tm, [(1024, [256], None)], seed=75)])
    m = c.models[0]
    X3 = torch.from_numpy(np.random.default_rng(76).standard_normal((3, 1024)).astype(np.float32)).cuda().half()
    out3 = torch.full((3, 256), POISON_OUT, dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()
    tm.binding.check(L.tmac_hip_defer(1))
    try:
        s0 = stats(tm)
        c.issue(0)
        tm.binding.check(L.tmac_hip_debug_defer_fail(1))
        with pytest.raises(tm.binding.TMACHipError) as ei:
            m.wr.fused(m.ws[0], X3, [out3], 3)
        assert ei.value.code == E_RUNTIME
        s1 = stats(tm)
        assert s1[0] == s0[0] + 1
        tm.binding.check(L.tmac_hip_flush(None))              # the queue is empty after the failed flush
        assert stats(tm) == s1
        torch.cuda.synchronize()
        assert bool((out3 == POISON_OUT).all()), "the N = 3 call was launched behind a failed flush"
        c.check_poison(0)
        m.wr.fused(m.ws[0], X3, [out3], 3)                     # ... and the next one runs
        torch.cuda.synchronize()
        want = rows_oracle(m, 0, f32(X3))
        assert rel_err(f32(out3), want) <= BOUND_ORACLE
    finally:
        L.tmac_hip_defer(0)
    c.free()


@pytest.mark.parametrize("leave", ["defer0", "reset_state"])
def test_deferred_mode_ends_whatever_the_last_flush_returns(tm, leave):
    """E5: tmac_hip_defer(0) / tmac_hip_reset_state with a failing flush: the error is returned, deferred mode is off and the queue empty --
    the next N = 1 fused call is launched at once (tests/conftest.py relies on tmac_hip_reset_state for isolation)"""
    import torch
    L = tm.lib()
    c = Calls(tm, [Model(tm, [(1024, [256], None), (512, [128], None)], seed=77)])
    tm.binding.check(L.tmac_hip_defer(1))
    try:
        c.issue(0)
        tm.binding.check(L.tmac_hip_debug_defer_fail(1))
        rc = L.tmac_hip_defer(0) if leave == "defer0" else L.tmac_hip_reset_state()
        assert rc == E_RUNTIME, rc
        s0 = stats(tm)
        if leave == "reset_state":                             # a freshly loaded library has counted nothing (tests that read absolute counters rely on it)
            assert s0 == (0, 0, 0, 0), s0
        c.issue(1)                                             # not queued: launched
        torch.cuda.synchronize()
        assert stats(tm) == s0
        c.check_right(1, f"E5 after a failed {leave}")
        c.check_poison(0)
        c.issue(0)                                             # the hook was one-shot, the queue is empty: call 0 runs now
        torch.cuda.synchronize()
        c.check_right(0, f"E5 after a failed {leave}")
        assert stats(tm) == s0
    finally:
        L.tmac_hip_defer(0)
    c.free()


def test_flush_launches_on_the_stream_the_calls_were_issued_on(tm):
    """E6: tmac_hip_flush(other stream) launches a queue issued on the null stream on the null stream"""
    import torch
    L = tm.lib()
    c = Calls(tm, [Model(tm, [(1024, [256], None), (512, [128, 256], None), (2688, [128], None)], seed=78)])
    other = torch.cuda.Stream()
    tm.binding.check(L.tmac_hip_defer(1))
    try:
        s0 = stats(tm)
        for j in range(3):
            c.issue(j)
        tm.binding.check(L.tmac_hip_flush(other.cuda_stream))
        s1 = stats(tm)
        assert s1[0] == s0[0] + 1
        torch.cuda.current_stream().synchronize()              # the issuing stream only
        for j in range(3):
            c.check_right(j, "E6 flush(other stream)")
    finally:
        L.tmac_hip_defer(0)
    c.free()
