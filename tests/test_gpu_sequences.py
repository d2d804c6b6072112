"""Call-sequence parity: what a call computes depends on that call alone, not on the calls a process made before it.

The library keeps state that outlives a call: the per-(device, stream) workspace of the fused entry point's N >= 2 routes (its LUT, its LUT
image and whether that image is valid), a caller's workspace on the split entry points, the knobs.  Every other GPU file makes one kind of
call on a freshly reset library; this one runs calls of different plans after each other on one stream, without a reset in between.

The catalogue.  Two matrices (Mw 128 and 192) per kind, K = 1024 or 512, three activation sets.  planes_crossover is 8 to 13 rows for these
shapes, so N = 24 pays for k_gemm_planes at default knobs and N = 4 / 5 does not.  Each call asserts the plan (tmac_hip_debug_fused_plan, or
tmac_hip_debug_xf_rows_plan for the transformed N >= 2 kinds) and the launches it made (tmac_hip_debug_route_stats): a sequence test that
never reaches the state it is about fails instead of passing.

  kind  call                                                   plan (route, LUT build)        launches counted
  a     N = 1, W2 pair                                         k_gemv_quad, none              quad 1
  b     N = 1, fused_xf NORM (residual, gamma), W2 pair        k_gemv_quad (XF), none         quad 1
  c     N = 4, W2 pair                                         k_gemv_quad grid.y = N, none   quad 1
  d     N = 4, W2 pair, rows kernel forced for the call        k_gemv_rows, half tables       rows 1
  e     N = 24, W2 pair                                        k_gemm_planes, image           planes 1
  f     N = 24, W2 pair, zero points on the first only         row loop, half tables          loop 1, quad 2
  f2    N = 24, W2 + W4                                        row loop, half tables          loop 1, quad 2
  g     N = 24, W1 pair, zero points on the first only         row loop, every layout         loop 1, planes 2
  g2    N = 24, W3 + W2                                        row loop, every layout         loop 1, planes 2
  h     N = 24, W2 pair, k_gemm_onehot selected for the call   k_gemm_onehot, half tables     onehot 1
  i     N = 24, unified-scale W2 pair                          k_gemm_planes_us, image        planes 1
  j     N = 24, unified W2 + W4                                row loop, half tables          loop 1, quad 2
  k     N = 24, unified W1 + W3                                row loop, every layout         loop 1, planes 2
  l     N = 24, fused_xf_rows GLU, W2 pair                     k_gemm_planes, image           planes 1
  m     N = 5, fused_xf_rows NORM, W2 pair                     row loop, half tables          loop 1, quad 2
  n     N = 70, W2 pair (image padded to 128 rows)             k_gemm_planes, image           planes 1

Kind h needs two knobs, not one: with tmac_hip_debug_gemm_kernel(1) alone k_gemm_onehot's own crossover applies (32 rows and a grid that fills
the chip), and N = 24 plans as kind c does.  tmac_hip_set_gemm_min_n(24) for the call puts it on k_gemm_onehot, the route the kind is about.
A knob a kind needs is set just before its call and put back to its default right after it.

Bars, the project's own: fp32 outputs rel_err <= 2e-5 against the oracle (orc.preprocessor + orc.qgemm_float); unified-scale outputs bit
for bit orc.qgemm_scale_final's; the transformed kinds (fp16 in, fp16 out) within 2e-3 of the oracle on the numpy-transformed rows, the bar
and the reference functions of tests/test_gpu_xf.py and tests/test_gpu_xf_rows.py.  Where a test says "fresh bits" the outputs are also bit
for bit those of the same call made first after a reset.

The sequences of test_stale_image_regressions used to fail: the half-table build of an untransformed row-loop call left gimg_valid as the
call before it on the stream had set it, and plan_split then ran k_gemm_planes on the earlier call's LUT image (outputs W_B x_A).
"""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest

from test_gpu_xf_rows import EPS, np_transform
from xf_common import Mat, poison, rel_err

pytestmark = pytest.mark.gpu
E_ARG = -4
MWS = (128, 192)
KS = (1024, 512)
PLANES, ONEHOT, QUAD, ROWS, LOOP = 0, 1, 2, 3, 7                     # enum Route (include/tmac_hip.h, tmac_hip_debug_fused_plan)
LUT_NONE, LUT_IMAGE, LUT_HALF, LUT_ALL = 0, 1, 2, 3                  # enum LutBuild
ROUTE_NAMES = ("planes", "onehot", "quad", "rows", "fused", "lo", "ref", "loop")

W1, W1N, W2, W2N, W3, W4 = dict(bits=1), dict(bits=1, zp=False), dict(bits=2), dict(bits=2, zp=False), dict(bits=3), dict(bits=4)
U1, U2, U3, U4 = (dict(bits=b, m_groups=1) for b in (1, 2, 3, 4))
ROWS_FORCED = (("tmac_hip_debug_rows_kernel", 2, 0),)                # (setter, value for the call, default)
ONEHOT_SELECTED = (("tmac_hip_debug_gemm_kernel", 1, 0), ("tmac_hip_set_gemm_min_n", 24, 32))

Kind = namedtuple("Kind", "N mats plan stats xf knobs", defaults=(None, ()))
CATALOGUE = {
    "a": Kind(1, (W2, W2), (QUAD, LUT_NONE), {QUAD: 1}),
    "b": Kind(1, (W2, W2), (QUAD, LUT_NONE), {QUAD: 1}, xf="norm1"),
    "c": Kind(4, (W2, W2), (QUAD, LUT_NONE), {QUAD: 1}),
    "d": Kind(4, (W2, W2), (ROWS, LUT_HALF), {ROWS: 1}, knobs=ROWS_FORCED),
    "e": Kind(24, (W2, W2), (PLANES, LUT_IMAGE), {PLANES: 1}),
    "f": Kind(24, (W2, W2N), (LOOP, LUT_HALF), {LOOP: 1, QUAD: 2}),
    "f2": Kind(24, (W2, W4), (LOOP, LUT_HALF), {LOOP: 1, QUAD: 2}),
    "g": Kind(24, (W1, W1N), (LOOP, LUT_ALL), {LOOP: 1, PLANES: 2}),
    "g2": Kind(24, (W3, W2), (LOOP, LUT_ALL), {LOOP: 1, PLANES: 2}),
    "h": Kind(24, (W2, W2), (ONEHOT, LUT_HALF), {ONEHOT: 1}, knobs=ONEHOT_SELECTED),
    "i": Kind(24, (U2, U2), (PLANES, LUT_IMAGE), {PLANES: 1}),
    "j": Kind(24, (U2, U4), (LOOP, LUT_HALF), {LOOP: 1, QUAD: 2}),
    "k": Kind(24, (U1, U3), (LOOP, LUT_ALL), {LOOP: 1, PLANES: 2}),
    "l": Kind(24, (W2, W2), (PLANES, LUT_IMAGE), {PLANES: 1}, xf="glu"),
    "m": Kind(5, (W2, W2), (LOOP, LUT_HALF), {LOOP: 1, QUAD: 2}, xf="norm"),
    "n": Kind(70, (W2, W2), (PLANES, LUT_IMAGE), {PLANES: 1}),
}
KINDS = list(CATALOGUE)


@pytest.fixture(scope="module")
def tm():
    import torch
    import tmac_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return tmac_amd


# ---- the module's caches: weights, activations, oracle results and fresh-state bits, each made once and never changed -----------------
_WR, _MATS, _VEC, _DEV, _ORACLE, _FRESH = [], {}, {}, {}, {}, {}


def wrapper(tm):
    if not _WR:
        _WR.append(tm.TMACGeMMWrapper(act_group_size=64))
    return _WR[0]


def mat(tm, spec, slot, K):
    """the matrix of `spec` in slot 0 / 1 of a call (Mw 128 / 192); kinds that name the same spec in the same slot share it"""
    key = (tuple(sorted(spec.items())), slot, K)
    if key not in _MATS:
        seed = K + 100 * spec["bits"] + 20 * int(spec.get("zp", True)) + 10 * int(spec.get("m_groups", -1) >= 1) + slot
        _MATS[key] = Mat(tm, wrapper(tm), seed, MWS[slot], K, **spec)
    return _MATS[key]


def mats_of(tm, kind, K):
    return [mat(tm, spec, i, K) for i, spec in enumerate(CATALOGUE[kind].mats)]


def vectors(N, K, aset, f16):
    key = (N, K, aset, f16)
    if key not in _VEC:
        rng = np.random.default_rng(1000003 * aset + 1009 * N + K + (7 if f16 else 0))
        dt = np.float16 if f16 else np.float32
        x, x2 = (rng.standard_normal((N, K)).astype(dt) for _ in range(2))
        res = rng.standard_normal((N, K)).astype(np.float32)
        gam = (1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)
        _VEC[key] = dict(x=x, x2=x2, res=res, gam=gam)
    return _VEC[key]


def dev_vectors(N, K, aset, f16):
    import torch
    key = (N, K, aset, f16)
    if key not in _DEV:
        _DEV[key] = {k: torch.from_numpy(a).cuda() for k, a in vectors(N, K, aset, f16).items()}
    return _DEV[key]


def oracle_outputs(tm, kind, K, aset):
    key = (kind, K, aset)
    if key not in _ORACLE:
        k = CATALOGUE[kind]
        v = vectors(k.N, K, aset, k.xf is not None)
        X = v["x"].astype(np.float32) if k.xf is None else np_transform(v, "glu" if k.xf == "glu" else "norm")
        _ORACLE[key] = [m.oracle(X) for m in mats_of(tm, kind, K)]
    return _ORACLE[key]


# ---- one call of the catalogue ---------------------------------------------------------------------------------------------------------
def route_stats(tm):
    counts = (C.c_uint64 * 8)()
    tm.binding.check(tm.lib().tmac_hip_debug_route_stats(counts))
    return list(counts)


def stats_delta(before, after):
    return {r: b - a for r, (a, b) in enumerate(zip(before, after)) if b != a}


def named(stats):
    return {ROUTE_NAMES[r]: n for r, n in stats.items()}


def planned(tm, kind, mats, outs):
    k = CATALOGUE[kind]
    n = len(mats)
    wa = (C.c_void_p * n)(*[m.w.handle.value for m in mats])
    ca = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
    r, l = C.c_int32(-1), C.c_int32(-1)
    fn = tm.lib().tmac_hip_debug_xf_rows_plan if k.xf in ("glu", "norm") else tm.lib().tmac_hip_debug_fused_plan
    tm.binding.check(fn(wa, n, ca, k.N, C.byref(r), C.byref(l)))
    return r.value, l.value


def new_outputs(tm, kind, K):
    import torch
    k = CATALOGUE[kind]
    return [poison((k.N, m.Mw), torch.float16 if k.xf else torch.float32) for m in mats_of(tm, kind, K)]


def launch(tm, kind, K, aset, stream=None, outs=None, check_stats=True):
    """the call of `kind` on activation set `aset`, into NaN-filled outputs: asserts the plan, returns (outputs, route-stats delta)"""
    k = CATALOGUE[kind]
    wr, mats = wrapper(tm), mats_of(tm, kind, K)
    d = dev_vectors(k.N, K, aset, k.xf is not None)
    outs = outs if outs is not None else new_outputs(tm, kind, K)
    L, chk = tm.lib(), tm.binding.check
    for fn, on, _ in k.knobs:
        chk(getattr(L, fn)(on))
    try:
        plan = planned(tm, kind, mats, outs)
        assert plan == k.plan, f"kind {kind} K={K}: planned (route, lut) {plan}, the catalogue says {k.plan}"
        before = route_stats(tm)
        ws = [m.w for m in mats]
        if k.xf is None:
            wr.fused(ws, d["x"], outs, k.N, stream=stream)
        elif k.xf == "norm1":
            wr.fused_xf(ws, d["x"], outs, "norm", residual=d["res"], gamma=d["gam"], eps=EPS, stream=stream)
        elif k.xf == "glu":
            wr.fused_xf_rows(ws, d["x"], outs, "glu", k.N, in2=d["x2"], stream=stream)
        else:
            wr.fused_xf_rows(ws, d["x"], outs, "norm", k.N, residual=d["res"], gamma=d["gam"], eps=EPS, stream=stream)
        delta = stats_delta(before, route_stats(tm))
    finally:
        for fn, _, off in k.knobs:
            chk(getattr(L, fn)(off))
    if check_stats:
        assert delta == k.stats, f"kind {kind} K={K}: launched {named(delta)}, the catalogue says {named(k.stats)}"
    return outs, delta


def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def to_host(outs):
    """(after a synchronisation) the outputs as numpy arrays in their own dtype"""
    return [o.cpu().numpy() for o in outs]


def check_oracle(tm, kind, K, aset, got, what=""):
    k = CATALOGUE[kind]
    for i, (g, ref) in enumerate(zip(got, oracle_outputs(tm, kind, K, aset))):
        assert np.isfinite(g).all(), f"{what}kind {kind} K={K} matrix {i}: NaN left in the output"
        if k.mats[i].get("m_groups", -1) >= 1:
            same = np.array_equal(bits_of(g), bits_of(ref))
            assert same, f"{what}kind {kind} K={K} set {aset} matrix {i}: unified-scale output is not the oracle's bit for bit (rel err {rel_err(g, ref):.3e})"
        else:
            e, bar = rel_err(g.astype(np.float32), ref), 2e-3 if k.xf else 2e-5
            assert e <= bar, f"{what}kind {kind} K={K} set {aset} matrix {i}: rel err {e:.3e} > {bar:g} against the oracle"


def reset(tm):
    tm.binding.check(tm.lib().tmac_hip_reset_state())


def fresh_bits(tm, kind, K, aset):
    """the outputs of the call made FIRST after a reset (numpy, cached): resets the library, so ask before a sequence starts"""
    import torch
    key = (kind, K, aset)
    if key not in _FRESH:
        reset(tm)
        outs, _ = launch(tm, kind, K, aset)
        torch.cuda.synchronize()
        _FRESH[key] = to_host(outs)
        reset(tm)
    return _FRESH[key]


def check_fresh(tm, kind, K, aset, got, what=""):
    for i, (g, f) in enumerate(zip(got, _FRESH[(kind, K, aset)])):
        assert np.array_equal(bits_of(g), bits_of(f)), \
            f"{what}kind {kind} K={K} set {aset} matrix {i}: not the bits of the same call on a fresh library (rel err {rel_err(g.astype(np.float32), f.astype(np.float32)):.3e})"


def run_sequence(tm, calls, fresh=True, stats=True):
    """calls: (kind, K, aset) in order, on the current stream, no reset in between; every call against the oracle (and its fresh bits)"""
    import torch
    if fresh:
        for c in calls:
            fresh_bits(tm, *c)
    reset(tm)
    done = [launch(tm, *c, check_stats=stats) for c in calls]
    torch.cuda.synchronize()
    what = "sequence " + " -> ".join(f"{k}/K{K}/s{a}" for k, K, a in calls) + ": "
    for idx, (c, (outs, _)) in enumerate(zip(calls, done)):
        got = to_host(outs)
        check_oracle(tm, *c, got, what=f"{what}call {idx}, ")
        if fresh:
            check_fresh(tm, *c, got, what=f"{what}call {idx}, ")
    return done


# ---- 1. every kind alone ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("kind", KINDS)
def test_kind_alone(tm, kind, K):
    """the first call after a reset, against the oracle: with f, f2, g, g2, j and k the fused N >= 2 calls whose matrices differ in
    quantisation config, the (row loop, half tables) and (row loop, every layout) answers of plan_fused"""
    got = fresh_bits(tm, kind, K, 1)
    check_oracle(tm, kind, K, 1, got)


# ---- 2. every ordered pair --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K2", KS)
@pytest.mark.parametrize("second", KINDS)
@pytest.mark.parametrize("first", KINDS)
def test_transition(tm, first, second, K2):
    """`first` (K = 1024, set 0) then `second` (K2, set 1) on the default stream, no reset in between: the second call meets its bars, is
    bit for bit what it is on a fresh library, and launches what it launches there.  No pair is exempt: no state carries from call to call."""
    run_sequence(tm, [(first, 1024, 0), (second, K2, 1)])


# ---- 3. the stale LUT image, sequence by sequence ---------------------------------------------------------------------------------------
STALE = {
    # a row loop behind the three-layout build leaves a valid chunk-major image (g: k_gemm_planes per matrix); the row loop behind the
    # half-table build of other activations (f, f2) must not find it
    "g-f-same-K": [("g", 1024, 0), ("f", 1024, 1)],
    "g-f-K-1024-512": [("g", 1024, 0), ("f", 512, 1)],
    "g-a-f": [("g", 1024, 0), ("a", 1024, 2), ("f", 1024, 1)],        # an N = 1 call in between does not touch the workspace
    "g-f2": [("g", 1024, 0), ("f2", 1024, 1)],
    "k-j": [("k", 1024, 0), ("j", 1024, 1)],                          # the unified-scale twin: the row-wise image
}


@pytest.mark.parametrize("name", list(STALE))
def test_stale_image_regressions(tm, name):
    """default knobs throughout.  Precondition, asserted by the first call's route stats: it ran k_gemm_planes twice from the image of the
    three-layout build.  Then the last call's outputs against the oracle on ITS activations, and its launches: k_gemv_quad per matrix."""
    import torch
    calls = STALE[name]
    reset(tm)
    first, d0 = launch(tm, *calls[0])
    assert d0 == {LOOP: 1, PLANES: 2}, named(d0)
    for c in calls[1:-1]:
        launch(tm, *c)
    outs, delta = launch(tm, *calls[-1], check_stats=False)
    torch.cuda.synchronize()
    check_oracle(tm, *calls[0], to_host(first), what=f"{name}: first call, ")
    check_oracle(tm, *calls[-1], to_host(outs), what=f"{name}: last call (launched {named(delta)}), ")
    assert delta == {LOOP: 1, QUAD: 2}, f"{name}: the last call launched {named(delta)}"


# ---- 4. two streams ---------------------------------------------------------------------------------------------------------------------
def test_two_streams_do_not_share_tables(tm):
    """g then f on one stream, e then f on another, interleaved call by call, other activations on each stream: the per-stream workspaces"""
    import torch
    reset(tm)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    order = [(s1, ("g", 1024, 0)), (s2, ("e", 1024, 2)), (s1, ("f", 1024, 1)), (s2, ("f", 1024, 0))]
    outs = [new_outputs(tm, c[0], c[1]) for _, c in order]
    for _, c in order:
        dev_vectors(CATALOGUE[c[0]].N, c[1], c[2], False)
    torch.cuda.synchronize()              # the NaN fills and the uploads ran on the default stream
    for (st, c), o in zip(order, outs):
        launch(tm, *c, stream=st, outs=o)
    s1.synchronize(); s2.synchronize()
    for idx, ((_, c), o) in enumerate(zip(order, outs)):
        check_oracle(tm, *c, to_host(o), what=f"two streams, call {idx}: ")


# ---- 5. the workspace grows, then serves smaller calls ----------------------------------------------------------------------------------
def test_workspace_growth_and_shrink(tm):
    """N = 70 (image rows padded to 128) -> N = 24 -> 70 -> 24 at K = 512 -> 70 at K = 1024 on one stream: the workspace keeps the largest
    K and N it has seen, every call reads its own tables in it"""
    run_sequence(tm, [("n", 1024, 0), ("e", 1024, 1), ("n", 1024, 2), ("e", 512, 0), ("n", 1024, 1)])


# ---- 6. a random walk -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [11, 12, 13])
def test_random_walk(tm, seed):
    """40 calls drawn from the catalogue (kind, K, activation set) on one wrapper and one stream, no reset; the drawn sequence is in every
    assertion message"""
    rng = np.random.default_rng(seed)
    calls = [(KINDS[int(rng.integers(len(KINDS)))], KS[int(rng.integers(2))], int(rng.integers(3))) for _ in range(40)]
    run_sequence(tm, calls, fresh=False)


# ---- 7. the split entry points on a caller's workspace ----------------------------------------------------------------------------------
# state: (how the LUT gets there, N, K, the matrices it serves, the route tmac_hip_qgemm_dev then takes per matrix)
SPLIT_STATES = {
    "init-n24-k1024": ("init", 24, 1024, (W2, W2), PLANES),
    "init-n4-k512": ("init", 4, 512, (W2, W2), QUAD),
    "init-unified-n24-k1024": ("init", 24, 1024, (U2, U2), PLANES),
    "write-n24-k1024": ("write", 24, 1024, (W2, W2), QUAD),          # a caller-built LUT has no image, and 24 rows are below k_gemm_onehot's crossover
}


def make_state(tm, wr, name, aset):
    from oracle import oracle as orc
    how, N, K, specs, _ = SPLIT_STATES[name]
    ags = K if specs[0].get("m_groups", -1) >= 1 else 64
    if how == "init":
        wr.llama_cpp_init(dev_vectors(N, K, aset, False)["x"], MWS[0], K, N, specs[0]["bits"], act_group_size=ags)
    else:
        q, ls, lb = orc.preprocessor(vectors(N, K, aset, False)["x"], ags)
        wr.workspace.write(q, ls, lb, ags)


@pytest.mark.parametrize("second", list(SPLIT_STATES))
@pytest.mark.parametrize("first", list(SPLIT_STATES))
def test_split_entry_sequences(tm, first, second):
    """a caller's Workspace(1024, 24): the first state (activation set 0), then the second (set 1), then llama_cpp_compute on the weights
    of the second against the oracle; weights of another K or act group size stay refused"""
    import torch
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    wr.set_workspace(1024, 24)
    make_state(tm, wr, first, 0)
    make_state(tm, wr, second, 1)
    _, N, K, specs, route = SPLIT_STATES[second]
    mats = [mat(tm, spec, i, K) for i, spec in enumerate(specs)]
    outs = [poison((N, m.Mw), torch.float32) for m in mats]
    before = route_stats(tm)
    for m, o in zip(mats, outs):
        wr.llama_cpp_compute(m.w, o, N)
    delta = stats_delta(before, route_stats(tm))
    torch.cuda.synchronize()
    X = vectors(N, K, 1, False)["x"]
    for i, (m, o) in enumerate(zip(mats, outs)):
        got, ref = o.cpu().numpy(), m.oracle(X)
        assert np.isfinite(got).all()
        if m.mg >= 1:
            assert np.array_equal(bits_of(got), bits_of(ref)), (first, second, i)
        else:
            assert rel_err(got, ref) <= 2e-5, (first, second, i, rel_err(got, ref))
    assert delta == {route: 2}, (first, second, named(delta))
    unified = specs[0].get("m_groups", -1) >= 1
    for spec, Kw in ((specs[0], 1536 - K), (W2 if unified else U2, K)):          # another K | another act group size
        wrong = mat(tm, spec, 0, Kw)
        o = poison((N, wrong.Mw), torch.float32)
        with pytest.raises(tm.binding.TMACHipError) as ei:
            wr.llama_cpp_compute(wrong.w, o, N)
        assert ei.value.code == E_ARG and "does not match" in str(ei.value)
        torch.cuda.synchronize()
        assert torch.isnan(o).all(), "a refused call wrote its output"


# ---- 8. a caller's workspace through a permuted build, a write and a smaller build ------------------------------------------------------
def test_split_workspace_perm_write_shrink(tm):
    """a caller's Workspace(256, 13), W2 with groups of 64, Mw = 64, K = 256, N = 13 -- the first N past PLANES_MIN_N, so the builds
    come with the LUT image.  What the workspace holds after each step decides what the next call may read:
    1. a permuted init: the image is there, the permuted handle computes (the oracle on x[perm], the bar of test_gpu_actorder's split path);
    2. workspace.write of the oracle's LUT of x[perm]: no image any more, the plain handle of the gathered matrix computes on k_gemv_quad,
       the permuted handle is refused and its output stays as it was;
    3. a plain init of 4 rows: the image tap of 13 rows is refused."""
    import torch
    from oracle import oracle as orc
    from test_gpu_actorder import acts, gathered, mat as perm_mat
    bits, K, N, gs = 2, 256, 13, 64
    m = perm_mat(tm, 310, 64, K, bits, gs, "random")
    wr = tm.TMACGeMMWrapper(act_group_size=64)
    wr.set_workspace(K, N)
    x = acts(311, N, K, torch.float32)
    xg = gathered(m, x)
    xg_host = xg.cpu().numpy()
    ref = m.oracle(xg_host)

    def close(out, what):
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.isfinite(got).all(), what
        assert np.abs(got - ref).max() < 1e-3 * np.abs(ref).max(), (what, float(np.abs(got - ref).max()))

    # 1
    wr.llama_cpp_init(x, m.Mw, K, N, bits, kperm=m.kperm)
    wr.workspace.read_gemm_image(K, N)
    out = poison((N, m.Mw), torch.float32)
    wr.llama_cpp_compute(m.wp, out, N)
    close(out, "permuted handle after the permuted init")
    # 2
    wr.workspace.write(*orc.preprocessor(xg_host, 64), 64)
    with pytest.raises(tm.binding.TMACHipError) as ei:
        wr.workspace.read_gemm_image(K, N)
    assert ei.value.code == E_ARG and "holds no LUT image" in str(ei.value)
    out = poison((N, m.Mw), torch.float32)
    before = route_stats(tm)
    wr.llama_cpp_compute(m.wt, out, N)
    delta = stats_delta(before, route_stats(tm))
    close(out, "plain handle after the write")
    assert delta == {QUAD: 1}, named(delta)
    out = poison((N, m.Mw), torch.float32)
    with pytest.raises(tm.binding.TMACHipError) as ei:
        wr.llama_cpp_compute(m.wp, out, N)
    assert ei.value.code == E_ARG and "K permutation" in str(ei.value)
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused call wrote its output"
    # 3
    wr.llama_cpp_init(xg[:4].contiguous(), m.Mw, K, 4, bits)
    with pytest.raises(tm.binding.TMACHipError) as ei:
        wr.comb_sums(m.wt, N)
    assert ei.value.code == E_ARG and "holds no LUT image" in str(ei.value)
