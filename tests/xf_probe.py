"""What tests/test_gpu_xf_exact.py and tests/test_xf_probe_cpu.py share: float64 references of the vector transforms (TMAC_XF_NORM / _GLU /
_GLU_NORM with the silu, relu^2 and tanh-GELU gates, include/tmac_hip.h), the rounding margin of a transformed vector, a deterministic search
for rounding-safe inputs, the input regimes, the case list, and the mutants of the reference.  A plain module like xf_common.py and
footprint.py: no test, no fixture.

Why a margin: the LUT build quantises q = rne(v / ls), v a signed sum of four activations and ls the act group's scale.  A GPU x that differs
from the reference x by a relative eps moves v / ls by at most about 127 * eps, so q can flip only where some v / ls lies that close to a
half-integer.  Inputs whose smallest such distance (lut_margin) is at least 127 * 4 eps give the SAME QLUT from the GPU's x and from the
float64 reference x: the integer sums are equal and the fp32 outputs agree to the plain path's bar, 2e-5 of max |C|, instead of the 2e-3 the
transform tests had to allow.  (The factor 4: N = 1 and the chain evaluate the same expressions as the N >= 2 builders but cannot be tapped.)
"""
import math
import numpy as np

from oracle import oracle as orc
from xf_common import KF, pick_bm, rel_err

F32, F64 = np.float32, np.float64

# ---- measured on an MI355X (profiles/r17_xf_exact.txt): the largest |x_tap - x_ref| / |x_ref| of silu and GELU on the N >= 2 tap against
# float64 -- hardware exp and reciprocal plus the roundings around them; exp's argument carries its own rounding, about |z| * 2^-23, into the
# result, so the error grows with the gate's |z|: GELU's z grows like v^3.  tests/test_gpu_xf_exact.py holds every tapped element to these.
#   measured (tools/measure_xf_eps.py): silu 3.5e-7 (plain), 1.78e-6 (tails, at -30); GELU 1.39e-6 (plain, at in = -5.1), 6.56e-6 (tails, at -9.5:
#   z = -76; 8.9e-6 on a band 64 ulps wide, before the bands were cut to a factor of 2.8).  The asserted values leave room for other seeds.
EPS_HW = {"plain": {"silu": 5e-7, "gelu": 2e-6}, "tails": {"silu": 2.5e-6, "gelu": 1.2e-5}}


def eps_hw(c):
    """the eps of a case: by regime (`tails` against the rest) and gate; NORM and relu^2 (roundings only) take silu's"""
    gate = c["kind"].partition(":")[2]
    return EPS_HW["tails" if c["regime"] == "tails" else "plain"]["gelu" if gate == "gelu" else "silu"]


def margin_of(c):
    """what pick_safe asks of a case: 127 * 4 eps (4: N = 1 and the chain evaluate the same expressions but cannot be tapped)"""
    return 127 * 4 * eps_hw(c)


TIGHT = 2e-5               # the plain path's bar on fp32 outputs, relative to max |C|

GATES = ("silu", "relu2", "gelu")
GELU_C1, GELU_C2 = F64(F32(1.5957691216)), F64(F32(0.044715))      # the header's fp32 constants
MUTANTS = ("no_eps", "eps_outside", "drop_last8", "double_last8", "gamma_shift", "swap", "erf_gelu", "f16_product")


def norm_bound(K):
    """relative bound of the scalar r = rsq(mean(t^2) + eps): a K-term fp32 sum of non-negative terms in any order plus the single roundings
    behind it (tests/test_gpu_xf_rows.py::test_a_row_is_a_row)"""
    return (K / 2 + 16) * 2.0 ** -24


def tight_bar(kind, K, gamma=True):
    """2e-5 of max |C|; NORM with gamma and GLU_NORM add r's bound: r is common to the vector, it rescales ls and moves no table value"""
    base = kind.split(":")[0]
    return TIGHT + (norm_bound(K) if (base == "glu_norm" or (base == "norm" and gamma)) else 0.0)


def compare(c, ref, bar):
    """the comparison of the GPU file: (passes, rel err of max |C|)"""
    e = rel_err(np.asarray(c, F32), np.asarray(ref, F32))
    return bool(np.isfinite(np.asarray(c, F32)).all() and e <= bar), e


# ---- float64 references --------------------------------------------------------------------------------------------------------------
def gate64(gate, v, u):
    """gate(v) * u in float64 from the operands' own values; relu2 is specified to the bit: (max(v,0) * max(v,0)) * u, each product fp32 rn"""
    if gate == "relu2":
        m = np.maximum(np.asarray(v).astype(F32), F32(0))
        return ((m * m).astype(F32) * np.asarray(u).astype(F32)).astype(F32).astype(F64)
    v, u = np.asarray(v).astype(F64), np.asarray(u).astype(F64)
    with np.errstate(over="ignore"):
        if gate == "silu":
            return v / (1.0 + np.exp(-v)) * u
        if gate == "gelu":
            return v / (1.0 + np.exp(-(GELU_C1 * v * (1.0 + GELU_C2 * v * v)))) * u
        if gate == "gelu_erf":
            return 0.5 * v * (1.0 + np.vectorize(math.erf)(v / math.sqrt(2.0))) * u
    raise KeyError(gate)


def ref_x(kind, gate, a, b=None, residual=None, gamma=None, eps=0.0, handed_over_f16=False, mutant=None):
    """the transformed vector [K] (or rows [N][K], gamma shared) in float64, rounded once to fp32.  kind "norm" (t = fp32(in) + residual, one fp32
    add as specified; x = t * gamma / sqrt(mean(t^2) + eps), or t without gamma), "glu" (gate(in) * in2), "glu_norm" (the norm of that product).
    handed_over_f16: the product went through a chain's fp16 hand-off (xf_common.np_gated).  mutant: one of MUTANTS, CPU tests only."""
    assert mutant is None or mutant in MUTANTS
    if kind == "norm":
        t = np.asarray(a).astype(F32)
        if residual is not None:
            t = t + np.asarray(residual).astype(F32)
        t = t.astype(F64)
        if gamma is None:
            return t.astype(F32)
    else:
        if mutant == "swap":
            a, b = b, a
        g = gate64("gelu_erf" if (mutant == "erf_gelu" and gate == "gelu") else gate, a, b)
        if handed_over_f16 or mutant == "f16_product":
            g = g.astype(np.float16).astype(F64)
        if kind == "glu":
            return g.astype(F32)
        assert kind == "glu_norm", kind
        t = g
    K = t.shape[-1]
    sq = t * t
    s = sq.sum(axis=-1, keepdims=True)
    if mutant == "drop_last8":
        s = s - sq[..., -8:].sum(axis=-1, keepdims=True)
    if mutant == "double_last8":
        s = s + sq[..., -8:].sum(axis=-1, keepdims=True)
    e = F64(F32(eps))
    gam = np.asarray(gamma).astype(F64)
    if mutant == "gamma_shift":
        gam = np.roll(gam, 1)
    with np.errstate(divide="ignore"):
        if mutant == "no_eps":
            r = 1.0 / np.sqrt(s / K)
        elif mutant == "eps_outside":
            r = 1.0 / (np.sqrt(s / K) + e)
        else:
            r = 1.0 / np.sqrt(s / K + e)
    with np.errstate(invalid="ignore"):
        return np.nan_to_num(t * gam * r, nan=0.0, posinf=3e38, neginf=-3e38).astype(F32)


def case_ref(inp, mutant=None, handed_over_f16=False):
    base, _, gate = inp["kind"].partition(":")
    return ref_x(base, gate or "silu", inp["a"], inp.get("b"), inp.get("res"), inp.get("gam"), inp["eps"], handed_over_f16, mutant)


# ---- the margin -----------------------------------------------------------------------------------------------------------------------
_SIGNS = np.array([[1.0 if (g >> j) & 1 else -1.0 for j in range(4)] for g in range(16)])      # table entry g: +x_j where bit j of g is set


def lut_values(x, ags):
    """the preprocessor's pre-rounding table values v / ls in float64, [K / 4][16] (oracle/tmac_oracle.c: tables of four activations, entry g =
    +-x0 +-x1 +-x2 +-x3, ls = the act group's largest abs-sum / 127; a zero group has zero tables)"""
    x = np.asarray(x, F32).astype(F64).reshape(-1, ags // 4, 4)
    ls = np.abs(x).sum(axis=-1).max(axis=-1) / 127.0
    v = x @ _SIGNS.T
    safe = np.where(ls > 0, ls, 1.0)[:, None, None]
    return (v / safe).reshape(-1, 16)


def lut_q(x, ags):
    return np.clip(np.rint(lut_values(x, ags)), -128, 127).astype(np.int8)


def lut_margin(x, ags):
    """the smallest distance of any table value to a half-integer, in LUT steps (0.5 at best)"""
    q = lut_values(x, ags)
    return float(np.abs(q - np.floor(q) - 0.5).min())


def lut_slack(x, ags, delta):
    """what is left of every table value's distance to a half-integer after a relative perturbation of up to delta of EVERY element, to
    first order: v moves by at most delta * A (A the abs-sum of the table's four activations) and ls by delta * ls, so v / ls moves by at
    most delta * (A / ls + |v / ls|) -- up to twice the 127 * delta the uniform margin allows for, in the tables next to the group's largest.
    4e-5 steps are kept for the oracle's own fp32 roundings (four of them on values up to 127).  >= 0: no entry can flip."""
    x = np.asarray(x, F32).astype(F64).reshape(-1, ags // 4, 4)
    asum = np.abs(x).sum(axis=-1)
    ls = np.where(asum.max(axis=-1) > 0, asum.max(axis=-1), 127.0)[:, None] / 127.0
    q = lut_values(x, ags).reshape(x.shape[0], x.shape[1], 16)
    dist = np.abs(q - np.floor(q) - 0.5)
    return float((dist - 1.01 * delta * ((asum / ls)[:, :, None] + np.abs(q)) - 4e-5).min())


def pick_safe(make_inputs, margin, max_seeds, delta=0.0):
    """the first of seeds 0, 1, ... whose inputs' reference x (every row of it) has lut_margin >= margin -- and, with delta, lut_slack >= 0:
    the uniform margin does not count the movement of ls itself, which matters in the tables next to a group's largest.  Raises when there
    is none: a case that silently dropped out would hide failures."""
    best = 0.0
    for seed in range(max_seeds):
        inp = make_inputs(seed)
        m = min(lut_margin(row, inp["ags"]) for row in np.atleast_2d(inp["x"]))
        if m >= margin and delta and min(lut_slack(row, inp["ags"], delta) for row in np.atleast_2d(inp["x"])) < 0:
            continue
        if m >= margin:
            inp["seed"], inp["margin"] = seed, m
            return inp
        best = max(best, m)
    raise LookupError(f"no rounding-safe input within {max_seeds} seeds: margin wanted {margin:.3e}, best {best:.3e}")


# ---- input regimes --------------------------------------------------------------------------------------------------------------------
# every value finite and normal in its dtype; outside `plain` the magnitudes of an act group stay within a factor of 4, so that the group's
# LUT scale makes every element visible
def _rng(*key):
    return np.random.default_rng([abs(hash_int(k)) for k in key])


def hash_int(k):
    return k if isinstance(k, int) else int.from_bytes(str(k).encode(), "little") % (2 ** 31)


def _logu(rng, lo, hi, n, signs=True):
    m = np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    return m * rng.choice([-1.0, 1.0], n) if signs else m


def _gamma(K):
    """the norm weights of a K: one vector whatever the seed, so that the rows of an N >= 2 call share it"""
    return (1.0 + 0.1 * _rng("gamma", K).standard_normal(K)).astype(F32)


def _dt(act):
    return np.float16 if act == "f16" else F32


def _finish(kind, K, ags, act, eps, **v):
    inp = dict(kind=kind, K=K, ags=ags, act=act, eps=eps, **v)
    inp["x"] = case_ref(inp)
    for k in ("a", "b", "res", "gam", "x"):
        if inp.get(k) is not None:
            f = np.asarray(inp[k]).astype(F64)
            tiny = np.finfo(inp[k].dtype).tiny
            assert np.isfinite(f).all() and not ((f != 0) & (np.abs(f) < tiny)).any(), (kind, k, "not finite and normal")
    return inp


def make_plain(kind, K, ags, act, seed, eps=1e-5):
    """the N(0,1) vectors of the existing transform tests (test_gpu_xf.vectors); magnitudes below 2^-10 are raised to it (fp16 stays normal)"""
    rng = _rng("plain", kind, K, act, seed)
    lift = lambda z: np.where(np.abs(z) < 2.0 ** -10, np.copysign(2.0 ** -10, z), z)
    a, b = (lift(rng.standard_normal(K)).astype(_dt(act)) for _ in range(2))
    res, gam = rng.standard_normal(K).astype(F32), _gamma(K)
    if kind == "norm":
        return _finish(kind, K, ags, act, eps, a=a, res=res, gam=gam)
    return _finish(kind, K, ags, act, eps, a=a, b=b, gam=gam if kind.startswith("glu_norm") else None)


def make_eps(kind, K, ags, seed, eps, ratio, act=None):
    """mean(t^2) / eps == ratio (about: the scaled operands are rounded to their dtype).  act None: fp16 operands where they stay normal, else
    fp32; "f16" / "f32": that dtype (the same values before rounding; _finish refuses fp16 operands that would go denormal)"""
    rng = _rng("eps", kind, K, seed, int(round(-100 * math.log10(eps))), int(round(100 * math.log10(ratio))))
    gam = _gamma(K)
    if kind == "norm":
        a0, r0 = _logu(rng, 1.0, 2.0, K), _logu(rng, 0.125, 0.25, K)          # |t| within [0.75, 2.25] s
        s = math.sqrt(ratio * eps / float(((a0 + r0) ** 2).mean()))
        act = act or ("f16" if s >= 2.0 ** -13 else "f32")
        return _finish(kind, K, ags, act, eps, a=(a0 * s).astype(_dt(act)), res=(r0 * s).astype(F32), gam=gam)
    gate = kind.split(":")[1]
    a0 = _logu(rng, 1.0, 1.4, K, signs=False).astype(np.float16)               # gate(a) within a factor of 2 (relu2: 1.96)
    b0 = _logu(rng, 1.0, 2.0, K)
    s = math.sqrt(ratio * eps / float((gate64(gate, a0, b0) ** 2).mean()))
    act = act or ("f16" if s >= 2.0 ** -13 else "f32")
    return _finish(kind, K, ags, act, eps, a=a0.astype(_dt(act)), b=(b0 * s).astype(_dt(act)), gam=gam)


def sparse_gamma(K):
    """distinct per index, neighbours 18 % or 32 % apart"""
    i = np.arange(K, dtype=np.int64)
    return (1.0 + 0.5 * ((i * 6007) % 16381) / 16381.0).astype(F32)


def sparse_indices(K, ft=None):
    idx = [0, 7, 8, K // 2 - 1, K - 9, K - 8, K - 1]
    if ft is not None and 8 * ft < K:
        idx += [8 * ft - 1, 8 * ft]
    return sorted(set(idx))


def make_sparse(kind, K, ags, i, act="f16", eps=1e-5):
    """t zero except element i: the pipeline is exactly linear in x_i (|q| = 127 in its tables, every other table zero), so the outputs carry
    x_i to fp32 precision; no seed search.  NORM: in_i = 1, residual_i = 0.5.  GLU_NORM: in = 1 everywhere, in2_i = 1.5 and zero elsewhere."""
    gam = sparse_gamma(K)
    if kind == "norm":
        a, res = np.zeros(K, _dt(act)), np.zeros(K, F32)
        a[i], res[i] = 1.0, 0.5
        return _finish(kind, K, ags, act, eps, a=a, res=res, gam=gam)
    a, b = np.ones(K, _dt(act)), np.zeros(K, _dt(act))
    b[i] = 1.5
    return _finish(kind, K, ags, act, eps, a=a, b=b, gam=gam if kind.startswith("glu_norm") else None)


TAIL_CENTRES = [2.0 ** -12, 2.0 ** -8, 2.0 ** -4, 0.25, 1.0, 2.0, 4.0, 8.0, 16.0, 30.0]
TAILS_K = 128              # two bands per vector: the tails' own, smaller K (their eps is larger)
N_TAILS = 10


def tail_band(c, gate):
    """64 fp16-exact gate inputs from c towards 0: |c| >= 4 in steps of fp16's ulp there, below in steps of c / 256 (down to 0.75 c) -- as many
    of them as keep |gate(v)| within a factor of 2.8 of |gate(c)| (silu(-30 ... -29): a factor e; GELU at -8 falls by 2.8 within 8 ulps), repeated
    in turn to fill the group"""
    j = np.arange(64)
    m = abs(c)
    step = 2.0 ** (math.floor(math.log2(m)) - 10) if m >= 4 else m / 256
    v = np.copysign(m - j * step, c)
    assert np.array_equal(v.astype(np.float16).astype(F64), v)
    g = np.abs(gate64(gate, v, np.ones(64)))
    if g[0] > 0:
        inside = (g >= g[0] / 2.8) & (g <= g[0] * 2.8)
        n = 64 if inside.all() else int(np.argmin(inside))
        v = v[j % n]
    return v


def tail_bands(gate):
    """one magnitude band per act group, +c and -c for every centre.  GELU at -16 and -30 overflows exp and underflows the product (out of
    scope here): its two lowest bands are -9 and -9.5, the last where gelu(v) * in2 is a normal fp32"""
    out = []
    for c in TAIL_CENTRES:
        out += [c, -({16.0: 9.0, 30.0: 9.5}.get(c, c) if gate == "gelu" else c)]
    return out


def make_tails(kind, part, seed, act="f16"):
    """gate inputs: the fixed grid, bands 2 * part and 2 * part + 1 (fp16-exact values, held in the act dtype); in2: random, rounded to the act
    dtype, magnitude [1, 1.4] * {0.5, 1, 1.4} per group, within [0.5, 2]"""
    gate = kind.split(":")[1]
    rng = _rng("tails", kind, part, seed)
    a = np.concatenate([tail_band(c, gate) for c in tail_bands(gate)[2 * part: 2 * part + 2]]).astype(_dt(act))
    b = np.concatenate([_logu(rng, 1.0, 1.4, 64) * rng.choice([0.5, 1.0, 1.4]) for _ in range(2)]).astype(_dt(act))
    return _finish(kind, TAILS_K, 64, act, 1e-5, a=a, b=b)


# ---- the case list ----------------------------------------------------------------------------------------------------------------------
GLU_KINDS = tuple(f"glu:{g}" for g in GATES)
GLU_NORM_KINDS = tuple(f"glu_norm:{g}" for g in GATES)
ALL_KINDS = ("norm",) + GLU_KINDS + GLU_NORM_KINDS
EPS_COMBOS = [(e, r) for e in (1e-6, 1e-5) for r in (1e-2, 1.0, 1e2)] + [(1e-2, 1e2)]      # the last: eps = 1e-2 on an O(1) vector
MAX_SEEDS = 1200


def case(regime, kind, K, ags, **kw):
    """a case of the list: what resolve() needs to build its inputs"""
    return dict(regime=regime, kind=kind, K=K, ags=ags, **kw)


def case_id(c):
    s = f"{c['regime']}-{c['kind'].replace(':', '_')}-k{c['K']}" + ("-us" if c["ags"] == c["K"] and c["K"] > 64 else "")
    if c["regime"] == "plain":
        s += "-" + c["act"]
    if c["regime"] == "eps":
        s += f"-eps{c['eps']:g}-ratio{c['ratio']:g}"
    if c["regime"] == "tails":
        s += f"-part{c['part']}"
    if c["regime"] == "sparse":
        s += f"-i{c['i']}"
    if c["regime"] != "plain" and c.get("act"):
        s += "-" + c["act"]
    return s


_RESOLVED = {}


def resolve(c, row=0):
    """the inputs of a case: found once by pick_safe, shared, never changed.  row > 0: the next safe seeds (rows of an N >= 2 call)"""
    key = (case_id(c), row)
    if key not in _RESOLVED:
        if c["regime"] == "sparse":
            inp = make_sparse(c["kind"], c["K"], c["ags"], c["i"], c.get("act", "f16"), c.get("eps", 1e-5))
            assert lut_margin(inp["x"], c["ags"]) > 0.499      # +-127 and 0, to float64 rounding
            inp["seed"], inp["margin"] = 0, 0.5
        else:
            first = 0 if row == 0 else resolve(c, row - 1)["seed"] + 1
            if c["regime"] == "plain":
                mk = lambda s: make_plain(c["kind"], c["K"], c["ags"], c["act"], first + s)
            elif c["regime"] == "eps":
                mk = lambda s: make_eps(c["kind"], c["K"], c["ags"], first + s, c["eps"], c["ratio"], c.get("act"))
            else:
                mk = lambda s: make_tails(c["kind"], c["part"], first + s, c.get("act", "f16"))
            inp = pick_safe(mk, margin_of(c), MAX_SEEDS, delta=4 * eps_hw(c))
            inp["seed"] += first
        _RESOLVED[key] = inp
    return _RESOLVED[key]


def rows_of(c, N):
    """N rounding-safe rows of a case, stacked: a, b, res [N][K], gam [K], x [N][K]"""
    rows = [resolve(c, n) for n in range(N)]
    out = dict(rows[0])
    for k in ("a", "b", "res", "x"):
        out[k] = None if rows[0].get(k) is None else np.stack([r[k] for r in rows])
    return out


# GELU's eps is four times silu's (its z grows like v^3), so its margin is: the GELU kinds take K = 1024 where the others take 2112 and 4160
NO_GELU = tuple(k for k in ALL_KINDS if not k.endswith("gelu"))
GELU_KINDS = ("glu:gelu", "glu_norm:gelu")
ACTS = ("f16", "f32")      # k_gemv_quad loads fp32 operands on a path of its own: every N = 1 regime runs both where fp16 stays normal


def eps_acts(eps, ratio):
    """the activation dtypes of an eps case: at mean(t^2) = 1e-8 the operands are about 1e-4 and fp16 would go denormal"""
    return ACTS if eps * ratio > 5e-8 else ("f32",)


# N = 1 (fused_xf): per K the kinds of the plain regime; the weight flavour follows K (test_gpu_xf_exact.N1_MATS)
N1_PLAIN = [case("plain", k, 64, 64, act=act) for act in ACTS for k in ALL_KINDS]                               # one workgroup, lanes clamped
N1_PLAIN += [case("plain", k, K, 64, act=act) for K in (2112, 4160) for act in ACTS for k in NO_GELU]           # fewer pairs than threads; a second round
N1_PLAIN += [case("plain", k, 1024, 64, act=act) for act in ACTS for k in GELU_KINDS]
N1_PLAIN += [case("plain", k, 3200, 3200, act=act) for act in ACTS for k in ("norm", "glu:silu", "glu_norm:relu2")]    # unified scale
N1_PLAIN += [case("plain", k, 256, 64, act=act) for act in ACTS for k in ("norm", "glu:gelu", "glu_norm:silu")]        # W4 / W1 / W3 / gs = 64
N1_EPS = [case("eps", k, 1024 if k.endswith("gelu") else 2112, 64, eps=e, ratio=r, act=act)
          for e, r in EPS_COMBOS for act in eps_acts(e, r) for k in ("norm",) + GLU_NORM_KINDS]
N1_EPS += [case("eps", k, 3200, 3200, eps=1e-6, ratio=1.0, act=act) for act in ACTS for k in ("norm", "glu_norm:relu2")]
N1_TAILS = [case("tails", k, TAILS_K, 64, part=p, act=act) for k in GLU_KINDS for act in ACTS for p in range(N_TAILS)]
# ... under every launch configuration: K = 4160, K = 6144 (three even steps for (768, 3)), K = 12288 (six tables per thread), and eps in play.
# (At K >= 6144 a plain N(0,1) NORM and a plain silu GLU -- kinds "norm" and "glu:silu" -- have no rounding-safe seed within the budget;
# "glu_norm:silu" still finds one at 6144, relu^2 products find one at 6144 and 12288, and the sparse regime covers NORM there.)
N1_CONFIG = [case("plain", k, 4160, 64, act=act) for act in ACTS for k in ("norm", "glu:silu", "glu_norm:relu2")] \
    + [case("plain", k, 6144, 64, act=act) for act in ACTS for k in ("glu:relu2", "glu_norm:silu")] \
    + [case("plain", "glu_norm:relu2", 12288, 64, act=act) for act in ACTS] \
    + [case("eps", k, 2112, 64, eps=1e-6, ratio=1.0, act=act) for act in ACTS for k in ("norm", "glu_norm:silu")]
SPARSE_KS = (4160, 12288)                    # 8 * 512 < 4160; 8 * 768 and 8 * 1024 < 12288


def sparse_cases(kind, K, ft=None, ags=64, act="f16"):
    return [case("sparse", kind, K, ags, i=i, act=act) for i in sparse_indices(K, ft)]


# N >= 2 (fused_xf_rows + the tap): K of the flavours of tests/test_gpu_xf_rows.py, up to the 65 rows its routes take.  max_n: with ONE act
# group of 4160 elements a rounding-safe "glu_norm:silu" row turns up about once in 80 seeds -- 65 rows are 5050 seeds and 4.6 s of search --
# so that kind stops at N = 33 (bitnet-k4160 planes-n65 then runs NORM and relu^2, which find their rows within 0.3 s)
ROWS_PLAIN = {128: [case("plain", k, 128, 64, act="f16") for k in ("norm",) + GLU_KINDS + ("glu_norm:silu",)],
              2112: [case("plain", k, 2112, 64, act="f16") for k in ("norm", "glu:silu", "glu:relu2", "glu_norm:silu")],
              4160: [case("plain", k, 4160, 4160, act="f16") for k in ("norm", "glu:relu2")]
              + [case("plain", "glu_norm:silu", 4160, 4160, act="f16", max_n=33)]}
ROWS_TOP_N = 65


def rows_max_n(c):
    return c.get("max_n", ROWS_TOP_N)


ROWS_EPS = [case("eps", k, 128, 64, eps=e, ratio=r) for e, r in EPS_COMBOS for k in ("norm", "glu_norm:silu")]
ROWS_TAILS = N1_TAILS
ROWS_SPARSE_K = 2112
# the chain (reader form): vectors in memory, fp16 (a chain's GLU takes fp16 operands)
CHAIN_CASES = [case("plain", k, 1024, 64, act="f16") for k in ("norm",) + GLU_KINDS] \
    + [case("eps", "norm", 1024, 64, eps=e, ratio=r) for e, r in ((1e-5, 1.0), (1e-6, 1e2), (1e-2, 1e2))] \
    + [case("tails", k, TAILS_K, 64, part=p) for k in ("glu:silu", "glu:gelu") for p in (4, 9)]
CHAIN_SPARSE_K = 4160


def searched_cases():
    """every case the GPU file resolves by seed search, once each, with the rows it needs"""
    seen, out = set(), []
    groups = [(N1_PLAIN + N1_EPS + N1_TAILS + N1_CONFIG + CHAIN_CASES, 1), (ROWS_EPS + ROWS_TAILS, 3)]
    groups += [([c], rows_max_n(c)) for v in ROWS_PLAIN.values() for c in v]
    for cases, n in groups:
        for c in cases:
            if (case_id(c), n) not in seen:
                seen.add((case_id(c), n))
                out.append((c, n))
    return out


# ---- an oracle-only matrix (the host half of xf_common.Mat) ------------------------------------------------------------------------------
class HostMat:
    """the host half of xf_common.Mat, without the registration, for CPU tests of the comparison; tests/test_gpu_xf_exact.py asserts that it
    builds Mat's weights and scales from the same arguments"""

    def __init__(self, seed, Mw, K, bits=2, gs=128, zp=True, m_groups=-1, ags=64):
        self.Mw, self.K, self.bits, self.gs, self.mg, self.zp = Mw, K, bits, gs, m_groups, zp and m_groups < 1
        self.ags = K if m_groups >= 1 else ags
        self.bm = pick_bm(Mw, bits)
        c = 1.0 / np.sqrt(2.5 * K)
        if m_groups >= 1:
            case = orc.make_case(seed, Mw, K, bits=bits, ags=K, m_groups=m_groups, zero_point=False)
            self.S = (case["sc"] * c).astype(F32)
        else:
            case = orc.make_case(seed, Mw, K, bits=bits, gs=gs, ags=self.ags, zero_point=self.zp, fp16_values=True)
            sc = (case["sc"] * c).astype(np.float16).astype(F32)
            zr = None
            if self.zp:
                lvl = (2 ** bits - 1) / 2.0 - 2 ** (bits - 1)
                zr = (case["zr"] * c + lvl * sc).astype(np.float16).astype(F32)
            self.S = orc.preprocess_scales(sc, zr, bits, self.bm)
        self.A = orc.preprocess_weights(case["w"], bits, self.bm, KF)

    def sums(self, x):
        """the oracle's integer sums on the vector x: per-group scales PS [M][K / ags], unified scales the per-plane totals [M]"""
        q, ls, lb = orc.preprocessor(np.ascontiguousarray(x[None, :], F32), self.ags)
        if self.mg >= 1:
            return orc.qgemm_scale_final(self.A, q, self.S, ls[:, 0], lb[:, 0], self.Mw, self.K, 1, self.bits, self.bm, KF, self.mg)[1][0]
        return orc.partial_sums(self.A, q[0], self.Mw, self.K, self.bits, self.bm, KF, self.ags)

    def oracle(self, x):
        X = np.ascontiguousarray(x if x.ndim == 2 else x[None, :], F32)
        N = X.shape[0]
        q, ls, lb = orc.preprocessor(X, self.ags)
        if self.mg >= 1:
            out = orc.qgemm_scale_final(self.A, q, self.S, ls[:, 0], lb[:, 0], self.Mw, self.K, N, self.bits, self.bm, KF, self.mg)[0]
        else:
            out = orc.qgemm_float(self.A, q, self.S, ls, lb, self.Mw, self.K, N, self.bits, self.bm, KF, self.gs, self.ags, self.zp)
        return out if x.ndim == 2 else out[0]
