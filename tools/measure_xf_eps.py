"""The relative error of the transformed vector x on the N >= 2 tap (tmac_hip_debug_xf_rows) against float64, element by element: the eps
behind tests/xf_probe.py::EPS_HW, on the inputs the tests are built from -- the committed tail grid (every band, fp16 and fp32 operands,
three seeds of in2) and N(0,1) operands (33 rows, any seed, not only rounding-safe ones), then NORM / GLU_NORM with eps in play.
usage: measure_xf_eps.py [output file]      (profiles/r17_xf_exact.txt is this output under a header)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import tmac_amd as tm
import xf_probe as P
from xf_common import dev, poison

out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
wr = tm.TMACGeMMWrapper(act_group_size=64)


def say(*a):
    s = " ".join(str(x) for x in a)
    print(s, flush=True)
    if out:
        out.write(s + "\n"); out.flush()


def tap(kind, a, b=None, res=None, gam=None, eps=1e-5):
    N, K = a.shape
    x = poison((N, K), torch.float32)
    kw = {}
    if b is not None:
        kw["in2"] = dev(b)
    if res is not None:
        kw["residual"] = dev(res)
    if gam is not None:
        kw.update(gamma=dev(gam), eps=eps)
    wr.xf_rows_tap(dev(a), x, kind, K, N, **kw)
    torch.cuda.synchronize()
    return x.cpu().numpy()


def relerr(x, ref):
    r64 = ref.astype(np.float64)
    d = np.abs(x.astype(np.float64) - r64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(r64 != 0, d / np.abs(r64), np.where(d == 0, 0.0, np.inf))


worst = {}
for gate in P.GATES:
    bands = P.tail_bands(gate)
    for act in P.ACTS:
        for part in range(P.N_TAILS):
            for seed in range(3):
                inp = P.make_tails(f"glu:{gate}", part, seed, act)
                x = tap(f"glu:{gate}", np.stack([inp["a"]] * 2), np.stack([inp["b"]] * 2))
                assert np.array_equal(x[0], x[1])
                r = relerr(x[0], inp["x"])
                for g in range(2):
                    key = (gate, "tails", bands[2 * part + g])
                    worst[key] = max(worst.get(key, 0.0), float(r[64 * g: 64 * g + 64].max()))
    for c in bands:
        say(f"{gate} tails band {c:+.6g} ({len(np.unique(P.tail_band(c, gate)))} points): max rel err {worst[(gate, 'tails', c)]:.3e}")
    say(f"{gate} tails: max over bands {max(v for k, v in worst.items() if k[:2] == (gate, 'tails')):.3e}")
    for act in P.ACTS:
        for K in (128, 2112, 4160):
            rows = [P.make_plain(f"glu:{gate}", K, 64, act, s) for s in range(33)]
            a, b, xr = (np.stack([r_[k] for r_ in rows]) for k in ("a", "b", "x"))
            r = relerr(tap(f"glu:{gate}", a, b), xr)
            i = np.unravel_index(np.argmax(r), r.shape)
            say(f"{gate} plain {act} K={K}: max rel err {r.max():.3e} at in={float(a[i]):.5g} in2={float(b[i]):.5g}; 99.9th pct {np.quantile(r, 0.999):.3e}")
            worst[(gate, "plain", act, K)] = float(r.max())
            gam = P._gamma(K)
            rr = relerr(tap(f"glu_norm:{gate}", a, b, gam=gam), P.ref_x("glu_norm", gate, a, b, None, gam, 1e-5))
            say(f"{gate} glu_norm plain {act} K={K}: max rel err {rr.max():.3e}  (r's bound {P.norm_bound(K):.3e} on top of the gate's)")
for gate in ("silu", "gelu"):
    say(f"{gate}: plain {max(v for k, v in worst.items() if k[:2] == (gate, 'plain')):.3e} (asserted {P.EPS_HW['plain'][gate]:g}), "
        f"tails {max(v for k, v in worst.items() if k[:2] == (gate, 'tails')):.3e} (asserted {P.EPS_HW['tails'][gate]:g})")
say(f"relu2 (specified to the bit): {max(v for k, v in worst.items() if k[0] == 'relu2'):.1e}")
for e, ratio in P.EPS_COMBOS:
    for kind in ("norm",) + P.GLU_NORM_KINDS:
        for act in P.eps_acts(e, ratio):
            inp = P.make_eps(kind, 2112, 64, 0, e, ratio, act)
            two = lambda k: None if inp.get(k) is None else np.stack([inp[k]] * 2)
            x = tap(kind, two("a"), two("b"), two("res"), inp["gam"], e)
            say(f"eps regime {kind} eps={e:g} ratio={ratio:g} {act}: max rel err {relerr(x[0], inp['x']).max():.3e} (r's bound {P.norm_bound(2112):.3e})")
