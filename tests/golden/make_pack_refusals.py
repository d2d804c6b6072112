#!/usr/bin/env python3
"""Generates tests/golden/pack_refusals.json: what the library answers at the fourteen doors in front of the pack kernels -- the six
tmac_hip_pack_*_dev, the six tmac_hip_register_weights_*_dev and the two tmac_hip_pack_*_perm_dev (with a NULL permutation: the rules of
the plain twin) -- to a fixed grid of faulty calls: per case (rc, tmac_hip_last_error()).

    TMAC_HIP_LIB=<the library to pin> python tests/golden/make_pack_refusals.py

The committed file was recorded from the library as it stood before the six formats shared one pack_to and one register_from
(tmac_pack_host.cpp); tests/test_pack_refusals_cpu.py replays the grid against the current library (grid() / replay() below).  Regenerate
only for a deliberate change of a rule, a message or the order of a door's checks.  The file is packed like fused_refusals.json: one entry
per door and answer with the names of the cases that got it (pack() / unpack()), and the hash of the grid's inputs.

No GPU is needed and none is touched: every case holds at least one fault, every fault is refused in front of the first call that touches
a device, so the pointers are small integers that nothing dereferences (PTR: aligned; + 8: misaligned).  replay() calls no case whose
recorded answer is not such a refusal.  The grid: every single fault a door names (FAULTS) and every unordered pair of faults that can
coexist in one call -- the pairs pin the order of a door's checks.  The register doors' dev_float rule is in the grid where the recorded
library had it (AWQ, ternary, RTN); tests/test_pack_refusals_cpu.py holds all register doors to it.
"""
import ctypes as C
import hashlib
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(HERE, "pack_refusals.json")
E_NOMATCH, E_ARG = -1, -4
MW, K0 = 128, 256
PTR = {n: 0x10000 + 0x1000 * i for i, n in enumerate(("qweight", "codes", "packed", "W", "scales", "zeros", "scales_in", "A", "S", "invalid"))}
CFG_FIELDS = ("bm", "simd_n_in", "simd_n_out", "kfactor", "group_size", "lut_scales_size", "scales_size", "n_tile_num", "act_group_size", "zero_point",
              "m_groups")

# format: (the C names of its pointers in the library's messages, by their key in PTR; bits; unified scales?)
FORMATS = {
    "gptq": (dict(qweight="qweight", scales="scales", zeros="qzeros"), 2, False),
    "codes": (dict(codes="codes", scales="scales", zeros="zeros"), 2, False),
    "awq": (dict(qweight="qweight", scales="scales", zeros="qzeros"), 4, False),
    "absmean": (dict(W="W_dev", scales_in="scales_in_dev"), 2, True),
    "ternary": (dict(packed="packed_dev", scales="scales_dev"), 2, True),
    "rtn": (dict(W="W_dev"), 2, False),
}
# door: (format, registers?, takes a permutation?)
DOORS = {f"pack_{f}": (f, False, False) for f in FORMATS}
DOORS.update({f"register_{f}": (f, True, False) for f in FORMATS})
DOORS.update({f"pack_{f}_perm": (f, False, True) for f in ("gptq", "codes")})
# the register doors through a permutation are no part of the grid (a permutation is a device object: tests/test_gpu_actorder.py);
# tests/test_pack_refusals_cpu.py calls them with a NULL one
BESIDE = {f"register_{f}_perm": (f, True, True) for f in ("gptq", "codes")}
OPTIONAL = ("zeros", "scales_in", "invalid")


def base(door):
    """the valid call every case of a door starts from (it would pack a 128 x 256 matrix)"""
    fmt, reg, _ = {**DOORS, **BESIDE}[door]
    ptrs, bits, unified = FORMATS[fmt]
    p = {k: PTR[k] for k in ptrs}
    if reg:
        out = True
    else:
        p.update(A=PTR["A"], S=PTR["S"])
        out = None
        if fmt in ("ternary", "rtn"):
            p["invalid"] = None
    cfg = dict(zip(CFG_FIELDS, (128, 16, 8, 16, 128, K0 // 64, 1 if unified else MW * (K0 // 128) * 2, MW * bits // 128, K0 if unified else 64,
                                0 if unified else 1, 1 if unified else -1)))
    return dict(door=door, p=p, out=out, cfg=cfg, Mw=MW, K=K0, bits=bits, sdt=1, src=1, ref=0, dev=1, eps="1e-5", v2=1)


def _p(key, value):
    def f(c):
        c["p"][key] = value
    return f


def _cfg(**kv):
    return lambda c: c["cfg"].update(kv)


def _set(**kv):
    return lambda c: c.update(kv)


def faults(door):
    """{name: (the keys it claims -- two faults that claim a key cannot coexist --, what it does to the call)} of a door"""
    fmt, reg, _ = {**DOORS, **BESIDE}[door]
    unified = FORMATS[fmt][2]
    b = base(door)
    F = {"cfg-null": ({"cfg"}, _set(cfg=None))}
    if reg:
        F["out-null"] = ({"out"}, _set(out=False))
    for k in b["p"]:
        if k == "zeros":        # (NULL against zero_point: below)
            pass
        elif k not in OPTIONAL:
            F[f"null-{k}"] = ({k}, _p(k, None))
        F[f"mis-{k}"] = ({k}, _p(k, PTR[k] + 8))
    if "zeros" in b["p"]:
        F["zeros-absent"] = ({"zeros", "cfg.zero_point"}, _p("zeros", None))
        F["zeros-given-no-zp"] = ({"zeros", "cfg.zero_point"}, _cfg(zero_point=0))
    if fmt in ("gptq", "codes", "awq"):
        F["bad-scales-dtype"] = ({"sdt"}, _set(sdt=7))
    if fmt in ("absmean", "rtn"):
        F["bad-src-dtype"] = ({"src"}, _set(src=7))
    F["bad-ref-dtype"] = ({"ref"}, _set(ref=7))
    if fmt != "codes":          # (the codes form takes both kinds of scales)
        F["m_groups-wrong-side"] = ({"cfg.m_groups"}, _cfg(m_groups=-1 if unified else 1))
    if unified:
        F["Mw-mod-m_groups"] = ({"cfg.m_groups"}, _cfg(m_groups=3))
    if fmt == "gptq":
        F["bits-3"] = ({"bits"}, _set(bits=3))
    if fmt == "awq":
        F["awq-tiles"] = ({"cfg.n_tile_num"}, _cfg(n_tile_num=3))
    if fmt == "absmean":
        F["eps-0"] = ({"eps"}, _set(eps="0"))
        F["eps-nan"] = ({"eps"}, _set(eps="nan"))
    F["bm-bad"] = ({"cfg.bm", "cfg.n_tile_num"}, _cfg(bm=96, n_tile_num=0))        # (n_tile_num 0: nothing for the AWQ rule to contradict)
    if door in ("register_awq", "register_ternary", "register_rtn"):
        F["dev-float-7"] = ({"dev"}, _set(dev=7))
    return F


def _coexist(a, b):
    (ka, _), (kb, _) = a, b
    if ka & kb:
        return False
    return not (("cfg" in ka and any(k.startswith("cfg.") for k in kb)) or ("cfg" in kb and any(k.startswith("cfg.") for k in ka)))


def grid():
    cases = []
    for door in DOORS:
        F = faults(door)
        for n, (_, do) in F.items():
            c = base(door)
            do(c)
            cases.append(dict(c, name=n))
        for a, b in itertools.combinations(F, 2):
            if not _coexist(F[a], F[b]):
                continue
            c = base(door)
            F[a][1](c); F[b][1](c)
            cases.append(dict(c, name=f"{a}+{b}"))
    return cases


def run(L, KCfg, c):
    """(rc, message) of one case"""
    fmt, reg, perm = {**DOORS, **BESIDE}[c["door"]]
    p = c["p"]
    cfg = C.byref(KCfg(*(c["cfg"][k] for k in CFG_FIELDS))) if c["cfg"] is not None else None
    h = C.c_void_p()
    head = [C.byref(h) if c["out"] else None] if reg else []
    dims = [c["Mw"], c["K"]] + ([c["bits"]] if fmt in ("gptq", "codes", "rtn") else [])
    tail = [c["ref"], c["dev"], None] if reg else [p["A"], p["S"], c["ref"]] + ([p["invalid"]] if "invalid" in p else []) + [None]
    pm = [None] if perm else []
    if fmt == "gptq":
        args = [p["qweight"], p["scales"], p["zeros"], c["sdt"], c["v2"]] + pm + dims
    elif fmt == "codes":
        args = [p["codes"], p["scales"], p["zeros"], c["sdt"]] + pm + dims
    elif fmt == "awq":
        args = [p["qweight"], p["scales"], p["zeros"], c["sdt"]] + dims
    elif fmt == "absmean":
        args = [p["W"], c["src"], p["scales_in"], float(c["eps"])] + dims
    elif fmt == "ternary":
        args = [p["packed"], p["scales"]] + dims
    else:
        args = [p["W"], c["src"]] + dims
    name = "tmac_hip_" + ("register_weights_" + fmt if reg else "pack_" + fmt) + ("_perm" if perm else "") + "_dev"
    rc = getattr(L, name)(*(head + args + [cfg] + tail))
    return rc, (L.tmac_hip_last_error().decode() if rc else "")


def replay(cases, recorded=None):
    """[(rc, message)] of the cases.  recorded: {(door, name): (rc, message)} -- a case it does not show refused for its arguments is not
    called (its pointers are no memory)"""
    import tmac_amd
    L = tmac_amd.lib()
    for c in cases:
        assert recorded is None or recorded[c["door"], c["name"]][0] in (E_ARG, E_NOMATCH), (c["door"], c["name"])
    return [run(L, tmac_amd.KCfg, c) for c in cases]


RECORDED = ("rc", "msg")


def grid_digest(cases):
    """the inputs of the grid as one hash: the recording names its cases, this pins what the names stand for"""
    return hashlib.sha256(json.dumps(cases, sort_keys=True).encode()).hexdigest()


def pack(cases):
    """the recording, one entry per (door, answer): the names of the cases that got it"""
    classes = {}
    for c in cases:
        classes.setdefault(json.dumps([c["door"]] + [c[k] for k in RECORDED]), []).append(c["name"])
    return [dict(zip(("door",) + RECORDED, json.loads(k)), cases=names) for k, names in classes.items()]


def unpack(classes):
    """{(door, name): the RECORDED values} of a packed recording"""
    return {(e["door"], n): tuple(e[k] for k in RECORDED) for e in classes for n in e["cases"]}


def main():
    cases = grid()
    digest = grid_digest(cases)
    for c, res in zip(cases, replay(cases)):
        c.update(zip(RECORDED, res))
    stray = [(c["door"], c["name"], c["rc"], c["msg"]) for c in cases if c["rc"] not in (E_ARG, E_NOMATCH)]
    assert not stray, ("cases that were not refused for their arguments", stray[:5])
    with open(OUT, "w") as f:
        f.write('{"grid_sha256": "%s",\n "classes": [\n' % digest)
        f.write(",\n".join("  " + json.dumps(e) for e in pack(cases)))
        f.write("\n]}\n")
    print(f"{OUT}: {len(cases)} cases, all refused")
    for d in DOORS:
        print(f"  {d}: {sum(1 for c in cases if c['door'] == d)} cases, {len({(c['rc'], c['msg']) for c in cases if c['door'] == d})} answers")


if __name__ == "__main__":
    main()
