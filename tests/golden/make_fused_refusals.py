#!/usr/bin/env python3
"""Generates tests/golden/fused_refusals.json: what the library answers at the seven doors of the fused call to a fixed grid of matrix
lists and arguments -- per case (rc, tmac_hip_last_error()), whether device memory was left as it was, the tmac_hip_debug_route_stats
delta and, for an accepted case, the plan the door's debug twin names (tmac_hip_debug_fused_plan / tmac_hip_debug_xf_rows_plan).

    TMAC_HIP_LIB=<the library to pin> python tests/golden/make_fused_refusals.py

The committed file was recorded from the library as it stood before the fused call became one value (FusedCall) with named checks;
tests/test_gpu_fused_refusals.py replays the grid against the current library (grid() / replay() below).  Regenerate only for a
deliberate change of a rule, a message or the order of a door's checks.  The file is packed: one entry per door and answer with the
names of the cases that got it (pack() / unpack()), and the hash of the grid's inputs, which says what the names stand for.

Doors: "fused" tmac_hip_qgemm_fused_dev | "xf" tmac_hip_qgemm_fused_xf_dev and "xf_rows" tmac_hip_qgemm_fused_xf_rows_dev, both with a
NORM transform that names gamma alone | "perm" the fused call on act-order handles | "record" / "defer" the fused call between
tmac_hip_chain_begin and _abort / tmac_hip_defer(1) and (0) | "tap" tmac_hip_qgemm_fused_partial_sums.

Every pointer is an offset into ONE zero-filled device arena, the output regions filled with 0xff bytes before every case: a case the
library accepts is an ordinary valid launch on zero activations.  The weights (WEIGHTS) are the smallest that reach each rule.  The grid:
every matrix set at N = 1, 2, 3 under the default knobs, tmac_hip_set_gemm_min_n(2), and tmac_hip_debug_rows_kernel 1 and 2; every single
fault (FAULTS) at N = 1 and 2; every unordered pair of faults that can coexist in one call -- the pairs pin the order of a door's checks.
"""
import ctypes as C
import hashlib
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(HERE, "fused_refusals.json")
MW, K0, KBIG = 16, 128, 12352                 # KBIG: one 64-step above PAIRS_ROW_MAX_K = 12288
PERM_MW, PERM_K, PERM_GS = 128, 256, 128      # act-order handles: two groups of 128 columns, shuffled
# name: xf_common.Mat arguments (Mw = 16 throughout) | ("perm", seed of the matrix, seed of the permutation)
WEIGHTS = {
    "base": dict(seed=1, dev="f32"), "base2": dict(seed=2, dev="f32"), "w4": dict(seed=3, dev="f32", bits=4), "k256": dict(seed=4, dev="f32", K=256),
    "nozp": dict(seed=5, dev="f32", zp=False), "f16": dict(seed=6, dev="f16"), "uni": dict(seed=7, m_groups=1), "unibig": dict(seed=8, K=KBIG, m_groups=1),
    "lo": dict(seed=9, dev="f32", ags=32), "fa": dict(seed=10, dev="f32", fa=1),
    "permA": ("perm", 11, 21), "permA2": ("perm", 12, 21), "permB": ("perm", 13, 22), "k256f16": dict(seed=14, dev="f16", K=256),
}
B_REGION, G_REGION, C_REGION = 160 * 1024, 64 * 1024, 4096
OFF = {"B": 0, "gamma": B_REGION, "C": B_REGION + G_REGION}
ARENA = OFF["C"] + 5 * C_REGION
DOORS = ("fused", "xf", "xf_rows", "perm", "record", "defer", "tap")
SETS = (["base"], ["base", "base2"], ["w4"], ["k256"], ["nozp"], ["f16"], ["uni"], ["unibig"], ["lo"], ["fa"])
PERM_SETS = (["permA"], ["permA", "permA2"])
KNOBS = (dict(), dict(min_n=2), dict(rows=1), dict(rows=2))


def call(door, name, w, N, **over):
    """one case: w matrix names per slot (None: a NULL slot), nmat (None: len(w)), B / C shifts in bytes (None: NULL), wl / Cl False: a NULL
    list, out the output dtype, the knobs variant, min_n (0: not set) and rows"""
    c = dict(door=door, name=name, w=list(w), nmat=None, N=N, B=0, C=[0] * len(w), wl=True, Cl=True, out="f32", variant=0, min_n=0, rows=0)
    c.update(over)
    return c


def _second(c):
    if len(c["w"]) < 2:
        c["w"].append(c["w"][0]); c["C"].append(0)


def _pair(other):
    def f(c):
        _second(c); c["w"][1] = other
    return f


def _every(name):
    """every (non-null) slot holds this matrix"""
    def f(c):
        c["w"] = [n and name for n in c["w"]]
    return f


def _slot1_matrix_null(c):
    _second(c); c["w"][1] = None


def _slot1_output_null(c):
    _second(c); c["C"][1] = None


def _set(**kv):
    return lambda c: c.update(kv)


def _c0(shift, out):
    def f(c):
        c["C"][0] = shift; c["out"] = out
    return f


# name: (the keys it claims -- two faults that claim a key cannot coexist --, the doors it can be asked at (None: all), what it does)
LISTS = ("fused", "xf", "xf_rows", "perm", "record", "defer")
PLAIN = ("fused", "xf", "xf_rows", "record", "defer", "tap")
FAULTS = {
    "nmat-0": ({"nmat"}, LISTS, _set(nmat=0)), "nmat-5": ({"nmat"}, LISTS, _set(nmat=5)), "N-0": ({"N"}, ("fused", "xf_rows", "perm", "record", "defer"), _set(N=0)),
    "wl-null": ({"wl"}, None, _set(wl=False)), "C-list-null": ({"Cl"}, LISTS, _set(Cl=False)), "B-null": ({"B"}, None, _set(B=None)),
    "matrix-1-null": ({"w"}, LISTS, _slot1_matrix_null), "output-1-null": ({"C1"}, LISTS, _slot1_output_null),
    "B-off-8": ({"B"}, None, _set(B=8)), "C-off-4-f32": ({"C0", "out"}, LISTS, _c0(4, "f32")), "C-off-4-f16": ({"C0", "out"}, LISTS, _c0(4, "f16")),
    "pair-w4": ({"w"}, PLAIN[:-1], _pair("w4")), "pair-k256": ({"w"}, PLAIN[:-1], _pair("k256")), "pair-nozp": ({"w"}, PLAIN[:-1], _pair("nozp")),
    "pair-f16": ({"w"}, PLAIN[:-1], _pair("f16")), "pair-lo": ({"w"}, PLAIN[:-1], _pair("lo")),
    "pair-perm-plain": ({"w"}, ("perm",), _pair("k256f16")), "pair-permA-permB": ({"w"}, ("perm",), _pair("permB")),
    "permuted-handle": ({"w"}, PLAIN, _every("permA")),
    "variant-3": ({"variant"}, None, _set(variant=3)), "variant-7": ({"variant"}, None, _set(variant=7)),
    "fast-aggregation": ({"w"}, None, _every("fa")),
}


def grid():
    cases = []
    for door in DOORS:
        rows = door != "xf"                                        # (tmac_hip_qgemm_fused_xf_dev takes one row)
        home = ["permA"] if door == "perm" else ["base"]
        for w in (PERM_SETS if door == "perm" else SETS):
            if door == "tap" and len(w) > 1:
                continue
            for N in ((1, 2, 3) if rows else (1,)):
                for kn in KNOBS:
                    tag = "-".join(f"{k}{v}" for k, v in kn.items()) or "default"
                    cases.append(call(door, f"{'+'.join(w)}-N{N}-{tag}", w, N, **kn))
        asked = [n for n, (_, doors, _) in FAULTS.items() if doors is None or door in doors]
        for n in asked:
            for N in ((1, 2) if rows else (1,)):
                c = call(door, f"{n}-N{N}", home, N)
                FAULTS[n][2](c)
                cases.append(c)
        for a, b in itertools.combinations(asked, 2):
            if FAULTS[a][0] & FAULTS[b][0]:
                continue
            c = call(door, f"{a}+{b}", home, 2 if door == "xf_rows" else 1)
            FAULTS[a][2](c); FAULTS[b][2](c)
            cases.append(c)
    return cases


class Bench:
    """the arena, the registered matrices and the doors"""

    def __init__(self):
        import torch
        import tmac_amd
        import pack_common as pc
        import xf_common as xc
        assert torch.cuda.is_available(), "the refusal grid runs on a GPU"
        self.torch, self.tm, self.L = torch, tmac_amd, tmac_amd.lib()
        tm = tmac_amd
        dt = {"f32": tm.F32, "f16": tm.F16}
        self.keep, self.h, perms = [], {}, {}
        for name, a in WEIGHTS.items():
            if isinstance(a, tuple):
                _, seed, pseed = a
                if pseed not in perms:
                    g = np.arange(PERM_K, dtype=np.int32) // PERM_GS
                    np.random.default_rng(pseed).shuffle(g)
                    perms[pseed] = tm.KPerm(g, PERM_GS)
                    assert not perms[pseed].identity
                wr = tm.TMACGeMMWrapper(act_group_size=64)
                w = wr.register_gptq(*pc.make_gptq(seed, PERM_MW, PERM_K, 2, PERM_GS, np.float16, hard=False),
                                     tm.KCfg.make(PERM_MW, PERM_K, 2, 128, 16, PERM_GS, 64, True), True, tm.F16, g_idx=perms[pseed])
                self.keep.append((wr, w))
            else:
                a = dict(a)
                seed, dev, Kw = a.pop("seed"), a.pop("dev", None), a.pop("K", K0)
                wr = tm.TMACGeMMWrapper(act_group_size=Kw if a.get("m_groups", -1) >= 1 else a.get("ags", 64))
                m = xc.Mat(tm, wr, seed, MW, Kw, dev_dtype=dt[dev] if dev else None, **a)
                self.keep.append((wr, m))
                w = m.w
            self.h[name] = w.handle.value
        self.keep.append(perms)
        image = np.zeros(ARENA, np.uint8)
        image[OFF["C"]:] = 0xff
        self.image = torch.from_numpy(image).cuda()
        self.arena = torch.zeros(ARENA, dtype=torch.uint8, device="cuda")
        self.base = self.arena.data_ptr()
        assert self.base % 256 == 0
        self.ps = np.zeros(1 << 20, np.int32)                      # host side of the tap: N x M x act groups integers at the most
        self.xf = tm.binding.XForm()
        self.xf.kind, self.xf.eps, self.xf.gamma = 1, 1e-5, self.base + OFF["gamma"]

    def stats(self):
        counts = (C.c_uint64 * 8)()
        self.tm.binding.check(self.L.tmac_hip_debug_route_stats(counts))
        return list(counts)

    def run(self, c):
        """(rc, message, arena left as it was, status of the door's closing call, route_stats delta, plan of an accepted case) of one case"""
        tm, L, torch, ck = self.tm, self.L, self.torch, self.tm.binding.check
        self.arena.copy_(self.image)
        ck(L.tmac_hip_set_variant(c["variant"]))
        ck(L.tmac_hip_set_gemm_min_n(c["min_n"] or 32))
        ck(L.tmac_hip_debug_rows_kernel(c["rows"]))
        door, N, w = c["door"], c["N"], c["w"]
        nmat = len(w) if c["nmat"] is None else c["nmat"]
        hs = [None if n is None else self.h[n] for n in w]
        cs = [None if s is None else self.base + OFF["C"] + i * C_REGION + s for i, s in enumerate(c["C"])]
        while len(hs) < 5:                                         # (a list is never shorter than the count the call names)
            hs.append(hs[0]); cs.append(self.base + OFF["C"] + len(cs) * C_REGION)
        wa, ca = (C.c_void_p * 5)(*hs), (C.c_void_p * 5)(*cs)
        wl, cl = (wa if c["wl"] else None), (ca if c["Cl"] else None)
        B = None if c["B"] is None else self.base + OFF["B"] + c["B"]
        out = tm.F16 if c["out"] == "f16" else tm.F32
        before = self.stats()
        after_rc = 0
        if door == "record":
            ck(L.tmac_hip_chain_begin())
        if door == "defer":
            ck(L.tmac_hip_defer(1))
        if door == "xf":
            rc = L.tmac_hip_qgemm_fused_xf_dev(wl, nmat, B, tm.F32, C.byref(self.xf), cl, out, None)
        elif door == "xf_rows":
            rc = L.tmac_hip_qgemm_fused_xf_rows_dev(wl, nmat, B, tm.F32, C.byref(self.xf), cl, out, N, None)
        elif door == "tap":
            rc = L.tmac_hip_qgemm_fused_partial_sums(hs[0] if c["wl"] else None, B, tm.F32, self.ps.ctypes.data, None, None, N, None)
        else:
            rc = L.tmac_hip_qgemm_fused_dev(wl, nmat, B, tm.F32, cl, out, N, None)
        msg = L.tmac_hip_last_error().decode() if rc else ""
        if door == "record":
            ck(L.tmac_hip_chain_abort())
        if door == "defer":
            after_rc = L.tmac_hip_defer(0)                         # (flushes what was queued)
        torch.cuda.synchronize()
        delta = {str(r): b - a for r, (a, b) in enumerate(zip(before, self.stats())) if b != a}
        plan = None
        if rc == 0:
            several = door in ("xf_rows", "perm") and N >= 2      # (a transformed or permuted call of several rows: xf_rows_plan's rules)
            route, lut = C.c_int32(-1), C.c_int32(-1)
            prc = (L.tmac_hip_debug_xf_rows_plan if several else L.tmac_hip_debug_fused_plan)(wa, nmat, ca, N, C.byref(route), C.byref(lut))
            plan = [prc, route.value, lut.value]
        ck(L.tmac_hip_set_variant(0)); ck(L.tmac_hip_set_gemm_min_n(32)); ck(L.tmac_hip_debug_rows_kernel(0))
        return rc, msg, bool(torch.equal(self.arena, self.image)), after_rc, delta, plan


RECORDED = ("rc", "msg", "untouched", "after", "routes", "plan")


def replay(cases):
    bench = Bench()
    return [bench.run(c) for c in cases]


def grid_digest(cases):
    """the inputs of the grid as one hash: the recording names its cases, this pins what the names stand for"""
    return hashlib.sha256(json.dumps(cases, sort_keys=True).encode()).hexdigest()


def pack(cases):
    """the recording, one entry per (door, answer): the names of the cases that got it"""
    classes = {}
    for c in cases:
        classes.setdefault(json.dumps([c["door"]] + [c[k] for k in RECORDED], sort_keys=True), []).append(c["name"])
    return [dict(zip(("door",) + RECORDED, json.loads(k)), cases=names) for k, names in classes.items()]


def unpack(classes):
    """{(door, name): the RECORDED values} of a packed recording"""
    return {(e["door"], n): tuple(e[k] for k in RECORDED) for e in classes for n in e["cases"]}


def main():
    cases = grid()
    digest = grid_digest(cases)
    for c, res in zip(cases, replay(cases)):
        c.update(zip(RECORDED, res))
    with open(OUT, "w") as f:
        f.write('{"weights": %s, "off": %s, "grid_sha256": "%s",\n "classes": [\n' % (json.dumps(WEIGHTS), json.dumps(OFF), digest))
        f.write(",\n".join("  " + json.dumps(e) for e in pack(cases)))
        f.write("\n]}\n")
    refused = [c for c in cases if c["rc"]]
    print(f"{OUT}: {len(cases)} cases, {len(refused)} refused, {len(cases) - len(refused)} accepted, "
          f"{sum(1 for c in refused if not c['untouched'])} refused but touched, {sum(1 for c in cases if c['after'])} failed closing calls")
    for d in DOORS:
        dc = [c for c in cases if c["door"] == d]
        print(f"  {d}: {len(dc)} cases, {sum(1 for c in dc if c['rc'])} refused")


if __name__ == "__main__":
    main()
