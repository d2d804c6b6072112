#!/usr/bin/env python3
"""Generates tests/golden/xf_refusals.json: what the library answers to a fixed grid of tmac_hip_xform values at its four transform
sites -- (rc, tmac_hip_last_error()) per case, and whether device memory was left as it was.

    TMAC_HIP_LIB=<the library to pin> python tests/golden/make_xf_refusals.py

The committed file was recorded from the library as it stood before the field rules moved into tmac_amd/csrc/tmac_xform.cpp;
tests/test_gpu_xf_refusals.py replays the grid against the current library (grid() / replay() below) and tests/test_xf_resolve_cpu.py
replays the part the resolver alone decides without a GPU.  Regenerate only for a deliberate change of a rule or a message.

Every pointer of the grid is an offset into ONE zero-filled device arena (REGION bytes per operand: room for a vector moved by 8 bytes
or laid over the last 16 bytes of another), the weights one W2 matrix of K = 128, Mw = 16, gs = 128: a case the library accepts is an
ordinary valid launch.  The outputs, residual_out's own region and the tap's x_out are filled with 0xff bytes before every case.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(HERE, "xf_refusals.json")
K, MW, BITS, GS, AGS, BM, KF = 128, 16, 2, 128, 64, 32, 16
REGION = 2048
OFF = {n: i * REGION for i, n in enumerate(("B", "in2", "residual", "gamma", "residual_out", "C", "x_out"))}
ARENA = 8 * REGION
POISONED = ("residual_out", "C", "x_out")
# site: (entry point, activation rows)
SITES = {"xf": ("tmac_hip_qgemm_fused_xf_dev", 1), "rows": ("tmac_hip_qgemm_fused_xf_rows_dev", 2), "tap": ("tmac_hip_debug_xf_rows", 2),
         "chain": ("tmac_hip_chain_xform", 1)}
FIELDS = ("in2", "residual", "gamma", "residual_out")
NATURAL = {1: ("residual", "gamma", "residual_out"), 2: ("in2",), 4: ("in2", "gamma")}      # the operands a valid call of the kind names
CARRY = "carry"


def vec_bytes(name, N):
    """bytes of an operand of an N-row call (fp32 activations and outputs)"""
    return {"B": N * K * 4, "in2": N * K * 4, "residual": N * K * 4, "gamma": K * 4, "residual_out": N * K * 4, "C": N * MW * 4}[name]


def grid():
    """the cases: dicts of site, name, kind, keep and the four fields as arena offsets (None: NULL, "carry": TMAC_XF_CARRY)"""
    cases = []
    for site, (_, N) in SITES.items():
        def add(name, kind, keep=0, **over):
            f = {n: (OFF[n] if n in NATURAL.get(kind & 0xff, ()) else None) for n in FIELDS}
            f.update(over)
            cases.append(dict(site=site, name=name, kind=kind, keep=keep, **f))
        for kind in range(6):
            for gate in (0x000, 0x100, 0x200, 0x300):
                add(f"kind-{kind}-gate-{gate:#05x}", kind | gate)
        for kind in (2, 4):
            add(f"kind-{kind}-gate-above-15", kind | 0x10000)
        for kind in (1, 2, 4):
            for n in FIELDS:
                for state, val in (("absent", None), ("present", OFF[n]), ("off8", OFF[n] + 8)):
                    add(f"kind-{kind}-{n}-{state}", kind, **{n: val})
            add(f"kind-{kind}-carry", kind, residual=CARRY)
            add(f"kind-{kind}-keep", kind, keep=1)
        for target in ("B", "residual", "gamma", "in2", "C"):
            for how, off in (("whole", OFF[target]), ("last16", OFF[target] + vec_bytes(target, N) - 16)):
                add(f"rout-over-{target}-{how}", 1, in2=OFF["in2"], residual_out=off)
    return cases


class Bench:
    """the arena, the registered matrix and the four entry points"""

    def __init__(self):
        import torch
        import tmac_amd
        from oracle import oracle as orc
        assert torch.cuda.is_available(), "the refusal grid runs on a GPU"
        self.torch, self.tm, self.L = torch, tmac_amd, tmac_amd.lib()
        case = orc.make_case(0, MW, K, bits=BITS, gs=GS, ags=AGS, zero_point=True)
        A = orc.preprocess_weights(case["w"], BITS, BM, KF)
        S = orc.preprocess_scales(case["sc"], case["zr"], BITS, BM)
        self.wr = tmac_amd.TMACGeMMWrapper(act_group_size=AGS)
        self.w = self.wr.register_weights(A, S, MW, K, BITS, tmac_amd.KCfg.make(MW, K, BITS, BM, KF, GS, AGS, True))
        image = np.zeros(ARENA, np.uint8)
        for n in POISONED:
            image[OFF[n]:OFF[n] + REGION] = 0xff
        self.image = torch.from_numpy(image).cuda()
        self.arena = torch.zeros(ARENA, dtype=torch.uint8, device="cuda")
        self.base = self.arena.data_ptr()
        assert self.base % 256 == 0

    def ptr(self, off):
        return None if off is None else 1 if off == CARRY else self.base + off

    def run(self, case):
        """(rc, message, arena left as it was) of one case"""
        tm, L, torch = self.tm, self.L, self.torch
        self.arena.copy_(self.image)
        xf = tm.binding.XForm()
        xf.kind, xf.eps, xf.keep = case["kind"], 1e-5, case["keep"]
        xf.in2, xf.residual, xf.gamma, xf.residual_out = (self.ptr(case[n]) for n in FIELDS)
        site = case["site"]
        N = SITES[site][1]
        wa, ca = (C.c_void_p * 1)(self.w.handle.value), (C.c_void_p * 1)(self.base + OFF["C"])
        B = self.base + OFF["B"]
        if site == "xf":
            rc = L.tmac_hip_qgemm_fused_xf_dev(wa, 1, B, tm.F32, C.byref(xf), ca, tm.F32, None)
        elif site == "rows":
            rc = L.tmac_hip_qgemm_fused_xf_rows_dev(wa, 1, B, tm.F32, C.byref(xf), ca, tm.F32, N, None)
        elif site == "tap":
            rc = L.tmac_hip_debug_xf_rows(B, tm.F32, C.byref(xf), K, N, self.base + OFF["x_out"], None)
        else:
            tm.binding.check(L.tmac_hip_chain_begin())
            rc = L.tmac_hip_chain_xform(C.byref(xf))
        msg = L.tmac_hip_last_error().decode() if rc else ""
        if site == "chain":
            tm.binding.check(L.tmac_hip_chain_abort())
        torch.cuda.synchronize()
        return rc, msg, bool(torch.equal(self.arena, self.image))


def replay(cases):
    bench = Bench()
    return [bench.run(c) for c in cases]


def main():
    cases = grid()
    for c, (rc, msg, untouched) in zip(cases, replay(cases)):
        c.update(rc=rc, msg=msg, untouched=untouched)
    with open(OUT, "w") as f:
        f.write('{"K": %d, "Mw": %d, "region": %d, "off": %s,\n "cases": [\n' % (K, MW, REGION, json.dumps(OFF)))
        f.write(",\n".join("  " + json.dumps(c) for c in cases))
        f.write("\n]}\n")
    refused = sum(1 for c in cases if c["rc"])
    print(f"{OUT}: {len(cases)} cases, {refused} refused, {sum(1 for c in cases if c['rc'] and not c['untouched'])} refused but touched")


if __name__ == "__main__":
    main()
