#!/usr/bin/env python3
"""Generates tests/golden/*.npz and lut_ctor_kat.json FROM THE REFERENCE ITSELF.

Run where the reference's sources lie (oracle.REF_ROOT) after `make -C oracle ref`:

    python tests/golden/make_golden.py             # everything
    python tests/golden/make_golden.py vs_ref      # ref/oracle_vs_ref.npz alone (tests/test_oracle_vs_ref.py)
    python tests/golden/make_golden.py saturating  # ref/saturating.npz alone (the saturating inputs of tests/test_oracle_vs_ref.py)
    python tests/golden/make_golden.py convert     # ref/convert_ref.json and ref/kcfg/ alone (tests/test_convert.py)

Sources of truth used here (never our own restatement):
  * weight/scale permutation : python/t_mac/weights.py:preprocess_weights, imported from /root/reference
  * QLUT / lut_scales / lut_biases, CBits, integer partial sums :
        python/t_mac/intrins/{lut_ctor,tbl}.cc compiled by oracle/Makefile into oracle/_ref/
  * one case through a checked-in prebuilt kernel set (deploy/tuned/aarch64-llama-2-7b-2bit/kernels.cc)
  * the known-answer vector printed by the reference's own tests/test_lut_ctor.cc
The vectors are committed; the GPU box has no /root/reference.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import oracle as orc  # noqa: E402  (only its _ref loaders + case generator are used)

REF = orc.REF_ROOT
sys.path.insert(0, os.path.join(REF, "python"))
from t_mac.weights import preprocess_weights as ref_preprocess_weights  # noqa: E402


def gen(name, seed, Mw, K, bits, bm, kfactor, gs, ags, zp, m_groups=-1):
    case = orc.make_case(seed, Mw, K, bits=bits, gs=gs, ags=ags, zero_point=zp, m_groups=m_groups)
    A, S = ref_preprocess_weights(case["w"], case["sc"], case["zr"], bits=bits, g=4, bm=bm, kfactor=kfactor)
    A = np.ascontiguousarray(A, np.uint8)
    S = np.ascontiguousarray(S, np.float32)
    q, ls, lb = orc.ref_preprocessor(case["B"][0], ags)
    out = dict(w=case["w"], sc=case["sc"], B=case["B"], A_ref=A, S_ref=S, qlut=q, lut_scales=ls, lut_biases=lb,
               meta=np.array([Mw, K, bits, bm, kfactor, gs, ags, int(zp), m_groups], np.int64))
    if case["zr"] is not None:
        out["zr"] = case["zr"]
    if m_groups == -1:
        cbits = orc.ref_cbits_float(A, q, S, ls, lb, Mw, K, bits, bm, kfactor, gs, ags, zp)
        out["cbits"] = cbits
        out["C"] = orc.combine_planes(cbits, Mw, bits)
        out["PS"] = orc.ref_partial_sums(A, q, Mw, K, bits, bm, kfactor, ags)
    else:
        out["cbits32"] = orc.ref_cbits_int32(A, q, Mw, K, bits, bm, kfactor)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print(name, {k: v.shape for k, v in out.items()})


def gen_fa(name):
    """(a9) the same inputs through the reference's FastAggregation = true instantiation of the tbl intrinsic (its AVX2
    flavour, the one that runs on this host): tests/golden/fa/<name>.npz holds only the outputs."""
    d = dict(np.load(os.path.join(HERE, name + ".npz")))
    Mw, K, bits, bm, kfactor, gs, ags, zp, mg = [int(x) for x in d["meta"]]
    cbits = orc.ref_cbits_float(d["A_ref"], d["qlut"], d["S_ref"], d["lut_scales"], d["lut_biases"], Mw, K, bits, bm,
                                kfactor, gs, ags, bool(zp), fa=True)
    os.makedirs(os.path.join(HERE, "fa"), exist_ok=True)
    np.savez_compressed(os.path.join(HERE, "fa", name + ".npz"), cbits_fa=cbits, C_fa=orc.combine_planes(cbits, Mw, bits),
                        meta=d["meta"])
    print("fa/" + name)


def gen_prebuilt(name, setname, seed, Mw, K, bits, bm, mname):
    """Through the checked-in prebuilt C-ABI kernels, driven tile by tile like llama.cpp."""
    L = orc.ref_lib(setname)
    case = orc.make_case(seed, Mw, K, bits=bits, zero_point=True)
    A, S = ref_preprocess_weights(case["w"], case["sc"], case["zr"], bits=bits, g=4, bm=bm, kfactor=16)
    A = np.ascontiguousarray(A, np.uint8); S = np.ascontiguousarray(S, np.float32)
    B = np.ascontiguousarray(case["B"][0])
    G = K // 64
    ls = np.zeros(G, np.float32); lb = np.zeros(G, np.float32); q = np.zeros((K // 4, 16), np.int8)
    assert getattr(L, f"preprocessor_t1_int8_m{mname}_k{K}_n1_b{bits}")(orc._p(B), orc._p(ls), orc._p(lb), orc._p(q)) == 0
    qg = getattr(L, f"qgemm_lut_t1_int8_m{bm}_k{K}_n1_b{bits}")
    rpt = bm // bits
    Cout = np.zeros(Mw, np.float32)
    for tile in range(Mw * bits // bm):
        c = np.zeros(rpt, np.float32)
        assert qg(orc._p(A[tile]), orc._p(q), orc._p(S[tile]), orc._p(ls), orc._p(lb), orc._p(c)) == 0
        Cout[tile * rpt:(tile + 1) * rpt] = c
    np.savez_compressed(os.path.join(HERE, name + ".npz"), w=case["w"], sc=case["sc"], zr=case["zr"], B=case["B"],
                        A_ref=A, S_ref=S, qlut=q, lut_scales=ls, lut_biases=lb, C=Cout,
                        PS=orc.ref_partial_sums(A, q, Mw, K, bits, bm, 16, 64),
                        meta=np.array([Mw, K, bits, bm, 16, 128, 64, 1, -1], np.int64))
    print(name, "via", setname)


def gen_kat():
    """Compile and run the reference's own tests/test_lut_ctor.cc; record what it prints."""
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "t")
        subprocess.run(["g++", "-O2", "-mavx2", "-mfma", "-ffp-contract=off", "-std=c++17", "-w", "-fpermissive",
                        "-include", "cstdio", "-I", os.path.join(REF, "python/t_mac/intrins"),
                        os.path.join(REF, "tests/test_lut_ctor.cc"), "-o", exe], check=True)
        txt = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    lines = txt.strip().splitlines()
    kat = dict(source="tests/test_lut_ctor.cc (b[i]=i, i<32; act_k=32)", raw=lines,
               lut_scales=float(lines[1].split(":")[1]), lut_biases=float(lines[2].split(":")[1]),
               qlut=[[int(x) for x in l.split()] for l in lines[3:11]])
    json.dump(kat, open(os.path.join(HERE, "lut_ctor_kat.json"), "w"), indent=1)
    print("KAT", kat["lut_scales"], kat["lut_biases"])


def call_prebuilt(setname, bm, K, bits, Mw_total_bits_name, case, gs=128, ags=64):
    """Drive a checked-in prebuilt kernel set exactly as llama.cpp would (per-tile pointers)."""
    L = orc.ref_lib(setname)
    Mw = case["w"].shape[0]
    kfactor = 16
    A = orc.preprocess_weights(case["w"], bits, bm, kfactor)
    S = orc.preprocess_scales(case["sc"], case["zr"], bits, bm)
    B = np.ascontiguousarray(case["B"][0])
    G = K // ags
    ls = np.zeros(G, np.float32); lb = np.zeros(G, np.float32); q = np.zeros((K // 4, 16), np.int8)
    pre = getattr(L, f"preprocessor_t1_int8_m{Mw_total_bits_name}_k{K}_n1_b{bits}")
    assert pre(orc._p(B), orc._p(ls), orc._p(lb), orc._p(q)) == 0
    qg = getattr(L, f"qgemm_lut_t1_int8_m{bm}_k{K}_n1_b{bits}")
    Cout = np.zeros(Mw, np.float32)
    rpt = bm // bits
    for tile in range(Mw * bits // bm):
        c = np.zeros(rpt, np.float32)
        assert qg(orc._p(A[tile]), orc._p(q), orc._p(S[tile]), orc._p(ls), orc._p(lb), orc._p(c)) == 0
        Cout[tile * rpt:(tile + 1) * rpt] = c
    return A, S, q, ls, lb, Cout



def gen_vs_ref():
    """ref/oracle_vs_ref.npz: the reference's answers for the inputs tests/test_oracle_vs_ref.py draws (its helpers build them)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_oracle_vs_ref as T
    out = {}
    for K, ags in T.PRE_CASES:
        for n, v in zip(("q", "ls", "lb"), orc.ref_preprocessor(T.preprocessor_input(K, ags)[0], ags)):
            out[T.key("pre", K, ags, n)] = v
    for n, v in zip(("q", "ls", "lb"), orc.ref_preprocessor(T.edge_input()[0], 64)):
        out[T.key("edge", n)] = v
    for bits, bm, kf in T.PW_CASES:
        case = T.pw_case(bits, bm, kf)
        A, S = ref_preprocess_weights(case["w"], case["sc"], case["zr"], bits=bits, g=4, bm=bm, kfactor=kf)
        _, S1 = ref_preprocess_weights(case["w"], case["sc"], None, bits=bits, g=4, bm=bm, kfactor=kf)
        out[T.key("pw", bits, bm, kf, "A")] = np.ascontiguousarray(A, np.uint8)
        out[T.key("pw", bits, bm, kf, "S")] = np.asarray(S)
        out[T.key("pw", bits, bm, kf, "S1")] = np.asarray(S1)
    for tag, cfgs, fa in (("fp", T.CFGS, False), ("fa", T.FA_CFGS, True)):
        for bits, bm, kf, gs, ags, zp in cfgs:
            A, S, q, ls, lb, case = T.float_case(bits, bm, kf, gs, ags, zp, fa=fa)
            Mw, K = case["w"].shape
            out[T.key(tag, bits, bm, kf, gs, ags, zp, "cbits")] = orc.ref_cbits_float(A, q[0], S, ls[0], lb[0], Mw, K, bits, bm, kf, gs, ags, zp, fa=fa)
            if not fa and T.has_int_partial_sums(bits, kf, ags):
                out[T.key(tag, bits, bm, kf, gs, ags, zp, "ps")] = orc.ref_partial_sums(A, q[0], Mw, K, bits, bm, kf, ags)
    for setname, bits, bm, Mw, K, mname in T.PREBUILT_CASES:
        _, _, case = T.prebuilt_case(bits, bm, Mw, K)
        _, _, q, ls, lb, C = call_prebuilt(setname, bm, K, bits, mname, case)
        for n, v in zip(("q", "ls", "lb", "C"), (q, ls, lb, C)):
            out[T.key("pb", setname, Mw, K, n)] = v
    for bits, bm, Mw, K in T.INT32_CASES:
        A, q, ls, lb, case = T.int32_case(bits, bm, Mw, K)
        out[T.key("i32", bits, bm, Mw, K, "cb")] = orc.ref_cbits_int32(A, q[0], Mw, K, bits, bm, 16)
    os.makedirs(os.path.join(HERE, "ref"), exist_ok=True)
    np.savez_compressed(os.path.join(HERE, "ref", "oracle_vs_ref.npz"), **out)
    print("ref/oracle_vs_ref.npz", len(out), "arrays")


def gen_saturating():
    """ref/saturating.npz: the reference's answers for the saturating inputs of tests/test_oracle_vs_ref.py (oracle.make_hard_case;
    its helpers build them)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_oracle_vs_ref as T
    out = {}
    for K, ags in T.SAT_PRE_CASES:
        for acts in orc.HARD_ACTS:
            for n, v in zip(("q", "ls", "lb"), orc.ref_preprocessor(orc.hard_acts(acts, K), ags)):
                out[T.key("pre", acts, K, ags, n)] = v
    for weights in T.SAT_WEIGHTS:
        for tag, cfgs, fa in (("fp", T.CFGS, False), ("fa", T.FA_CFGS, True)):
            for bits, bm, kf, gs, ags, zp in cfgs:
                A, S, q, ls, lb, case = T.sat_float_case(bits, bm, kf, gs, ags, zp, weights)
                Mw, K = case["w"].shape
                out[T.key(tag, weights, bits, bm, kf, gs, ags, zp, "cbits")] = orc.ref_cbits_float(A, q[0], S, ls[0], lb[0], Mw, K, bits, bm, kf, gs, ags, zp, fa=fa)
                if not fa and T.has_int_partial_sums(bits, kf, ags):
                    out[T.key(tag, weights, bits, bm, kf, gs, ags, zp, "ps")] = orc.ref_partial_sums(A, q[0], Mw, K, bits, bm, kf, ags)
    for weights in ("max", "rows"):
        for bits, bm, Mw, K in T.SAT_INT32_CASES:
            A, q, ls, lb, case = T.sat_int32_case(bits, bm, Mw, K, weights)
            out[T.key("i32", weights, bits, bm, Mw, K, "cb")] = orc.ref_cbits_int32(A, q[0], Mw, K, bits, bm, 16)
    np.savez_compressed(os.path.join(HERE, "ref", "saturating.npz"), **out)
    print("ref/saturating.npz", len(out), "arrays")


def gen_convert_ref():
    """ref/convert_ref.json: what the reference's model_utils returns for the inputs tests/test_convert.py draws (its helpers build them);
    arrays as digests.  ref/kcfg/*.ini: the kcfg.ini files the reference ships for two prebuilt sets."""
    import shutil
    from pathlib import Path
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_convert as T
    import t_mac.model_utils as mu
    out = {"unpack_gptqv2": {}}
    for bits, K, M, gs, v2 in T.UNPACK_CASES:
        qw, sc, qz, _, _ = T.gptq_case(bits * 100 + K, K, M, bits, gs)
        w, s, z, b, g = mu.unpack_gptqv2(qw, sc, qz, gptq_v2=v2)
        out["unpack_gptqv2"]["%d_%d_%d_%d_%d" % (bits, K, M, gs, v2)] = {"bits_group": [int(b), int(g)], "w_s_z": [T.digest(w), T.digest(s), T.digest(z)]}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "kcfg.ini")
        T.write_llama_kcfg(path)
        Mw, K, bits, w, sc, zr = T.blob_case()
        out["preprocess_for_t_mac"] = T.digest(mu.preprocess_for_t_mac(path, w, sc, zr, bits=bits))
        ck = os.path.join(d, "ck"); os.makedirs(ck)
        T._fake_checkpoint(ck, T.CHECKPOINT_LAYERS)
        out["model_utils"] = {"preset_models": sorted(mu.get_preset_models()),
                              "kernel_shapes": {n: mu.extract_kernel_shapes(n) for n in mu.get_preset_models() if n != "gptq-auto"},
                              "gptq_auto_shapes": mu.extract_kernel_shapes("gptq-auto", ck),
                              "quantization_config": mu.get_quantization_config(Path(ck))}
    os.makedirs(os.path.join(HERE, "ref", "kcfg"), exist_ok=True)
    json.dump(out, open(os.path.join(HERE, "ref", "convert_ref.json"), "w"), indent=1)
    for setname in ("aarch64-llama-2-7b-2bit", "aarch64-hf-bitnet-3b"):
        shutil.copyfile(os.path.join(REF, "deploy", "tuned", setname, "kcfg.ini"), os.path.join(HERE, "ref", "kcfg", setname + ".ini"))
    print("ref/convert_ref.json")


if __name__ == "__main__":
    if sys.argv[1:] == ["convert"]:
        gen_convert_ref()
        sys.exit(0)
    if sys.argv[1:] == ["vs_ref"]:
        gen_vs_ref()
        sys.exit(0)
    if sys.argv[1:] == ["saturating"]:
        gen_saturating()
        sys.exit(0)
    gen_vs_ref()
    gen_saturating()
    gen_convert_ref()
    gen_kat()
    gen("w2_zp_g128_a64", 1, 128, 512, 2, 128, 16, 128, 64, True)
    gen("w2_nozp_g128_a64", 2, 128, 512, 2, 128, 16, 128, 64, False)
    gen("w4_zp_g128_a64", 3, 128, 512, 4, 256, 16, 128, 64, True)
    gen("w1_zp_g128_a64", 4, 256, 256, 1, 128, 16, 128, 64, True)
    gen("w3_nozp_g128_a64", 5, 128, 256, 3, 192, 16, 128, 64, False)
    gen("w2_zp_g128_a32_kf8", 6, 64, 512, 2, 128, 8, 128, 32, True)
    gen("bitnet_w2_int32_k640", 7, 160, 640, 2, 320, 16, 128, 640, False, m_groups=1)
    for n in ("w2_zp_g128_a64", "w2_nozp_g128_a64", "w4_zp_g128_a64", "w1_zp_g128_a64", "w3_nozp_g128_a64", "w2_zp_g128_a32_kf8"):
        gen_fa(n)
    gen_prebuilt("prebuilt_llama2_7b_w2_k4096", "aarch64-llama-2-7b-2bit", 0, 64, 4096, 2, 128, 8192)
