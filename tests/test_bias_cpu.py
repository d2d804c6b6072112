"""Biased linear layers (y = W x + b) without a GPU: what the checkpoint scans make of ``<layer>.bias`` tensors, the loaders' refusals that
must come before anything is registered, and the planner of k_gemv_quad's bias instantiations (tmac_amd/csrc/tmac_launch_plan.cpp,
quad_plan_bias) through a small g++ program (tests/cpp/bias_plan_main.cc: its own main), built as tests/cpp/launch_plan_main.cc is.

The planner's rules, as the issue states them: the bias block takes the configuration the plain call's block takes -- with the LUT built
in-kernel the covered set (512,1), (512,2), (768,3), (1024,4) with quad_plan_xf's fall-back, with a copied LUT the 512-thread
configurations of the plain copy form -- per-group scales only, with a transform NORM and the silu GLU only, and every plan names an
instantiation that exists (quad_bi_inst_exists)."""
import os
import subprocess

import numpy as np
import pytest

import bitnet_common as bc
import bitnet_packed_common as bpc
import pack_common as pc
import rtn_common as rc
from tmac_amd import checkpoint

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GPTQ_LAYERS = [("model.layers.0.self_attn.q_proj", 71, 128, 256, 2, 64), ("model.layers.0.self_attn.o_proj", 72, 256, 128, 2, 64),
               ("model.layers.0.mlp.down_proj", 73, 128, 256, 2, 64)]


def bias_of(seed, Mw, dtype):
    return np.random.default_rng(seed).standard_normal(Mw).astype(dtype)


def add_part(d, tensors, dtype_names=None):
    """one more part of the checkpoint in d, holding `tensors`"""
    fn = os.path.join(d, "model-extra.safetensors")
    return fn, pc.write_safetensors(fn, tensors, dtype_names)


# ---- the scans -----------------------------------------------------------------------------------------------------------------------
def test_gptq_scan_finds_bias(tmp_path):
    d = str(tmp_path)
    pc.write_gptq_checkpoint(d, GPTQ_LAYERS)
    q, o = GPTQ_LAYERS[0][0], GPTQ_LAYERS[1][0]
    b16, b32 = bias_of(1, 128, np.float16), bias_of(2, 256, np.float32)
    fn, where = add_part(d, {q + ".bias": b16, o + ".bias": b32.view(np.float32)})
    scan = checkpoint.scan_gptq_dir(d)
    by = {L.name: L for L in scan.layers}
    assert by[GPTQ_LAYERS[2][0]].bias is None
    for name, arr, dt in ((q, b16, "F16"), (o, b32, "F32")):
        ref = by[name].bias
        assert ref == checkpoint.TensorRef(fn, dt, (arr.shape[0],), *where[name + ".bias"])
        assert np.array_equal(np.array(checkpoint.read_tensor(ref)), arr)
    assert checkpoint.GptqLayer._fields[-1] == "bias" and checkpoint.GptqLayer._field_defaults["bias"] is None


def test_dense_scan_finds_bias(tmp_path):
    d = str(tmp_path)
    name, _, Mw, _, _ = rc.CKPT_LAYERS[0]
    bb = bc.f32_to_bf16_bits(bias_of(3, Mw, np.float32))        # bf16 words travel as fp16 bytes under the name BF16
    _, where = rc.write_dense_checkpoint(d, extra={name + ".bias": bb.view(np.float16)}, dtype_names={name + ".bias": "BF16"})
    scan = checkpoint.scan_dense_dir(d)
    by = {L.name: L for L in scan.layers}
    ref = by[name].bias
    assert ref.dtype == "BF16" and ref.shape == (Mw,) and (ref.begin, ref.end) == where[name + ".bias"][1:]
    assert np.array_equal(np.array(checkpoint.read_tensor(ref)), bb)
    assert all(L.bias is None for L in scan.layers if L.name != name)
    assert checkpoint.DenseLayer._fields[-1] == "bias" and checkpoint.DenseLayer._field_defaults["bias"] is None


@pytest.mark.parametrize("what", ("dtype", "shape_len", "shape_2d", "bytes"))
def test_scans_refuse_a_malformed_bias(tmp_path, what):
    name, _, Mw, _, _ = rc.CKPT_LAYERS[0]
    arr, names = bias_of(4, Mw, np.float16), {}
    if what == "dtype":
        arr = np.arange(Mw, dtype=np.int32)
    elif what == "shape_len":
        arr = arr[:-4]
    elif what == "shape_2d":
        arr = arr.reshape(1, Mw)
    else:
        names = {name + ".bias": "F32"}             # fp16 bytes under the name F32: shape [Mw], half the bytes
    for sub, write, scan in (("dense", lambda d: rc.write_dense_checkpoint(d, extra={name + ".bias": arr}, dtype_names=names), checkpoint.scan_dense_dir),
                             ("gptq", None, checkpoint.scan_gptq_dir)):
        d = str(tmp_path / sub)
        os.makedirs(d)
        if write is not None:
            write(d)
            tensor = name + ".bias"
        else:
            pc.write_gptq_checkpoint(d, GPTQ_LAYERS)
            tensor = GPTQ_LAYERS[0][0] + ".bias"
            add_part(d, {tensor: arr}, {tensor: names[name + ".bias"]} if names else None)
        with pytest.raises(RuntimeError) as e:
            scan(d)
        assert tensor in str(e.value), str(e.value)


# ---- loaders: refused before anything is registered (no GPU is touched) ------------------------------------------------------------------
class NoWrapper:
    _act_group_size = 64

    def __getattr__(self, name):
        raise AssertionError("the loader reached the wrapper ({}): it must refuse first".format(name))


def test_act_order_with_a_bias_raises_naming_the_layer(tmp_path):
    d = str(tmp_path)
    pc.write_gptq_checkpoint(d, GPTQ_LAYERS, desc_act=True)
    layer = GPTQ_LAYERS[2][0]                        # the LAST layer: nothing in front of it may have been registered
    add_part(d, {layer + ".bias": bias_of(5, 128, np.float16)})
    assert {L.name: L for L in checkpoint.scan_gptq_dir(d, act_order=True).layers}[layer].bias is not None
    with pytest.raises(RuntimeError) as e:
        checkpoint.load_gptq_dir(d, NoWrapper(), act_order=True)
    assert layer in str(e.value) and "bias" in str(e.value)


def test_bitnet_directories_with_a_bias_raise_naming_the_layer(tmp_path):
    d1, d2 = str(tmp_path / "masters"), str(tmp_path / "packed")
    os.makedirs(d1), os.makedirs(d2)
    layer = bc.CKPT_LAYERS[1][0]
    bc.write_bitnet_checkpoint(d1, extra={layer + ".bias": bias_of(6, bc.CKPT_LAYERS[1][2], np.float16)})
    with pytest.raises(RuntimeError) as e:
        checkpoint.load_bitnet_dir(d1, NoWrapper())
    assert layer + ".bias" in str(e.value)
    layer = bpc.CKPT_LAYERS[2][0]
    bpc.write_packed_checkpoint(d2, extra={layer + ".bias": bias_of(7, bpc.CKPT_LAYERS[2][2], np.float16)})
    with pytest.raises(RuntimeError) as e:
        checkpoint.load_bitnet_packed_dir(d2, NoWrapper())
    assert layer + ".bias" in str(e.value)


# ---- the planner ---------------------------------------------------------------------------------------------------------------------
COVERED = {(512, 1), (512, 2), (768, 3), (1024, 4)}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("bias_plan")), "bias_plan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "bias_plan_main.cc"),
                    os.path.join(ROOT, "tmac_amd", "csrc", "tmac_launch_plan.cpp")], check=True)
    return exe


def ask(exe, qs):
    out = subprocess.run([exe], input="\n".join(qs) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
    assert len(out) == len(qs) and "?" not in out
    res = []
    for line in out:
        if line == "refuse":
            res.append(None)
            continue
        plan, flags, inst, twin = (p.strip() for p in line.split(" | "))
        res.append(dict(plan=plan, f=[int(x) for x in plan.split()], bi=flags == "bi 1 ga 0", inst=inst == "inst 1",
                        twin=None if twin == "twin refuse" else twin[len("twin "):]))
    return res


FORCED = [(0, 0), (512, 1), (512, 2), (768, 1), (768, 2), (768, 3), (1024, 1), (1024, 2), (1024, 4)]
GRID = [(bits, K, tq) for bits in (1, 2, 3, 4) for K in (512, 1024, 2304, 4096, 11008, 14336) for tq in (32, 48, 1024, 3072, 5504)]


def test_bias_plans_take_the_plain_blocks_configuration_and_name_an_instantiation(program):
    qs, meta = [], []
    for bits, K, tq in GRID:
        for ft, wq in FORCED:
            for bl, kind in ((1, 0), (0, 0), (1, 1), (1, 2)):
                for strict in ((0, 1) if ft else (0,)):
                    qs.append(f"b {bits} {K} 0 {tq} {bl} {kind} {ft} {wq} {strict}")
                    meta.append((bl, kind, ft, wq, strict))
    res = ask(program, qs)
    assert sum(r is not None for r in res) > len(res) // 2
    for q, (bl, kind, ft, wq, strict), r in zip(qs, meta, res):
        if r is None:
            continue
        f = r["f"]          # ft wpq nr early dump acc lutsrc xf gn gt gx lds
        assert r["bi"] and r["inst"], q
        assert (f[0], f[1]) in COVERED and f[4] == 0 and f[5] == 1 and f[6] == bl and f[7] == (1 if kind else 0) and f[8] == 0 and f[9] == 0, (q, r)
        if not bl:
            assert f[0] == 512 and f[2] == 2 and f[3] == 0, (q, r)
        # the configuration, grid, tables per thread, EARLY and LDS of the call without a bias (the gather's rule stands for "LUT built, covered set")
        assert r["twin"] is not None, q
        tw = r["twin"].split()
        assert [tw[i] for i in (0, 1, 2, 3, 10, 11)] == [str(f[i]) for i in (0, 1, 2, 3, 10, 11)], (q, r)
    # a forced configuration outside the covered set: refused with a built LUT (strict), the covered ones are served where the shape allows
    for q, (bl, kind, ft, wq, strict), r in zip(qs, meta, res):
        if bl and strict and (ft, wq) not in COVERED:
            assert r is None, q
    served = {(m[2], m[3]) for m, r in zip(meta, res) if r is not None and m[0] and m[4]}
    assert served == COVERED


def test_bias_plans_refuse_what_has_no_instantiation(program):
    qs = ["b 2 4096 2 1024 1 0 0 0 0",            # unified scales
          "b 2 4096 2 1024 0 0 0 0 0",
          "b 2 4096 0 1024 1 4 0 0 0",            # GLU_NORM
          "b 2 4096 0 1024 1 258 0 0 0",          # relu^2 GLU (gate 1 << 8 | GLU)
          "b 2 4096 0 1024 1 514 0 0 0",          # GELU GLU
          "b 2 4096 0 1024 0 1 0 0 0",            # a transform needs the in-kernel build
          "b 2 4096 0 1024 0 0 1024 4 1",         # copy form: 512-thread workgroups only
          "b 2 4096 0 1024 0 0 768 3 1",
          "b 5 4096 0 1024 1 0 0 0 0",            # no such width
          "b 2 4100 0 1024 1 0 0 0 0"]            # K % 64
    assert ask(program, qs) == [None] * len(qs)
    ok = ask(program, ["b 2 4096 0 1024 1 1 0 0 0", "b 2 4096 0 1024 1 2 0 0 0", "b 2 4096 0 1024 1 0 0 0 0", "b 2 4096 0 1024 0 0 0 0 0"])
    assert all(r is not None and r["inst"] for r in ok)
