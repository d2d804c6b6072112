"""Converter-side formats (tmac_amd/convert.py) against the reference's own Python and against the kcfg parser of the C library.
What the reference's python/t_mac/model_utils.py returns for the inputs drawn here is recorded in tests/golden/ref/convert_ref.json
(digests of its arrays, its shape tables) by tests/golden/make_golden.py; tests/golden/ref/kcfg/ holds the kcfg.ini files the reference
ships for two of its prebuilt sets.  CPU only."""
import hashlib
import json
import os

import numpy as np
import pytest

import tmac_amd
from tmac_amd import convert

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref")
UNPACK_CASES = [(2, 256, 64, 128, True), (4, 512, 96, 128, True), (4, 256, 32, 64, False), (2, 128, 160, 32, True)]
CHECKPOINT_LAYERS = [(2, 64, 256, 128), (2, 160, 256, 128), (2, 64, 256, 128), (4, 96, 512, 128), (2, 64, 640, 128)]


def recorded():
    with open(os.path.join(GOLDEN, "convert_ref.json")) as f:
        return json.load(f)


def digest(a):
    """sha256 of an array's dtype, shape and bytes: what convert_ref.json records of the reference's arrays"""
    a = np.ascontiguousarray(a)
    return hashlib.sha256(("%s%s" % (a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()


def blob_case():
    rng = np.random.default_rng(5)
    Mw, K, bits = 4096, 4096, 2
    w = rng.integers(0, 4, size=(Mw, K), dtype=np.uint8)
    sc = np.abs(rng.standard_normal((Mw, K // 128))).astype(np.float16)
    zr = rng.standard_normal((Mw, K // 128)).astype(np.float16)
    return Mw, K, bits, w, sc, zr


def write_llama_kcfg(path):
    kernels = convert.PRESET_KERNELS["llama-2-7b-2bit"] + convert.PRESET_KERNELS["hf-bitnet-3b"][:1]
    convert.write_kcfg(path, kernels[:3], bm={(2, 4096, 4096): 128, (2, 11008, 4096): 128, (2, 4096, 11008): 128})


def gptq_case(seed, K, M, bits, gs, fp16=True):
    rng = np.random.default_rng(seed)
    per = 32 // bits
    w = rng.integers(0, 2 ** bits, size=(K, M), dtype=np.uint32)
    qweight = np.zeros((K // per, M), np.uint32)
    for f in range(per):
        qweight |= w[f::per] << np.uint32(bits * f)
    z = rng.integers(0, 2 ** bits, size=(K // gs, M), dtype=np.uint32)
    qzeros = np.zeros((K // gs, M // per), np.uint32)
    for f in range(per):
        qzeros |= z[:, f::per] << np.uint32(bits * f)
    scales = np.abs(rng.standard_normal((K // gs, M))).astype(np.float16 if fp16 else np.float32)
    return qweight.view(np.int32), scales, qzeros.view(np.int32), w.T.astype(np.uint8), z.T


@pytest.mark.parametrize("bits,K,M,gs,v2", UNPACK_CASES)
def test_unpack_gptq(bits, K, M, gs, v2):
    qw, sc, qz, w_true, z_true = gptq_case(bits * 100 + K, K, M, bits, gs)
    assert convert.parse_gptq(qw, sc, qz) == (K, M, bits, gs)
    w, s, z, b, g = convert.unpack_gptq(qw, sc, qz, gptq_v2=v2)
    assert b == bits and g == gs
    assert np.array_equal(w, w_true)
    assert np.array_equal(s, sc.T)
    zt = (z_true.astype(sc.dtype) + (0 if v2 else 1) - 2 ** (bits - 1)) * sc.T
    assert np.array_equal(z, zt)
    # the reference's unpack_gptqv2 on the same tensors
    r = recorded()["unpack_gptqv2"]["%d_%d_%d_%d_%d" % (bits, K, M, gs, v2)]
    assert [bits, gs] == r["bits_group"]
    assert [digest(w), digest(s), digest(z)] == r["w_s_z"]


def test_kcfg_roundtrip_and_blob(tmp_path):
    path = str(tmp_path / "kcfg.ini")
    write_llama_kcfg(path)
    e = convert.read_kcfg_entry(path, 4096, 11008, 2)
    assert e == dict(bm=128, simd_n_in=16, simd_n_out=8, kfactor=16, group_size=128, lut_scales_size=172,
                     scales_size=704512, n_tile_num=64)
    # byte-identical in content with the file the reference ships for this model
    import configparser
    a, b = configparser.ConfigParser(), configparser.ConfigParser()
    a.read(path)
    assert b.read(os.path.join(GOLDEN, "kcfg", "aarch64-llama-2-7b-2bit.ini"))
    for sec in a.sections():
        assert dict(a[sec]) == dict(b[sec]), sec
    # the C library parses what we wrote
    L = tmac_amd.lib()
    tmac_amd.binding.check(L.tmac_hip_load_kcfg(path.encode()))
    cfg = tmac_amd.TMACGeMMWrapper(act_group_size=64).get_kcfg(4096, 11008, 1, 2)
    assert (cfg.bm, cfg.kfactor, cfg.group_size, cfg.n_tile_num) == (128, 16, 128, 64)

    # blob: [weight bytes][fp32 scales], identical to the reference's, and split_blob inverts the concatenation
    Mw, K, bits, w, sc, zr = blob_case()
    blob = convert.preprocess_for_t_mac(path, w, sc, zr, bits=bits)
    assert blob.dtype == np.uint8 and blob.size == Mw * K * bits // 8 + Mw * (K // 128) * 2 * 4
    A, S = convert.split_blob(blob, Mw, K, bits)
    A2, S2 = tmac_amd.weights.preprocess_weights(w, sc, zr, bits=bits, bm=128, kfactor=16)
    assert np.array_equal(A, A2.reshape(-1)) and np.array_equal(S, S2.astype(np.float32).reshape(-1))
    assert digest(blob) == recorded()["preprocess_for_t_mac"]          # the reference's preprocess_for_t_mac on the same file and tensors


def test_bitnet_kcfg_entry(tmp_path):
    path = str(tmp_path / "k.ini")
    convert.write_kcfg(path, convert.PRESET_KERNELS["hf-bitnet-3b"], act_group_size=-1, zero_point=False,
                       bm={(2, 3200, 8640): 128, (2, 8640, 3200): 128, (2, 3200, 3200): 320})
    e = convert.read_kcfg_entry(path, 3200, 8640, 2)
    assert e["scales_size"] == 1 and e["lut_scales_size"] == 1 and e["bm"] == 128 and e["n_tile_num"] == 50
    # the shipped (ARM) set keeps act_group_size = 64 with one weight scale (lut_scales_size = K/64)
    import configparser
    path2 = str(tmp_path / "k64.ini")
    convert.write_kcfg(path2, convert.PRESET_KERNELS["hf-bitnet-3b"], act_group_size=64, zero_point=False,
                       bm={(2, 3200, 8640): 128, (2, 8640, 3200): 128, (2, 3200, 3200): 320})
    b = configparser.ConfigParser()
    assert b.read(os.path.join(GOLDEN, "kcfg", "aarch64-hf-bitnet-3b.ini"))
    a = configparser.ConfigParser()
    a.read(path2)
    common = [sec for sec in a.sections() if sec in b]
    assert common
    for sec in common:
        assert dict(a[sec]) == dict(b[sec]), sec


def _fake_checkpoint(d, layers, desc_act=False):
    """config.json + two safetensors parts holding GPTQ-packed linear layers (qweight / scales / qzeros) and an unquantised tensor"""
    import json
    from safetensors.numpy import save_file
    parts = [{}, {}]
    for i, (bits, M, K, gs) in enumerate(layers):
        qw, sc, qz, _, _ = gptq_case(50 + i, K, M, bits, gs)
        pre = f"model.layers.{i}.proj"
        parts[i % 2].update({pre + ".qweight": qw, pre + ".scales": sc, pre + ".qzeros": qz})
    parts[0]["model.embed_tokens.weight"] = np.zeros((8, 4), np.float16)
    save_file(parts[0], os.path.join(d, "model-00001-of-00002.safetensors"))
    save_file(parts[1], os.path.join(d, "model-00002-of-00002.safetensors"))
    cfg = {"quantization_config": {"bits": layers[0][0], "group_size": layers[0][3], "sym": False, "quant_method": "gptq", "desc_act": desc_act,
                                   "meta": {"quantizer": "gptqmodel:1.0"}}, "hidden_size": 64}
    json.dump(cfg, open(os.path.join(d, "config.json"), "w"))


def test_presets_and_checkpoint_discovery(tmp_path):
    """preset shape table, kernel shapes read from a GPTQ checkpoint's safetensors HEADERS, and the quantisation config -- equal to the
    reference's model_utils (which loads the tensors to learn their shapes)"""
    d = str(tmp_path)
    _fake_checkpoint(d, CHECKPOINT_LAYERS)
    ks = convert.extract_kernel_shapes("gptq-auto", d)
    assert sorted(ks) == sorted([[2, 64, 256, 1, -1], [2, 160, 256, 1, -1], [4, 96, 512, 1, -1], [2, 64, 640, 1, -1]])    # distinct (bits, M, K), each once
    assert convert.checkpoint_group_size(d) == 128
    qc = convert.get_quantization_config(d)
    assert qc["bits"] == 2 and qc["group_size"] == 128 and qc["quant_method"] == "gptq" and qc["quantizer"] == "gptqmodel:1.0"
    with pytest.raises(KeyError):
        convert.extract_kernel_shapes("no-such-model")
    # the reference's model_utils on the same presets and checkpoint
    r = recorded()["model_utils"]
    assert set(convert.get_preset_models()) == set(r["preset_models"])
    for name, shapes in r["kernel_shapes"].items():
        assert convert.extract_kernel_shapes(name) == shapes, name
    assert sorted(ks) == sorted(r["gptq_auto_shapes"])
    assert qc == r["quantization_config"]
    # mixed group sizes and act-order checkpoints are refused, as in the reference
    d2 = os.path.join(d, "mixed"); os.makedirs(d2)
    _fake_checkpoint(d2, [(2, 64, 256, 128), (2, 64, 256, 64)])
    with pytest.raises(RuntimeError):
        convert.extract_kernel_shapes("gptq-auto", d2)
    d3 = os.path.join(d, "actorder"); os.makedirs(d3)
    _fake_checkpoint(d3, [(2, 64, 256, 128)], desc_act=True)
    with pytest.raises(AssertionError):
        convert.get_quantization_config(d3)


def test_corrupt_checkpoint_parts_are_named(tmp_path):
    """a truncated or malformed safetensors part surfaces as a RuntimeError that names the file, not as a bare struct / JSON /
    ZeroDivisionError"""
    import json
    import struct
    from tmac_amd import convert as cv
    d = tmp_path / "ckpt"; d.mkdir()
    p = d / "model.safetensors"
    p.write_bytes(b"\x10\x00\x00")                                       # shorter than the length field
    with pytest.raises(RuntimeError, match="model.safetensors"):
        cv.extract_kernel_shapes("gptq-auto", str(d))
    p.write_bytes(struct.pack("<Q", 1 << 40) + b"{}")                     # header length beyond the file
    with pytest.raises(RuntimeError, match="corrupt safetensors header"):
        cv.extract_kernel_shapes("gptq-auto", str(d))
    p.write_bytes(struct.pack("<Q", 5) + b"{oops")                        # not JSON
    with pytest.raises(RuntimeError, match="corrupt safetensors header"):
        cv.extract_kernel_shapes("gptq-auto", str(d))
    hdr = {"l.qweight": {"dtype": "I32", "shape": [256, 64], "data_offsets": [0, 0]}, "l.scales": {"dtype": "F16", "shape": [32, 64], "data_offsets": [0, 0]},
           "l.qzeros": {"dtype": "I32", "shape": [32, 0], "data_offsets": [0, 0]}}
    raw = json.dumps(hdr).encode()
    p.write_bytes(struct.pack("<Q", len(raw)) + raw)                     # a zero-width qzeros tensor
    with pytest.raises(RuntimeError, match="not GPTQ-packed shapes"):
        cv.extract_kernel_shapes("gptq-auto", str(d))
