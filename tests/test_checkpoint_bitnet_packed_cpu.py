"""checkpoint.scan_bitnet_packed_dir without a GPU: a synthetic two-part checkpoint of PACKED ternary weights
(bitnet_packed_common.write_packed_checkpoint, through pack_common.write_safetensors: U8 layers with weight_scale in BF16, F16 and F32,
shapes [1] and [], an embedding, norms and a bf16 lm_head that are no layers) -- names, order, shapes, byte ranges, both linear_class
values and the default, the use_rms_norm fields, every refusal by its message, and the unchanged refusal of the same directory by
scan_bitnet_dir.
"""
import numpy as np
import pytest

import bitnet_packed_common as bp
import pack_common as pc
from tmac_amd import checkpoint, convert

ST = {"bf16": "BF16", "f16": "F16", "f32": "F32"}


def test_scan_names_order_shapes_and_bytes(tmp_path):
    made, where = bp.write_packed_checkpoint(str(tmp_path))
    scan = checkpoint.scan_bitnet_packed_dir(str(tmp_path))
    assert (scan.linear_class, scan.use_rms_norm, scan.rms_norm_eps) == ("autobitlinear", False, 1e-6)
    assert scan.quantization_config["quant_method"] == "bitnet"
    # order of first appearance: part 1 holds layers 0 and 2, part 2 layer 1; the embedding, the norms and lm_head are no layers
    assert [L.name for L in scan.layers] == [bp.CKPT_LAYERS[i][0] for i in (0, 2, 1)]
    by_name = {c[0]: c for c in bp.CKPT_LAYERS}
    for L in scan.layers:
        _, _, Mw, K, form, shape, _ = by_name[L.name]
        lv, packed, stored, v = made[L.name]
        fn, b, e = where[L.name + ".weight"]
        assert (L.Mw, L.K, L.weight.shape, L.weight.dtype) == (Mw, K, (Mw // 4, K), "U8")
        assert (L.weight.path, L.weight.begin, L.weight.end) == (fn, b, e)
        assert (L.weight_scale.dtype, L.weight_scale.shape) == (ST[form], shape)
        assert (L.weight_scale.path, L.weight_scale.begin, L.weight_scale.end) == where[L.name + ".weight_scale"]
        got = np.array(checkpoint.read_tensor(L.weight))
        assert got.dtype == np.uint8 and np.array_equal(got, packed)                       # the file's bytes
        assert np.array_equal(convert.unpack_bitnet_packed(got)[0], lv)
        ws = np.array(checkpoint.read_tensor(L.weight_scale._replace(shape=(1,))))        # BF16: its 16-bit word
        assert ws.dtype == stored.dtype and np.array_equal(pc.raw_bits(ws), pc.raw_bits(stored))
        assert convert.bitnet_packed_scale(ws, "autobitlinear") == v


def test_linear_class_both_values_and_the_default(tmp_path):
    for key, lc, want in (("auto", "autobitlinear", "autobitlinear"), ("bit", "bitlinear", "bitlinear"), ("absent", None, "bitlinear")):
        d = tmp_path / key
        d.mkdir()
        bp.write_packed_checkpoint(str(d), linear_class=lc)
        assert checkpoint.scan_bitnet_packed_dir(str(d)).linear_class == want


def test_use_rms_norm_is_carried(tmp_path):
    bp.write_packed_checkpoint(str(tmp_path), quantization_config={"quant_method": "bitnet", "linear_class": "autobitlinear", "use_rms_norm": True,
                                                                    "rms_norm_eps": 1e-5},
                               extra={bp.CKPT_LAYERS[0][0] + ".rms_norm.weight": np.ones(256, np.float16)})
    scan = checkpoint.scan_bitnet_packed_dir(str(tmp_path))
    assert (scan.use_rms_norm, scan.rms_norm_eps) == (True, 1e-5) and len(scan.layers) == 3      # the norm vector is no layer


def test_refusals_name_the_tensor_or_the_field(tmp_path):
    name = bp.CKPT_LAYERS[0][0] + ".weight"
    f16_name = bp.CKPT_LAYERS[1][0] + ".weight"
    cases = {
        "no_qc": (dict(quantization_config=None), ["quant_method", "bitnet"]),
        "method": (dict(quantization_config={"quant_method": "gptq"}), ["quant_method", "'gptq'"]),
        "online": (dict(quantization_config={"quant_method": "bitnet", "quantization_mode": "online"}), ["quantization_mode", "master weights: load_bitnet_dir"]),
        "class": (dict(quantization_config={"quant_method": "bitnet", "linear_class": "fancylinear"}), ["linear_class", "'fancylinear'"]),
        "no_scale": (dict(drop=(name + "_scale",)), [name + "_scale", "missing"]),
        "scale_two": (dict(extra={name + "_scale": np.ones(2, np.float32)}), [name + "_scale", "one element"]),
        "scale_2d": (dict(extra={name + "_scale": np.ones((1, 1), np.float32)}), [name + "_scale", "one element"]),
        "scale_dtype": (dict(extra={name + "_scale": np.ones(1, np.int32)}), [name + "_scale", "I32", "BF16, F16 or F32"]),
        "scale_bytes": (dict(dtype_names={f16_name + "_scale": "F32"}), [f16_name + "_scale", "one element"]),       # two bytes under a 4-byte name
        "ndim": (dict(extra={"model.layers.5.mlp.up_proj.weight": np.ones((2, 4, 8), np.uint8),
                             "model.layers.5.mlp.up_proj.weight_scale": np.ones(1, np.float32)}), ["model.layers.5.mlp.up_proj.weight", "2-D"]),
        "bytes": (dict(extra={"model.layers.6.mlp.up_proj.weight": np.ones((4, 8), np.float16),
                              "model.layers.6.mlp.up_proj.weight_scale": np.ones(1, np.float32)},
                       dtype_names={"model.layers.6.mlp.up_proj.weight": "U8"}), ["model.layers.6.mlp.up_proj.weight", "bytes"]),
        "none": (dict(layers=[]), ["no packed ternary layer"]),
    }
    for key, (kw, words) in cases.items():
        d = tmp_path / key
        d.mkdir()
        bp.write_packed_checkpoint(str(d), **kw)
        with pytest.raises(RuntimeError) as e:
            checkpoint.scan_bitnet_packed_dir(str(d))
        assert all(w in str(e.value) for w in words), (key, str(e.value))


def test_the_master_weight_scanner_still_refuses_the_directory(tmp_path):
    bp.write_packed_checkpoint(str(tmp_path))
    name = bp.CKPT_LAYERS[0][0] + ".weight"
    with pytest.raises(RuntimeError) as e:
        checkpoint.scan_bitnet_dir(str(tmp_path))
    assert str(e.value) == "{} comes with {}_scale: a pre-packed ternary checkpoint, not master weights".format(name, name)
    assert len(checkpoint.scan_bitnet_packed_dir(str(tmp_path)).layers) == 3
