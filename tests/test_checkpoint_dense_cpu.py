"""checkpoint.scan_dense_dir without a GPU: a synthetic two-part UNQUANTISED checkpoint (rtn_common.write_dense_checkpoint: F16, BF16 and F32
layers, an embedding, norm vectors and a head that are no layers) -- names, order, shapes, byte ranges, every refusal naming the tensor or
the config key, and that the quantised formats' scanners and this one each refuse the other's directories, the existing ones with the
words they always had.
"""
import numpy as np
import pytest

import bitnet_common as bc
import bitnet_packed_common as bp
import pack_common as pc
import rtn_common as rc
from tmac_amd import checkpoint


def test_scan_names_order_shapes_and_bytes(tmp_path):
    tensors, where = rc.write_dense_checkpoint(str(tmp_path))
    scan = checkpoint.scan_dense_dir(str(tmp_path))
    # order of first appearance: part 1 holds layers 0 and 2, part 2 layer 1
    assert [L.name for L in scan.layers] == [rc.CKPT_LAYERS[i][0] for i in (0, 2, 1)]
    by_name = {n: (Mw, K, src) for n, _, Mw, K, src in rc.CKPT_LAYERS}
    for L in scan.layers:
        Mw, K, src = by_name[L.name]
        fn, b, e = where[L.name + ".weight"]
        assert (L.Mw, L.K, L.weight.shape, L.weight.dtype) == (Mw, K, (Mw, K), bc.ST_NAME[src])
        assert (L.weight.path, L.weight.begin, L.weight.end) == (fn, b, e)
        got = np.array(checkpoint.read_tensor(L.weight))
        want = tensors[L.name + ".weight"]
        assert got.dtype == want.dtype and np.array_equal(pc.raw_bits(got), pc.raw_bits(want))      # BF16: its 16-bit words, as they lie


def test_a_directory_without_config_is_an_unquantised_one(tmp_path):
    rc.write_dense_checkpoint(str(tmp_path), config=False)
    assert len(checkpoint.scan_dense_dir(str(tmp_path)).layers) == 3


def test_refusals_name_the_tensor(tmp_path):
    name = rc.CKPT_LAYERS[0][0] + ".weight"
    cases = {
        "dtype": (dict(dtype_names={name: "I8"}), [name, "I8"]),
        "ndim": (dict(extra={"model.layers.5.mlp.up_proj.weight": np.ones((2, 4, 8), np.float16)}), ["model.layers.5.mlp.up_proj.weight", "2-D"]),
        "bytes": (dict(dtype_names={name: "F32"}), [name, "bytes"]),          # fp16 bytes under a 4-byte name
        "scale": (dict(extra={name + "_scale": np.ones(1, np.float32)}), [name, "weight_scale", "pre-packed"]),
    }
    for key, (kw, words) in cases.items():
        d = tmp_path / key
        d.mkdir()
        rc.write_dense_checkpoint(str(d), **kw)
        with pytest.raises(RuntimeError) as e:
            checkpoint.scan_dense_dir(str(d))
        assert all(w in str(e.value) for w in words), (key, str(e.value))


def test_refusals_name_the_config_key_and_the_loader_to_use(tmp_path):
    cases = {
        "gptq": ({"quantization_config": {"quant_method": "gptq", "bits": 4, "group_size": 128}}, ["quantization_config", "gptq", "load_gptq_dir"]),
        "gptq_v2": ({"quantization_config": {"quant_method": "gptq_v2", "bits": 2}}, ["quantization_config", "load_gptq_dir"]),
        "packed": ({"quantization_config": {"quant_method": "bitnet", "linear_class": "autobitlinear"}}, ["quantization_config", "load_bitnet_packed_dir"]),
        "online": ({"quantization_config": {"quant_method": "bitnet", "quantization_mode": "online"}}, ["quantization_config", "load_bitnet_dir"]),
        "other": ({"quantization_config": {"quant_method": "awq"}}, ["quantization_config", "awq"]),
        "masters": ({"model_type": "bitnet", "weight_bits": 1}, ["weight_bits", "load_bitnet_dir"]),
    }
    for key, (config, words) in cases.items():
        d = tmp_path / key
        d.mkdir()
        rc.write_dense_checkpoint(str(d), config=config)
        with pytest.raises(RuntimeError) as e:
            checkpoint.scan_dense_dir(str(d))
        assert all(w in str(e.value) for w in words), (key, str(e.value))


def test_a_directory_without_layers_or_without_parts_is_refused(tmp_path):
    a, b = tmp_path / "nolayers", tmp_path / "noparts"
    a.mkdir(); b.mkdir()
    rc.write_dense_checkpoint(str(a), layers=[])
    with pytest.raises(RuntimeError, match="_proj.weight"):
        checkpoint.scan_dense_dir(str(a))
    with pytest.raises(RuntimeError, match="safetensors"):
        checkpoint.scan_dense_dir(str(b))


def test_each_scanner_refuses_the_other_formats(tmp_path):
    g, b, p, d = (tmp_path / n for n in ("gptq", "bitnet", "packed", "dense"))
    for x in (g, b, p, d):
        x.mkdir()
    pc.write_gptq_checkpoint(str(g), [("model.layers.0.self_attn.q_proj", 41, 128, 256, 2, 128)])
    bc.write_bitnet_checkpoint(str(b))
    bp.write_packed_checkpoint(str(p))
    rc.write_dense_checkpoint(str(d))
    # the dense scanner refuses every quantised directory, naming where to go instead
    for x, use in ((g, "load_gptq_dir"), (b, "load_bitnet_dir"), (p, "load_bitnet_packed_dir")):
        with pytest.raises(RuntimeError, match=use):
            checkpoint.scan_dense_dir(str(x))
    # ... and the existing scanners refuse a dense one with their own words
    with pytest.raises(RuntimeError, match="GPTQ"):
        checkpoint.scan_gptq_dir(str(d))
    with pytest.raises(RuntimeError, match="weight_bits"):
        checkpoint.scan_bitnet_dir(str(d))
    with pytest.raises(RuntimeError, match="quant_method"):
        checkpoint.scan_bitnet_packed_dir(str(d))
    assert len(checkpoint.scan_dense_dir(str(d)).layers) == 3
