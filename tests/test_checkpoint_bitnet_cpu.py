"""checkpoint.scan_bitnet_dir without a GPU: a synthetic two-part BitNet checkpoint of master weights (bitnet_common.write_bitnet_checkpoint:
F16, BF16 and F32 layers, an embedding and norm vectors that are no layers, weight_bits in config.json) -- names, order, shapes, byte
ranges, every refusal, and that the GPTQ and the BitNet scanners each refuse the other's directory.
"""
import numpy as np
import pytest

import bitnet_common as bc
import pack_common as pc
from tmac_amd import checkpoint


def test_scan_names_order_shapes_and_bytes(tmp_path):
    tensors, where = bc.write_bitnet_checkpoint(str(tmp_path))
    scan = checkpoint.scan_bitnet_dir(str(tmp_path))
    assert scan.weight_bits == 1
    # order of first appearance: part 1 holds layers 0 and 2, part 2 layer 1
    assert [L.name for L in scan.layers] == [bc.CKPT_LAYERS[i][0] for i in (0, 2, 1)]
    by_name = {n: (Mw, K, src) for n, _, Mw, K, src in bc.CKPT_LAYERS}
    for L in scan.layers:
        Mw, K, src = by_name[L.name]
        fn, b, e = where[L.name + ".weight"]
        assert (L.Mw, L.K, L.weight.shape, L.weight.dtype) == (Mw, K, (Mw, K), bc.ST_NAME[src])
        assert (L.weight.path, L.weight.begin, L.weight.end) == (fn, b, e)
        got = np.array(checkpoint.read_tensor(L.weight))
        want = tensors[L.name + ".weight"]
        assert got.dtype == want.dtype and np.array_equal(pc.raw_bits(got), pc.raw_bits(want))      # BF16: its 16-bit words, as they lie


def test_refusals_name_the_tensor(tmp_path):
    name = bc.CKPT_LAYERS[0][0] + ".weight"
    cases = {
        "dtype": (dict(dtype_names={name: "I8"}), ["I8"]),       # (same bytes per element count is not the point: the dtype is refused first)
        "ndim": (dict(extra={"model.layers.5.mlp.up_proj.weight": np.ones((2, 4, 8), np.float16)}), ["model.layers.5.mlp.up_proj.weight", "2-D"]),
        "bytes": (dict(dtype_names={name: "F32"}), [name, "bytes"]),          # fp16 bytes under a 4-byte name
        "scale": (dict(extra={name + "_scale": np.ones(1, np.float32)}), [name, "weight_scale", "pre-packed"]),
    }
    for key, (kw, words) in cases.items():
        d = tmp_path / key
        d.mkdir()
        bc.write_bitnet_checkpoint(str(d), **kw)
        with pytest.raises(RuntimeError) as e:
            checkpoint.scan_bitnet_dir(str(d))
        assert all(w in str(e.value) for w in words + ([name] if key == "dtype" else [])), (key, str(e.value))


def test_config_without_weight_bits_is_refused(tmp_path):
    bc.write_bitnet_checkpoint(str(tmp_path), weight_bits=0)
    with pytest.raises(RuntimeError, match="weight_bits"):
        checkpoint.scan_bitnet_dir(str(tmp_path))


def test_a_directory_without_layers_is_refused(tmp_path):
    bc.write_bitnet_checkpoint(str(tmp_path), layers=[])
    with pytest.raises(RuntimeError, match="_proj.weight"):
        checkpoint.scan_bitnet_dir(str(tmp_path))


def test_each_scanner_refuses_the_other_format(tmp_path):
    g, b = tmp_path / "gptq", tmp_path / "bitnet"
    g.mkdir(); b.mkdir()
    pc.write_gptq_checkpoint(str(g), [("model.layers.0.self_attn.q_proj", 41, 128, 256, 2, 128)])
    bc.write_bitnet_checkpoint(str(b))
    with pytest.raises(RuntimeError, match="weight_bits"):
        checkpoint.scan_bitnet_dir(str(g))
    with pytest.raises(RuntimeError, match="GPTQ"):
        checkpoint.scan_gptq_dir(str(b))
    assert len(checkpoint.scan_gptq_dir(str(g)).layers) == 1 and len(checkpoint.scan_bitnet_dir(str(b)).layers) == 3
