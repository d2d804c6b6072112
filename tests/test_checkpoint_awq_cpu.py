"""scan_awq_dir on a synthetic two-part AutoAWQ checkpoint (no GPU, no tensor loaded): what it finds, what it skips, and every refusal,
each naming its field or tensor; the GPTQ and dense loaders send an AWQ directory to load_awq_dir."""
import numpy as np
import pytest

import awq_common as ac
from tmac_amd import checkpoint

Q, D = "model.layers.0.self_attn.q_proj", "model.layers.0.mlp.down_proj"
LAYERS = [(Q, 41, 64, 256, 128), (D, 42, 32, 384, 128)]


def test_scan_finds_the_triples_their_biases_and_the_dense_layers(tmp_path):
    tensors = ac.write_awq_checkpoint(str(tmp_path), LAYERS, biases=(Q,))
    scan = checkpoint.scan_awq_dir(str(tmp_path))
    assert [L.name for L in scan.layers] == [Q, D]
    assert [(L.K, L.Mw, L.group_size) for L in scan.layers] == [(256, 64, 128), (384, 32, 128)]
    assert scan.layers[0].bias is not None and scan.layers[0].bias.shape == (64,) and scan.layers[0].bias.dtype == "F16"
    assert scan.layers[1].bias is None
    assert sorted(scan.skipped) == ["lm_head", "model.layers.0.mlp.gate"]          # dense: no .qweight; the 1-D norm is no matrix
    assert scan.quantization_config["version"] == "gemm"
    for L in scan.layers:
        for suffix, ref in ((".qweight", L.qweight), (".scales", L.scales), (".qzeros", L.qzeros)):
            assert np.array_equal(checkpoint.read_tensor(ref), tensors[L.name + suffix])
    assert np.array_equal(checkpoint.read_tensor(scan.layers[0].bias), tensors[Q + ".bias"])
    # the version is matched without regard to case; group_size -1 is one group per row
    ac.write_awq_checkpoint(str(tmp_path), LAYERS, config={"version": "GEMM"})
    assert len(checkpoint.scan_awq_dir(str(tmp_path)).layers) == 2
    d = tmp_path / "rowwise"
    d.mkdir()
    ac.write_awq_checkpoint(str(d), [(Q, 41, 64, 256, 256)], config={"group_size": -1})
    assert checkpoint.scan_awq_dir(str(d)).layers[0].group_size == 256


def refused(tmp_path, key, words, **kw):
    d = tmp_path / key
    d.mkdir()
    ac.write_awq_checkpoint(str(d), LAYERS, **kw)
    with pytest.raises(RuntimeError) as e:
        checkpoint.scan_awq_dir(str(d))
    assert all(w in str(e.value) for w in words), (key, str(e.value))


def test_refusals_name_the_field(tmp_path):
    refused(tmp_path, "method", ["quant_method", "gptq", "awq"], config={"quant_method": "gptq"})
    for v in ("gemv", "GEMV_FAST", "marlin"):
        refused(tmp_path, "version_" + v, ["version", v, "gemv", "gemv_fast", "marlin"], config={"version": v})
    refused(tmp_path, "bits", ["bits", "3"], config={"bits": 3})
    refused(tmp_path, "sym", ["zero_point"], config={"zero_point": False})
    refused(tmp_path, "gs", ["group_size", "64", Q + ".scales"], config={"group_size": 64})


def test_refusals_name_the_tensor(tmp_path):
    (qw, sc, qz), _ = ac.make_awq(41, 64, 256, 128, np.float16, hard=False)
    refused(tmp_path, "no_scales", [Q + ".scales", "missing"], drop=(Q + ".scales",))
    refused(tmp_path, "no_qzeros", [D + ".qzeros", "missing"], drop=(D + ".qzeros",))
    refused(tmp_path, "qw_dtype", [Q + ".qweight", "dtype", "F32"], replace={Q + ".qweight": qw.view(np.float32)})
    refused(tmp_path, "qz_dtype", [Q + ".qzeros", "dtype", "F16"], replace={Q + ".qzeros": np.zeros((2, 16), np.float16)})
    refused(tmp_path, "sc_dtype", [Q + ".scales", "dtype", "BF16"], dtype_names={Q + ".scales": "BF16"})
    refused(tmp_path, "sc_dtype_i32", [Q + ".scales", "dtype", "I32"], replace={Q + ".scales": np.zeros((2, 64), np.int32)})
    refused(tmp_path, "qw_shape", [Q + ".qweight", "shapes"], replace={Q + ".qweight": qw[:, :4]})                  # Mw / 8 against the scales' Mw
    refused(tmp_path, "qz_shape", [Q + ".qweight", "qzeros", "shapes"], replace={Q + ".qzeros": qz[:1]})
    refused(tmp_path, "sc_rank", [Q + ".scales", "shape"], replace={Q + ".scales": sc.reshape(-1)})
    refused(tmp_path, "bytes", [Q + ".qzeros", "bytes"], replace={Q + ".qzeros": np.zeros(qz.shape, np.float16)}, dtype_names={Q + ".qzeros": "I32"})
    refused(tmp_path, "bias", [Q + ".bias", "shape"], replace={Q + ".bias": np.zeros(8, np.float16)}, biases=(Q,))


def test_a_directory_without_awq_layers(tmp_path):
    ac.write_awq_checkpoint(str(tmp_path), LAYERS, drop=tuple(n + s for n in (Q, D) for s in (".qweight", ".scales", ".qzeros")))
    with pytest.raises(RuntimeError, match="no AWQ layer"):
        checkpoint.scan_awq_dir(str(tmp_path))


def test_the_other_loaders_name_load_awq_dir(tmp_path):
    ac.write_awq_checkpoint(str(tmp_path), LAYERS)
    with pytest.raises(RuntimeError) as e:
        checkpoint.load_gptq_dir(str(tmp_path), None)
    assert "AWQ" in str(e.value) and "load_awq_dir" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        checkpoint.scan_dense_dir(str(tmp_path))
    assert all(w in str(e.value) for w in ("quantization_config", "awq", "load_awq_dir"))
