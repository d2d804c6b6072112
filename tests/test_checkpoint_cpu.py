"""tmac_amd/checkpoint.py without a GPU: the parsing half of the GPTQ loader on a synthetic two-part safetensors checkpoint written into
tmp_path (headers with data_offsets, I32 / F16 tensors, a config.json).  The triples must come out with the right shapes, byte ranges
and v1 / v2 decision; act-order checkpoints, a missing scales tensor and BF16 scales are refused, naming the tensor."""
import numpy as np
import pytest

import pack_common as pc
from tmac_amd import checkpoint

LAYERS = [("model.layers.0.self_attn.q_proj", 1, 128, 256, 2, 128), ("model.layers.0.mlp.down_proj", 2, 64, 384, 4, 128),
          ("model.layers.1.self_attn.q_proj", 3, 128, 256, 2, 128)]


def test_scan_finds_the_triples(tmp_path):
    tensors, where = pc.write_gptq_checkpoint(str(tmp_path), LAYERS)
    scan = checkpoint.scan_gptq_dir(str(tmp_path))
    assert scan.gptq_v2 and scan.zero_point
    # parts in file-name order, tensors in header order: layers 0 and 2 lie in part 1, layer 1 in part 2
    assert [L.name for L in scan.layers] == [LAYERS[0][0], LAYERS[2][0], LAYERS[1][0]]
    for L in scan.layers:
        name, _, Mw, K, bits, gs = next(x for x in LAYERS if x[0] == L.name)
        assert (L.Mw, L.K, L.bits, L.group_size) == (Mw, K, bits, gs)
        for ref, suffix, dt in ((L.qweight, ".qweight", "I32"), (L.scales, ".scales", "F16"), (L.qzeros, ".qzeros", "I32")):
            a = tensors[name + suffix]
            assert ref.dtype == dt and ref.shape == a.shape
            assert (ref.path, ref.begin, ref.end) == where[name + suffix]
            got = checkpoint.read_tensor(ref)
            assert got.dtype == a.dtype and np.array_equal(got, a)
        assert L.qweight.shape == (K * bits // 32, Mw) and L.scales.shape == (K // gs, Mw) and L.qzeros.shape == (K // gs, Mw * bits // 32)


@pytest.mark.parametrize("quantizer,method,v2", [("gptqmodel:1.2.3", "gptq", True), (["gptqmodel:1.0.0"], "gptq", True), ("autogptq:0.7", "gptq", False),
                                                 ("", "gptq", False), ("", "gptq_v2", True)])
def test_v1_v2_decision(tmp_path, quantizer, method, v2):
    pc.write_gptq_checkpoint(str(tmp_path), LAYERS[:2], quantizer=quantizer, quant_method=method)
    assert checkpoint.scan_gptq_dir(str(tmp_path)).gptq_v2 == v2


def test_symmetric_checkpoint_has_no_zero_points(tmp_path):
    pc.write_gptq_checkpoint(str(tmp_path), LAYERS[:2], sym=True)
    assert not checkpoint.scan_gptq_dir(str(tmp_path)).zero_point


def test_desc_act_is_refused(tmp_path):
    pc.write_gptq_checkpoint(str(tmp_path), LAYERS[:2], desc_act=True)
    with pytest.raises(AssertionError, match="desc_act"):
        checkpoint.scan_gptq_dir(str(tmp_path))


def test_missing_scales_names_the_tensor(tmp_path):
    victim = LAYERS[1][0] + ".scales"
    pc.write_gptq_checkpoint(str(tmp_path), LAYERS[:2], drop=(victim,))
    with pytest.raises(RuntimeError) as e:
        checkpoint.scan_gptq_dir(str(tmp_path))
    assert victim in str(e.value) and "missing" in str(e.value)


def test_bf16_scales_name_the_tensor(tmp_path):
    victim = LAYERS[0][0] + ".scales"
    pc.write_gptq_checkpoint(str(tmp_path), LAYERS[:2], dtype_names={victim: "BF16"})
    with pytest.raises(RuntimeError) as e:
        checkpoint.scan_gptq_dir(str(tmp_path))
    assert victim in str(e.value) and "BF16" in str(e.value)


def test_offsets_outside_the_file_are_refused(tmp_path):
    import json
    import struct
    _, where = pc.write_gptq_checkpoint(str(tmp_path), LAYERS[:2])
    fn = where[LAYERS[0][0] + ".qweight"][0]
    raw = open(fn, "rb").read()
    (n,) = struct.unpack("<Q", raw[:8])
    hdr = json.loads(raw[8:8 + n])
    hdr[LAYERS[0][0] + ".qweight"]["data_offsets"][1] = len(raw)          # past the end of the data section
    text = json.dumps(hdr).encode()
    open(fn, "wb").write(struct.pack("<Q", len(text)) + text + raw[8 + n:])
    with pytest.raises(RuntimeError, match="corrupt safetensors header"):
        checkpoint.scan_gptq_dir(str(tmp_path))
