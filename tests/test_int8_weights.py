"""INT8 W8A8 checkpoints, the parts that need no GPU: detection and refusals from config.json, the on-disk form as the loader's SafeTensors reader sees it, the
planted rows of the op tests doing what they claim."""
import json

import numpy as np
import pytest

from blazr_amd import _lib as L
from blazr_amd import runtime
import int8_cases as I

BASE = dict(model_type="llama", vocab_size=1024, hidden_size=256, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, intermediate_size=512)


def _qc(weights=None, drop=None, **act_over):
    qc = I.quantization_config("channel", **act_over)
    qc["config_groups"]["group_0"]["weights"].update(weights or {})
    qc["config_groups"]["group_0"].pop(drop, None)
    return qc


@pytest.mark.parametrize("strategy", ["channel", "tensor"])
@pytest.mark.parametrize("td,act", [("bfloat16", L.BF16), ("float16", L.F16)])
def test_config_detection(strategy, td, act):
    """Without the feature: BZ_E_UNSUPPORTED naming `format`."""
    c, q = runtime.config_from_hf_json(json.dumps(dict(BASE, torch_dtype=td, quantization_config=I.quantization_config(strategy))))
    assert q["quant_method"] == "int8" and c.act_dtype == act          # activations keep torch_dtype


@pytest.mark.parametrize("qc,field", [
    (_qc(dynamic=False), "input_activations.dynamic"),                 # static activation scales
    (_qc(symmetric=False), "input_activations.symmetric"),
    (_qc(strategy="tensor"), "input_activations.strategy"),
    (_qc(num_bits=16), "input_activations: num_bits"),
    (_qc(drop="input_activations"), "input_activations"),              # weight-only int8
    (_qc(dict(symmetric=False)), "weights.symmetric"),
    (_qc(dict(strategy="group", group_size=128)), "weights.strategy"),
    (_qc(dict(strategy="block", block_structure=[128, 128])), "weights.strategy"),
    (_qc(dict(num_bits=4)), "weights: num_bits"),
    (dict(_qc(), format="pack-quantized"), "format"),
])
def test_config_refusals_name_the_field(qc, field):
    with pytest.raises(L.BlazrHipError) as e:
        runtime.config_from_hf_json(json.dumps(dict(BASE, torch_dtype="bfloat16", quantization_config=qc)))
    assert e.value.code == L.E_UNSUPPORTED and field in str(e.value)


@pytest.mark.parametrize("name", list(I.MODELS))
def test_checkpoint_on_disk_as_the_loader_reads_it(tmp_path, name):
    I.write_int8_checkpoint(str(tmp_path), I.make(name), zero_point=0)
    d = runtime.safetensors_describe(str(tmp_path))["tensors"]
    w, s = d["model.layers.1.mlp.down_proj.weight"], d["model.layers.1.mlp.down_proj.weight_scale"]
    assert w["dtype"] == "I8" and w["shape"] == [256, 512] and w["bytes"] == 256 * 512
    assert (s["dtype"], s["shape"]) == (("BF16", [256, 1]) if "channel" in name else ("F32", [1]))
    assert d["model.layers.1.mlp.down_proj.weight_zero_point"]["dtype"] == "I8" and ("model.layers.1.mlp.down_proj.bias" in d) == ("tensor" in name)
    assert runtime.config_from_hf_json(open(str(tmp_path / "config.json")).read())[1]["quant_method"] == "int8"


@pytest.mark.parametrize("act", ["bf16", "f16"])
def test_planted_rows_do_what_they_claim(act):
    K = 704
    x = I.planted_rows(K, act, 1)
    amax, rest = np.abs(x).max(axis=1), np.arange(K) != K // 2
    sx = np.where(amax == 0, 1, amax / np.float32(127)).astype(np.float32)
    codes = np.clip(np.rint(x / sx[:, None]), -127, 127)
    frac, whole = np.modf(np.abs(x[3] / sx[3])[rest])
    assert amax[2] == 0 and (I.ref_linear(x, np.ones((64, K), np.int8), np.ones(1, np.float32))[2] == 0).all()
    assert sx[3] == 0.125 and (frac == 0.5).all() and set(whole.astype(int) % 2) == {0, 1} and (codes[3][rest] % 2 == 0).all()          # ties of both parities go to even
    assert (np.abs(x[4]) < (2.0 ** -126 if act == "bf16" else 2.0 ** -14)).all() and (x[4] != 0).all() and np.abs(codes[4]).max() == 127   # subnormals use the whole range
    assert amax[5] == np.float32(3.3895313892515355e38 if act == "bf16" else 65504.0) and (codes[5] != 0).sum() == 1
    assert np.signbit(x[6, ::2]).all() and (x[6, ::2] == 0).all()

