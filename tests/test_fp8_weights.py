"""FP8 (E4M3) weight checkpoints, the parts that need no GPU: the exact f32 restatement the CPU oracle runs, checkpoint detection and refusals from
config.json, the on-disk form as the loader's SafeTensors reader sees it, the ABI symbol."""
import json

import numpy as np
import pytest

from blazr_amd import _lib as L
from blazr_amd import runtime, synth
from oracle import orc_py
import ckpt_writer as W
import fp8_cases as F


def test_synth_encoder_is_the_pinned_quantiser():
    """synth.e4m3_encode / e4m3_table against the numpy side pinned by tests/test_kv_fp8.py"""
    import kv_fp8_ref
    x = (np.random.default_rng(3).standard_normal(200000) * 150.0).astype(np.float32)
    x[:8] = [0.0, -0.0, 448.0, -448.0, 1e9, 2.0 ** -10, 2.0 ** -9 * 1.5, 2.0 ** -9 * 2.5]     # clamp, ties on the subnormal grid
    assert np.array_equal(synth.e4m3_encode(x), kv_fp8_ref.quant(x, 0))
    t = synth.e4m3_table()
    fin = F.FINITE_CODES
    assert np.array_equal(t[fin], F.TABLE[fin]) and np.isnan(t[0x7F]) and np.isnan(t[0xFF])
    assert np.array_equal(synth.e4m3_encode(t[fin]), fin)      # every finite code round-trips


@pytest.mark.parametrize("strategy", ["channel", "tensor"])
def test_restate_f32_is_exact_and_the_oracle_linear_is_the_float64_product(strategy):
    spec = synth.fp8_linear("model.layers.0.mlp.down_proj", 128, 704, strategy, bias=True)
    assert spec["weight"].dtype == np.uint8 and ((spec["weight"] & 0x7F) != 0x7F).all()
    s = spec["scale"]
    assert s.size == (128 if strategy == "channel" else 1)
    assert np.array_equal(synth._repr(s, "bf16"), s)                       # 8 significant bits
    d = F.restate_linear(spec)
    assert d["kind"] == "dense" and d["weight"].dtype == np.float32
    assert np.array_equal(d["weight"].astype(np.float64), F.weight_f64(spec))
    x = synth._repr(np.random.default_rng(5).standard_normal((3, 704)).astype(np.float32), "bf16")
    got = orc_py.OrcLinear(d).forward(x)
    want = (x.astype(np.float64) @ F.weight_f64(spec).T).astype(np.float32) + d["bias"]       # the oracle's own rounding: one to f32, then the bias in f32
    assert np.array_equal(got, want)


def test_restate_f32_covers_every_linear_of_a_model():
    m = F.make("tiny-fp8-channel-bf16")
    r = F.restate_f32(m)
    kinds = {lay[k]["kind"] for lay in m["layers"] for k in ("q", "k", "v", "o", "gate", "up", "down")}
    assert kinds == {"fp8"}
    assert all(lay[k]["kind"] == "dense" and lay[k]["weight"].dtype == np.float32 for lay in r["layers"] for k in ("q", "k", "v", "o", "gate", "up", "down"))
    assert m["layers"][0]["q"]["kind"] == "fp8"                            # the input is left as it was
    assert synth.PRESETS["tiny-fp8"]["hidden"] == synth.PRESETS["tiny-bf16"]["hidden"] and synth.PRESETS["llama3.1-8b-fp8"]["inter"] == synth.PRESETS["llama3-8b-awq"]["inter"]


BASE = dict(model_type="llama", vocab_size=1024, hidden_size=256, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, intermediate_size=512,
            torch_dtype="bfloat16")


def _ct(weights, fmt="float-quantized"):
    return dict(quant_method="compressed-tensors", format=fmt, ignore=["lm_head"], config_groups=dict(group_0=dict(targets=["Linear"], weights=weights)))


def test_config_detection_fp8_and_compressed_tensors():
    """Without the feature the quant method of both reads 0 (None)."""
    c, q = runtime.config_from_hf_json(json.dumps(dict(BASE, quantization_config=dict(quant_method="fp8", activation_scheme="dynamic"))))
    assert q["quant_method"] == "fp8" and c.act_dtype == L.BF16            # FP8 checkpoints keep their torch_dtype (AWQ / GPTQ force f16)
    c, q = runtime.config_from_hf_json(json.dumps(dict(BASE, torch_dtype="float16", quantization_config=dict(quant_method="fp8", activation_scheme="static"))))
    assert q["quant_method"] == "fp8" and c.act_dtype == L.F16
    for strategy in ("tensor", "channel"):
        c, q = runtime.config_from_hf_json(json.dumps(dict(BASE, quantization_config=_ct(dict(num_bits=8, type="float", strategy=strategy)))))
        assert q["quant_method"] == "fp8" and c.act_dtype == L.BF16
    c, q = runtime.config_from_hf_json(json.dumps(dict(BASE, quantization_config=F.quantization_config("compressed-tensors"))))
    assert q["quant_method"] == "fp8"
    _, q = runtime.config_from_hf_json(json.dumps(dict(BASE, quantization_config=dict(quant_method="awq", bits=4, group_size=128))))
    assert q["quant_method"] == "awq"                                      # the existing routes are as they were
    _, q = runtime.config_from_hf_json(json.dumps(BASE))
    assert q["quant_method"] is None


@pytest.mark.parametrize("qc,field", [
    (dict(quant_method="fp8", weight_block_size=[128, 128]), "weight_block_size"),
    (_ct(dict(num_bits=8, type="float", strategy="block", block_structure=[128, 128])), "strategy"),
    (_ct(dict(num_bits=8, type="float", strategy="group", group_size=128)), "strategy"),
    (_ct(dict(num_bits=4, type="int", strategy="group", group_size=128), fmt="pack-quantized"), "format"),
])
def test_config_refusals_name_the_field(qc, field):
    with pytest.raises(L.BlazrHipError) as e:
        runtime.config_from_hf_json(json.dumps(dict(BASE, quantization_config=qc)))
    assert e.value.code == L.E_UNSUPPORTED and field in str(e.value)


def test_fp8_null_block_size_is_not_a_refusal():
    _, q = runtime.config_from_hf_json(json.dumps(dict(BASE, quantization_config=dict(quant_method="fp8", weight_block_size=None))))
    assert q["quant_method"] == "fp8"


@pytest.mark.parametrize("form", ["compressed-tensors", "fp8"])
def test_checkpoint_on_disk_as_the_loader_reads_it(tmp_path, form):
    """The third detection route's evidence (an F8_E4M3 .weight with a .weight_scale beside it) and the .weight_scale_inv the loader refuses are tensor
    facts: bz_safetensors_describe is the loader's reader, so what it lists is what bz_load_model decides on (the decisions themselves need a device:
    tests/test_gpu_fp8_weights.py)."""
    m = F.make("tiny-fp8-channel-bf16" if form == "compressed-tensors" else "tiny-fp8-tensor-bf16")
    F.write_fp8_checkpoint(str(tmp_path), m, form)
    d = runtime.safetensors_describe(str(tmp_path))["tensors"]
    w = d["model.layers.1.mlp.down_proj.weight"]
    assert w["dtype"] == "F8_E4M3" and w["shape"] == [256, 512] and w["bytes"] == 256 * 512
    s = d["model.layers.1.mlp.down_proj.weight_scale"]
    assert (s["dtype"], s["shape"]) == (("BF16", [256, 1]) if form == "compressed-tensors" else ("F32", []))
    assert d["model.layers.1.mlp.down_proj.input_scale"]["shape"] == []
    assert d["model.embed_tokens.weight"]["dtype"] == "BF16"
    _, q = runtime.config_from_hf_json(open(str(tmp_path / "config.json")).read())
    assert q["quant_method"] == "fp8"
    # a block-scaled file: the name the loader refuses is listed as such
    F.write_safetensors(str(tmp_path / "inv.safetensors"), {"model.layers.0.mlp.down_proj.weight": F.F8(np.zeros((64, 128), np.uint8)),
                                                            "model.layers.0.mlp.down_proj.weight_scale_inv": np.ones((1, 1), np.float32)})
    assert "model.layers.0.mlp.down_proj.weight_scale_inv" in runtime.safetensors_describe(str(tmp_path / "inv.safetensors"))["tensors"]
    # an F8 tensor whose byte count disagrees with its shape is a malformed file
    hdr = {"w.weight": {"dtype": "F8_E4M3", "shape": [64, 64], "data_offsets": [0, 64 * 64 * 2]}}
    import struct
    h = json.dumps(hdr).encode()
    (tmp_path / "bad.safetensors").write_bytes(struct.pack("<Q", len(h)) + h + bytes(64 * 64 * 2))
    with pytest.raises(L.BlazrHipError):
        runtime.safetensors_describe(str(tmp_path / "bad.safetensors"))


def test_abi_symbol_is_exported():
    """Without the feature the symbol is missing."""
    assert "bz_model_add_fp8" in L.SYMBOLS
    assert hasattr(L.lib(), "bz_model_add_fp8")
    assert L.lib().bz_abi_version() == 4


def test_split_rule_restated():
    assert F.choose_sk(256, 4096) > 1 and F.choose_sk(64, 14336) > 1 and F.choose_sk(64, 64) == 1 and F.choose_sk(1408, 768) == 1 and F.choose_sk(4096, 4096) == 1 and F.choose_sk(2048, 4096) == 4


def test_bytes_per_token_counts_one_byte_per_weight():
    cfg8, cfg16 = synth.make_config("llama3.1-8b-fp8"), synth.make_config("llama3.1-8b-fp8", quant="none")
    b8, b16 = synth.algorithmic_bytes_per_token(cfg8), synth.algorithmic_bytes_per_token(cfg16)
    head = cfg8["vocab"] * cfg8["hidden"] * 2
    assert 0.5 < (b8 - head) / (b16 - head) < 0.51
