"""LoRA without a GPU: the numpy reference against itself, the PEFT loader's rules through bz_lora_describe (engine/lora.rs:138-257 rule for rule, plus the
refusals), and the two conditions that keep the GPU tests honest -- the gap between adapted and base logits, and the stability of the op-test references."""
import json
import os

import numpy as np
import pytest

from blazr_amd import _lib as L
from blazr_amd import runtime
import lora_cases
import lora_ref
import npref

BARS = {"tiny-awq": 1.5e-3, "tiny-awq-hd128": 1.5e-3, "tiny-bf16": 2.0 ** -7, "tiny-q4km": 1e-5}      # test_gpu_lora.py's bar per model


def _rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def test_zero_b_is_the_base_model_bit_for_bit():
    m = lora_cases.model("tiny-awq")
    ad = lora_cases.make_adapter(m["config"], lora_cases.TARGETS, rank=8, alpha=16.0)
    ad["pairs"] = {k: (A, np.zeros_like(B)) for k, (A, B) in ad["pairs"].items()}
    toks = lora_cases.tokens("tiny-awq")[:4]
    assert np.array_equal(lora_ref.run(lora_ref.LoraLlama(m, ad), toks), lora_ref.run(npref.NpLlama(m), toks))


@pytest.mark.parametrize("key", list(lora_cases.MODELS))
@pytest.mark.parametrize("mask", list(lora_cases.MASKS))
def test_adapter_moves_the_logits_far_beyond_the_bar(key, mask):
    """what makes the GPU model tests fail without the feature: every row at least 10 bars from the base model, the median row 50"""
    r = lora_cases.reference(key, mask)
    gaps = [_rel(r["base"][i], r["ref"][i]) for i in range(lora_cases.N_TOKENS)]
    print("%s / %s: gap min %.3e median %.3e (bar %.1e)" % (key, mask, min(gaps), float(np.median(gaps)), BARS[key]))
    assert min(gaps) >= 10 * BARS[key] and np.median(gaps) >= 50 * BARS[key], (min(gaps), float(np.median(gaps)))


@pytest.mark.parametrize("case", [c["id"] for c in lora_cases.OP_CASES])
def test_op_references_do_not_depend_on_the_summation_order(case):
    """the exact sums, a float64 accumulation in index order and one in reversed order give the same bits on every op-test input: what licenses the GPU's
    bit-for-bit comparison (its double accumulators add in yet another order)"""
    want = lora_cases.op_expected(case)
    assert np.array_equal(lora_cases.op_expected(case, "fwd"), want)
    assert np.array_equal(lora_cases.op_expected(case, "rev"), want)
    inp = lora_cases.op_inputs(case)
    on = [i for i, s in enumerate(inp["slots"]) if s >= 0]
    assert not np.array_equal(want[on], inp["base"][on])      # the adapters do something on these inputs


def test_scaling_is_f32():
    assert lora_ref.scaling(8, 16.0) == np.float32(2.0)
    assert lora_ref.scaling(3, 1.0) == np.float32(1.0) / np.float32(3.0)
    assert lora_ref.scaling(8, 16.0, True) == np.float32(16.0) / np.sqrt(np.float32(8.0))


# ---- loader rules (bz_lora_describe: host only) ---------------------------------------------------------------------------------------
@pytest.fixture()
def small():
    cfg = lora_cases.op_config("f16")
    return lora_cases.make_adapter(cfg, ("q", "v"), rank=4, alpha=8.0, layers=[0, 1])


def _refused(path, code, *words):
    with pytest.raises(L.BlazrHipError) as e:
        runtime.lora_describe(path)
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_describe_directory_and_file(tmp_path, small):
    d = lora_cases.write_peft_dir(str(tmp_path / "a"), small)
    for p in (d, os.path.join(d, "adapter_model.safetensors")):
        info = runtime.lora_describe(p)
        assert info["rank"] == 4 and info["alpha"] == 8.0 and info["use_rslora"] is False and info["scaling"] == 2.0
        assert sorted(info["pairs"]) == sorted(small["pairs"])                      # "base_model." stripped, ".lora_{A,B}.weight" stripped
        assert info["pairs"]["model.layers.1.self_attn.v_proj"] == {"dtype": "F16", "rank": 4, "in": 256, "out": 128}


def test_describe_config_rank_wins_and_alpha_defaults(tmp_path, small):
    d = lora_cases.write_peft_dir(str(tmp_path / "a"), small, config=dict(r=16, lora_alpha=8))
    info = runtime.lora_describe(d)
    assert info["rank"] == 16 and info["scaling"] == 0.5 and info["pairs"]["model.layers.0.self_attn.q_proj"]["rank"] == 4
    for kw in (dict(config=False), dict(config_text="{ not json")):                 # no config, unparseable config: rank from lora_A, alpha = rank
        info = runtime.lora_describe(lora_cases.write_peft_dir(str(tmp_path / ("b%d" % len(kw.get("config_text", "")))), small, **kw))
        assert info["rank"] == 4 and info["alpha"] == 4.0 and info["scaling"] == 1.0
    info = runtime.lora_describe(lora_cases.write_peft_dir(str(tmp_path / "c"), small, config=dict(r=4)))
    assert info["alpha"] == 4.0
    info = runtime.lora_describe(lora_cases.write_peft_dir(str(tmp_path / "d"), small, config=dict(r=4, lora_alpha=8, use_rslora=True)))
    assert info["use_rslora"] is True and info["scaling"] == 4.0


def test_describe_prefix_and_unpaired_a(tmp_path, small):
    d = lora_cases.write_peft_dir(str(tmp_path / "a"), small, prefix="", drop_b=["model.layers.0.self_attn.q_proj"],
                                  extra={"unrelated.weight": np.zeros((2, 2), np.float32)})
    info = runtime.lora_describe(d)
    assert "model.layers.0.self_attn.q_proj" not in info["pairs"] and len(info["pairs"]) == 3       # an A without a B is skipped
    d = lora_cases.write_peft_dir(str(tmp_path / "b"), small, prefix="base_model.model.")
    assert "model.model.layers.0.self_attn.q_proj" in runtime.lora_describe(d)["pairs"]             # only "base_model." is stripped


def test_describe_errors_in_the_reference_words(tmp_path, small):
    os.makedirs(str(tmp_path / "empty"))
    _refused(str(tmp_path / "empty"), L.E_NOTFOUND, "No adapter_model.safetensors found in")
    d = lora_cases.write_peft_dir(str(tmp_path / "noa"), dict(small, pairs={}), extra={"x.weight": np.zeros((2, 2), np.float32)})
    _refused(d, L.E_INVALID, "No lora_A weights found in", "base_model.model.<layer>.lora_A.weight")
    d = lora_cases.write_peft_dir(str(tmp_path / "nob"), small, drop_b=list(small["pairs"]))
    _refused(d, L.E_INVALID, "No complete lora_A + lora_B pairs found in")
    open(str(tmp_path / "bad.safetensors"), "wb").write(b"\x00" * 4)
    _refused(str(tmp_path / "bad.safetensors"), L.E_INVALID, "Failed to open adapter safetensors")


def test_describe_refusals_beyond_the_reference(tmp_path, small):
    for i, (extra, word) in enumerate([(dict(use_dora=True), "use_dora"), (dict(bias="all"), "bias"), (dict(bias="lora_only"), "bias"),
                                       (dict(modules_to_save=["lm_head"]), "modules_to_save")]):
        _refused(lora_cases.write_peft_dir(str(tmp_path / ("c%d" % i)), small, config_extra=extra), L.E_UNSUPPORTED, word)
    runtime.lora_describe(lora_cases.write_peft_dir(str(tmp_path / "ok"), small, config_extra=dict(use_dora=False, bias="none", modules_to_save=None)))
    A, B = small["pairs"]["model.layers.0.self_attn.q_proj"]
    for i, name in enumerate(("lm_head", "model.embed_tokens")):
        pairs = dict(small["pairs"])
        pairs[name] = (A, B)
        _refused(lora_cases.write_peft_dir(str(tmp_path / ("h%d" % i)), dict(small, pairs=pairs)), L.E_UNSUPPORTED, name)
    pairs = dict(small["pairs"])
    pairs["model.layers.0.self_attn.q_proj"] = (A, np.zeros((B.shape[0], 6), B.dtype))
    _refused(lora_cases.write_peft_dir(str(tmp_path / "rk"), dict(small, pairs=pairs)), L.E_UNSUPPORTED, "model.layers.0.self_attn.q_proj", "rank 4", "rank 6")


def test_peft_writer_round_trips_the_values(tmp_path, small):
    """the directory the GPU tests load holds the adapter's stored values"""
    d = lora_cases.write_peft_dir(str(tmp_path / "a"), small)
    info = runtime.safetensors_describe(os.path.join(d, "adapter_model.safetensors"))
    assert info["tensors"]["base_model.model.layers.0.self_attn.q_proj.lora_A.weight"]["shape"] == [4, 256]
    assert json.load(open(os.path.join(d, "adapter_config.json")))["r"] == 4
