"""Sliding-window attention, the parts that need no GPU: config.json / GGUF metadata -> bz_model_config.sliding_window[_pattern], the struct
layout (the two fields took reserved slots: size and every older offset unchanged), and the numpy references of tests/swa_ref.py."""
import ctypes as C
import json

import numpy as np

from blazr_amd import _lib as L
from blazr_amd import runtime, synth
import ckpt_writer as W
import npref
import swa_ref

BASE = dict(model_type="mistral", hidden_size=256, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, intermediate_size=512,
            vocab_size=1024, max_position_embeddings=32768, torch_dtype="float16")


def _hf(**kw):
    c, _ = runtime.config_from_hf_json(json.dumps(dict(BASE, **kw)))
    return c.sliding_window, c.sliding_window_pattern


def test_hf_json_window():
    assert _hf() == (0, 0)                                   # no key
    assert _hf(sliding_window=None) == (0, 0)                # Mistral v0.2+: null
    assert _hf(sliding_window=4096) == (4096, 0)             # Mistral v0.1
    assert _hf(sliding_window=2047, model_type="phi3") == (2047, 0)
    # Qwen2 ships a window it does not use; with use_sliding_window = true only the layers from max_window_layers on are windowed -- not a
    # scheme the config carries, so anything but "every layer" is window off
    assert _hf(model_type="qwen2", sliding_window=4096, use_sliding_window=False, max_window_layers=28) == (0, 0)
    assert _hf(model_type="qwen2", sliding_window=4096, use_sliding_window=True, max_window_layers=28) == (0, 0)
    assert _hf(model_type="qwen2", sliding_window=4096, use_sliding_window=True, max_window_layers=0) == (4096, 0)
    # Gemma2 alternates windowed and global layers without a key for it; Gemma3 names the period
    assert _hf(model_type="gemma2", sliding_window=4096) == (4096, 2)
    assert _hf(sliding_window=1024, sliding_window_pattern=6) == (1024, 6)
    assert _hf(sliding_window=1024, sliding_window_pattern=1) == (1024, 0)


def test_gguf_window(tmp_path):
    model = synth.make_llama("tiny-q8_0")
    p = str(tmp_path / "plain.gguf")
    W.write_gguf(p, model)
    c, _ = runtime.config_from_gguf(p)
    assert (c.sliding_window, c.sliding_window_pattern) == (0, 0)
    p = str(tmp_path / "win.gguf")
    W.write_gguf(p, model, extra_kv=[("llama.attention.sliding_window", W.GG_U32, 4096)])
    c, _ = runtime.config_from_gguf(p)
    assert (c.sliding_window, c.sliding_window_pattern) == (4096, 0)
    p = str(tmp_path / "gemma2.gguf")
    W.write_gguf(p, model, arch="gemma2", extra_kv=[("gemma2.attention.sliding_window", W.GG_U32, 4096)])
    c, _ = runtime.config_from_gguf(p)
    assert (c.sliding_window, c.sliding_window_pattern) == (4096, 2)


def test_struct_layout_unchanged():
    """the fields took two of the four reserved ints: same size, same offsets of everything before them, and ABI version 4 still"""
    F = L.ModelConfig
    assert L.ABI_VERSION == 4
    assert C.sizeof(F) == 46 * 4
    assert F.mla_softmax_mscale.offset == 41 * 4 and F.rope_beta_fast.offset == 38 * 4 and F.moe_routed_scale.offset == 37 * 4
    assert F.sliding_window.offset == 42 * 4 and F.sliding_window_pattern.offset == 43 * 4 and F.reserved.offset == 44 * 4
    assert F.abi_version.offset == 0 and F.max_seq_len.offset == 9 * 4 and F.rope_theta.offset == 13 * 4
    names = [n for n, _ in F._fields_]
    assert names[-3:] == ["sliding_window", "sliding_window_pattern", "reserved"]


def test_make_config_mirrors_the_field():
    cfg = synth.make_config("tiny-awq")
    assert runtime.make_config(cfg).sliding_window == 0                     # presets carry no window: bench shapes are what they were
    c = runtime.make_config(dict(cfg, sliding_window=16, sliding_window_pattern=2))
    assert (c.sliding_window, c.sliding_window_pattern) == (16, 2)
    assert all("sliding_window" not in p for p in synth.PRESETS.values())


def test_reference_window_semantics():
    model = synth.make_llama("tiny-awq")
    toks = synth.prompt_tokens(20, model["config"]["vocab"], seed=3)
    base = swa_ref.run(npref.NpLlama(model), toks)
    assert np.array_equal(swa_ref.run(swa_ref.SwaLlama(model, window=0), toks), base)
    assert np.array_equal(swa_ref.run(swa_ref.SwaLlama(model, window=20), toks), base)       # W >= context: the base class, bit for bit
    win = swa_ref.run(swa_ref.SwaLlama(model, window=6), toks)
    assert np.array_equal(win[:6], base[:6])                                                 # positions < W see the same keys
    assert all(not np.array_equal(win[i], base[i]) for i in range(6, 20))
    tb = swa_ref.run(npref.NpLlamaTruth(model), toks)
    assert np.array_equal(swa_ref.run(swa_ref.SwaTruth(model, window=32), toks), tb)
    tw = swa_ref.run(swa_ref.SwaTruth(model, window=6), toks)
    assert np.array_equal(tw[:6], tb[:6]) and not np.array_equal(tw[6:], tb[6:])
    # pattern 2: layer 0 windowed, layer 1 global -- differs from both "all windowed" and "none"
    pat = swa_ref.run(swa_ref.SwaLlama(model, window=6, pattern=2), toks)
    assert not np.array_equal(pat[10], win[10]) and not np.array_equal(pat[10], base[10])
    assert swa_ref.layer_window(6, 2, 0) == 6 and swa_ref.layer_window(6, 2, 1) == 0 and swa_ref.layer_window(6, 0, 1) == 6
    assert swa_ref.first_key(10, 4) == 7 and swa_ref.first_key(2, 4) == 0 and swa_ref.first_key(10, 0) == 0


def test_reference_takes_the_window_from_the_config():
    model = synth.make_llama("tiny-awq", sliding_window=6)
    toks = synth.prompt_tokens(12, model["config"]["vocab"], seed=3)
    a = swa_ref.run(swa_ref.SwaLlama(model), toks)
    b = swa_ref.run(swa_ref.SwaLlama(synth.make_llama("tiny-awq"), window=6), toks)
    assert np.array_equal(a, b)
