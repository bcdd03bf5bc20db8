"""What the whole-model tests of packed prompt batches share (tests/test_gpu_embed_batch.py, tests/test_gpu_score_batch.py): the fixtures, built once per session,
the oracle's rows of every input alone, computed once, and the bars single MFMA prompts are held to."""
import numpy as np

import irregular_cases
import packed_cases as PC
from blazr_amd import runtime, synth
from oracle import orc_py

F = np.float32
_MODELS, _ORC = {}, {}
# name -> how the fixture is made; max_seq_len bounds the longest INPUT (the rotary table), not the packed batch
FIXTURES = {
    "tiny-awq": lambda: synth.make_llama("tiny-awq"),
    "tiny-bf16": lambda: synth.make_llama("tiny-bf16", max_seq_len=2048),
    "tiny-q4km": lambda: synth.make_llama("tiny-q4km"),
    "tiny-dsv2": lambda: synth.make_dsv2("tiny-dsv2"),
    "bf16-g2-w768": lambda: _irregular("bf16-g2-w768", max_seq_len=2048),      # the shapes of irregular_cases, with room for set E's 2040-token input
    "awq-g4-w768": lambda: _irregular("awq-g4-w768", max_seq_len=2048),
    "bf16-g3-hd64": lambda: irregular_cases.make("bf16-g3-hd64"),
}


def _irregular(name, **more):
    preset, over = irregular_cases.CASES[name]
    return synth.make_llama(preset, **dict(over, **more))


def get(device, name):
    """(synth model, LoadedModel, oracle or None)"""
    if name not in _MODELS:
        m = FIXTURES[name]()
        om = None if name == "tiny-dsv2" else orc_py.OrcLlama(m)
        _MODELS[name] = (m, runtime.LoadedModel.from_synth(device, m), om)
    return _MODELS[name]


def scratch(lm, lens):
    """a scratch cache for a packed batch of these lengths: its capacity is the batch, whatever the model's longest context"""
    T = int(np.sum(lens))
    return lm.new_kv_cache(T, max_seq_len=max(T, lm.c.max_seq_len))


def inputs(name, set_name, lens=None):
    lens = PC.SETS[set_name] if lens is None else lens
    return lens, PC.token_lists(lens, VOCAB[name], seed=100 + ord(set_name[0]))


VOCAB = {"tiny-awq": 1024, "tiny-bf16": 1024, "tiny-q4km": 1024, "tiny-dsv2": 1024, "bf16-g2-w768": 1003, "awq-g4-w768": 1001, "bf16-g3-hd64": 1003}


def oracle_rows(device, name, set_name):
    """the oracle's all-logits rows of every input of the set, each run alone from position 0: list of float64 [len_i, vocab]"""
    key = (name, set_name)
    if key not in _ORC:
        _, _, om = get(device, name)
        lens, toks = inputs(name, set_name)
        rows = []
        for t in toks:
            kv = om.new_kv(len(t) + 8)
            rows.append(np.asarray(om.forward_kv([int(x) for x in t], kv, 0, all_logits=True), dtype=np.float64).reshape(len(t), -1))
            orc_py.lib().orc_kv_free(kv)
        _ORC[key] = rows
    return _ORC[key]


def bar(cfg, int4):
    """relative L2 a single MFMA prompt is held to: 1e-3 for f16, 1.25 x 2^-7 for bf16, 1.25e-3 on the int4 MFMA path; twice that on hidden-256 fixtures"""
    base = 1.25e-3 if int4 else (1e-3 if cfg["act_dtype"] == "f16" else 1.25 * 2.0 ** -7)
    return base * (2.0 if cfg["hidden"] == 256 else 1.0)


def rel_l2(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30))


def lm_head64(model):
    w, act = model["lm_head"]["weight"], model["config"]["act_dtype"]
    return (synth.bf16_bits_to_f32(w) if act == "bf16" else w.astype(F)).astype(np.float64)


def log_softmax64(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def rows_equal(a, b):
    """two SCORE_ROW arrays, field for field"""
    return all(np.array_equal(a[n], b[n]) for n in a.dtype.names)
