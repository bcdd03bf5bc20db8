"""GPU: GGUF files in llama.cpp's k-quant layouts, loaded with runtime.load_model (the path a user takes).
  * Q5_K (ggml type 13) as a decode GEMV format: lossless repack, GEMV at the existing GGUF bar, slim and generic kernels;
  * block-quantised token_embd (Q8_0 / Q4_K / Q5_K / Q6_K) kept as raw rows: the gathered rows are ggml's dequantisation bit for bit;
  * tied files (no output.weight): the lm_head is a repacked copy of the quantised table;
  * whole Q4_K_M / Q5_K_M / Q4_K_S-shaped models against the CPU oracle, and the decode / graph / paged / batched paths against each other.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import kquant_ref as kq
from blazr_amd import _lib as L
from blazr_amd import runtime, synth
from oracle import orc_py

pytestmark = pytest.mark.gpu

BAR = 1e-5          # relative L2 per logit row vs the oracle
PATH_BAR = 2e-5     # batched prompt rows vs token-by-token (test_gpu_gguf_prefill.py)
SHORT = {"q": "self_attn.q_proj", "k": "self_attn.k_proj", "v": "self_attn.v_proj", "o": "self_attn.o_proj", "gate": "mlp.gate_proj",
         "up": "mlp.up_proj", "down": "mlp.down_proj"}
MISTRAL2 = dict(preset="mistral-7b-q4km", n_layers=2, vocab=8192, max_seq_len=256)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


_FILES = {}


def _file(tmp_path_factory, key, ftype, **kw):
    if key not in _FILES:
        model = kq.make_model(ftype, **kw)
        path = str(tmp_path_factory.mktemp("kq") / (key + ".gguf"))
        kq.write_gguf(path, model)
        _FILES[key] = (model, path)
    return _FILES[key]


def _load(device, model, path):
    lm = runtime.load_model(device, path)
    for i, lay in enumerate(model["layers"]):
        for short, nm in SHORT.items():
            lm._shapes["model.layers.%d.%s.weight" % (i, nm)] = (lay[short]["N"], lay[short]["K"])
    return lm


def _name(i, short):
    return "model.layers.%d.%s.weight" % (i, SHORT[short])


# ---- 1. the repack is lossless ------------------------------------------------------------------------------------------------------------------
def test_q5k_repack_lossless(device, tmp_path_factory):
    model, path = _file(tmp_path_factory, "q5km", "q5_k_m")
    lm = _load(device, model, path)
    n = 0
    for i, lay in enumerate(model["layers"]):
        for short in SHORT:
            spec = lay[short]
            if spec["ggml_type"] != kq.GGML_Q5_K:
                continue
            got = lm.dequant(_name(i, short))
            want = kq.q5k_dequant(spec["blocks"], spec["N"], spec["K"])
            assert np.array_equal(got, want), (i, short, np.abs(got - want).max())
            n += 1
    assert n >= 40


# ---- 2. Q5_K GEMV -------------------------------------------------------------------------------------------------------------------------------
def _x(K, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((3, K)).astype(np.float32)
    x[1] *= 50.0
    x[2, ::5] = 0.0
    return x


@pytest.mark.parametrize("short", ["q", "o", "gate", "down"])
def test_q5k_gemv_tiny(device, tmp_path_factory, short):
    model, path = _file(tmp_path_factory, "q5km", "q5_k_m")
    lm = _load(device, model, path)
    spec = model["layers"][1][short]
    assert spec["ggml_type"] == kq.GGML_Q5_K
    x = _x(spec["K"], 6)
    want = x.astype(np.float64) @ kq.q5k_dequant(spec["blocks"], spec["N"], spec["K"]).astype(np.float64).T
    got = lm.quant_matmul(_name(1, short), x)
    tol = 3e-6 * np.abs(want).max() + 1e-7
    assert np.abs(got - want).max() <= tol, (np.abs(got - want).max(), tol)


@pytest.mark.watchdog(600)
def test_q5k_gemv_mistral_widths(device, tmp_path_factory):
    model, path = _file(tmp_path_factory, "q5km_mistral", "q5_k_m", **MISTRAL2)
    lm = _load(device, model, path)
    for short in ("o", "gate", "down"):        # 4096x4096, 14336x4096, 4096x14336
        spec = model["layers"][1][short] if short != "down" else model["layers"][0]["down"]
        layer = 1 if short != "down" else 0
        if spec["ggml_type"] != kq.GGML_Q5_K:
            layer, spec = 1 - layer, model["layers"][1 - layer][short]
        assert spec["ggml_type"] == kq.GGML_Q5_K, short
        x = _x(spec["K"], 7)
        want = x.astype(np.float64) @ kq.q5k_dequant(spec["blocks"], spec["N"], spec["K"]).astype(np.float64).T
        got = lm.quant_matmul(_name(layer, short), x)
        tol = 3e-6 * np.abs(want).max() + 1e-7
        assert np.abs(got - want).max() <= tol, (short, np.abs(got - want).max(), tol)


# ---- 3. the embedding gather is exact -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("etype", [kq.GGML_Q8_0, kq.GGML_Q4_K, kq.GGML_Q5_K, kq.GGML_Q6_K])
@pytest.mark.parametrize("vocab", [1024, 1000])
def test_quantised_embedding_rows_exact(device, tmp_path, etype, vocab):
    model = kq.make_model("q4_k_m", embed_type=etype, vocab=vocab, n_layers=2)
    path = str(tmp_path / "e.gguf")
    kq.write_gguf(path, model)
    lm = _load(device, model, path)
    V = vocab
    toks = [0, 1, V - 1] + [int(t) for t in np.random.default_rng(3).integers(0, V, 13)]
    got = lm.forward_embed(toks).to_numpy().reshape(len(toks), -1)
    table = kq.dequant(model["embed"])
    assert np.array_equal(got, table[toks])


# ---- 4 / 5. whole models vs the oracle ----------------------------------------------------------------------------------------------------------
def _vs_oracle(device, model, path, S=12, steps=8, ngen=16):
    cfg = model["config"]
    lm = _load(device, model, path)
    om = orc_py.OrcLlama(kq.oracle_model(model))
    p = [int(t) for t in synth.prompt_tokens(S, cfg["vocab"], seed=31)]
    kv = lm.new_kv_cache(S + steps + 4)
    okv = om.new_kv(S + steps + 4)
    got = np.stack([lm.forward_with_kv_cache([t], kv, i).to_numpy().reshape(-1) for i, t in enumerate(p)])
    want = om.forward_kv(p, okv, 0, all_logits=True).reshape(S, -1)
    per = [_rel(got[i], want[i]) for i in range(S)]
    tok = int(want[-1].argmax())
    for i in range(steps):                                    # teacher-forced: the oracle's token feeds both
        g = lm.forward_with_kv_cache([tok], kv, S + i).to_numpy().reshape(-1)
        o = om.forward_kv([tok], okv, S + i).reshape(-1)
        per.append(_rel(g, o))
        tok = int(o.argmax())
    orc_py.lib().orc_kv_free(okv)
    assert max(per) <= BAR, per
    ids = list(runtime.Executor(lm).generate(p, ngen))
    want_ids, trace = om.generate(p, ngen, trace=True)
    srt = np.sort(trace, axis=1)
    ties = [i for i in range(ngen) if srt[i, -1] - srt[i, -2] < 1e-4 * max(1.0, float(np.abs(trace[i]).max()))]
    upto = ties[0] if ties else ngen              # ids agree up to the first near-tie of the oracle's top two, if any
    assert ids[:upto] == list(want_ids)[:upto], (ids, list(want_ids), ties)
    return lm


def test_q5_k_m_vs_oracle(device, tmp_path_factory):
    model, path = _file(tmp_path_factory, "q5km", "q5_k_m")
    types = {lay[s]["ggml_type"] for lay in model["layers"] for s in SHORT}
    assert types == {kq.GGML_Q5_K, kq.GGML_Q6_K} and model["embed"]["ggml_type"] == kq.GGML_Q5_K
    _vs_oracle(device, model, path)


def test_q4_k_m_vs_oracle(device, tmp_path_factory):
    model, path = _file(tmp_path_factory, "q4km", "q4_k_m")
    assert model["embed"]["ggml_type"] == kq.GGML_Q4_K
    _vs_oracle(device, model, path)


def test_q4_k_s_vs_oracle(device, tmp_path_factory):
    model, path = _file(tmp_path_factory, "q4ks", "q4_k_s")
    assert model["layers"][0]["v"]["ggml_type"] == kq.GGML_Q5_K and model["layers"][0]["q"]["ggml_type"] == kq.GGML_Q4_K
    _vs_oracle(device, model, path)


@pytest.mark.watchdog(900)
def test_q5_k_m_mistral_width_vs_oracle(device, tmp_path_factory):
    model, path = _file(tmp_path_factory, "q5km_mistral", "q5_k_m", **MISTRAL2)
    _vs_oracle(device, model, path, ngen=8)


def test_tied_quantised_head_vs_oracle(device, tmp_path):
    model = kq.make_model("q4_k_m", embed_type=kq.GGML_Q6_K, tied=True)
    path = str(tmp_path / "tied.gguf")
    kq.write_gguf(path, model)
    lm = _vs_oracle(device, model, path)
    res, per_tok = lm.weight_bytes()
    cfg = model["config"]
    assert res >= 2 * kq.row_bytes(kq.GGML_Q6_K, cfg["hidden"]) * cfg["vocab"]      # raw table + its repacked lm_head copy


def test_tied_quantised_head_needs_vocab_multiple_of_64(device, tmp_path):
    model = kq.make_model("q4_k_m", embed_type=kq.GGML_Q6_K, tied=True, vocab=1000, n_layers=2)
    path = str(tmp_path / "tied1000.gguf")
    kq.write_gguf(path, model)
    with pytest.raises(L.BlazrHipError) as e:
        runtime.load_model(device, path)
    assert e.value.code == L.E_UNSUPPORTED and "1000" in str(e.value)


# ---- 6. the decode paths agree ------------------------------------------------------------------------------------------------------------------
def test_q5_k_m_paths_agree(device, tmp_path_factory):
    model, path = _file(tmp_path_factory, "q5km", "q5_k_m")
    cfg = model["config"]
    lm = _load(device, model, path)
    p = [int(t) for t in synth.prompt_tokens(12, cfg["vocab"], seed=32)]
    ex = runtime.Executor(lm)
    eager = list(ex.generate(p, 16))
    assert list(ex.generate(p, 16, use_graph=True)) == eager
    assert list(ex.generate(p, 16, paged=True)) == eager
    # 40-token prompt: the batched path (Q5_K split through gq_elem) vs token-by-token, contiguous and paged
    S = 40
    p40 = [int(t) for t in synth.prompt_tokens(S, cfg["vocab"], seed=33)]
    kv_a, kv_b = lm.new_kv_cache(S + 8), lm.new_kv_cache(S + 8)
    got = lm.forward_with_kv_cache(p40, kv_a, 0, all_logits=True).to_numpy().reshape(S, -1)
    step = np.stack([lm.forward_with_kv_cache([t], kv_b, i).to_numpy().reshape(-1) for i, t in enumerate(p40)])
    per = [_rel(got[i], step[i]) for i in range(S)]
    assert np.median(per) <= PATH_BAR and max(per) <= 10 * PATH_BAR, per
    bs = 16
    pk = runtime.LayeredPagedKvCache(device, cfg["n_layers"], 8, bs, cfg["n_kv_heads"], cfg["head_dim"], L.F32)
    pk.set_blocks([5, 1, 6])
    pk.set_seq_len(S)
    gp = lm.forward_with_paged_kv_cache(p40, pk, pk.compute_slot_mapping(0, S), pk.block_table_device_format(), S, 0, all_logits=True)
    gp = gp.to_numpy().reshape(S, -1)
    per = [_rel(gp[i], step[i]) for i in range(S)]
    assert np.median(per) <= PATH_BAR and max(per) <= 10 * PATH_BAR, per
    # three sequences in one forward_paged_batch == each sequence alone
    nseq, per_seq = 3, 2
    pool = runtime.LayeredPagedKvCache(device, cfg["n_layers"], nseq * per_seq, bs, cfg["n_kv_heads"], cfg["head_dim"], L.F32)
    tables = [[i + nseq * j for j in range(per_seq)] for i in range(nseq)]
    prompts = [[int(t) for t in synth.prompt_tokens(n, cfg["vocab"], seed=40 + i)] for i, n in enumerate((5, 9, 3))]
    toks, lens, alone = [], [], []
    for pr, tb in zip(prompts, tables):
        lg = lm.forward_with_paged_kv_cache(pr, pool, [tb[i // bs] * bs + i % bs for i in range(len(pr))], tb, len(pr), 0).to_numpy()
        toks.append(int(lg.reshape(-1).argmax()))
        lens.append(len(pr))
        alone.append(list(ex.generate(pr, 5)))
    outs = [[t] for t in toks]
    for step_i in range(4):
        lens = [n + 1 for n in lens]
        slots = [tb[(n - 1) // bs] * bs + (n - 1) % bs for n, tb in zip(lens, tables)]
        lg = lm.forward_paged_batch(toks, pool, slots, [tb[:(n + bs - 1) // bs] for n, tb in zip(lens, tables)], lens).to_numpy()
        toks = [int(r.argmax()) for r in lg.reshape(nseq, -1)]
        for o, t in zip(outs, toks):
            o.append(t)
    assert outs == alone, (outs, alone)


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[3])
from blazr_amd import runtime, synth
import kquant_ref as kq
dev = runtime.Device(0)
lm = runtime.load_model(dev, sys.argv[1])
p = [int(t) for t in synth.prompt_tokens(6, 8192, seed=34)]
kv = lm.new_kv_cache(16)
np.save(sys.argv[2], np.stack([lm.forward_with_kv_cache([t], kv, i).to_numpy().reshape(-1) for i, t in enumerate(p)]))
dev.close()
"""


@pytest.mark.watchdog(600)
def test_q5k_generic_kernel_matches_slim(tmp_path_factory, tmp_path):
    """BZ_NO_GQ_SLIM=1 (fresh child process) runs every Q5_K launch on the generic kernel: same logits as the slim kernel at the GEMV bar"""
    model, path = _file(tmp_path_factory, "q5km_mistral", "q5_k_m", **MISTRAL2)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = {}
    for name, env in (("slim", {}), ("generic", {"BZ_NO_GQ_SLIM": "1"})):
        f = str(tmp_path / (name + ".npy"))
        e = dict(os.environ)
        e.update(env)
        e["PYTHONPATH"] = root + os.pathsep + e.get("PYTHONPATH", "")
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", _CHILD, path, f, os.path.join(root, "tests")], env=e,
                           capture_output=True, text=True, timeout=270)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[name] = np.load(f)
    per = [_rel(a, b) for a, b in zip(outs["generic"], outs["slim"])]
    assert 0 < max(per) <= BAR, per


# ---- 7. rejection -------------------------------------------------------------------------------------------------------------------------------
def test_q3_k_rejected_naming_type(device, tmp_path):
    model = kq.make_model("q4_k_m", n_layers=2)
    path = str(tmp_path / "q3.gguf")
    kq.write_gguf(path, model)
    kq.patch_tensor_info(path, "blk.0.attn_q.weight", ggml_type=11)
    with pytest.raises(L.BlazrHipError) as e:
        runtime.load_model(device, path)
    assert e.value.code == L.E_UNSUPPORTED and "type 11" in str(e.value)


def test_q5k_extent_past_end_rejected(device, tmp_path):
    model = kq.make_model("q5_k_m", n_layers=2)
    path = str(tmp_path / "trunc.gguf")
    kq.write_gguf(path, model)
    kq.patch_tensor_info(path, "token_embd.weight", offset=os.path.getsize(path) - 1000)
    with pytest.raises(L.BlazrHipError) as e:
        runtime.load_model(device, path)
    assert e.value.code == L.E_INVALID and "past the end" in str(e.value)
