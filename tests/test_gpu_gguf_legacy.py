"""GPU: GGUF files in llama.cpp's legacy block formats (Q4_0, Q4_1, Q5_0, Q5_1: 32-weight blocks), loaded with runtime.load_model.
  * the load-time repack is lossless (bz_dequant of every linear equals ggml's dequantisation bit for bit);
  * the decode GEMVs meet the existing GGUF bar against a float64 reference, and the slim kernels agree with the generic ones;
  * block-quantised token_embd rows are ggml's dequantisation bit for bit;
  * whole models (tiny, Mistral-width, tied head, Q4_K_M with Q5_0 / Q5_1 v / down) against the CPU oracle, and the decode / graph / paged /
    batched paths against each other;
  * byte accounting equals the k-quant of the same bits per weight; bad shapes and unknown types are rejected.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import kquant_ref as kq
import legacy_quant_ref as lq
from blazr_amd import _lib as L
from blazr_amd import runtime, synth
from oracle import orc_py

pytestmark = pytest.mark.gpu

BAR = 1e-5          # relative L2 per logit row vs the oracle
PATH_BAR = 2e-5     # batched prompt rows vs token-by-token (test_gpu_gguf_prefill.py)
SHORT = lq.SHAPES_HF
MISTRAL2 = dict(preset="mistral-7b-q4km", n_layers=2, vocab=8192, max_seq_len=256)
FORMATS = ["q4_0", "q4_1", "q5_0", "q5_1"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


_FILES = {}


def _file(tmp_path_factory, key, ftype, **kw):
    if key not in _FILES:
        model = lq.make_model(ftype, **kw)
        path = str(tmp_path_factory.mktemp("lq") / (key + ".gguf"))
        lq.write_gguf(path, model)
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
@pytest.mark.parametrize("ftype", FORMATS + ["mixed"])
def test_legacy_repack_lossless(device, tmp_path_factory, ftype):
    model, path = _file(tmp_path_factory, ftype, ftype)
    lm = _load(device, model, path)
    n = 0
    for i, lay in enumerate(model["layers"]):
        for short in SHORT:
            spec = lay[short]
            if spec["ggml_type"] not in lq.LEGACY:
                continue
            got = lm.dequant(_name(i, short))
            want = lq.dequant(spec)
            assert np.array_equal(got, want), (i, short, np.abs(got - want).max())
            n += 1
    assert n == (7 * len(model["layers"]) if ftype != "mixed" else 2 * len(model["layers"]))


# ---- 2. GEMV at the GGUF bar --------------------------------------------------------------------------------------------------------------------
def _x(K, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((3, K)).astype(np.float32)
    x[1] *= 50.0            # a row of large scale
    x[2, ::5] = 0.0         # a row with zeros
    return x


def _check_gemv(lm, name, spec, seed):
    x = _x(spec["K"], seed)
    want = x.astype(np.float64) @ lq.dequant(spec).astype(np.float64).T
    got = lm.quant_matmul(name, x)
    tol = 3e-6 * np.abs(want).max() + 1e-7
    assert np.abs(got - want).max() <= tol, (name, np.abs(got - want).max(), tol)


@pytest.mark.parametrize("ftype", FORMATS)
def test_legacy_gemv_tiny(device, tmp_path_factory, ftype):
    model, path = _file(tmp_path_factory, ftype, ftype)
    lm = _load(device, model, path)
    for short in ("q", "k", "o", "gate", "down"):
        _check_gemv(lm, _name(1, short), model["layers"][1][short], 6)


@pytest.mark.watchdog(900)
@pytest.mark.parametrize("ftype", FORMATS)
def test_legacy_gemv_mistral_widths(device, ftype):
    """4096x4096 (o), 14336x4096 (gate), 4096x14336 (down) of a one-layer Mistral-width model built in memory"""
    model = lq.make_model(ftype, preset="mistral-7b-q4km", n_layers=1, vocab=512, max_seq_len=64)
    model["embed"] = dict(kind="dense", N=512, K=4096, weight=lq.dequant(model["embed"]))
    synth_like = dict(model, embed=model["embed"]["weight"])
    lm = runtime.LoadedModel.from_synth(device, synth_like)
    for short in ("o", "gate", "down"):
        _check_gemv(lm, _name(0, short), model["layers"][0][short], 7)
    del lm


# ---- 3. slim kernels against the generic ones (fresh child processes) ---------------------------------------------------------------------------
_CHILD = r"""
import sys
import numpy as np
from blazr_amd import runtime, synth
dev = runtime.Device(0)
outs = []
for path in sys.argv[2:]:
    lm = runtime.load_model(dev, path)
    p = [int(t) for t in synth.prompt_tokens(6, 8192, seed=34)]
    kv = lm.new_kv_cache(16)
    outs.append(np.stack([lm.forward_with_kv_cache([t], kv, i).to_numpy().reshape(-1) for i, t in enumerate(p)]))
    del kv, lm
np.save(sys.argv[1], np.stack(outs))
dev.close()
"""


@pytest.mark.watchdog(900)
def test_legacy_generic_kernel_matches_slim(tmp_path_factory, tmp_path):
    """BZ_NO_GQ_SLIM=1 runs every launch on the generic kernel: same logits as the slim kernels (q/k/v and gate/up at K = 4096 through the
    norm prologue, down at K = 2048 through SiLU) for each legacy format"""
    paths = []
    for ftype in FORMATS:
        _, path = _file(tmp_path_factory, ftype + "_slimw", ftype, preset="mistral-7b-q4km", n_layers=2, vocab=8192, max_seq_len=64,
                        inter=2048)
        paths.append(path)
    outs = {}
    for name, env in (("slim", {}), ("generic", {"BZ_NO_GQ_SLIM": "1"})):
        f = str(tmp_path / (name + ".npy"))
        e = dict(os.environ)
        e.update(env)
        e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
        r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, "-c", _CHILD, f] + paths, env=e, capture_output=True, text=True,
                           timeout=430)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[name] = np.load(f)
    for fi, ftype in enumerate(FORMATS):
        per = [_rel(a, b) for a, b in zip(outs["generic"][fi], outs["slim"][fi])]
        assert 0 < max(per) <= BAR, (ftype, per)


# ---- 4. the embedding gather is exact -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("etype", lq.LEGACY)
@pytest.mark.parametrize("vocab", [1024, 1000])
def test_legacy_embedding_rows_exact(device, tmp_path, etype, vocab):
    model = lq.make_model("q4_0", embed_type=etype, vocab=vocab, n_layers=2)
    path = str(tmp_path / "e.gguf")
    lq.write_gguf(path, model)
    lm = _load(device, model, path)
    toks = [0, 1, vocab - 1] + [int(t) for t in np.random.default_rng(3).integers(0, vocab, 13)]
    got = lm.forward_embed(toks).to_numpy().reshape(len(toks), -1)
    table = lq.dequant(model["embed"])
    assert np.array_equal(got, table[toks])


# ---- 5. whole models vs the oracle --------------------------------------------------------------------------------------------------------------
def _vs_oracle(device, model, path, S=12, steps=8, ngen=16):
    cfg = model["config"]
    lm = _load(device, model, path)
    om = orc_py.OrcLlama(lq.oracle_model(model))
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


@pytest.mark.parametrize("ftype", FORMATS)
def test_legacy_tiny_vs_oracle(device, tmp_path_factory, ftype):
    model, path = _file(tmp_path_factory, ftype, ftype)
    assert {lay[s]["ggml_type"] for lay in model["layers"] for s in SHORT} == {lq.TYPE_OF[ftype]}
    assert model["embed"]["ggml_type"] == lq.TYPE_OF[ftype] and model["lm_head"]["ggml_type"] == kq.GGML_Q6_K
    _vs_oracle(device, model, path)


@pytest.mark.watchdog(900)
def test_q4_0_mistral_width_vs_oracle(device, tmp_path_factory):
    model, path = _file(tmp_path_factory, "q4_0_mistral", "q4_0", **MISTRAL2)
    _vs_oracle(device, model, path, ngen=8)


def test_tied_q4_0_head_vs_oracle(device, tmp_path):
    model = lq.make_model("q4_0", tied=True)
    path = str(tmp_path / "tied.gguf")
    lq.write_gguf(path, model)
    lm = _vs_oracle(device, model, path)
    res, per_tok = lm.weight_bytes()
    cfg = model["config"]
    assert res >= 2 * lq.row_bytes(lq.GGML_Q4_0, cfg["hidden"]) * cfg["vocab"]      # raw table + its repacked lm_head copy


def test_mixed_q4_k_m_with_q5_0_v_and_q5_1_down_vs_oracle(device, tmp_path_factory):
    model, path = _file(tmp_path_factory, "mixed", "mixed")
    lay = model["layers"][0]
    assert (lay["q"]["ggml_type"], lay["v"]["ggml_type"], lay["down"]["ggml_type"]) == (kq.GGML_Q4_K, lq.GGML_Q5_0, lq.GGML_Q5_1)
    _vs_oracle(device, model, path)


# ---- 6. the decode paths agree ------------------------------------------------------------------------------------------------------------------
def test_q4_0_paths_agree(device, tmp_path_factory):
    model, path = _file(tmp_path_factory, "q4_0", "q4_0")
    cfg = model["config"]
    lm = _load(device, model, path)
    p = [int(t) for t in synth.prompt_tokens(12, cfg["vocab"], seed=32)]
    ex = runtime.Executor(lm)
    eager = list(ex.generate(p, 16))
    assert list(ex.generate(p, 16, use_graph=True)) == eager
    assert list(ex.generate(p, 16, paged=True)) == eager
    # 40-token prompt: the batched path (the legacy split through gq_elem) vs token-by-token, contiguous and paged
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


def test_bz_run_generates_from_a_q4_0_file(device, tmp_path_factory):
    """tools/bz_run.cpp (the C ABI from compiled code) on a *.Q4_0.gguf: the ids Executor.generate gives"""
    model, _ = _file(tmp_path_factory, "q4_0", "q4_0")
    path = str(tmp_path_factory.mktemp("lqrun") / "tiny.Q4_0.gguf")
    lq.write_gguf(path, model)
    exe = os.path.join(ROOT, "blazr_amd", "bz-run")
    p = [int(t) for t in synth.prompt_tokens(9, model["config"]["vocab"], seed=35)]
    want = list(runtime.Executor(runtime.load_model(device, path)).generate(p, 12))
    r = subprocess.run(["timeout", "-k", "10", "100", exe, path, "--prompt", ",".join(str(x) for x in p), "--max-tokens", "12"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [int(x) for x in r.stdout.strip().split(",")] == want, (r.stdout, r.stderr)


# ---- 7. byte accounting -------------------------------------------------------------------------------------------------------------------------
def _retype(model, to):
    """the same shapes with every legacy tensor replaced by blocks of type `to`"""
    def rt(name, spec):
        return kq.blocks(name, to, spec["N"], spec["K"]) if spec["kind"] == "gguf" and spec["ggml_type"] in lq.LEGACY else spec
    layers = [{k: (rt("l%d.%s" % (i, k), v) if isinstance(v, dict) else v) for k, v in lay.items()} for i, lay in enumerate(model["layers"])]
    return dict(model, embed=rt("embed", model["embed"]), layers=layers)


@pytest.mark.parametrize("ftype,kquant", [("q4_0", kq.GGML_Q4_K), ("q5_0", kq.GGML_Q5_K)])
def test_legacy_bytes_equal_the_k_quant_of_the_same_bits(device, tmp_path, ftype, kquant):
    model = lq.make_model(ftype, n_layers=2)
    per = []
    for tag, mdl in (("legacy", model), ("kquant", _retype(model, kquant))):
        path = str(tmp_path / (tag + ".gguf"))
        lq.write_gguf(path, mdl)
        lm = runtime.load_model(device, path)
        per.append(lm.weight_bytes()[1])
        del lm
    assert per[0] == per[1], per


# ---- 8. rejection -------------------------------------------------------------------------------------------------------------------------------
def test_q4_0_k_not_multiple_of_256_rejected_naming_k(device, tmp_path):
    model = lq.make_model("q4_0", n_layers=1, inter=320)          # ffn_down: K = 320 (a multiple of 32, not of 256)
    path = str(tmp_path / "k320.gguf")
    lq.write_gguf(path, model)
    with pytest.raises(L.BlazrHipError) as e:
        runtime.load_model(device, path)
    assert e.value.code == L.E_UNSUPPORTED and "K=320" in str(e.value), str(e.value)


def test_iq4_nl_rejected_naming_type(device, tmp_path):
    model = lq.make_model("q4_0", n_layers=2)
    path = str(tmp_path / "iq4nl.gguf")
    lq.write_gguf(path, model)
    lq.patch_tensor_info(path, "blk.0.attn_q.weight", ggml_type=20)
    with pytest.raises(L.BlazrHipError) as e:
        runtime.load_model(device, path)
    assert e.value.code == L.E_UNSUPPORTED and "type 20" in str(e.value)
