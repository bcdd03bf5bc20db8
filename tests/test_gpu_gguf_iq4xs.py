"""GPU: GGUF files in llama.cpp's IQ4_XS mix (ggml type 23: IQ4_XS linears and token_embd, Q5_K attn_v, Q6_K output).  Repack and embedding gather bit for bit
against the numpy restatement of the block spec; the generic GEMV and the prompt GEMM against float64; whole models against the oracle, which takes IQ4_XS /
Q5_K linears as their f32 dequantisation as in the Q5_K / legacy tests.  The slim GEMV and the fused MLP have no op-level entry (bz_quant_matmul runs the plain
prologue: the generic kernel), so they are held to the oracle and to the generic kernel through decode logits at hidden 2048, at BAR: an indirect and looser
bound than the generic kernel's 3e-6 max|want| against float64."""
import os
import subprocess
import sys

import numpy as np
import pytest

import iq4xs_ref as iq
import kquant_ref as kq
from blazr_amd import _lib as L
from blazr_amd import runtime, synth
from oracle import orc_py
from test_gpu_gguf_legacy import BAR, PATH_BAR, ROOT, SHORT, _CHILD, _load, _name, _rel, _x

pytestmark = pytest.mark.gpu
ORACLE_BAR = 1e-4      # test_gpu_gguf_prefill.py: rows of the split-f16 prompt GEMM against the reference
TINY = dict(n_layers=2, inter=768, n_kv_heads=1)      # k / v: N = 64; q / o / gate: K = 256 (one superblock); down: K = 768
H2048 = dict(preset="mistral-7b-q4km", hidden=2048, n_heads=16, n_kv_heads=4, inter=256, n_layers=1, vocab=8192, max_seq_len=64)      # vocab: _CHILD's tokens
_MODELS = {}


def make_model(inter=None, **over):
    """kquant_ref.make_model's dict in the IQ4_XS mix; `inter` resizes gate / up / down afterwards (also to a K that no k-quant generator takes)"""
    model = kq.make_model("q4_k_m", **over)
    model["embed"] = iq.blocks("embed", model["embed"]["N"], model["embed"]["K"])
    model["config"]["inter"] = inter or model["config"]["inter"]
    for i, lay in enumerate(model["layers"]):
        for s in SHORT:
            N, K = (inter if inter and s in ("gate", "up") else lay[s]["N"]), (inter if inter and s == "down" else lay[s]["K"])
            lay[s] = kq.q5k_blocks("l%d.v" % i, N, K) if s == "v" else iq.blocks("l%d.%s" % (i, s), N, K)
    return model


def dequant(spec):
    return iq.dequant_blocks(spec["blocks"], spec["N"], spec["K"]) if spec["ggml_type"] == iq.GGML_IQ4_XS else kq.dequant(spec)


def oracle_rows(model, tokens):
    dense = lambda s: dict(kind="dense", N=s["N"], K=s["K"], weight=dequant(s)) if s["ggml_type"] in (iq.GGML_IQ4_XS, kq.GGML_Q5_K) else s
    layers = [{k: (dense(v) if isinstance(v, dict) else v) for k, v in lay.items()} for lay in model["layers"]]
    om = orc_py.OrcLlama(dict(config=model["config"], embed=dequant(model["embed"]), final_norm=model["final_norm"], layers=layers,
                              lm_head=dense(model["lm_head"] or model["embed"])))
    okv = om.new_kv(len(tokens) + 8)
    want = om.forward_kv(tokens, okv, 0, all_logits=True).reshape(len(tokens), -1)
    orc_py.lib().orc_kv_free(okv)
    return want


def _file(tmp_path_factory, key, **kw):
    if key not in _MODELS:
        _MODELS[key] = (make_model(**kw), str(tmp_path_factory.mktemp("iq") / (key + ".gguf")))
        kq.write_gguf(_MODELS[key][1], _MODELS[key][0])
    return _MODELS[key]


def test_repack_lossless_and_bytes(device, tmp_path_factory):
    model, path = _file(tmp_path_factory, "tiny", **TINY)
    lm, cfg, n_iq = _load(device, model, path), model["config"], model["config"]["vocab"] * model["config"]["hidden"]
    for i, lay in enumerate(model["layers"]):
        for short in (s for s in SHORT if s != "v"):
            assert np.array_equal(lm.dequant(_name(i, short)), dequant(lay[short])), (i, short)
            n_iq += lay[short]["N"] * lay[short]["K"]
    assert {(lay[s]["N"], lay[s]["K"]) for s in SHORT} >= {(64, 256), (256, 768)}
    # resident weight bytes: the file's own 136 B per 256 weights for every IQ4_XS tensor, + the Q5_K v and the Q6_K head
    rest = sum(kq.row_bytes(kq.GGML_Q5_K, lay["v"]["K"]) * lay["v"]["N"] for lay in model["layers"]) + kq.row_bytes(kq.GGML_Q6_K, cfg["hidden"]) * cfg["vocab"]
    assert lm.weight_bytes()[0] == n_iq // 256 * 136 + rest


def test_embedding_rows_exact(device, tmp_path_factory):
    model, path = _file(tmp_path_factory, "v1000", vocab=1000, n_layers=2)      # not a multiple of 64: the table stays raw, the head is F32
    toks = [0, 1, 999] + [int(t) for t in np.random.default_rng(3).integers(0, 1000, 13)]
    assert np.array_equal(_load(device, model, path).forward_embed(toks).to_numpy().reshape(len(toks), -1), dequant(model["embed"])[toks])


@pytest.mark.parametrize("short", ["q", "k", "o", "gate", "down"])
def test_generic_gemv_vs_float64(device, tmp_path_factory, short):
    model, path = _file(tmp_path_factory, "tiny", **TINY)
    lm, spec = _load(device, model, path), model["layers"][1][short]
    x = _x(spec["K"], 6)
    want = x.astype(np.float64) @ dequant(spec).astype(np.float64).T
    err = np.abs(lm.quant_matmul(_name(1, short), x) - want).max()
    assert err <= 3e-6 * np.abs(want).max() + 1e-7, (short, err, np.abs(want).max())


@pytest.mark.parametrize("S", [17, 64])
def test_prefill_matmul_vs_float64(device, tmp_path_factory, S):
    model, path = _file(tmp_path_factory, "tiny", **TINY)
    lm, spec = _load(device, model, path), model["layers"][0]["down"]      # K = 768: three superblocks
    x = np.random.default_rng(S).standard_normal((S, spec["K"])).astype(np.float32)
    tx, ty = device.tensor(x), device.tensor(np.full((S + 1, spec["N"]), 7.0, np.float32))      # one guard row behind the output
    L.check(L.lib().bz_prefill_matmul(lm.h, _name(0, "down").encode(), tx.h, S, ty.h))
    got, want = ty.to_numpy(), x.astype(np.float64) @ dequant(spec).astype(np.float64).T
    assert np.all(got[S] == 7.0) and max(_rel(got[i], want[i]) for i in range(S)) <= ORACLE_BAR


@pytest.mark.parametrize("S,tied", [(6, False), (40, False), (6, True)])
def test_whole_model_vs_oracle_and_paths(device, tmp_path_factory, S, tied):
    """token-by-token decode and the batched prompt (S = 40: the split-f16 GEMM over gq_elem) against the oracle and each other; graph-replayed and paged decode
    against eager.  tied: no output.weight, the head is the repacked copy of the IQ4_XS token_embd"""
    model, path = _file(tmp_path_factory, "tied" if tied else "tiny", tied=tied, **TINY)
    lm = _load(device, model, path)
    p = [int(t) for t in synth.prompt_tokens(S, model["config"]["vocab"], seed=31)]
    want, kv, kvb = oracle_rows(model, p), lm.new_kv_cache(S + 8), lm.new_kv_cache(S + 8)
    step = np.stack([lm.forward_with_kv_cache([t], kv, i).to_numpy().reshape(-1) for i, t in enumerate(p)])
    rows = lm.forward_with_kv_cache(p, kvb, 0, all_logits=True).to_numpy().reshape(S, -1)
    assert max(_rel(step[i], want[i]) for i in range(S)) <= BAR and max(_rel(rows[i], want[i]) for i in range(S)) <= ORACLE_BAR
    per = [_rel(rows[i], step[i]) for i in range(S)]
    assert np.median(per) <= PATH_BAR and max(per) <= 10 * PATH_BAR, per
    ex = runtime.Executor(lm)
    eager = list(ex.generate(p, 12))
    assert list(ex.generate(p, 12, use_graph=True)) == eager and list(ex.generate(p, 12, paged=True)) == eager


@pytest.mark.watchdog(600)
def test_slim_and_fused_mlp_vs_oracle_and_generic(tmp_path_factory, tmp_path):
    """hidden 2048, one layer: q/k (IQ4_XS) + v (Q5_K), gate/up and the head through the slim kernel's norm prologue, down through SiLU; BZ_GGUF_MLP_FUSION=1 puts
    the MLP on k_mlp_gq<IQ4_XS, IQ4_XS>, BZ_NO_GQ_SLIM=1 every launch on the generic kernel.  Fresh child processes: the switches are read once"""
    model, path = _file(tmp_path_factory, "h2048", **H2048)
    outs = {}
    for name, env in (("slim", {}), ("fused", {"BZ_GGUF_MLP_FUSION": "1"}), ("generic", {"BZ_NO_GQ_SLIM": "1"})):
        e = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **env)
        r = subprocess.run(["timeout", "-k", "10", "150", sys.executable, "-c", _CHILD, str(tmp_path / name) + ".npy", path], env=e, capture_output=True, text=True, timeout=170)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[name] = np.load(str(tmp_path / name) + ".npy")[0]
    want = oracle_rows(model, [int(t) for t in synth.prompt_tokens(6, 8192, seed=34)])      # _CHILD's tokens
    for name in outs:
        assert max(_rel(a, b) for a, b in zip(outs[name], want)) <= BAR, name
    for a, b in (("slim", "generic"), ("fused", "generic"), ("fused", "slim")):      # different kernels (not bit-equal), same values
        assert 0 < max(_rel(x, y) for x, y in zip(outs[a], outs[b])) <= BAR, (a, b)


def test_k_not_multiple_of_256_and_truncation_refused(device, tmp_path):
    path = str(tmp_path / "bad.gguf")
    kq.write_gguf(path, make_model(inter=320, n_layers=1))      # ffn_down: K = 320
    with pytest.raises(L.BlazrHipError) as e:
        runtime.load_model(device, path)
    assert e.value.code == L.E_UNSUPPORTED and "K=320" in str(e.value), str(e.value)
    kq.write_gguf(path, make_model(n_layers=1))
    kq.patch_tensor_info(path, "token_embd.weight", offset=os.path.getsize(path) - 1000)
    with pytest.raises(L.BlazrHipError) as e:
        runtime.load_model(device, path)
    assert e.value.code == L.E_INVALID and "past the end" in str(e.value)
