"""Pooled contextual embeddings on the device (bz_pool_rows; bz_embed_kv / _ssm).  The rows an embed call returns are the rows the lm_head reads: checked against
the ALL_LOGITS rows through the lm_head in float64 (batched routes), and against the staged API + a numpy norm on the exact route; the pooled results against the
host definition (bz_pool_spec) of the same call's rows, across a chunk edge."""
import numpy as np
import pytest

import npref
import score_ref as SR
from blazr_amd import _lib as L
from blazr_amd import runtime, synth

pytestmark = pytest.mark.gpu
F = np.float32


# ---- op level ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", SR.POOL_S)
@pytest.mark.parametrize("H", SR.POOL_H)
def test_pool_rows_match_spec(device, S, H):
    h = SR.pool_rows_case(S, H)
    for p in SR.POOLINGS:
        assert np.array_equal(runtime.pool_rows(device, h, p), runtime.pool_spec(h, p)), p
        got, want = runtime.pool_rows(device, h, p, normalize=True), runtime.pool_spec(h, p, normalize=True)
        assert got.shape == want.shape and SR.within_ulp(got, want), p
    if S > 1:
        assert not runtime.pool_rows(device, h, "none", normalize=True)[1].any()     # the zero vector stays zero


def test_pool_rows_refusals(device):
    h = device.tensor(np.zeros((4, 8), F))
    out = device.zeros((8,), L.F32)
    assert L.lib().bz_pool_rows(device.h, h.h, 4, 8, L.EmbedConfig(pooling=7), out.h) == L.E_INVALID and b"pooling = 7" in L.lib().bz_last_error()
    assert L.lib().bz_pool_rows(device.h, h.h, 4, 8, L.EmbedConfig(pooling=L.POOL_NONE), out.h) == L.E_INVALID and b"128" in L.lib().bz_last_error()


# ---- the rows are the rows the head read ------------------------------------------------------------------------------------------------------
def _ulp_act(v, act):
    """spacing of the activation dtype at |v| (f16: 10 fraction bits, subnormals below 2^-14; bf16: 7 fraction bits)"""
    v = np.abs(np.asarray(v, dtype=np.float64))
    frac, emin = (10, -14) if act == "f16" else (7, -126)
    e = np.floor(np.log2(np.maximum(v, 2.0 ** emin)))
    return 2.0 ** (e - frac)


def _lm_head64(model):
    w, act = model["lm_head"]["weight"], model["config"]["act_dtype"]
    return (synth.bf16_bits_to_f32(w) if act == "bf16" else w.astype(F)).astype(np.float64)


def _make(kind, preset, **over):
    return {"llama": synth.make_llama, "mamba2": synth.make_mamba2, "dsv2": synth.make_dsv2}[kind](preset, **over)


def _cache(lm, kind, S):
    return runtime.LayeredSsmState(lm) if kind == "mamba2" else lm.new_kv_cache(S + 8)


def _all_logits(lm, kind, p, S):
    if kind == "mamba2":
        return lm.forward_with_ssm_state(p, _cache(lm, kind, S), all_logits=True).to_numpy().reshape(S, -1)
    return lm.forward_with_kv_cache(p, _cache(lm, kind, S), 0, all_logits=True).to_numpy().reshape(S, -1)


@pytest.mark.parametrize("kind,preset,S", [("llama", "tiny-bf16", 40), ("mamba2", "tiny-mamba2", 24), ("dsv2", "tiny-dsv2", 24)])
def test_embed_rows_are_what_the_head_read(device, kind, preset, S):
    """y = W x in float64 against the ALL_LOGITS row, within ulp_act(|y|) (one rounding of the logit) + sum_k |w_k| ulp_act(|x_k|) (the fused norm of a per-row head
    differs from the row norm by at most one activation ulp) + K 2^-23 sum_k |w_k x_k| (f32 accumulation over K).  Derived, not measured; far below the distance
    between two different rows, which is what this test is for."""
    model = _make(kind, preset)
    act, K = model["config"]["act_dtype"], model["config"]["hidden"]
    lm = runtime.LoadedModel.from_synth(device, model)
    p = synth.prompt_tokens(S, model["config"]["vocab"], seed=51)
    logits = _all_logits(lm, kind, p, S).astype(np.float64)
    cache = _cache(lm, kind, S)
    x = lm.embed(p, cache, 0, pooling="none").astype(np.float64)
    assert x.shape == (S, K)
    if kind != "mamba2":
        assert cache.seq_len() == S
    W = _lm_head64(model)
    y = x @ W.T
    bound = _ulp_act(y, act) + _ulp_act(x, act) @ np.abs(W).T + K * 2.0 ** -23 * (np.abs(x) @ np.abs(W).T)
    err = np.abs(y - logits)
    print("embed rows vs head: worst err / bound = %.3f" % float(np.max(err / bound)))
    assert np.all(err <= bound)
    # what the bound is for: the neighbouring position's row does not pass it (most of its logits are outside)
    assert np.mean(np.abs(y[1:] - logits[:-1]) > bound[1:]) > 0.5


def test_embed_rows_against_the_staged_api(device):
    """tiny-awq (f16 int4) at S = 12 runs the decode kernels' rows: forward_embed -> forward_layers_range(0, L) gives h and prev; the final RMSNorm of h + prev with the
    rounding points of the library's norm (sum of squares carried in double, every step after it rounded to f32, the two products to f16) must agree with
    embed(NONE) within one f16 ulp"""
    model = synth.make_llama("tiny-awq")
    cfg = model["config"]
    S, H = 12, cfg["hidden"]
    lm = runtime.LoadedModel.from_synth(device, model)
    p = synth.prompt_tokens(S, cfg["vocab"], seed=61)
    h, prev = lm.forward_layers_range(lm.forward_embed(p), None, lm.new_kv_cache(S + 8), 0, cfg["n_layers"], 0)
    h, prev = h.to_numpy().reshape(S, H), prev.to_numpy().reshape(S, H)
    v = npref.round_act(h + prev, "f16")
    ss = np.sum((v * v).astype(F).astype(np.float64), axis=1).astype(F)
    ms = (ss.astype(np.float64) / H).astype(F) + F(cfg["rms_eps"])
    rs = (1.0 / np.sqrt(ms.astype(np.float64)).astype(F).astype(np.float64)).astype(F)
    want = npref.round_act(model["final_norm"].astype(F) * npref.round_act(v * rs[:, None], "f16"), "f16")
    got = lm.embed(p, lm.new_kv_cache(S + 8), 0, pooling="none")
    bad = np.abs(got.astype(np.float64) - want) > _ulp_act(want, "f16")
    print("embed vs staged: %d of %d differ at all" % (int(np.count_nonzero(got != want)), got.size))
    assert not bad.any()


# ---- pooled results ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,preset,over,S", [("llama", "tiny-bf16", {}, 40), ("llama", "tiny-bf16", dict(max_seq_len=4096), 2060), ("mamba2", "tiny-mamba2", {}, 520)],
                         ids=["bf16-40", "bf16-2060", "mamba2-520"])
def test_pooled_results_match_spec_of_the_rows(device, kind, preset, over, S):
    """mean across two chunks, cls from the first chunk, last from the second"""
    model = _make(kind, preset, **over)
    lm = runtime.LoadedModel.from_synth(device, model)
    p = synth.prompt_tokens(S, model["config"]["vocab"], seed=71)
    rows = lm.embed(p, _cache(lm, kind, S), 0, pooling="none")
    assert np.array_equal(rows, lm.embed(p, _cache(lm, kind, S), 0, pooling="none"))     # a pure function of the call
    assert len(np.unique(rows, axis=0)) > S // 2
    for pooling in ("mean", "cls", "last"):
        got = lm.embed(p, _cache(lm, kind, S), 0, pooling=pooling)
        assert np.array_equal(got, runtime.pool_spec(rows, pooling)), pooling
        got = lm.embed(p, _cache(lm, kind, S), 0, pooling=pooling, normalize=True)
        assert SR.within_ulp(got, runtime.pool_spec(rows, pooling, normalize=True)), pooling
    assert SR.within_ulp(lm.embed(p, _cache(lm, kind, S), 0, pooling="none", normalize=True), runtime.pool_spec(rows, "none", normalize=True))


def test_embed_refusals(device):
    model = synth.make_llama("tiny-bf16")
    lm = runtime.LoadedModel.from_synth(device, model)
    p = device.tensor(synth.prompt_tokens(12, model["config"]["vocab"], seed=1))
    kv = lm.new_kv_cache(32)
    small = device.zeros((model["config"]["hidden"],), L.F32)
    assert L.lib().bz_embed_kv(lm.h, p.h, 12, kv.h, 0, L.EmbedConfig(pooling=9), small.h) == L.E_INVALID and b"pooling = 9" in L.lib().bz_last_error()
    assert L.lib().bz_embed_kv(lm.h, p.h, 12, kv.h, 0, L.EmbedConfig(pooling=L.POOL_NONE), small.h) == L.E_INVALID
    assert kv.seq_len() == 0


def test_rerank(device):
    """three documents: order and scores are the cosine of the returned mean-pooled vectors"""
    model = synth.make_llama("tiny-bf16")
    lm = runtime.LoadedModel.from_synth(device, model)
    V, H = model["config"]["vocab"], model["config"]["hidden"]
    query = synth.prompt_tokens(9, V, seed=81)
    docs = [synth.prompt_tokens(n, V, seed=82 + i) for i, n in enumerate((14, 30, 11))]
    docs[1][:9] = query                                      # one document starts with the query
    kv = lm.new_kv_cache(64)
    out = runtime.rerank(lm, kv, query, docs)
    vec = lambda t: lm.embed(t, lm.new_kv_cache(64), 0, pooling="mean")
    q = vec(query)
    want = [SR.cosine64(q, vec(d)) for d in docs]
    tol = 3 * H * 2.0 ** -24                                 # three f32 running sums of H products each
    gaps = np.diff(np.sort(want))
    assert np.all(gaps > 2 * tol), want
    assert [e["index"] for e in out] == list(np.argsort(-np.asarray(want), kind="stable"))
    for e in out:
        assert abs(e["relevance_score"] - want[e["index"]]) <= tol, (e, want)
    assert runtime.rerank(lm, kv, query, docs, top_n=1) == out[:1]
