"""Prompt scoring on the device (bz_score_rows; bz_score_kv / _paged / _ssm).  Op level: the kernels against the host definition (bz_score_row_spec), which
test_score_embed_ref.py pins against numpy.  Model level: a score call against the SAME call on a fresh cache with BZ_FWD_ALL_LOGITS -- every row's record must be
the record of that logits row (lse as returned within one f32 ulp of numpy's, everything else exact): the call runs the head ALL_LOGITS runs, into the library's
workspace.  Shapes: every route and head (exact rows, MFMA rows + GEMM head, f32 activations, token by token with a ragged 1003-row head, Mamba2, DeepSeek-V2), and
every chunk edge (2 048 rows for the Llama family, 512 for the other two)."""
import numpy as np
import pytest

import irregular_cases
import score_ref as SR
from blazr_amd import _lib as L
from blazr_amd import runtime, synth

pytestmark = pytest.mark.gpu
F = np.float32


# ---- op level ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", SR.VS)
@pytest.mark.parametrize("top_n", SR.TOP_NS)
def test_score_rows_match_spec(device, V, top_n):
    x = SR.make_rows(V)                                    # R = 5
    tg = np.array([0, V - 1, -1, V // 2, V - 1], dtype=np.int64)
    got = runtime.score_rows(device, x, tg, top_n)["rows"]
    for r in range(len(x)):
        SR.records_equal(got[r], runtime.score_row_spec(x[r], int(tg[r]), top_n), "V=%d row=%d" % (V, r))
        SR.check_record(got[r], x[r], int(tg[r]), top_n, "V=%d row=%d" % (V, r))


def test_score_rows_nan_logits(device):
    V = 1003
    x = np.stack([SR.nan_row(V, s) for s in range(3)])
    tg = np.array([0, V - 1, int(np.nonzero(~np.isnan(x[2]))[0][5])], dtype=np.int64)
    got = runtime.score_rows(device, x, tg, 20)["rows"]
    assert int(got[0]["rank"]) == -1
    for r in range(3):
        SR.records_equal(got[r], runtime.score_row_spec(x[r], int(tg[r]), 20), "row=%d" % r)
        SR.check_record(got[r], x[r], int(tg[r]), 20, "row=%d" % r)


def test_score_rows_beyond_the_samplers_512(device):
    """R = 600 rows at V = 1003: three sub-batches of the scoring kernels, a device-side target outside the row is not scored"""
    R, V = 600, 1003
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((R, V)) * 3.0).astype(F)
    x[300] = SR.make_rows(V)[2]
    tg = rng.integers(0, V, size=R).astype(np.int64)
    tg[::7] = -1
    res = runtime.score_rows(device, x, tg, 5)
    for r in range(R):
        SR.records_equal(res["rows"][r], runtime.score_row_spec(x[r], int(tg[r]), 5), "row=%d" % r)
    lp = res["rows"]["logprob"][tg >= 0]
    assert res["n_scored"] == int(np.count_nonzero(tg >= 0)) and res["sum_logprob"] == float(np.cumsum(lp.astype(np.float64))[-1])


# ---- model level ------------------------------------------------------------------------------------------------------------------------------
def _targets(tokens, seed):
    """the tokens shifted by one, a few rows not wanted, a few other ids"""
    tg = np.concatenate([tokens[1:], [-1]]).astype(np.int64)
    rng = np.random.default_rng(seed)
    tg[rng.random(len(tg)) < 0.1] = -1
    return tg


def _check_against_logits(res, logits, tg, top_n, where):
    rows = res["rows"]
    assert len(rows) == len(tg) == len(logits)
    for i in range(len(tg)):
        SR.check_record(rows[i], logits[i], int(tg[i]), top_n, "%s row=%d" % (where, i))
    lp = rows["logprob"][(rows["n_top"] >= 0) & np.isfinite(rows["logprob"])]
    assert res["n_scored"] == len(lp) and res["sum_logprob"] == float(np.cumsum(lp.astype(np.float64))[-1]), where
    assert res["perplexity"] == float(np.exp(-res["sum_logprob"] / res["n_scored"]))


LLAMA_CASES = [("tiny-awq", {}, 12, 5), ("tiny-awq", {}, 40, 20), ("tiny-bf16", {}, 40, 5), ("tiny-fp8", {}, 40, 1), ("tiny-q4km", {}, 24, 5),
               ("bf16-g3-hd64", None, 20, 5), ("tiny-bf16", dict(max_seq_len=4096), 2060, 0)]


@pytest.mark.parametrize("preset,over,S,top_n", LLAMA_CASES, ids=["%s-%d" % (c[0], c[2]) for c in LLAMA_CASES])
def test_score_kv_equals_all_logits(device, preset, over, S, top_n):
    model = irregular_cases.make(preset) if over is None else synth.make_llama(preset, **over)
    cfg = model["config"]
    lm = runtime.LoadedModel.from_synth(device, model)
    p = synth.prompt_tokens(S, cfg["vocab"], seed=11)
    tg = _targets(p, S)
    kv_a, kv_b = lm.new_kv_cache(S + 8), lm.new_kv_cache(S + 8)
    logits = lm.forward_with_kv_cache(p, kv_a, 0, all_logits=True).to_numpy().reshape(S, -1)
    res = lm.score(p, kv_b, 0, targets=tg, top_logprobs=top_n)
    _check_against_logits(res, logits, tg, top_n, "%s S=%d" % (preset, S))
    # cache state: what the forward call leaves
    assert kv_b.seq_len() == kv_a.seq_len() == S
    for layer in (0, cfg["n_layers"] - 1):
        assert np.array_equal(kv_a.read(layer, 0, 0, S), kv_b.read(layer, 0, 0, S))


def test_score_default_targets_and_second_call(device):
    """default targets = each token given its predecessors; a second, shorter call on the same model reuses the (larger) workspace"""
    model = synth.make_llama("tiny-bf16")
    lm = runtime.LoadedModel.from_synth(device, model)
    V = model["config"]["vocab"]
    for S in (40, 17):
        p = synth.prompt_tokens(S, V, seed=S)
        logits = lm.forward_with_kv_cache(p, lm.new_kv_cache(S + 8), 0, all_logits=True).to_numpy().reshape(S, -1)
        res = lm.score(p, lm.new_kv_cache(S + 8))
        tg = np.concatenate([p[1:], [-1]])
        _check_against_logits(res, logits, tg, 0, "S=%d" % S)
        assert res["n_scored"] == S - 1


def test_score_continuation(device):
    """a context of 20 tokens, then a continuation of 9 at position 20 on the same cache, against the same two forward calls"""
    model = synth.make_llama("tiny-bf16")
    lm = runtime.LoadedModel.from_synth(device, model)
    V = model["config"]["vocab"]
    ctx, cont = synth.prompt_tokens(20, V, seed=3), synth.prompt_tokens(9, V, seed=4)
    kv_a, kv_b = lm.new_kv_cache(40), lm.new_kv_cache(40)
    la = lm.forward_with_kv_cache(ctx, kv_a, 0, all_logits=True).to_numpy().reshape(20, -1)
    lb = lm.forward_with_kv_cache(cont, kv_a, 20, all_logits=True).to_numpy().reshape(9, -1)
    tg_a = np.concatenate([np.full(19, -1), cont[:1]]).astype(np.int64)          # the context's last row predicts the continuation's first token
    tg_b = np.concatenate([cont[1:], [-1]]).astype(np.int64)
    ra = lm.score(ctx, kv_b, 0, targets=tg_a, top_logprobs=5)
    rb = lm.score(cont, kv_b, 20, targets=tg_b, top_logprobs=5)
    _check_against_logits(ra, la, tg_a, 5, "context")
    _check_against_logits(rb, lb, tg_b, 5, "continuation")
    assert ra["n_scored"] == 1 and rb["n_scored"] == 8 and kv_b.seq_len() == 29


def test_score_paged_equals_all_logits(device):
    model = synth.make_llama("tiny-bf16")
    cfg = model["config"]
    lm = runtime.LoadedModel.from_synth(device, model)
    S = 40
    p = synth.prompt_tokens(S, cfg["vocab"], seed=21)
    tg = _targets(p, 21)
    blocks = [7, 2, 5, 0, 8, 3, 1, 11, 4, 10, 6]

    def pool():
        pk = runtime.LayeredPagedKvCache(device, cfg["n_layers"], 12, 4, cfg["n_kv_heads"], cfg["head_dim"], L.BF16)
        pk.set_blocks(blocks)
        return pk
    pa, pb = pool(), pool()
    sm = pa.compute_slot_mapping(0, S)
    logits = lm.forward_with_paged_kv_cache(p, pa, sm, pa.block_table_device_format(), S, 0, all_logits=True).to_numpy().reshape(S, -1)
    res = lm.score_paged(p, pb, sm, pb.block_table_device_format(), S, 0, targets=tg, top_logprobs=5)
    _check_against_logits(res, logits, tg, 5, "paged")
    assert pb.seq_len() == S
    assert np.array_equal(pa.read_block(0, 7, 0, cfg["n_kv_heads"], cfg["head_dim"], L.BF16), pb.read_block(0, 7, 0, cfg["n_kv_heads"], cfg["head_dim"], L.BF16))


@pytest.mark.parametrize("S", (24, 520))
def test_score_ssm_equals_all_logits(device, S):
    model = synth.make_mamba2("tiny-mamba2")
    lm = runtime.LoadedModel.from_synth(device, model)
    p = synth.prompt_tokens(S, model["config"]["vocab"], seed=31)
    tg = _targets(p, S)
    logits = lm.forward_with_ssm_state(p, runtime.LayeredSsmState(lm), all_logits=True).to_numpy().reshape(S, -1)
    res = lm.score(p, runtime.LayeredSsmState(lm), targets=tg, top_logprobs=5)
    _check_against_logits(res, logits, tg, 5, "mamba2 S=%d" % S)


@pytest.mark.parametrize("S", (24, 520))
def test_score_dsv2_equals_all_logits(device, S):
    model = synth.make_dsv2("tiny-dsv2", max_seq_len=640)
    lm = runtime.LoadedModel.from_synth(device, model)
    p = synth.prompt_tokens(S, model["config"]["vocab"], seed=41)
    tg = _targets(p, S)
    kv_a, kv_b = lm.new_kv_cache(S + 8), lm.new_kv_cache(S + 8)
    logits = lm.forward_with_kv_cache(p, kv_a, 0, all_logits=True).to_numpy().reshape(S, -1)
    res = lm.score(p, kv_b, 0, targets=tg, top_logprobs=5)
    _check_against_logits(res, logits, tg, 5, "dsv2 S=%d" % S)
    assert kv_b.seq_len() == kv_a.seq_len() == S


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_score_refusals_leave_the_cache_alone(device):
    model = synth.make_llama("tiny-bf16")
    lm = runtime.LoadedModel.from_synth(device, model)
    V = model["config"]["vocab"]
    p = synth.prompt_tokens(12, V, seed=1)
    kv = lm.new_kv_cache(32)
    lm.forward_with_kv_cache(p[:5], kv, 0)
    for kw, figure in ((dict(targets=[V] + [-1] * 11), str(V)), (dict(targets=[-2] + [-1] * 11), "-2"), (dict(top_logprobs=21), "21")):
        with pytest.raises(L.BlazrHipError) as e:
            lm.score(p, kv, 5, **kw)
        assert e.value.code == L.E_INVALID and figure in str(e.value), str(e.value)
        assert kv.seq_len() == 5
    mm = runtime.LoadedModel.from_synth(device, synth.make_mamba2("tiny-mamba2"))
    rows, cfg, tg = (L.ScoreRow * 12)(), L.ScoreConfig(top_n=0), np.full(12, -1, dtype=np.int64)
    t = device.tensor(p)
    assert L.lib().bz_score_kv(mm.h, t.h, 12, kv.h, 5, tg.ctypes.data, cfg, rows, None) == L.E_INVALID
    assert kv.seq_len() == 5
