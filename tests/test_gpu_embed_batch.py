"""embed_batch (bz_embed_batch): many inputs in one prompt pass against the single calls they replace and against the oracle's rows of every input alone.
Exact rows (f16 int4, tiny-awq): bit for bit the single calls' rows.  MFMA route: the rows through the lm_head in float64 at the bars single MFMA prompts are
held to, and bit-for-bit isolation between the inputs.  Pooled results: bz_pool_spec of the input's rows.  Fallbacks: the loop's bits."""
import numpy as np
import pytest

import packed_cases as PC
import packed_model as PM
import packed_probe
import score_ref as SR
from blazr_amd import _lib as L
from blazr_amd import runtime, synth

pytestmark = pytest.mark.gpu
MFMA_CASES = [(n, s) for n in ("tiny-bf16", "bf16-g2-w768", "awq-g4-w768") for s in ("B", "C", "E")]


def _check_exact(res, lens):
    assert res["packed"] == 1 and res["exact"] == 1 and res["attn"] == L.PF_ATTN_SCALAR_EXACT and res["scratch_len"] == 0
    assert np.array_equal(res["batch_rows"].view(np.uint32), res["single_rows"].view(np.uint32))
    off = PC.offsets(lens)
    for i in range(len(lens)):
        rows = res["single_rows"][off[i]:off[i + 1]]
        for pooling in ("mean", "cls", "last"):
            assert np.array_equal(res["batch_" + pooling][i], runtime.pool_spec(rows, pooling)), (i, pooling)
            assert SR.within_ulp(res["batch_norm_" + pooling][i], runtime.pool_spec(rows, pooling, normalize=True)), (i, pooling)


def test_exact_rows_are_the_single_calls_rows(device):
    """[5, 4, 7]: 16 packed rows, the default exact rows of an f16 int4 model; every single call (5, 4, 7 tokens) runs the decode step"""
    lens = [5, 4, 7]
    _, lm, _ = PM.get(device, "tiny-awq")
    _, toks = PM.inputs("tiny-awq", "probe", lens)
    _check_exact(packed_probe.compare(lm, runtime.prompt_traits(lm), lens, toks, PM.scratch(lm, lens)), lens)


def test_exact_rows_set_b(tmp_path):
    """set B (675 rows) with BZ_EXACT_PREFILL=1, in a process of its own"""
    _check_exact(packed_probe.child("tiny-awq", PC.SETS["B"], dict(BZ_EXACT_PREFILL="1"), tmp_path), PC.SETS["B"])


@pytest.mark.parametrize("name,set_name", MFMA_CASES, ids=["%s-%s" % c for c in MFMA_CASES])
def test_mfma_rows_at_the_bar(device, name, set_name):
    model, lm, _ = PM.get(device, name)
    lens, toks = PM.inputs(name, set_name)
    plan = runtime.packed_plan(runtime.prompt_traits(lm), lens, lm.c.act_dtype)
    assert plan["packed"] == 1 and plan["plan"]["attn"] == L.PF_ATTN_MFMA and plan["plan"]["exact"] == 0
    rows = lm.embed_batch(toks, PM.scratch(lm, lens), pooling="none")
    want = PM.oracle_rows(device, name, set_name)
    W, bar = PM.lm_head64(model), PM.bar(model["config"], int4=name.startswith("awq"))
    errs = [PM.rel_l2(rows[i].astype(np.float64) @ W.T, want[i]) for i in range(len(lens))]
    print("PACKED_EMBED_BAR %s %s worst %.3e of %.3e (input %d)" % (name, set_name, max(errs), bar, int(np.argmax(errs))))
    assert max(errs) <= bar, errs


@pytest.mark.parametrize("name", ["tiny-bf16", "awq-g4-w768"])
def test_isolation_whole_model(device, name):
    """other tokens in one input leave every other input's rows as they are, bit for bit"""
    _, lm, _ = PM.get(device, name)
    for set_name in ("B", "C"):
        lens, toks = PM.inputs(name, set_name)
        base = lm.embed_batch(toks, PM.scratch(lm, lens), pooling="none")
        for i in range(len(lens)):
            other = list(toks)
            other[i] = (toks[i] + 7) % PM.VOCAB[name]
            got = lm.embed_batch(other, PM.scratch(lm, lens), pooling="none")
            for j in range(len(lens)):
                assert np.array_equal(got[j], base[j]) == (j != i), (set_name, i, j)


def test_pooled_results_across_the_chunk_edge(device):
    """set E on tiny-bf16: the first input's mean is carried from the first chunk into the second; the last two inputs lie wholly in the second"""
    _, lm, _ = PM.get(device, "tiny-bf16")
    lens, toks = PM.inputs("tiny-bf16", "E")
    rows = lm.embed_batch(toks, PM.scratch(lm, lens), pooling="none")
    assert [len(r) for r in rows] == lens
    for pooling in ("mean", "cls", "last"):
        got = lm.embed_batch(toks, PM.scratch(lm, lens), pooling=pooling)
        gotn = lm.embed_batch(toks, PM.scratch(lm, lens), pooling=pooling, normalize=True)
        assert got.shape == (len(lens), lm.c.hidden)
        for i in range(len(lens)):
            assert np.array_equal(got[i], runtime.pool_spec(rows[i], pooling)), (pooling, i)
            assert SR.within_ulp(gotn[i], runtime.pool_spec(rows[i], pooling, normalize=True)), (pooling, i)
    nn = lm.embed_batch(toks, PM.scratch(lm, lens), pooling="none", normalize=True)
    assert SR.within_ulp(np.concatenate(nn), runtime.pool_spec(np.concatenate(rows), "none", normalize=True))


@pytest.mark.parametrize("name,lens", [("bf16-g3-hd64", [20, 3, 33]), ("tiny-dsv2", [24, 5, 19]), ("tiny-bf16", PC.BELOW_FLOOR)], ids=["g3", "dsv2", "below-floor"])
def test_fallbacks_are_the_loop(device, name, lens):
    _, lm, _ = PM.get(device, name)
    _, toks = PM.inputs(name, "fallback", lens)
    assert runtime.packed_plan(runtime.prompt_traits(lm), lens, lm.c.act_dtype)["packed"] == 0
    kv = PM.scratch(lm, lens)
    got = lm.embed_batch(toks, kv, pooling="none")
    assert kv.seq_len() == 0
    for i, t in enumerate(toks):
        assert np.array_equal(got[i], lm.embed(t, lm.new_kv_cache(len(t)), 0, pooling="none")), i
    got = lm.embed_batch(toks, kv, pooling="mean", normalize=True)
    for i, t in enumerate(toks):
        assert np.array_equal(got[i], lm.embed(t, lm.new_kv_cache(len(t)), 0, pooling="mean", normalize=True)), i


RERANK_SEED = 83      # the loop's scores lie 8.5e-2 apart at the closest; most seeds put two unrelated documents closer than twice the bar


def rerank_case(V, seed):
    """a query of 21 tokens and six documents of 18 .. 100; two of them hold the query"""
    query = PC.token_lists([21], V, seed=81)[0]
    docs = PC.token_lists([24, 40, 18, 65, 33, 100], V, seed=seed)
    docs[1][:21] = query
    docs[3][10:31] = query
    return query, docs


def test_rerank_batched(device):
    """six documents: batched=True orders them as the loop does, and every score is within the embedding bar of the loop's.  The bar is the relative L2 a single
    MFMA prompt's rows are held to, taken as it is for the cosine; the loop's scores lie more than twice the bar apart, so the order is
    decided by the documents and not by the rounding the bar allows."""
    model, lm, _ = PM.get(device, "tiny-bf16")
    query, docs = rerank_case(PM.VOCAB["tiny-bf16"], RERANK_SEED)
    kv = lm.new_kv_cache(sum(len(d) for d in docs) + len(query))
    want, got = runtime.rerank(lm, kv, query, docs), runtime.rerank(lm, kv, query, docs, batched=True)
    tol = PM.bar(model["config"], int4=False)
    ws, gs = {e["index"]: e["relevance_score"] for e in want}, {e["index"]: e["relevance_score"] for e in got}
    gaps = np.diff(np.sort([ws[i] for i in range(6)]))
    print("PACKED_RERANK worst score difference %.3e of %.3e, smallest gap of the loop's scores %.3e" % (max(abs(ws[i] - gs[i]) for i in ws), tol, gaps.min()))
    assert np.all(gaps > 2 * tol), ws
    assert [e["index"] for e in got] == [e["index"] for e in want]
    assert sorted(gs) == list(range(6)) and all(abs(ws[i] - gs[i]) <= tol for i in ws), (ws, gs)
    assert runtime.rerank(lm, kv, query, docs, top_n=2, batched=True) == got[:2]
    assert runtime.rerank(lm, kv, query, docs) == want                                     # the default is still the loop


def test_refusals(device):
    _, lm, _ = PM.get(device, "tiny-bf16")
    H = lm.c.hidden
    tok = device.tensor(np.arange(1, 41, dtype=np.int64))
    kv = lm.new_kv_cache(16, max_seq_len=32)
    out = device.zeros((4, H), L.F32)

    def call(lens, cache=kv, pooling=L.POOL_MEAN, o=out):
        sl = np.asarray(lens, dtype=np.int32)
        rc = L.lib().bz_embed_batch(lm.h, tok.h, sl.ctypes.data if len(sl) else None, len(sl), cache.h, L.EmbedConfig(pooling=pooling), o.h)
        return rc, L.lib().bz_last_error()
    for kw, figure in ((dict(lens=[]), b"n_seq = 0"), (dict(lens=[10, 0]), b"seq_lens[1] = 0"), (dict(lens=[20, 20]), b"40 packed rows, the scratch cache holds 32"),
                       (dict(lens=[10, 10], pooling=9), b"pooling = 9"), (dict(lens=[10, 10], pooling=L.POOL_NONE), b"[T, hidden]"),
                       (dict(lens=[5, 5, 5, 5, 5]), b"[n_seq, hidden]")):
        rc, msg = call(**kw)
        assert rc == L.E_INVALID and figure in msg, (kw, msg)
        assert kv.seq_len() == 0
    assert call([10, 10])[0] == L.OK
    with pytest.raises(ValueError):
        lm.embed_batch([[1, 2], []], kv)
    mamba = synth.make_mamba2("tiny-mamba2")
    mm = runtime.LoadedModel.from_synth(device, mamba)
    st = runtime.LayeredSsmState(mm)
    p = PC.token_lists([24, 9], mamba["config"]["vocab"], seed=1)
    got = mm.embed_batch(p, st, pooling="last")                     # a Mamba2 state object loops the single call
    assert np.array_equal(got[1], mm.embed(p[1], runtime.LayeredSsmState(mm), pooling="last"))
