"""Per-row logprobs and logit bias of the batched sampler on the GPU (blazr_amd/csrc/bz_logprobs.hip), through bz_batch_sampler_sample and the captured
batched step, against tests/logprobs_ref.py (which tests/test_logprobs_ref.py holds to the host routines and to float64 without a GPU).

Ids, their order and n_top are exact.  lse may differ from the restatement by one f32 ulp (the double log is the only platform-dependent step and is
rounded to f32 on either side); every logprob is then the f32 subtraction x - lse of the device's own lse, exactly."""
import numpy as np
import pytest

import logprobs_ref as R
from blazr_amd import _lib as L
from blazr_amd import runtime, synth

pytestmark = pytest.mark.gpu

F = np.float32
N, VS = 6, (7, 1001, 32003)
# a workgroup's slice is 256 ids out of every 32768: beyond that a thread holds more than one id of its slice (three here, the last pass partial)
VS_MORE = VS + (70001,)
# rows 0 and 5 sample with penalties (their history and draw counter matter from the second call on), the others are greedy
SAMPLED = {0: dict(temperature=0.9, top_k=40, top_p=0.95, min_p=0.0, repeat_penalty=1.2, frequency_penalty=0.1, presence_penalty=0.05, repeat_last_n=64, seed=41),
           5: dict(temperature=1.1, top_k=0, top_p=0.9, min_p=0.01, repeat_penalty=1.1, frequency_penalty=0.0, presence_penalty=0.0, repeat_last_n=8, seed=42)}
_RUNS = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _sampler(device, V, bias=False, logprobs=False):
    s = runtime.BatchSampler(device, N, V)
    if bias or logprobs:
        s.enable(bias=bias, logprobs=logprobs)
    for r, kw in SAMPLED.items():
        s.set_row(r, history=[1, 2, 1], **kw)
    return s


def _run(device, V):
    """Five calls on the rows of R.make_rows(V); in call k row r has top_n = TOP_NS[(r + k) % 5], so every kind of row meets every setting, mixed within a call.
    -> (x, [(top_n per row, tokens, records)] per call, the tokens of a sampler without the flags over the same five calls)"""
    if V not in _RUNS:
        x = R.make_rows(V)
        s, plain = _sampler(device, V, logprobs=True), _sampler(device, V)
        t = device.tensor(x)
        calls, plain_tokens = [], []
        for k in range(5):
            top = [R.TOP_NS[(r + k) % 5] for r in range(N)]
            for r in range(N):
                s.set_row_logprobs(r, top[r])
            tok = s.sample(t).to_numpy().tolist()
            calls.append((top, tok, s.read_logprobs()))
            plain_tokens.append(plain.sample(t).to_numpy().tolist())
        assert np.array_equal(_bits(t.to_numpy()), _bits(x))                           # without a bias the logits are not written
        _RUNS[V] = (x, calls, plain_tokens)
    return _RUNS[V]


@pytest.mark.parametrize("V", VS_MORE)
def test_ids_order_and_n_top_equal_the_reference(device, V):
    x, calls, _ = _run(device, V)
    seen = set()
    for top, tok, recs in calls:
        for r in range(N):
            if top[r] < 0:
                assert recs[r] is None, (r, top[r])                                    # n_top = -1
                continue
            want = R.logprobs_row(x[r], top[r])
            assert recs[r]["token"] == tok[r]
            assert len(recs[r]["top_ids"]) == want["n_top"] == min(top[r], V, 20), (R.ROW_KINDS[r], top[r])
            assert recs[r]["top_ids"] == want["top_ids"].tolist(), (R.ROW_KINDS[r], top[r])
            seen.add((r, top[r]))
    assert len(seen) == N * 4
    if V >= 20:
        assert [c for c in calls if c[0][1] == 20][0][2][1]["top_ids"] == list(range(20))   # the all-equal row: ids 0 .. n-1


@pytest.mark.parametrize("V", VS_MORE)
def test_lse_within_one_ulp_and_values_are_the_f32_subtraction(device, V):
    x, calls, _ = _run(device, V)
    for top, tok, recs in calls:
        for r in range(N):
            if top[r] < 0:
                continue
            ref_lse = R.lse_parts(x[r])[3]
            lse = F(recs[r]["lse"])
            print("V=%d %s top_n=%d lse gpu %.9g ref %.9g" % (V, R.ROW_KINDS[r], top[r], lse, ref_lse))
            assert abs(float(lse) - float(ref_lse)) <= R.ulp(ref_lse), (R.ROW_KINDS[r], float(lse), float(ref_lse))
            with np.errstate(all="ignore"):
                assert _bits(F(recs[r]["logprob"])) == _bits(F(x[r][tok[r]] - lse)), (R.ROW_KINDS[r], tok[r])
                want = (x[r][recs[r]["top_ids"]] - lse).astype(F) if recs[r]["top_ids"] else np.zeros(0, F)
            assert _bits(np.asarray(recs[r]["top_logprobs"], dtype=F)).tolist() == _bits(want).tolist(), (R.ROW_KINDS[r], top[r])


def test_error_against_float64_is_no_larger_than_the_host_routine(device):
    """bz_compute_logprobs sums f32 terms in index order and takes logf; the device sums 2^-40 fixed-point integers and takes a double log.  Over all test rows
    the device's largest |logprob - float64 log-softmax| must not exceed the host routine's on the same entries."""
    dev_err = host_err = 0.0
    kinds = {k: [0.0, 0.0] for k in R.ROW_KINDS}
    for V in VS:
        x, calls, _ = _run(device, V)
        dv = hv = 0.0
        for top, tok, recs in calls:
            for r in range(N):
                if top[r] < 0:
                    continue
                ref = R.log_softmax64(x[r])
                clp, hid, hlp = R.host_logprobs(x[r], tok[r], top[r])
                host = dict(zip(hid.tolist(), hlp.tolist()))
                pairs = [(tok[r], recs[r]["logprob"], float(clp))]
                pairs += [(i, lp, host[i]) for i, lp in zip(recs[r]["top_ids"], recs[r]["top_logprobs"]) if i in host]
                for i, d, h in pairs:
                    if np.isfinite(ref[i]):
                        dv, hv = max(dv, abs(d - ref[i])), max(hv, abs(h - ref[i]))
                        kinds[R.ROW_KINDS[r]] = [max(kinds[R.ROW_KINDS[r]][0], abs(d - ref[i])), max(kinds[R.ROW_KINDS[r]][1], abs(h - ref[i]))]
        print("V=%d largest error: device %.3e host %.3e" % (V, dv, hv))
        dev_err, host_err = max(dev_err, dv), max(host_err, hv)
    for k, (d, h) in kinds.items():
        print("%s rows: device %.3e host %.3e" % (k, d, h))
    print("all rows: device %.3e host %.3e" % (dev_err, host_err))
    assert dev_err <= host_err, (dev_err, host_err)


@pytest.mark.parametrize("V", VS_MORE)
def test_tokens_history_and_draws_equal_a_sampler_without_the_flags(device, V):
    x, calls, plain_tokens = _run(device, V)
    assert [c[1] for c in calls] == plain_tokens                                        # five calls: the later ones depend on history and draw index
    assert any(top[r] < 0 for top, _, _ in calls for r in SAMPLED)


def test_bias(device):
    V = 1001
    rng = np.random.default_rng(77)
    x = (rng.standard_normal((N, V)) * 2).astype(F)
    x[2, [10, 11, 500]] = -np.inf                                                       # what a grammar mask leaves
    x[4, 256] = F(30.0)
    many = rng.permutation(V)[:512]
    lists = [([7, 300, 7, V, V + 9, 300], [1.5, -2.0, 1000.0, 5.0, 5.0, 0.25]),        # duplicates (the last wins: +1000 on 7 forces it), ids >= V
             ([], []),
             ([10, 500, 40], [1000.0, -3.0, 2.0]),                                      # a bias on masked entries: they stay -inf
             (many.tolist(), (rng.standard_normal(512) * 3).astype(F).tolist()),        # 512 entries are accepted
             ([256], [-1000.0]),                                                        # a ban on what greedy would pick
             ([V - 1, 0], [0.5, -0.5])]
    s = runtime.BatchSampler(device, N, V)
    s.enable(bias=True, logprobs=True)
    for r, (ids, vals) in enumerate(lists):
        s.set_row_bias(r, list(zip(ids, vals)))
        s.set_row_logprobs(r, 5)
    t = device.tensor(x)
    tok = s.sample(t).to_numpy().tolist()
    after = t.to_numpy()
    recs = s.read_logprobs()
    for r, (ids, vals) in enumerate(lists):
        assert np.array_equal(_bits(after[r]), _bits(R.host_apply_bias(x[r], ids, vals))), r           # bz_apply_logit_bias, bit for bit
        assert tok[r] == int(np.argmax(after[r])), r                                                    # greedy on the biased row
        lse = F(recs[r]["lse"])
        assert abs(float(lse) - float(R.lse_parts(x[r])[3])) <= R.ulp(lse), r                           # logprobs are the RAW row's
        assert _bits(F(recs[r]["logprob"])) == _bits(F(x[r][tok[r]] - lse)), r
        assert recs[r]["top_ids"] == R.logprobs_row(x[r], 5)["top_ids"].tolist(), r
    assert tok[0] == 7 and recs[0]["logprob"] < -3.0                                                    # forced; its logprob is not the biased ~0
    assert np.isneginf(after[2, [10, 500]]).all() and tok[2] not in (10, 11, 500)
    assert tok[4] != 256 and int(np.argmax(x[4])) == 256
    # the next call without a recapture / re-enable: a cleared list leaves the row alone
    s.set_row_bias(0, None)
    t2 = device.tensor(x)
    tok2 = s.sample(t2).to_numpy().tolist()
    assert np.array_equal(_bits(t2.to_numpy()[0]), _bits(x[0])) and tok2[0] == int(np.argmax(x[0]))
    assert tok2[1:] == tok[1:]


def test_refusals_name_their_cause(device):
    V = 1001

    def refused(fn, *words):
        with pytest.raises(L.BlazrHipError) as e:
            fn()
        assert e.value.code == L.E_INVALID, str(e.value)
        assert all(w in str(e.value) for w in words), str(e.value)
    s = runtime.BatchSampler(device, N, V)
    s.enable(bias=True, logprobs=True)
    refused(lambda: s.set_row_bias(0, [(i, 1.0) for i in range(513)]), "513", "at most 512")
    s.set_row_bias(0, [(i % 512, 1.0) for i in range(2000)])                             # 512 after deduplication
    s.set_row_bias(0, [(i, 1.0) for i in range(512)] + [(V + i, 1.0) for i in range(50)])
    refused(lambda: s.set_row_bias(0, [(3, float("nan"))]), "not a finite number")
    refused(lambda: s.set_row_bias(0, [(3, float("inf"))]), "not a finite number")
    refused(lambda: s.set_row_bias(N, [(3, 1.0)]), "row %d" % N)
    refused(lambda: s.set_row_logprobs(0, 21), "top_n = 21")
    refused(lambda: s.set_row_logprobs(0, -2), "top_n = -2")
    refused(lambda: s.enable(bias=True), "already enabled")
    plain = runtime.BatchSampler(device, N, V)
    refused(lambda: plain.set_row_bias(0, [(3, 1.0)]), "BZ_BS_BIAS")
    refused(lambda: plain.set_row_logprobs(0, 5), "BZ_BS_LOGPROBS")
    refused(lambda: plain.read_logprobs(), "BZ_BS_LOGPROBS")
    refused(lambda: plain.enable(), "flags = 0")
    only = runtime.BatchSampler(device, N, V)
    only.enable(logprobs=True)
    refused(lambda: only.set_row_bias(0, [(3, 1.0)]), "BZ_BS_BIAS")
    plain.sample(device.zeros((N, V)))
    refused(lambda: plain.enable(logprobs=True), "sampled or been captured")
    assert s.sample(device.zeros((N, V))).to_numpy().tolist() == [0] * N                 # after the refusals the handle works; row 0: +1 on ids 0..511, id 0 first


def _kv_dt(cfg):
    return {"f16": L.F16, "bf16": L.BF16, "f32": L.F32}[cfg["act_dtype"]]


@pytest.mark.parametrize("preset", ["tiny-awq", "tiny-bf16"])
def test_captured_graph(device, preset):
    model = synth.make_llama(preset)
    cfg = model["config"]
    V = cfg["vocab"]
    lm = runtime.LoadedModel.from_synth(device, model)
    nseq, bs, per, steps = 4, 16, 3, 8
    tables = [[i + nseq * j for j in range(per)] for i in range(nseq)]
    plens = [3 + (13 * i) % 30 for i in range(nseq)]
    prompts = [synth.prompt_tokens(n, V, seed=70 + i) for i, n in enumerate(plens)]

    def pool_and_first():
        pool = runtime.LayeredPagedKvCache(device, cfg["n_layers"], nseq * per, bs, cfg["n_kv_heads"], cfg["head_dim"], _kv_dt(cfg))
        first = []
        for p, tb in zip(prompts, tables):
            slots = [tb[i // bs] * bs + i % bs for i in range(len(p))]
            first.append(int(lm.forward_with_paged_kv_cache(p, pool, slots, tb, len(p), 0).to_numpy()[0].argmax()))
        return pool, first
    pool_g, first = pool_and_first()
    pool_e, first_e = pool_and_first()
    assert first == first_e
    sampler = runtime.BatchSampler(device, nseq, V)
    sampler.enable(bias=True, logprobs=True)
    sampler.set_row(1, history=list(map(int, prompts[1])) + [first[1]], temperature=0.8, top_k=12, min_p=0.02, seed=211)
    top = [5, 0, -1, 20]
    bias = [None] * nseq
    for r in range(nseq):
        sampler.set_row_logprobs(r, top[r])
    g = runtime.BatchDecodeGraph(lm, pool_g, nseq, per, sampler=sampler)
    g.seed(first, [n + 1 for n in plens], tables)
    toks, lens = list(first), list(plens)
    for step in range(steps):
        g.replay()
        got = g.read_tokens(step).tolist()
        recs = g.read_logprobs(step)
        lens = [n + 1 for n in lens]
        slots = [tb[(n - 1) // bs] * bs + (n - 1) % bs for n, tb in zip(lens, tables)]
        raw = lm.forward_paged_batch(toks, pool_e, slots, tables, lens).to_numpy()       # the eager step at the same positions, fed what the replay was fed
        shown = g.read_logits()
        for r in range(nseq):
            want_row = raw[r] if bias[r] is None else R.host_apply_bias(raw[r], *zip(*bias[r]))
            assert np.array_equal(_bits(shown[r]), _bits(want_row)), (step, r)
            if top[r] < 0:
                assert recs[r] is None, (step, r)
                continue
            want = R.logprobs_row(raw[r], top[r])
            lse = F(recs[r]["lse"])
            assert recs[r]["token"] == got[r] and recs[r]["top_ids"] == want["top_ids"].tolist(), (step, r)
            assert abs(float(lse) - float(want["lse"])) <= R.ulp(want["lse"]), (step, r)
            assert _bits(F(recs[r]["logprob"])) == _bits(F(raw[r][got[r]] - lse)), (step, r)
            assert _bits(np.asarray(recs[r]["top_logprobs"], dtype=F)).tolist() == _bits((raw[r][recs[r]["top_ids"]] - lse).astype(F)).tolist(), (step, r)
        if bias[0] is not None:
            assert got[0] != bias[0][0][0]                                               # the banned id is not picked
        if bias[3] is not None:
            assert got[3] == 9                                                           # the forced one is
        if step == 3:                                                                    # between replays, no recapture
            top = [-1, 20, 1, 5]
            for r in range(nseq):
                sampler.set_row_logprobs(r, top[r])
            bias[0] = [(got[0], -1000.0)]
            bias[3] = [(9, 1000.0), (V + 3, 1.0)]
            sampler.set_row_bias(0, bias[0])
            sampler.set_row_bias(3, bias[3])
        toks = got
    del g
