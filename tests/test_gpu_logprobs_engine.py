"""Per-request logit bias and logprobs in the request engine (bz_engine_submit_ex / bz_engine_poll_logprobs; runtime.BatchEngine(logprobs=True)) on the device.
Token comparisons are exact: rows of the batched step do not see each other (tests/test_gpu_engine.py), and on the int4 preset the single-sequence loop gives the
engine's tokens (tests/test_gpu_lora_engine.py relies on the same), so a biased greedy request is held to Executor.generate(logit_bias=...)."""
import ctypes as C

import numpy as np
import pytest

import grammar_ref as G
from blazr_amd import _lib as L
from blazr_amd import runtime, synth
from test_gpu_grammar import _model
from test_grammar_rows import LITERALS

pytestmark = pytest.mark.gpu

PRESET = "tiny-awq"
NROWS, BS, MAXLEN, DEPTH = 4, 16, 80, 3
NONE = dict(repeat_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0, repeat_last_n=64)
GREEDY = dict(NONE, temperature=0.0, top_k=0, top_p=1.0, min_p=0.0, seed=0)
SAMPLED = dict(NONE, temperature=0.8, top_k=12, top_p=1.0, min_p=0.02, seed=211)
PENALISED = dict(temperature=1.0, top_k=10, top_p=0.9, min_p=0.0, repeat_penalty=1.2, frequency_penalty=0.0, presence_penalty=0.0, repeat_last_n=16, seed=212)
FORCED = 9


def _engine(lm, logprobs, grammar=None, sampler=True):
    per = -(-MAXLEN // BS)
    return runtime.BatchEngine(lm, NROWS, NROWS * per + NROWS, BS, MAXLEN, 0, DEPTH, sampler, grammar, logprobs=logprobs)


def _drive(eng, reqs, hook=None):
    """every request submitted before the first step -> (ids, {id: [(index, token)]}, {id: finish reason}, [logprobs records in arrival order])"""
    ids = [eng.submit(**kw) for kw in reqs]
    ev, fin, recs, step, busy = {}, {}, [], 0, True
    while busy:
        if hook is not None:
            hook(step, ids)
        busy = eng.step()
        for rid, tok, idx, reason, _ in eng.poll():
            if tok >= 0:
                ev.setdefault(rid, []).append((idx, int(tok)))
            if reason >= 0:
                fin[rid] = reason
        recs += eng.poll_logprobs()
        step += 1
        assert step < 2000
    return ids, ev, fin, recs


def _requests(V, first_plain):
    p = [synth.prompt_tokens(3 + (7 * i) % 20, V, seed=900 + i) for i in range(7)]
    return [dict(prompt=p[0], max_tokens=5, logprobs=True, top_logprobs=5, logit_bias={FORCED: 1000.0}, **GREEDY),      # a forcing bias; ends first: its row is reused
            dict(prompt=p[1], max_tokens=12, logprobs=True, top_logprobs=0, **SAMPLED),
            dict(prompt=p[2], max_tokens=14, logprobs=True, top_logprobs=20, **PENALISED),
            dict(prompt=p[3], max_tokens=10, logprobs=True, top_logprobs=5, logit_bias={first_plain: -1000.0} if first_plain is not None else None, **GREEDY),   # a ban
            dict(prompt=p[4], max_tokens=12, **GREEDY),                                                                # no extras; takes the row the forced request leaves
            dict(prompt=p[5], max_tokens=8, logprobs=True, top_logprobs=5, **GREEDY),
            dict(prompt=p[6], max_tokens=10, **GREEDY)]                                                                # in the main run: a grammar state plus a bias


def _plain(kw):
    return {k: v for k, v in kw.items() if k not in ("logprobs", "top_logprobs", "logit_bias", "grammar_state")}


def test_mixed_requests(device):
    model, lm = _model(device, PRESET)
    V = model["config"]["vocab"]
    vocab = G.synth_vocab(V, seed=21)[0]
    # the same engine with logprobs = 0, no request with extras
    base_reqs = _requests(V, None)
    ids0, ev0, fin0, recs0 = _drive(_engine(lm, False), [_plain(kw) for kw in base_reqs])
    assert recs0 == []
    base = [[t for _, t in ev0[i]] for i in ids0]
    # the main run
    dfa = runtime.GrammarDfa(LITERALS)
    dg = dfa.to_device(device, vocab)
    cur = runtime.GrammarCursor(dg, NROWS)
    g_plain = runtime.Executor(lm).generate(base_reqs[6]["prompt"], 10, grammar=runtime.GrammarDfa(LITERALS), vocab_bytes=vocab).tolist()
    reqs = _requests(V, base[3][0])
    reqs[6].update(grammar_state=0, logit_bias={g_plain[0]: -1000.0, V + 7: 3.0})
    eng = _engine(lm, True, grammar=cur)
    ids, ev, fin, recs = _drive(eng, reqs)
    toks = [[t for _, t in ev[i]] for i in ids]
    assert all(fin[i] == 0 and len(toks[k]) == reqs[k]["max_tokens"] for k, i in enumerate(ids))
    for k in (1, 2, 4, 5):                                               # without a bias: the tokens of the engine without the feature
        assert toks[k] == base[k], k
    assert toks[0] == [FORCED] * 5 and base[0] != toks[0]
    assert toks[3][0] != base[3][0] and base[3][0] not in toks[3]
    ex = runtime.Executor(lm)
    for k in (0, 3):                                                     # biased greedy requests: the single-sequence loop with the same bias
        assert toks[k] == ex.generate(reqs[k]["prompt"], reqs[k]["max_tokens"], logit_bias=reqs[k]["logit_bias"]).tolist(), k
    want6 = ex.generate(reqs[6]["prompt"], 10, grammar=runtime.GrammarDfa(LITERALS), vocab_bytes=vocab, logit_bias=reqs[6]["logit_bias"]).tolist()
    assert toks[6] == want6 and toks[6] != g_plain
    assert runtime.GrammarDfa(LITERALS).advance_tokens(vocab, toks[6]) == 0                    # the bias moved the pick inside the grammar
    # records: one per event of the asking requests, same id / index / token, in event order; none for the others
    asking = {ids[k]: reqs[k]["top_logprobs"] for k in (0, 1, 2, 3, 5)}
    by = {}
    for d in recs:
        by.setdefault(d["id"], []).append(d)
    assert set(by) == set(asking)
    for rid, top in asking.items():
        assert [(d["index"], d["token"]) for d in by[rid]] == ev[rid], rid
        for d in by[rid]:
            assert len(d["top_ids"]) == len(d["top_logprobs"]) == top and d["logprob"] <= 0.0, (rid, d)
            assert d["top_logprobs"] == sorted(d["top_logprobs"], reverse=True)
            if top:
                assert d["logprob"] <= d["top_logprobs"][0]
    for d in by[ids[5]]:                                                 # greedy without a bias: the token is the first alternative
        assert d["top_ids"][0] == d["token"] and d["logprob"] == d["top_logprobs"][0]
    assert any(d["top_ids"][0] != FORCED and d["logprob"] < d["top_logprobs"][0] for d in by[ids[0]])   # a forced token reports its RAW logprob
    # a sampled request's chosen logprob is its entry among the alternatives whenever the token is listed
    for d in by[ids[2]]:
        if d["token"] in d["top_ids"]:
            assert d["logprob"] == d["top_logprobs"][d["top_ids"].index(d["token"])]
    st = eng.stats()
    assert st["free_blocks"] == st["total_blocks"] - st["park_blocks"] and st["live_rows"] == 0
    assert (cur.read()[0] == runtime.GrammarCursor.FREE).all()
    # results through the convenience loop
    eng2 = _engine(lm, True)
    rid = eng2.submit(reqs[5]["prompt"], 8, logprobs=True, top_logprobs=5, **GREEDY)
    out = eng2.run_until_idle()
    assert out[rid][0] == toks[5] and [d["token"] for d in eng2.logprobs[rid]] == toks[5]
    assert [(d["top_ids"], d["top_logprobs"], d["logprob"]) for d in eng2.logprobs[rid]] == [(d["top_ids"], d["top_logprobs"], d["logprob"]) for d in by[ids[5]]]


def test_row_reuse_and_cancel(device):
    model, lm = _model(device, PRESET)
    V = model["config"]["vocab"]
    p = [synth.prompt_tokens(5 + 3 * i, V, seed=950 + i) for i in range(6)]
    plain = [dict(prompt=p[i], max_tokens=9, **GREEDY) for i in range(6)]
    ids0, ev0, _, _ = _drive(_engine(lm, False), plain)
    base = [[t for _, t in ev0[i]] for i in ids0]
    # four requests that all carry a forcing bias and logprobs fill the rows and end together; two plain ones then take rows 0 and 1
    first = [dict(plain[i], max_tokens=4, logprobs=True, top_logprobs=3, logit_bias={FORCED + i: 1000.0}) for i in range(4)]
    eng = _engine(lm, True)
    ids, ev, fin, recs = _drive(eng, first + plain[4:])
    for i in range(4):
        assert [t for _, t in ev[ids[i]]] == [FORCED + i] * 4
    for k in (4, 5):                                                    # the reused rows start with an empty bias list and logprobs off
        assert [t for _, t in ev[ids[k]]] == base[k], k
    assert {d["id"] for d in recs} == set(ids[:4]) and len(recs) == 16
    # cancel: the records of tokens still in flight are dropped with their events
    eng = _engine(lm, True)
    long = dict(prompt=p[0], max_tokens=40, logprobs=True, top_logprobs=2, **GREEDY)
    other = dict(prompt=p[1], max_tokens=20, logprobs=True, top_logprobs=1, **GREEDY)

    def hook(step, ids):
        if step == 6:
            eng.cancel(ids[0])
    ids, ev, fin, recs = _drive(eng, [long, other], hook)
    assert fin[ids[0]] == 2 and fin[ids[1]] == 0
    got = [(d["index"], d["token"]) for d in recs if d["id"] == ids[0]]
    assert got == ev[ids[0]] and len(got) <= 6
    assert [(d["index"], d["token"]) for d in recs if d["id"] == ids[1]] == ev[ids[1]] and len(ev[ids[1]]) == 20


def test_refusals_name_the_figure(device):
    model, lm = _model(device, PRESET)
    V = model["config"]["vocab"]
    p = synth.prompt_tokens(5, V, seed=980)

    def refused(fn, *words):
        with pytest.raises(L.BlazrHipError) as e:
            fn()
        assert e.value.code == L.E_INVALID and all(w in str(e.value) for w in words), str(e.value)
    off = _engine(lm, False)
    refused(lambda: off.submit(p, 4, logprobs=True), "logprobs = 0")
    refused(lambda: off.submit(p, 4, logit_bias={3: 1.0}), "logprobs = 0")
    on = _engine(lm, True)
    refused(lambda: on.submit(p, 4, logprobs=True, top_logprobs=21), "top_logprobs = 21")
    refused(lambda: on.submit(p, 4, logprobs=True, top_logprobs=-1), "top_logprobs = -1")
    refused(lambda: on.submit(p, 4, logit_bias={3: float("nan")}), "not a finite number")
    refused(lambda: on.submit(p, 4, logit_bias={i: 1.0 for i in range(513)}), "513")

    def negative():
        rq = L.Request(max_tokens=4, grammar_state=L.GRAMMAR_ROW_FREE)
        rq.sampling = L.RowSampling(**GREEDY)
        ex = L.RequestExtras(n_logit_bias=-1)
        pp = np.ascontiguousarray(p, dtype=np.int64)
        rid = C.c_int64()
        L.check(L.lib().bz_engine_submit_ex(on.h, pp.ctypes.data_as(C.c_void_p), len(pp), C.byref(rq), C.byref(ex), C.byref(rid)))
    refused(negative, "n_logit_bias = -1")
    assert on.step() is False and on.stats()["waiting"] == 0             # nothing of the above was queued
    refused(lambda: _engine(lm, True, sampler=False), "use_sampler = 0")
    rid = on.submit(p, 4, logprobs=True)                                 # and the engine still works
    assert len(on.run_until_idle()[rid][0]) == 4 and len(on.logprobs[rid]) == 4


def test_bz_run_logprobs(device, tmp_path):
    # tools/bz_run.cpp --requests with --logprobs / --logit-bias: the records on stderr, the biased tokens on stdout
    import os
    import subprocess
    import ckpt_writer as W
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "blazr_amd", "bz-run")
    assert os.path.exists(exe), "bz-run was not built (python -c 'import __graft_entry__ as g; g.build()')"
    model, lm = _model(device, PRESET)
    ck = tmp_path / "ck"
    ck.mkdir()
    W.write_hf_checkpoint(str(ck), model, shards=1)
    reqs = [(4, synth.prompt_tokens(5, 1024, seed=991)), (6, synth.prompt_tokens(11, 1024, seed=992)), (3, synth.prompt_tokens(2, 1024, seed=993))]
    (tmp_path / "requests.txt").write_text("".join("%d;%s\n" % (mt, ",".join(str(int(t)) for t in p)) for mt, p in reqs))
    r = subprocess.run([exe, str(ck), "--requests", str(tmp_path / "requests.txt"), "--rows", "2", "--logprobs", "3", "--logit-bias", "%d:1000,2000:1.5" % FORCED],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert [[int(x) for x in ln.split(",")] for ln in r.stdout.strip().split("\n")] == [[FORCED] * mt for mt, _ in reqs], (r.stdout, r.stderr)
    lines = [ln for ln in r.stderr.split("\n") if ln.startswith("logprobs: ")]
    assert len(lines) == sum(mt for mt, _ in reqs)
    assert all(" = %d -" % FORCED in ln and ln.count(":") == 1 + 3 and " top " in ln for ln in lines), lines     # a negative (raw) logprob and three alternatives
    assert sorted(ln.split(" = ")[0] for ln in lines) == sorted("logprobs: request %d token %d" % (i, k) for i, (mt, _) in enumerate(reqs) for k in range(mt))
    # the same engine from here
    eng = runtime.BatchEngine(lm, 2, 2 * 2 + 2, BS, 17, 0, 2, True, logprobs=True)
    rid = eng.submit(reqs[0][1], 4, logprobs=True, top_logprobs=3, logit_bias={FORCED: 1000.0, 2000: 1.5}, **GREEDY)
    eng.run_until_idle()
    first = [ln for ln in lines if ln.startswith("logprobs: request 0 token 0 ")][0]
    want = eng.logprobs[rid][0]
    assert first == "logprobs: request 0 token 0 = %d %.6f top %s" % (FORCED, want["logprob"], ",".join("%d:%.6f" % (i, v) for i, v in zip(want["top_ids"], want["top_logprobs"])))
