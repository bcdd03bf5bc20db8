"""The request engine (blazr_amd/csrc/bz_engine.hip, bz_sched.hip; runtime.BatchEngine) on the device.  Every token comparison is exact: the engine, the
static batch graph and a request run alone launch the same kernels at the same N, and a row of the multi-row step depends on nothing in the other rows
(tests/test_gpu_batch_sampler.py relies on the same).  References: the existing API driven from the test (forward_with_paged_kv_cache + BatchDecodeGraph), the
request's alone run (the same engine configuration, that request the only one ever submitted), and tests/engine_ref.py for the host's decisions."""
import numpy as np
import pytest

import engine_ref as R
import grammar_ref as G
from blazr_amd import _lib as L
from blazr_amd import runtime, synth
from test_gpu_grammar import _model
from test_gpu_llama import _kv_dt
from test_grammar_rows import LITERALS, REGULAR

pytestmark = pytest.mark.gpu

PRESETS = ["tiny-awq", "tiny-bf16"]
NROWS, BS = 4, 16
NONE = dict(repeat_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0, repeat_last_n=64)
GREEDY = dict(NONE, temperature=0.0, top_k=0, top_p=1.0, min_p=0.0, seed=0)
# the four parameter sets of test_sampled_batch_graph
PARAMS = [dict(NONE, temperature=0.8, top_k=12, top_p=1.0, min_p=0.02, seed=211),
          GREEDY,
          dict(temperature=1.0, top_k=10, top_p=0.9, min_p=0.0, repeat_penalty=1.2, frequency_penalty=0.0, presence_penalty=0.0, repeat_last_n=16, seed=212),
          dict(temperature=1.3, top_k=8, top_p=1.0, min_p=0.05, repeat_penalty=1.0, frequency_penalty=0.3, presence_penalty=0.1, repeat_last_n=64, seed=213)]
_ALONE = {}


def _engine(lm, max_seq_len=80, num_blocks=None, chunk=0, depth=2, sampler=True, grammar=None):
    per = -(-max_seq_len // BS)
    return runtime.BatchEngine(lm, NROWS, NROWS * per + NROWS if num_blocks is None else num_blocks, BS, max_seq_len, chunk, depth, sampler, grammar)


def _drive(eng, schedule, hook=None):
    """schedule: [(step, request kwargs)] by step; a request scheduled for step s is submitted before that step.  hook(step, ids) runs before every step.
    -> (ids, {id: dict(tokens, idx, reason, first: the replay of its first token)}, steps)"""
    pending, ids, res, step = list(schedule), [], {}, 0
    while True:
        while pending and pending[0][0] <= step:
            ids.append(eng.submit(**pending.pop(0)[1]))
        if hook is not None:
            hook(step, ids)
        busy = eng.step()
        for rid, tok, idx, fin, rep in eng.poll():
            r = res.setdefault(rid, dict(tokens=[], idx=[], reason=-1, first=None))
            if tok >= 0:
                r["tokens"].append(int(tok)); r["idx"].append(idx)
                if r["first"] is None:
                    r["first"] = rep
            if fin >= 0:
                assert r["reason"] == -1
                r["reason"] = fin
        step += 1
        assert step < 3000
        if not busy and not pending:
            return ids, res, step


def _alone(preset, lm, req, grammar_dg=None, **cfg):
    """the request's alone run on a fresh engine of the same configuration -> (tokens, finish reason)"""
    key = (preset, tuple(sorted(cfg.items())), repr(sorted((k, np.asarray(v).tolist()) for k, v in req.items())))
    if key not in _ALONE:
        cur = runtime.GrammarCursor(grammar_dg, NROWS) if grammar_dg is not None else None
        eng = _engine(lm, grammar=cur, **cfg)
        (rid,), res, _ = _drive(eng, [(0, req)])
        st = eng.stats()
        assert st["free_blocks"] == st["total_blocks"] - st["park_blocks"] and st["live_rows"] == 0 and st["unread"] == 0
        _ALONE[key] = (res[rid]["tokens"], res[rid]["reason"])
    return _ALONE[key]


def _cut(tokens, stop):
    """tokens up to and including the first stop id -> (tokens, finish reason)"""
    for i, t in enumerate(tokens):
        if t in stop:
            return tokens[:i + 1], 1
    return tokens, 0


def _static(device, model, lm, prompts, steps, per, params=None, chunks=None):
    """The loop through the existing API on a fresh pool: forward_with_paged_kv_cache(prompt[:-1]) (in `chunks`-token pieces if given), BatchDecodeGraph.seed(prompt[-1],
    len(prompt), tables), `steps` replays -> tokens [row][step]"""
    cfg = model["config"]
    nseq = len(prompts)
    pool = runtime.LayeredPagedKvCache(device, cfg["n_layers"], nseq * per, BS, cfg["n_kv_heads"], cfg["head_dim"], _kv_dt(cfg))
    tables = [[i + nseq * j for j in range(per)] for i in range(nseq)]
    for p, tb in zip(prompts, tables):
        n = len(p) - 1
        step = chunks if chunks else max(n, 1)
        for a in range(0, n, step):
            b = min(n, a + step)
            lm.forward_with_paged_kv_cache(p[a:b], pool, [tb[i // BS] * BS + i % BS for i in range(a, b)], tb, b, a)
    sampler = None
    if params is not None:
        sampler = runtime.BatchSampler(device, nseq, cfg["vocab"])
        for r in range(nseq):
            sampler.set_row(r, history=list(map(int, prompts[r])), draw_index=0, **params[r])
    g = runtime.BatchDecodeGraph(lm, pool, nseq, per, sampler=sampler)
    g.seed([int(p[-1]) for p in prompts], [len(p) for p in prompts], tables)
    for _ in range(steps):
        g.replay()
    out = np.stack([g.read_tokens(s) for s in range(steps)], axis=1)
    return [out[r].tolist() for r in range(nseq)]


def _four_prompts(V):
    return [synth.prompt_tokens(3 + (13 * i) % 30, V, seed=70 + i) for i in range(NROWS)]


@pytest.mark.parametrize("preset", PRESETS)
def test_static_equivalence_greedy(device, preset):
    model, lm = _model(device, preset)
    prompts = _four_prompts(model["config"]["vocab"])
    want = _static(device, model, lm, prompts, 24, 5)
    for depth in (1, 4):
        eng = _engine(lm, depth=depth, sampler=False)
        ids, res, _ = _drive(eng, [(0, dict(prompt=p, max_tokens=24)) for p in prompts])
        for r, rid in enumerate(ids):
            assert res[rid]["tokens"] == want[r], (depth, r)
            assert res[rid]["reason"] == 0 and res[rid]["idx"] == list(range(24)) and res[rid]["first"] == 0
        assert eng.stats()["replays"] == 24 + depth - 1              # the host learns of the end `depth` - 1 replays late


@pytest.mark.parametrize("preset", PRESETS)
def test_static_equivalence_sampled(device, preset):
    model, lm = _model(device, preset)
    prompts = _four_prompts(model["config"]["vocab"])
    want = _static(device, model, lm, prompts, 24, 5, params=PARAMS)
    assert len({tuple(w) for w in want}) == 4
    for depth in (1, 4):
        eng = _engine(lm, depth=depth)
        ids, res, _ = _drive(eng, [(0, dict(prompt=p, max_tokens=24, **PARAMS[r])) for r, p in enumerate(prompts)])
        for r, rid in enumerate(ids):
            assert res[rid]["tokens"] == want[r], (depth, r)


@pytest.mark.parametrize("preset", PRESETS)
def test_churn(device, preset):
    model, lm = _model(device, preset)
    V = model["config"]["vocab"]
    cfg = dict(max_seq_len=96, depth=3)
    plens = [1, 2, 15, 16, 17, 31, 33, 40, 5, 24]                   # 1 token .. across three blocks
    mts = [40, 5, 1, 2, 17, 40, 5, 17, 2, 1]                        # from {1, 2, 5, 17, 40}
    reqs = []
    for i in range(10):
        kw = dict(prompt=synth.prompt_tokens(plens[i], V, seed=300 + i), max_tokens=mts[i], **PARAMS[i % 4])   # greedy and sampled mixed
        full, reason = _alone(preset, lm, kw, **cfg)
        assert len(full) == mts[i] and reason == 0
        if i % 2 == 0:                                              # half carry stop ids from their own output, so that stops certainly fire
            kw["stop"] = tuple(sorted({full[min(2, len(full) - 1)], full[min(8, len(full) - 1)]}))
        reqs.append((kw, _cut(full, kw.get("stop", ()))))
    schedule = [(0 if i < 5 else 3 * (i - 4), kw) for i, (kw, _) in enumerate(reqs)]
    eng = _engine(lm, **cfg)
    ids, res, _ = _drive(eng, schedule)
    assert ids == list(range(10))
    for rid, (kw, (want, reason)) in zip(ids, reqs):
        assert res[rid]["tokens"] == want, rid
        assert res[rid]["reason"] == reason, rid
        assert res[rid]["idx"] == list(range(len(want))), rid
    assert {r[1][1] for r in reqs} == {0, 1}                        # both ends occur
    sim = R.simulate_engine(NROWS, NROWS * 6 + NROWS, BS, 96, 0, 3, [(s, len(kw["prompt"]), kw["max_tokens"], len(w)) for (s, kw), (_, (w, _)) in zip(schedule, reqs)])
    st = eng.stats()
    assert st["replays"] == sim["replays"]
    assert {rid: res[rid]["first"] for rid in ids} == sim["first_replay"]
    assert st["free_blocks"] == st["total_blocks"] - st["park_blocks"] == NROWS * 6 and st["live_rows"] == 0 and st["waiting"] == 0 and st["unread"] == 0
    assert st["generated_tokens"] == sum(len(w) for _, (w, _) in reqs) and st["prompt_tokens"] == sum(n - 1 for n in plens)
    assert eng.step() is False                                      # busy == 0


@pytest.mark.parametrize("preset", PRESETS)
def test_the_device_ends_rows_by_itself(device, preset):
    model, lm = _model(device, preset)
    V = model["config"]["vocab"]
    cfg = dict(max_seq_len=80, depth=8, sampler=False)
    a = dict(prompt=synth.prompt_tokens(9, V, seed=401), max_tokens=30)
    b = dict(prompt=synth.prompt_tokens(20, V, seed=402), max_tokens=30)
    c = dict(prompt=synth.prompt_tokens(18, V, seed=403), max_tokens=6)
    full_a, _ = _alone(preset, lm, a, **cfg)
    stop = full_a[2]
    want_a, _ = _cut(full_a, (stop,))
    a = dict(a, stop=(stop,))
    eng = _engine(lm, **cfg)
    state = dict(c_at=None)

    def hook(step, ids):
        if state["c_at"] is None and len(ids) == 2 and eng.stats()["admitted"] == 1:   # a's end has been harvested: its row and blocks are free
            state["c_at"] = step
            ids.append(eng.submit(**c))
    ids, res, _ = _drive(eng, [(0, a), (0, b)], hook)
    assert res[ids[0]]["tokens"] == want_a and res[ids[0]]["reason"] == 1
    assert res[ids[1]] ["tokens"] == _alone(preset, lm, b, **cfg)[0] and res[ids[1]]["reason"] == 0
    assert res[ids[2]]["tokens"] == _alone(preset, lm, c, **cfg)[0]
    end = len(want_a) - 1                                           # a's last replay
    # the host harvests replay `end` in step end + depth: every replay up to end + depth - 1 was enqueued while the host still took the row for live
    assert state["c_at"] == end + 8 + 1 and res[ids[2]]["first"] == end + 8 + 1
    for r in range(res[ids[2]]["first"]):
        st, live = eng.read_status(r)
        assert st[0] == (1 if r < end else 6 if r == end else 0), (r, st)       # 6 = finished, reason stop
        assert st[1] == 1 and st[2] == 0 and st[3] == 0 and live == (2 if r < end else 1), (r, st, live)
    st, _ = eng.read_status(res[ids[2]]["first"])
    assert st[0] == 1 and st[1] == 1                                # c took the released row 0
    # the finish rule of the restatement on replay `end`
    toks = np.array([want_a[-1], res[ids[1]]["tokens"][end], 0, 0])
    stops = np.zeros((4, 8), dtype=np.int64); stops[0, 0] = stop
    left, ended, reason = R.finish_rule(np.array([True, True, False, False]), np.array([30 - end, 30 - end, 0, 0]), toks, stops, np.array([1, 0, 0, 0]))
    assert ended.tolist() == [True, False, False, False] and reason[0] == 1


@pytest.mark.parametrize("preset", PRESETS)
def test_pool_pressure(device, preset):
    model, lm = _model(device, preset)
    V = model["config"]["vocab"]
    cfg = dict(max_seq_len=64, num_blocks=7 + NROWS, depth=2)       # every request needs 3 blocks: two at a time
    reqs = [dict(prompt=synth.prompt_tokens(20 + 2 * i, V, seed=500 + i), max_tokens=13 + i, **PARAMS[i % 4]) for i in range(6)]
    eng = _engine(lm, **cfg)
    seen = []
    ids, res, _ = _drive(eng, [(0, kw) for kw in reqs], lambda step, ids: seen.append(eng.stats()["admitted"]))
    assert max(seen) == 2
    for rid, kw in zip(ids, reqs):
        assert (res[rid]["tokens"], res[rid]["reason"]) == _alone(preset, lm, kw, **cfg), rid
    firsts = [res[rid]["first"] for rid in ids]
    assert firsts == sorted(firsts) and firsts[2] > firsts[1]       # in submission order
    sim = R.simulate_engine(NROWS, 7 + NROWS, BS, 64, 0, 2, [(0, len(kw["prompt"]), kw["max_tokens"], kw["max_tokens"]) for kw in reqs])
    assert sim["admitted"] == ids and sim["first_replay"] == dict(zip(ids, firsts)) and sim["replays"] == eng.stats()["replays"]


@pytest.mark.parametrize("preset", PRESETS)
def test_chunked_prefill(device, preset):
    model, lm = _model(device, preset)
    V = model["config"]["vocab"]
    cfg = dict(max_seq_len=176, chunk=32, depth=2, sampler=False)
    old = [dict(prompt=synth.prompt_tokens(5 + 7 * i, V, seed=600 + i), max_tokens=30) for i in range(3)]
    new = dict(prompt=synth.prompt_tokens(150, V, seed=610), max_tokens=12)
    eng = _engine(lm, **cfg)
    ids, res, _ = _drive(eng, [(0, kw) for kw in old] + [(3, new)])
    ids0, res0, _ = _drive(_engine(lm, **cfg), [(0, kw) for kw in old])
    for i in range(3):
        assert res[ids[i]]["tokens"] == res0[ids0[i]]["tokens"] and len(res0[ids0[i]]["tokens"]) == 30, i      # the newcomer changes nothing for the others
    assert res[ids[3]]["first"] == 3 + 4                             # prompt[:-1] = 149 tokens = 5 chunks over steps 3 .. 7
    assert res[ids[3]]["tokens"] == _alone(preset, lm, new, **cfg)[0]
    # the existing API: the same chunks through forward_with_paged_kv_cache, then a seeded static graph (its other rows are one-token sequences)
    filler = [np.array([1 + i], dtype=np.int64) for i in range(3)]
    assert res[ids[3]]["tokens"] == _static(device, model, lm, [new["prompt"]] + filler, 12, 11, chunks=32)[0]
    assert eng.stats()["prompt_tokens"] == 149 + sum(len(kw["prompt"]) - 1 for kw in old)


@pytest.mark.parametrize("preset", PRESETS)
def test_grammar_rows(device, preset):
    model, lm = _model(device, preset)
    V = model["config"]["vocab"]
    vocab = G.synth_vocab(V, seed=21)[0]
    parts = [runtime.GrammarDfa(LITERALS), runtime.GrammarDfa(REGULAR, regular=True)]
    cat, starts = runtime.GrammarDfa.concat(parts)
    dg = cat.to_device(device, vocab)
    prompts = _four_prompts(V)
    reqs = [dict(prompt=prompts[0], max_tokens=16, grammar_state=starts[0], **GREEDY),
            dict(prompt=prompts[1], max_tokens=16, grammar_state=starts[1], **dict(NONE, temperature=0.8, top_k=12, top_p=1.0, min_p=0.02, seed=311)),
            dict(prompt=prompts[2], max_tokens=16, **dict(NONE, temperature=1.0, top_k=10, top_p=0.9, min_p=0.0, seed=312)),
            dict(prompt=prompts[3], max_tokens=16, **GREEDY)]
    cur = runtime.GrammarCursor(dg, NROWS)
    eng = _engine(lm, grammar=cur)
    ids, res, _ = _drive(eng, [(0, kw) for kw in reqs])
    for i in (0, 1):                                                # accepted by the host DFA: no byte without a transition
        assert len(res[ids[i]]["tokens"]) == 16
        assert parts[i].advance_tokens(vocab, res[ids[i]]["tokens"]) == 0, i
    for i, kw in enumerate(reqs):
        assert (res[ids[i]]["tokens"], res[ids[i]]["reason"]) == _alone(preset, lm, kw, grammar_dg=dg), i
    free = _alone(preset, lm, dict(reqs[0], grammar_state=None), grammar_dg=dg)[0]
    assert free != res[ids[0]]["tokens"]                            # the constraint binds
    st, rej = cur.read()
    assert (st == runtime.GrammarCursor.FREE).all()                 # rows that ended were freed on the device


@pytest.mark.parametrize("preset", PRESETS)
def test_cancel(device, preset):
    model, lm = _model(device, preset)
    V = model["config"]["vocab"]
    cfg = dict(max_seq_len=80, depth=3)
    reqs = [dict(prompt=synth.prompt_tokens(6 + 5 * i, V, seed=700 + i), max_tokens=28, **PARAMS[i]) for i in range(3)]
    late = dict(prompt=synth.prompt_tokens(21, V, seed=710), max_tokens=9, **PARAMS[3])
    eng = _engine(lm, **cfg)

    def hook(step, ids):
        if step == 6:
            eng.cancel(ids[1])
            ids.append(eng.submit(**late))
    ids, res, _ = _drive(eng, [(0, kw) for kw in reqs], hook)
    for i in (0, 2):
        assert (res[ids[i]]["tokens"], res[ids[i]]["reason"]) == _alone(preset, lm, reqs[i], **cfg), i
    gone = res[ids[1]]
    assert gone["reason"] == 2 and gone["tokens"] == _alone(preset, lm, reqs[1], **cfg)[0][:len(gone["tokens"])] and len(gone["tokens"]) <= 6
    assert (res[ids[3]]["tokens"], res[ids[3]]["reason"]) == _alone(preset, lm, late, **cfg)
    st, _ = eng.read_status(res[ids[3]]["first"])
    assert st.tolist()[:3] == [1, 1, 1]                             # the cancelled row 1 is in use again
    s = eng.stats()
    assert s["free_blocks"] == s["total_blocks"] - s["park_blocks"] and s["live_rows"] == 0


def test_refusals(device):
    model, lm = _model(device, "tiny-awq")
    V = model["config"]["vocab"]
    p = synth.prompt_tokens(40, V, seed=800)

    def refused(fn, code, *words):
        with pytest.raises(L.BlazrHipError) as e:
            fn()
        assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)
    eng = _engine(lm, max_seq_len=80, num_blocks=2 + NROWS, sampler=False)
    refused(lambda: eng.submit(p, 41), L.E_INVALID, "81", "max_seq_len = 80")
    refused(lambda: eng.submit(p, 8), L.E_INVALID, "3 blocks", "could never fit")
    refused(lambda: eng.submit(p[:5], 8, stop=range(9)), L.E_INVALID, "n_stop = 9")
    refused(lambda: eng.submit(p[:5], 8, temperature=0.7), L.E_INVALID, "temperature = 0.7", "without a sampler")
    refused(lambda: eng.submit(p[:5], 8, repeat_penalty=1.1), L.E_INVALID, "without a sampler")
    refused(lambda: eng.submit(p[:5], 8, grammar_state=3), L.E_INVALID, "grammar_state = 3", "without a grammar cursor")
    assert eng.step() is False and eng.stats()["waiting"] == 0      # nothing of the above was queued
    rid = eng.submit(p[:5], 8)                                      # and the engine still works
    assert len(eng.run_until_idle()[rid][0]) == 8
    refused(lambda: runtime.BatchEngine(lm, 1, 16), L.E_INVALID, "n_rows = 1")
    refused(lambda: runtime.BatchEngine(lm, 4, 16, depth=65), L.E_INVALID, "depth = 65")
    refused(lambda: runtime.BatchEngine(lm, 4, 4), L.E_INVALID, "num_blocks = 4")
    _, mlm = _model(device, "tiny-mamba2")
    refused(lambda: runtime.BatchEngine(mlm, 4, 16, max_seq_len=64), L.E_UNSUPPORTED, "llama family")


def test_bz_run_requests(device, tmp_path):
    # tools/bz_run.cpp --requests: the engine driven from compiled C++ over a checkpoint on disk, against the same engine driven from here
    import os
    import subprocess
    import ckpt_writer as W
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "blazr_amd", "bz-run")
    assert os.path.exists(exe), "bz-run was not built (python -c 'import __graft_entry__ as g; g.build()')"
    model, lm = _model(device, "tiny-awq")
    ck = tmp_path / "ck"
    ck.mkdir()
    W.write_hf_checkpoint(str(ck), model, shards=1)
    reqs = [(6, synth.prompt_tokens(4, 1024, seed=901)), (20, synth.prompt_tokens(37, 1024, seed=902)), (1, synth.prompt_tokens(1, 1024, seed=903)),
            (11, synth.prompt_tokens(18, 1024, seed=904)), (9, synth.prompt_tokens(9, 1024, seed=905))]
    (tmp_path / "requests.txt").write_text("".join("%d;%s\n" % (mt, ",".join(str(int(t)) for t in p)) for mt, p in reqs))
    # what bz-run sets up: max_seq_len = the longest request (57), the default pool, depth 2, no sampler for greedy options
    eng = runtime.BatchEngine(lm, 2, 2 * 4 + 2, BS, 57, 16, 2, False)
    ids, res, _ = _drive(eng, [(0, dict(prompt=p, max_tokens=mt)) for mt, p in reqs])
    r = subprocess.run([exe, str(ck), "--requests", str(tmp_path / "requests.txt"), "--rows", "2", "--prefill-chunk", "16"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    assert [[int(x) for x in ln.split(",")] for ln in lines] == [res[i]["tokens"] for i in ids], (r.stdout, r.stderr)
    assert "engine: %d replays" % eng.stats()["replays"] in r.stderr and "47 generated tokens" in r.stderr
    r = subprocess.run([exe, str(ck), "--requests", str(tmp_path / "requests.txt")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--rows" in r.stderr
