"""Per-request LoRA adapters in the batched decode graph and the request engine, in the comparison style of tests/test_gpu_engine.py: token ids, exactly.

Two references per request.  (1) Its ALONE run -- the same engine configuration, that request the only one ever submitted: the same kernels at the same N, and a
row of the multi-row step depends on nothing in the other rows, so the ids are equal without condition.  (2) Single-sequence generation under the same adapter
(Executor.generate: the decode GEMVs, not the multi-row GEMMs): the ids are equal up to the first near-tie of the single-sequence logits (top-2 gap below
2e-3 of the largest magnitude, the rule of smoke()), where two correct paths may pick different tokens; for the int4 model, whose multi-row step runs the decode
kernels' exact sums, the whole run is compared whatever the gaps."""
import ctypes as C

import numpy as np
import pytest

from blazr_amd import _lib as L
from blazr_amd import runtime, synth
import lora_cases
from test_gpu_llama import _kv_dt

pytestmark = pytest.mark.gpu

NROWS, BS, STEPS = 4, 16, 16
SPLIT_BARS = {"f16": 1.5e-3, "bf16": 2.0 ** -7}      # test_gpu_long_context.py
CASES = [("tiny-awq", "all"), ("tiny-bf16", "qv")]
ROWS = [None, "a1", "a2", "a1"]           # the adapters of the four rows


def _setup(device, key, mask):
    model = lora_cases.model(key)
    lm = runtime.LoadedModel.from_synth(device, model)
    lm.enable_lora(n_slots=4, max_rank=16, targets=lora_cases.MASKS[mask])
    for s in (1, 2):
        ad = lora_cases.adapter(key, mask, s)
        lm.load_lora(runtime.LoraAdapter.from_arrays(device, ad["rank"], ad["alpha"], ad["pairs"]), "a%d" % s)
    return model, lm


def _prompts(V, n=NROWS, seed=80):
    return [[int(t) for t in synth.prompt_tokens(3 + (11 * i) % 23, V, seed=seed + i)] for i in range(n)]


def _engine(lm, max_seq_len=64, prefix_cache=False, depth=2):
    per = -(-max_seq_len // BS)
    return runtime.BatchEngine(lm, NROWS, NROWS * per + NROWS, BS, max_seq_len, 0, depth, False, None, prefix_cache)


def _drive(eng, schedule, hook=None):
    """schedule: [(step, submit kwargs)]; -> (ids in submission order, {id: tokens})"""
    pending, ids, res, step = list(schedule), [], {}, 0
    while True:
        while pending and pending[0][0] <= step:
            ids.append(eng.submit(**pending.pop(0)[1]))
        if hook is not None:
            hook(step, ids)
        busy = eng.step()
        for rid, tok, idx, fin, rep in eng.poll():
            if tok >= 0:
                res.setdefault(rid, []).append(int(tok))
        step += 1
        assert step < 2000
        if not busy and not pending:
            return ids, res


_ALONE = {}


def _alone(key, mask, lm, prompt, n, name, **cfg):
    k = (key, mask, tuple(prompt), n, name, tuple(sorted(cfg.items())))
    if k not in _ALONE:
        (rid,), res = _drive(_engine(lm, **cfg), [(0, dict(prompt=prompt, max_tokens=n, lora=name))])
        _ALONE[k] = res[rid]
    return _ALONE[k]


def _single(lm, prompt, n, name):
    """single-sequence greedy generation under `name` -> (tokens, number of leading tokens before the first near-tie)"""
    toks = [int(t) for t in runtime.Executor(lm).generate(prompt, n, lora_adapter=name)]
    lm.set_lora(name)
    kv = lm.new_kv_cache(len(prompt) + n + 8)
    for i, t in enumerate(prompt):
        lg = lm.forward_with_kv_cache([t], kv, i).to_numpy().reshape(-1)
    sure = n
    for j in range(n):
        srt = np.sort(lg)
        assert int(np.argmax(lg)) == toks[j]
        if srt[-1] - srt[-2] < 2e-3 * max(1.0, float(np.abs(lg).max())):
            sure = j
            break
        lg = lm.forward_with_kv_cache([toks[j]], kv, len(prompt) + j).to_numpy().reshape(-1)
    lm.set_lora(None)
    return toks, sure


def _check_single(key, got, lm, prompt, n, name):
    want, sure = _single(lm, prompt, n, name)
    if key == "tiny-awq":
        assert got == want, (name, got, want)
    else:
        assert got[:sure] == want[:sure], (name, sure, got, want)


@pytest.mark.parametrize("key,mask", CASES)
def test_batch_graph_rows_under_their_own_adapters(device, key, mask):
    model, lm = _setup(device, key, mask)
    cfg = model["config"]
    prompts, per = _prompts(cfg["vocab"]), 4
    pool = runtime.LayeredPagedKvCache(device, cfg["n_layers"], NROWS * per, BS, cfg["n_kv_heads"], cfg["head_dim"], _kv_dt(cfg))
    tables = [[i + NROWS * j for j in range(per)] for i in range(NROWS)]
    g = runtime.BatchDecodeGraph(lm, pool, NROWS, per)                 # captured before any row has an adapter
    for p, tb, name in zip(prompts, tables, ROWS):
        lm.set_lora(name)                                              # the prompt runs under the row's adapter
        n = len(p) - 1
        lm.forward_with_paged_kv_cache(p[:n], pool, [tb[i // BS] * BS + i % BS for i in range(n)], tb, n, 0)
    lm.set_lora(None)
    g.set_adapters(ROWS)
    g.seed([p[-1] for p in prompts], [len(p) for p in prompts], tables)
    for _ in range(STEPS):
        g.replay()
    out = np.stack([g.read_tokens(s) for s in range(STEPS)], axis=1)
    for r in range(NROWS):
        _check_single(key, out[r].tolist(), lm, prompts[r], STEPS, ROWS[r])
    # the logits of the last replay, row by row: the single-sequence step under the row's own adapter at the 16-bit bar, under any other setting far away
    last = g.read_logits()
    bar = SPLIT_BARS[cfg["act_dtype"]]
    for r in range(NROWS):
        seq = prompts[r] + out[r].tolist()[:STEPS - 1]
        rel = {}
        for name in (None, "a1", "a2"):
            lm.set_lora(name)
            kv = lm.new_kv_cache(len(seq) + 8)
            for i, t in enumerate(seq):
                lg = lm.forward_with_kv_cache([t], kv, i).to_numpy().reshape(-1)
            rel[name] = float(np.linalg.norm(last[r].astype(np.float64) - lg) / np.linalg.norm(lg))
        lm.set_lora(None)
        print("%s / %s row %d (%s): last-replay logits vs single-sequence under none / a1 / a2: %.3e / %.3e / %.3e" % (key, mask, r, ROWS[r], rel[None], rel["a1"], rel["a2"]))
        assert rel[ROWS[r]] <= bar, (r, rel)
        assert min(v for k, v in rel.items() if k != ROWS[r]) >= 10 * bar, (r, rel)
    # the rows' slots are in use: detach is refused until the graph lets go of them
    with pytest.raises(L.BlazrHipError) as e:
        lm.unload_lora("a2")
    assert e.value.code == L.E_INVALID and "batch row" in str(e.value)
    g.set_adapters([None] * NROWS)
    assert lm.unload_lora("a2") is True
    with pytest.raises(KeyError):
        g.set_adapters([None, "a2", None, None])


@pytest.mark.parametrize("key,mask", CASES)
def test_engine_mixed_adapters_staggered(device, key, mask):
    model, lm = _setup(device, key, mask)
    prompts = _prompts(model["config"]["vocab"])
    eng = _engine(lm)
    ids, res = _drive(eng, [(s, dict(prompt=p, max_tokens=STEPS, lora=name)) for s, p, name in zip((0, 0, 3, 7), prompts, ROWS)])
    for r, rid in enumerate(ids):
        assert res[rid] == _alone(key, mask, lm, prompts[r], STEPS, ROWS[r]), r
        _check_single(key, res[rid], lm, prompts[r], STEPS, ROWS[r])
    # the same prompt under the three settings gives three different runs: the rows did not all run the base model
    # (tiny-bf16 ties its embeddings and repeats one token under every setting: its rows are told apart by their logits, in the batch graph test)
    if key == "tiny-awq":
        runs = {name: _alone(key, mask, lm, prompts[1], STEPS, name) for name in (None, "a1", "a2")}
        assert len({tuple(v) for v in runs.values()}) == 3, runs


@pytest.mark.parametrize("key,mask", CASES)
def test_engine_rows_readmitted_under_other_adapters(device, key, mask):
    """ten short requests over four rows: every row serves several requests, each under its own adapter"""
    model, lm = _setup(device, key, mask)
    prompts = _prompts(model["config"]["vocab"], n=10, seed=90)
    names = ["a1", None, "a2", "a2", None, "a1", "a2", "a1", None, "a2"]
    lens = [5, 9, 4, 7, 6, 8, 5, 9, 4, 6]
    eng = _engine(lm)
    ids, res = _drive(eng, [(0, dict(prompt=p, max_tokens=n, lora=name)) for p, n, name in zip(prompts, lens, names)])
    for r, rid in enumerate(ids):
        assert res[rid] == _alone(key, mask, lm, prompts[r], lens[r], names[r]), (r, names[r])
    st = eng.stats()
    assert st["free_blocks"] == st["total_blocks"] - st["park_blocks"] and st["live_rows"] == 0


def _raw_submit(eng, prompt, lora_slot):
    rq = L.Request(max_tokens=4, grammar_state=L.GRAMMAR_ROW_FREE, lora_slot=lora_slot)
    rq.sampling = L.RowSampling(temperature=0.0, top_p=1.0, repeat_penalty=1.0, repeat_last_n=64)
    p = np.ascontiguousarray(prompt, dtype=np.int64)
    rid = C.c_int64()
    return L.lib().bz_engine_submit(eng.h, p.ctypes.data, len(p), C.byref(rq), C.byref(rid))


def test_engine_submit_and_detach_rules(device):
    key, mask = "tiny-awq", "qv"
    model, lm = _setup(device, key, mask)
    prompt = _prompts(model["config"]["vocab"])[1]
    eng = _engine(lm)
    for bad in (3, 5, -1):                       # slot 2 is empty, slot 4 does not exist
        assert _raw_submit(eng, prompt, bad) == L.E_INVALID
        assert ("lora_slot = %d" % bad) in L.lib().bz_last_error().decode()
    seen = []

    def hook(step, ids):
        if step == 2:                            # admitted and decoding
            with pytest.raises(L.BlazrHipError) as e:
                lm.unload_lora("a1")
            assert e.value.code == L.E_INVALID and "admitted request" in str(e.value)
            seen.append(step)

    ids, res = _drive(eng, [(0, dict(prompt=prompt, max_tokens=8, lora="a1"))], hook)
    assert seen == [2] and res[ids[0]] == _alone(key, mask, lm, prompt, 8, "a1")
    assert lm.unload_lora("a1") is True          # finished and read: the slot is free to go
    plain = runtime.LoadedModel.from_synth(device, model)             # no table: only lora_slot 0 is accepted
    assert _raw_submit(_engine(plain), prompt, 1) == L.E_INVALID and "no LoRA table" in L.lib().bz_last_error().decode()


def test_engine_prefix_cache_ignores_requests_under_an_adapter(device):
    key, mask = "tiny-awq", "all"
    model, lm = _setup(device, key, mask)
    prompt = [int(t) for t in synth.prompt_tokens(2 * BS + 5, model["config"]["vocab"], seed=95)]      # two full blocks to share
    eng = _engine(lm, max_seq_len=80, prefix_cache=True)
    ids, res = _drive(eng, [(0, dict(prompt=prompt, max_tokens=8, lora="a1")), (6, dict(prompt=prompt, max_tokens=8, lora="a2"))])
    for rid, name in zip(ids, ("a1", "a2")):
        assert res[rid] == _alone(key, mask, lm, prompt, 8, name, max_seq_len=80)
        _check_single(key, res[rid], lm, prompt, 8, name)
    assert res[ids[0]] != res[ids[1]]
    ps = eng.prefix_stats()
    assert ps["hits"] == 0 and ps["misses"] == 0 and ps["cached_blocks"] == 0 and ps["prompt_tokens_skipped"] == 0, ps      # neither looked up nor published
    # without an adapter the same prompt still publishes and hits
    ids, res = _drive(eng, [(0, dict(prompt=prompt, max_tokens=8))])
    ids2, res2 = _drive(eng, [(0, dict(prompt=prompt, max_tokens=8))])
    ps = eng.prefix_stats()
    assert ps["hits"] == 1 and ps["misses"] == 1 and ps["cached_blocks"] >= 2 and ps["prompt_tokens_skipped"] >= 2 * BS, ps
    assert res[ids[0]] == res2[ids2[0]] == _alone(key, mask, lm, prompt, 8, None, max_seq_len=80)
    # and a request under an adapter does not read those blocks either
    ids3, res3 = _drive(eng, [(0, dict(prompt=prompt, max_tokens=8, lora="a1"))])
    assert res3[ids3[0]] == _alone(key, mask, lm, prompt, 8, "a1", max_seq_len=80)
    assert eng.prefix_stats()["hits"] == 1
