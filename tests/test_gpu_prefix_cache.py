"""The request engine's prefix cache (bz_engine_config.prefix_cache, k_kv_copy_slots, the scheduler's shared blocks) on the device.  Every comparison is
exact.  The reference is the existing API on a fresh pool (as _static of tests/test_gpu_engine.py): the donor's prompt chunks through
forward_with_paged_kv_cache into the recipient's private table, then the recipient's own p[done : n-1] at position `done` into the same table, then a seeded
BatchDecodeGraph -- the same chunks, so the same KV bits, without any sharing.

Hit == miss (a request served from the cache against the same request with the cache off, whose prompt is prefilled from position 0 in other chunks) was
measured with the existing API before it was asserted here: see HIT_EQUALS_MISS below and DESIGN.md section 4."""
import os
import subprocess

import numpy as np
import pytest

import grammar_ref as G
from blazr_amd import _lib as L
from blazr_amd import runtime, synth
from test_gpu_engine import BS, GREEDY, NROWS, PARAMS, _drive
from test_gpu_grammar import _model
from test_gpu_llama import _kv_dt
from test_grammar_rows import LITERALS, REGULAR

pytestmark = pytest.mark.gpu

PRESETS = ["tiny-awq", "tiny-bf16"]
MAXLEN = 96
PER = MAXLEN // BS
# Measured with the existing API before anything was asserted (prefill p[:-1] in one piece against the same prompt split at 16 / 32 / 40 / 47 and in 16-token chunks,
# then the same seeded greedy decode of 24 tokens; three prompts of 53 and of 49 tokens per preset): the KV bits of a position depend on the chunk it was prefilled
# in, and the decode tokens differed in 1 of 30 runs on tiny-awq and in 2 of 30 on tiny-bf16.  So hit == cache off is claimed for neither preset and is not asserted.
HIT_EQUALS_MISS = {"tiny-awq": False, "tiny-bf16": False}


def _engine(lm, num_blocks=None, chunk=0, depth=2, sampler=True, grammar=None, prefix=True, max_seq_len=MAXLEN):
    per = -(-max_seq_len // BS)
    return runtime.BatchEngine(lm, NROWS, NROWS * per + NROWS if num_blocks is None else num_blocks, BS, max_seq_len, chunk, depth, sampler, grammar, prefix_cache=prefix)


def _stem(V, seed, n=64):
    return synth.prompt_tokens(n, V, seed=seed)


def _cat(*parts):
    return np.concatenate([np.asarray(p, dtype=np.int64) for p in parts])


def _ref(device, model, lm, history, steps, params=None, grammar=None, per=PER, use_sampler=True, rows=NROWS):
    """history: [(prompt, [(a, b), ...])]: prompt[a:b] at position a, in this order, all into ONE private table of a fresh pool; the last prompt is the request's.
    Then the seeded static graph at the engine's width `rows` (the other rows are one-token sequences) -> the request's `steps` tokens."""
    cfg = model["config"]
    NROWS = rows
    pool = runtime.LayeredPagedKvCache(device, cfg["n_layers"], NROWS * per, BS, cfg["n_kv_heads"], cfg["head_dim"], _kv_dt(cfg))
    tables = [[i + NROWS * j for j in range(per)] for i in range(NROWS)]
    tb = tables[0]
    for p, ranges in history:
        for a, b in ranges:
            lm.forward_with_paged_kv_cache(p[a:b], pool, [tb[i // BS] * BS + i % BS for i in range(a, b)], tb, b, a)
    prompts = [history[-1][0]] + [np.array([1 + i], dtype=np.int64) for i in range(NROWS - 1)]
    sampler = cursor = None
    if use_sampler:
        sampler = runtime.BatchSampler(device, NROWS, cfg["vocab"])
        for r in range(NROWS):
            sampler.set_row(r, history=list(map(int, prompts[r])), draw_index=0, **(params if r == 0 and params is not None else GREEDY))
    if grammar is not None:
        dg, state = grammar
        cursor = runtime.GrammarCursor(dg, NROWS)
        for r in range(NROWS):
            cursor.set_row(r, state if r == 0 and state is not None else runtime.GrammarCursor.FREE)
    g = runtime.BatchDecodeGraph(lm, pool, NROWS, per, sampler=sampler, grammar=cursor)
    g.seed([int(p[-1]) for p in prompts], [len(p) for p in prompts], tables)
    for _ in range(steps):
        g.replay()
    return [int(g.read_tokens(s)[0]) for s in range(steps)]


def _accounting(eng):
    st, ps = eng.stats(), eng.prefix_stats()
    assert st["free_blocks"] + ps["private_blocks"] + ps["cached_blocks"] == st["total_blocks"] - st["park_blocks"], (st, ps)
    assert ps["evictable_blocks"] + ps["referenced_blocks"] <= ps["cached_blocks"]
    return st, ps


def _blocks(pool, cfg, blocks):
    return {(layer, which, b): pool.read_block(layer, b, which, cfg["n_kv_heads"], cfg["head_dim"], _kv_dt(cfg))
            for layer in range(cfg["n_layers"]) for which in (0, 1) for b in blocks}


@pytest.mark.parametrize("j", [1, 15])
@pytest.mark.parametrize("preset", PRESETS)
def test_copy_slots_alone(device, preset, j):
    model, lm = _model(device, preset)
    cfg = model["config"]
    assert cfg["head_dim"] % 8 == 0
    pool = runtime.LayeredPagedKvCache(device, cfg["n_layers"], 6, BS, cfg["n_kv_heads"], cfg["head_dim"], _kv_dt(cfg))
    p, q = _stem(cfg["vocab"], 1201, 32), _stem(cfg["vocab"], 1202, 16)
    lm.forward_with_paged_kv_cache(p, pool, [[4, 1][i // BS] * BS + i % BS for i in range(32)], [4, 1], 32, 0)       # blocks 4 and 1
    lm.forward_with_paged_kv_cache(q, pool, [2 * BS + i for i in range(16)], [2], 16, 0)                             # other data in block 2
    before = _blocks(pool, cfg, range(6))
    assert all(before[(0, w, b)].any() for w in (0, 1) for b in (1, 2, 4)) and not before[(0, 0, 3)].any()
    pool.copy_slots(1, 2, j)
    after = _blocks(pool, cfg, range(6))
    for (layer, which, b), got in after.items():
        was = before[(layer, which, b)]
        if b != 2:
            assert np.array_equal(got, was), (layer, which, b)                       # the source and every other block are untouched
            continue
        assert np.array_equal(got[:, :j], before[(layer, which, 1)][:, :j]), (layer, which)       # the first j slots of every head are the source's
        assert np.array_equal(got[:, j:], was[:, j:]), (layer, which)                              # the rest of the destination is untouched
        assert not np.array_equal(got[:, :j], was[:, :j])


@pytest.mark.parametrize("preset", PRESETS)
def test_full_blocks_and_copy_on_write(device, preset):
    model, lm = _model(device, preset)
    V = model["config"]["vocab"]
    stem = _stem(V, 1210)
    a = stem[:53]
    b = _cat(stem[:40], synth.prompt_tokens(13, V, seed=1211))
    assert b[40] != stem[40]
    eng = _engine(lm, sampler=False)
    (ia,), res, _ = _drive(eng, [(0, dict(prompt=a, max_tokens=6))])
    assert res[ia]["tokens"] == _ref(device, model, lm, [(a, [(0, 52)])], 6, use_sampler=False)
    st, ps = _accounting(eng)
    assert st["prompt_tokens"] == 52 and ps["misses"] == 1 and ps["hits"] == 0 and ps["cached_blocks"] == 3 == ps["evictable_blocks"]
    (ib,), res, _ = _drive(eng, [(0, dict(prompt=b, max_tokens=10))])
    assert res[ib]["tokens"] == _ref(device, model, lm, [(a, [(0, 52)]), (b, [(40, 52)])], 10, use_sampler=False)     # m = 2 blocks, j = 8 slots copied
    st, ps = _accounting(eng)
    assert ps["cached_tokens"] == 40 == ps["prompt_tokens_skipped"] and ps["hits"] == 1 and ps["copied_blocks"] == 1 == ps["copy_launches"]
    assert st["prompt_tokens"] == 52 + 12
    assert ps["cached_blocks"] == 4                                                  # b's own third block is in the index beside a's


@pytest.mark.parametrize("preset", PRESETS)
def test_two_copies_of_one_step_share_a_launch(device, preset):
    # two sharers admitted in the same step with different j: one launch of k_kv_copy_slots, two triples under a grid sized for the larger j
    model, lm = _model(device, preset)
    V = model["config"]["vocab"]
    stem = _stem(V, 1215)
    a = stem[:53]
    b = _cat(stem[:40], synth.prompt_tokens(13, V, seed=1216))                       # m = 2, j = 8
    c = _cat(stem[:45], synth.prompt_tokens(8, V, seed=1217))                        # m = 2, j = 13
    assert b[40] != stem[40] and c[45] != stem[45]
    eng = _engine(lm, sampler=False)
    _drive(eng, [(0, dict(prompt=a, max_tokens=4))])
    ids, res, _ = _drive(eng, [(0, dict(prompt=b, max_tokens=10)), (0, dict(prompt=c, max_tokens=10))])
    st, ps = _accounting(eng)
    assert ps["copy_launches"] == 1 and ps["copied_blocks"] == 2 and ps["hits"] == 2 and ps["cached_tokens"] == 40 + 45
    assert st["prompt_tokens"] == 52 + 12 + 7
    assert res[ids[0]]["tokens"] == _ref(device, model, lm, [(a, [(0, 52)]), (b, [(40, 52)])], 10, use_sampler=False)
    assert res[ids[1]]["tokens"] == _ref(device, model, lm, [(a, [(0, 52)]), (c, [(45, 52)])], 10, use_sampler=False)


@pytest.mark.parametrize("preset", PRESETS)
def test_zero_prefill(device, preset):
    model, lm = _model(device, preset)
    p = _stem(model["config"]["vocab"], 1220)[:49]                                   # n_prompt - 1 = 48 = three whole blocks
    eng = _engine(lm, depth=3)
    kw = dict(prompt=p, max_tokens=9, **PARAMS[2])
    (i0,), res0, _ = _drive(eng, [(0, kw)])
    assert res0[i0]["tokens"] == _ref(device, model, lm, [(p, [(0, 48)])], 9, params=PARAMS[2])
    before = eng.stats()
    (i1,), res1, _ = _drive(eng, [(0, kw)])
    st, ps = _accounting(eng)
    assert st["prompt_tokens"] == before["prompt_tokens"] == 48                      # nothing was prefilled
    assert res1[i1]["first"] == before["replays"]                                    # the first token comes from the admission step's replay
    assert res1[i1]["tokens"] == res0[i0]["tokens"] and len(res1[i1]["tokens"]) == 9
    assert ps["hits"] == 1 and ps["cached_tokens"] == 48 and ps["copied_blocks"] == 0


@pytest.mark.parametrize("preset", PRESETS)
def test_sharing_while_the_donor_is_live_and_finishes_first(device, preset):
    model, lm = _model(device, preset)
    V = model["config"]["vocab"]
    stem = _stem(V, 1230)
    a = dict(prompt=stem[:53], max_tokens=5, **PARAMS[0])
    b = dict(prompt=_cat(stem[:47], synth.prompt_tokens(9, V, seed=1231)), max_tokens=30, **PARAMS[3])       # m = 2, j = 15: all but one slot of the third block
    assert b["prompt"][47] != stem[47]
    eng = _engine(lm, depth=2)
    seen = []
    ids, res, _ = _drive(eng, [(0, a), (2, b)], lambda step, ids: seen.append(_accounting(eng)[1]["referenced_blocks"]))
    assert max(seen) == 4                                                            # a's three blocks, two of them held by b as well, and b's own third
    assert res[ids[0]]["tokens"] == _ref(device, model, lm, [(a["prompt"], [(0, 52)])], 5, params=PARAMS[0])
    assert res[ids[1]]["tokens"] == _ref(device, model, lm, [(a["prompt"], [(0, 52)]), (b["prompt"], [(47, 55)])], 30, params=PARAMS[3])
    assert res[ids[0]]["reason"] == 0 == res[ids[1]]["reason"] and len(res[ids[1]]["tokens"]) == 30
    st, ps = _accounting(eng)
    assert ps["cached_tokens"] == 47 and ps["referenced_blocks"] == 0 and 0 < ps["cached_blocks"] == ps["evictable_blocks"]
    assert st["free_blocks"] == st["total_blocks"] - st["park_blocks"] - ps["cached_blocks"]
    assert eng.prefix_flush() == ps["cached_blocks"]
    st, ps = _accounting(eng)
    assert st["free_blocks"] == st["total_blocks"] - st["park_blocks"] and ps["cached_blocks"] == 0


@pytest.mark.parametrize("preset", PRESETS)
def test_eviction(device, preset):
    model, lm = _model(device, preset)
    V = model["config"]["vocab"]
    stems = [_stem(V, 1240 + i)[:53] for i in range(3)]
    eng = _engine(lm, num_blocks=9 + NROWS, sampler=False)                          # every request takes 4 blocks; three stems would keep 9 cached
    order = [0, 1, 2, 0, 1, 2]
    got = []
    for k in order:
        (rid,), res, _ = _drive(eng, [(0, dict(prompt=stems[k], max_tokens=7))], lambda step, ids: _accounting(eng))
        got.append(res[rid]["tokens"])
    st, ps = _accounting(eng)
    assert ps["evictions"] > 0 and ps["hits"] == 3 and ps["cached_tokens"] == 3 * 32    # a leaf of each stem went: two blocks matched, 20 tokens prefilled again
    for k, tokens in zip(order[:3], got[:3]):
        assert tokens == _ref(device, model, lm, [(stems[k], [(0, 52)])], 7, use_sampler=False), k
    for k, tokens in zip(order[3:], got[3:]):
        assert tokens == _ref(device, model, lm, [(stems[k], [(0, 52)]), (stems[k], [(32, 52)])], 7, use_sampler=False), k
    assert st["prompt_tokens"] == 3 * 52 + 3 * 20


@pytest.mark.parametrize("preset", PRESETS)
def test_with_the_rest_of_the_engine(device, preset):
    # prefill_chunk 16, depth 4, the sampler with the penalty parameter sets (history = the whole prompt, most of it never prefilled), a grammar row, a cancelled sharer
    model, lm = _model(device, preset)
    V = model["config"]["vocab"]
    vocab = G.synth_vocab(V, seed=21)[0]
    parts = [runtime.GrammarDfa(LITERALS), runtime.GrammarDfa(REGULAR, regular=True)]
    cat, starts = runtime.GrammarDfa.concat(parts)
    dg = cat.to_device(device, vocab)
    stem = _stem(V, 1250)
    a = dict(prompt=stem[:53], max_tokens=40, **PARAMS[0])                           # chunks [0,16) [16,32) [32,48) [48,52): live in step 3
    b = dict(prompt=_cat(stem[:40], synth.prompt_tokens(13, V, seed=1251)), max_tokens=20, **PARAMS[2])       # step 5: m = 2, j = 8, chunk [40,52)
    c = dict(prompt=stem[:49], max_tokens=30, **PARAMS[3])                           # step 6: three whole blocks, no prefill; cancelled before step 12
    d = dict(prompt=_cat(stem[:45], synth.prompt_tokens(4, V, seed=1252)), max_tokens=16, grammar_state=starts[1], **PARAMS[0])   # step 7: m = 2, j = 13 from a's block
    e = dict(prompt=stem[:49], max_tokens=12, **PARAMS[3])                           # step 13: takes c's row, no prefill either
    a_chunks = [(0, 16), (16, 32), (32, 48), (48, 52)]
    cur = runtime.GrammarCursor(dg, NROWS)
    eng = _engine(lm, chunk=16, depth=4, grammar=cur)

    def hook(step, ids):
        _accounting(eng)
        if step == 12:
            eng.cancel(ids[2])
        if step == 13:
            ids.append(eng.submit(**e))
    ids, res, _ = _drive(eng, [(0, a), (5, b), (6, c), (7, d)], hook)

    def want(kw, own, gstate=None):
        return _ref(device, model, lm, [(a["prompt"], a_chunks), (kw["prompt"], own)], kw["max_tokens"], params={k: v for k, v in kw.items() if k in PARAMS[2]},
                    grammar=(dg, gstate))
    assert res[ids[0]]["tokens"] == _ref(device, model, lm, [(a["prompt"], a_chunks)], 40, params=PARAMS[0], grammar=(dg, None))
    assert res[ids[1]]["tokens"] == want(b, [(40, 52)])
    full_c = want(c, [])
    gone = res[ids[2]]
    assert gone["reason"] == 2 and 0 < len(gone["tokens"]) <= 6 and gone["tokens"] == full_c[:len(gone["tokens"])]
    assert res[ids[3]]["tokens"] == want(d, [(45, 48)], starts[1])
    assert parts[1].advance_tokens(vocab, res[ids[3]]["tokens"]) == 0              # the grammar row kept to its grammar
    assert res[ids[4]]["tokens"] == want(e, []) == full_c[:12]
    st, ps = _accounting(eng)
    assert ps["hits"] == 4 and ps["misses"] == 1 and ps["cached_tokens"] == 40 + 48 + 45 + 48 and ps["copied_blocks"] == 2
    assert st["prompt_tokens"] == 52 + 12 + 0 + 3 + 0 and ps["referenced_blocks"] == 0
    eng.prefix_flush()
    st, _ = _accounting(eng)
    assert st["free_blocks"] == st["total_blocks"] - st["park_blocks"] and st["live_rows"] == 0


@pytest.mark.parametrize("preset", [p for p in PRESETS if HIT_EQUALS_MISS[p]] or [None])
def test_hit_equals_miss(device, preset):
    """Asserted only for the presets where prefilling a prompt whole and prefilling it split at the hit boundary gave the same decode tokens through the existing API
    (HIT_EQUALS_MISS); elsewhere the bar is the reference of the same chunks, which the tests above hold.  With no such preset this only states that none is claimed."""
    if preset is None:
        assert not any(HIT_EQUALS_MISS.values())
        return
    model, lm = _model(device, preset)
    V = model["config"]["vocab"]
    stem = _stem(V, 1260)
    reqs = [dict(prompt=stem[:53], max_tokens=12, **PARAMS[0]), dict(prompt=_cat(stem[:40], synth.prompt_tokens(13, V, seed=1261)), max_tokens=12, **PARAMS[2]),
            dict(prompt=stem[:49], max_tokens=12, **PARAMS[3])]
    out = {}
    for prefix in (False, True):
        eng = _engine(lm, prefix=prefix)
        out[prefix] = []
        for kw in reqs:
            (rid,), res, _ = _drive(eng, [(0, kw)])
            out[prefix].append(res[rid]["tokens"])
        assert eng.prefix_stats()["hits"] == (2 if prefix else 0)
    assert out[True] == out[False]


def test_refusals(device):
    model, lm = _model(device, "tiny-awq")
    cfg = model["config"]

    def refused(fn, *words):
        with pytest.raises(L.BlazrHipError) as e:
            fn()
        assert e.value.code == L.E_INVALID and all(w in str(e.value) for w in words), str(e.value)
    s = runtime.Scheduler(2, 8, BS, 64)
    s.submit(5, 5)
    refused(s.enable_prefix, "after a submit")
    pool = runtime.LayeredPagedKvCache(device, cfg["n_layers"], 4, BS, cfg["n_kv_heads"], cfg["head_dim"], _kv_dt(cfg))
    refused(lambda: pool.copy_slots(4, 0, 1), "blocks 4 -> 0", "pool's 4")
    refused(lambda: pool.copy_slots(0, -1, 1), "outside the pool")
    refused(lambda: pool.copy_slots(1, 1, 1), "both block 1")
    refused(lambda: pool.copy_slots(0, 1, 0), "0 slots")
    refused(lambda: pool.copy_slots(0, 1, BS + 1), "17 slots", "block_size = 16")
    refused(lambda: runtime.BatchEngine(lm, 4, 16, prefix_cache=2), "prefix_cache = 2")
    off = _engine(lm, prefix=False, sampler=False)
    rid = off.submit(_stem(cfg["vocab"], 1270)[:20], 4)
    assert len(off.run_until_idle()[rid][0]) == 4
    ps = off.prefix_stats()
    assert ps["enabled"] == 0 and ps["cached_blocks"] == 0 and ps["hits"] == 0 and ps["misses"] == 0 and off.prefix_flush() == 0


def test_bz_run_prefix_cache(device, tmp_path):
    import ckpt_writer as W
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "blazr_amd", "bz-run")
    assert os.path.exists(exe), "bz-run was not built (python -c 'import __graft_entry__ as g; g.build()')"
    model, lm = _model(device, "tiny-awq")
    ck = tmp_path / "ck"
    ck.mkdir()
    W.write_hf_checkpoint(str(ck), model, shards=1)
    stem = _stem(1024, 1280)
    a, b = stem[:53], _cat(stem[:40], synth.prompt_tokens(13, 1024, seed=1281))
    (tmp_path / "requests.txt").write_text("".join("%d;%s\n" % (6, ",".join(str(int(t)) for t in p)) for p in (a, b)))
    # max_seq_len = 59: four blocks per request; a pool of five lets the second request in only when the first has finished, so it finds the first one's blocks
    cmd = [exe, str(ck), "--requests", str(tmp_path / "requests.txt"), "--rows", "2", "--pool-blocks", "7"]
    r = subprocess.run(cmd + ["--prefix-cache"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = [[int(x) for x in ln.split(",")] for ln in r.stdout.strip().split("\n")]
    assert "prefix cache: 1 hits, 1 misses, 40 cached tokens, 0 evictions" in r.stderr and "64 prompt tokens" in r.stderr, r.stderr
    # the reference of the same chunks through the existing API at bz-run's width (2 rows, 4 blocks per row, greedy without a sampler)
    assert got[0] == _ref(device, model, lm, [(a, [(0, 52)])], 6, per=4, use_sampler=False, rows=2)
    assert got[1] == _ref(device, model, lm, [(a, [(0, 52)]), (b, [(40, 52)])], 6, per=4, use_sampler=False, rows=2)
    if HIT_EQUALS_MISS["tiny-awq"]:
        r0 = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert r0.returncode == 0 and r0.stdout == r.stdout and "prefix cache" not in r0.stderr and "104 prompt tokens" in r0.stderr, r0.stderr
