"""Batched decode attention at long contexts: the split-KV pair over block tables (blazr_amd/csrc/bz_rows_attn.hip) on the device.

A decode batch's attention keeps a row's scores in LDS up to 38 888 / 18 416 / 8 180 / 3 062 positions (REP 1 / 2 / 4 / 8); beyond, the step now runs
k_rows_attn_split + k_rows_attn_merge.  BZ_ROWS_SPLIT_MIN=1 (read per call) sends every supported shape there, so the op-level tests run the pair at tiny
shapes; the model-level tests at the end run with no switch, at contexts the parent commit refuses with BZ_E_UNSUPPORTED.

Op level (bz_paged_attn_decode_rows over pools injected with write_block): every row of a batch is a sequence with its own length and its own planted
construction (tests/rows_attn_cases.py).  Two bars, both from what the project already has:
  * relative L2 to a float64 softmax attention over the injected rows <= the activation dtype's unit roundoff (2^-11 f16, 2^-8 bf16): what a correctly
    rounded row can reach, the f32 sums add orders less;
  * no further from that truth than TRUTH_FACTOR = 1.25 x the distance of bz_paged_attn_decode's row (the exact single-row kernel on the same pool).
Every planted case first proves on the CPU that removing the planted row moves the truth by at least 20x the first bar.
"""
import numpy as np
import pytest

import npref
import rows_attn_cases as RC
import swa_ref
from blazr_amd import _lib as L
from blazr_amd import runtime, synth
from oracle import orc_py

pytestmark = pytest.mark.gpu

BS = RC.BS
SPLIT_BARS, TRUTH_FACTOR, FLOOR = {"f16": 1.5e-3, "bf16": 2.0 ** -7}, 1.25, 4e-6          # test_gpu_long_context.py
TOKEN = 5
SHAPES = {"hd64-rep2": (64, 4, 2), "hd128-rep1": (128, 2, 2), "hd128-rep4": (128, 8, 2), "hd128-rep8": (128, 8, 1)}     # head_dim, n_heads, n_kv_heads
PRESET = {"f16": "tiny-awq", "bf16": "tiny-bf16"}


@pytest.fixture
def switch(monkeypatch):
    monkeypatch.setenv("BZ_ROWS_SPLIT_MIN", "1")


def _op_model(device, act, hd, nq, nkv, **over):
    model = synth.make_llama(PRESET[act], n_layers=1, n_heads=nq, n_kv_heads=nkv, head_dim=hd, **over)
    return model, runtime.LoadedModel.from_synth(device, model)


def _single(lm, pool, q, blocks, T, layer=0):
    """bz_paged_attn_decode: the exact single-row kernel over the same pool"""
    dev = lm.dev
    tq, tb, out = dev.tensor(np.ascontiguousarray(q, np.float32)), dev.tensor(np.asarray(blocks, np.int32)), dev.zeros(q.shape, L.F32)
    L.check(L.lib().bz_paged_attn_decode(lm.h, tq.h, pool.kv.h, layer, tb.h, int(T), out.h))
    return out.to_numpy().reshape(q.shape)


def _chunks(n, rng):
    """a seeded order of n sequences cut into calls of 3 to 5 rows"""
    order, out = list(rng.permutation(n)), []
    while order:
        k = 5 if len(order) >= 8 or len(order) == 5 else 4 if len(order) in (4, 7) else 3
        out.append(order[:k])
        order = order[k:]
    return out


def _check_rows(name, act, got, single, want, sens):
    bar = RC.UNIT[act]
    gt, st = RC.rel(got, want), RC.rel(single, want)
    msg = "%s: rows vs f64 truth %.3e (bar %.3e); single-row kernel vs truth %.3e; planted sensitivity %.3e" % (name, gt, bar, st, sens)
    print(msg)
    assert gt <= bar, msg
    assert gt <= TRUTH_FACTOR * st, msg


def _run_sequences(lm, pool, seqs, act, rng, window=0, truth_fn=None):
    """seqs: dicts with q, K, V, T, name, sens (their blocks are written here); runs them in calls of 3 to 5 rows and holds every row to both bars"""
    for s in seqs:
        s["blocks"] = pool.take(s["T"])
        pool.write(0, s["blocks"], s["K"], s["V"])
    for call in _chunks(len(seqs), rng):
        rows = [seqs[i] for i in call]
        got = lm.paged_attn_decode_rows(np.stack([s["q"] for s in rows]), pool.kv, 0, [s["blocks"] for s in rows], [s["T"] for s in rows])
        for s, g in zip(rows, got):
            want = truth_fn(s) if truth_fn else RC.truth(s["q"], s["K"], s["V"], window)
            _check_rows("%s len %d, %s (call of %d, lengths %s)" % (act, s["T"], s["name"], len(rows), [r["T"] for r in rows]), act, g,
                        _single(lm, pool, s["q"], s["blocks"], s["T"]), want, s["sens"])


# ------------------------------------------------------------------------------------------------------------------------------------------
# 1. op level, injected pool
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.watchdog(300)
@pytest.mark.parametrize("act", ["f16", "bf16"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_rows_op_planted_cases(device, switch, shape, act):
    hd, nq, nkv = SHAPES[shape]
    _, lm = _op_model(device, act, hd, nq, nkv, max_seq_len=16384)
    S = RC.slice_len(1)
    D = next(n for n in range(S, 1 << 20) if RC.slice_len(n) != S)       # the first length at which the slice length doubles
    assert RC.slice_len(D - 1) == S and RC.slice_len(D) == 2 * S
    lens = [1, 2, 16, 17, S - 1, S, S + 1, 2 * S + 3, D, D + 1]
    rng = np.random.default_rng(hd + nq + (act == "bf16"))
    seqs = []
    for T in lens:
        cases = RC.planted_cases(T)
        if T == D + 1:                                # the second long row: the two constructions that see every slice
            cases = [c for c in cases if c[0] == "all keys equal" or c[0] == "dominant row %d" % ((-(-T // RC.slice_len(T)) - 1) * RC.slice_len(T))]
        for name, rows in cases:
            q = RC.make_q(rng, nq, nkv, hd, act)
            K, V, sens = RC.build_case(rng, q, T, name, rows, nkv, act)
            assert sens >= 20 * RC.UNIT[act], "%s at %d: removing the planted row moves the truth by only %.3e" % (name, T, sens)
            seqs.append(dict(q=q, K=K, V=V, T=T, name=name, sens=sens))
    pool = RC.Pool(device, 1, 1 + sum(-(-s["T"] // BS) for s in seqs), nkv, hd, act, seed=hd)
    _run_sequences(lm, pool, seqs, act, rng)


# ------------------------------------------------------------------------------------------------------------------------------------------
# 2. independence and staleness
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,act", [("hd128-rep4", "f16"), ("hd64-rep2", "bf16"), ("hd128-rep8", "bf16")])
def test_row_bits_depend_on_the_row_alone(device, switch, shape, act):
    """the same row alone, among four others, with a table twice as wide, and after a call in which that row index was 40 slices long"""
    hd, nq, nkv = SHAPES[shape]
    _, lm = _op_model(device, act, hd, nq, nkv, max_seq_len=8192)
    rng = np.random.default_rng(17)
    long_T = 40 * RC.slice_len(1)
    assert RC.slice_len(long_T) == RC.slice_len(1)
    others = [300, 9, 2000, 64, long_T]
    targets = [17, 2 * RC.slice_len(1) + 3, 1500]
    pool = RC.Pool(device, 1, 1 + sum(-(-t // BS) for t in others + targets), nkv, hd, act, seed=3)
    seqs = []
    for T in others + targets:
        q = RC.make_q(rng, nq, nkv, hd, act)
        K, V = RC.background(rng, T, nkv, hd, act)
        K[T // 2], V[T // 2] = RC.key_with_score(q, nkv, 16.0, act), RC.pattern(1, nkv, hd, act)
        s = dict(q=q, T=T, blocks=pool.take(T))
        pool.write(0, s["blocks"], K, V)
        seqs.append(s)
    o, tg = seqs[:5], seqs[5:]
    run = lambda rows, tables=None: lm.paged_attn_decode_rows(np.stack([s["q"] for s in rows]), pool.kv, 0, tables if tables is not None else [s["blocks"] for s in rows],
                                                              [s["T"] for s in rows])
    for t in tg:
        alone = run([t])[0]
        assert np.isfinite(alone).all() and np.abs(alone).max() > 1.0          # the planted pattern came through
        among = run([o[0], o[1], t, o[2], o[3]])[2]
        wide = np.zeros((1, 2 * len(t["blocks"]) + 3), np.int32)
        wide[0, :len(t["blocks"])] = t["blocks"]
        widened = run([t], wide)[0]
        run([o[4], o[0], o[1]])                                                 # row index 0 is 40 slices long ...
        after = run([t])[0]                                                     # ... and then short again
        run([o[4], o[0]])
        beside = run([t, o[4]])[0]                                              # same grid as the long call
        for name, x in (("among four others", among), ("table twice as wide", widened), ("after a 40-slice row", after), ("beside a 40-slice row", beside)):
            assert np.array_equal(alone, x), (t["T"], name, float(np.abs(alone - x).max()))


def test_rows_beyond_one_workspace_pass(device, switch):
    """512 rows at 64 slices of 8 heads x 128 need 512 x 270 336 bytes of partials, more than the 128 MiB the workspace is bound to: the plan passes over the rows in
    sub-chunks of 496.  Rows on either side of the cut, and the long row that sets the grid, equal the same rows computed alone."""
    act, (hd, nq, nkv) = "bf16", SHAPES["hd128-rep8"]
    _, lm = _op_model(device, act, hd, nq, nkv, max_seq_len=16384)
    lens = [8193] + [1 + (7 * i) % 40 for i in range(1, 512)]
    plan = runtime.rows_attn_plan(nq, nkv, hd, L.BF16, 0, len(lens), max(lens))
    assert plan["kernel"] == 1 and plan["grid_slices"] == 64 and plan["rows_per_pass"] == 496 and plan["ws_bytes"] == 496 * nq * 64 * (hd + 4) * 4, plan
    rng = np.random.default_rng(512)
    pool = RC.Pool(device, 1, 1 + sum(-(-t // BS) for t in lens), nkv, hd, act, seed=512)
    seqs = []
    for T in lens:
        q = RC.make_q(rng, nq, nkv, hd, act)
        K, V = RC.background(rng, T, nkv, hd, act)
        K[T // 2], V[T // 2] = RC.key_with_score(q, nkv, 4.0, act), RC.pattern(T % 5, nkv, hd, act)
        s = dict(q=q, K=K, V=V, T=T, blocks=pool.take(T))
        pool.write(0, s["blocks"], K, V)
        seqs.append(s)
    run = lambda rows: lm.paged_attn_decode_rows(np.stack([s["q"] for s in rows]), pool.kv, 0, [s["blocks"] for s in rows], [s["T"] for s in rows])
    got = run(seqs)
    for i in (0, 1, 250, 495, 496, 497, 511):
        assert np.array_equal(got[i], run([seqs[i]])[0]), i
        assert RC.rel(got[i], RC.truth(seqs[i]["q"], seqs[i]["K"], seqs[i]["V"])) <= RC.UNIT[act], i


# ------------------------------------------------------------------------------------------------------------------------------------------
# 3. sliding window
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act,W,lens", [("f16", 24, [5, 24, 25, 60]), ("bf16", 300, [128, 129, 300, 301, 429, 700])], ids=["w24-ctx60", "w300"])
def test_rows_under_a_window(device, switch, act, W, lens):
    """the slices are laid over [att_lo(len, W), len): rows on either side of the window's start and of its slice boundaries, against swa_ref's float64 truth.
    One extra construction per row longer than the window: a key with score 120 just OUTSIDE the window, which must not be read into the result."""
    hd, nq, nkv = 128, 4, 2
    _, lm = _op_model(device, act, hd, nq, nkv, sliding_window=W, max_seq_len=1024)
    assert lm.c.sliding_window == W
    rng = np.random.default_rng(W)
    seqs = []
    for T in lens:
        for name, rows in RC.planted_cases(T, W):
            q = RC.make_q(rng, nq, nkv, hd, act)
            K, V, sens = RC.build_case(rng, q, T, name, rows, nkv, act, W)
            assert sens >= 20 * RC.UNIT[act], (name, T, sens)
            seqs.append(dict(q=q, K=K, V=V, T=T, name=name, sens=sens))
        if T > W:
            q = RC.make_q(rng, nq, nkv, hd, act)
            K, V = RC.background(rng, T, nkv, hd, act)
            K[T - W - 1], V[T - W - 1] = RC.key_with_score(q, nkv, 120.0, act), RC.pattern(4, nkv, hd, act)
            sens = RC.rel(swa_ref.attn_decode(q, K, V, 0), swa_ref.attn_decode(q, K, V, W))     # how far the full-attention answer is
            assert sens >= 20 * RC.UNIT[act], (T, sens)
            seqs.append(dict(q=q, K=K, V=V, T=T, name="score 120 at row %d, outside the window" % (T - W - 1), sens=sens))
    pool = RC.Pool(device, 1, 1 + sum(-(-s["T"] // BS) for s in seqs), nkv, hd, act, seed=W)
    _run_sequences(lm, pool, seqs, act, rng, W, truth_fn=lambda s: swa_ref.attn_decode(s["q"], s["K"], s["V"], W))


# ------------------------------------------------------------------------------------------------------------------------------------------
# models of tests 4 - 6: REP 8, one layer; no switch set
# ------------------------------------------------------------------------------------------------------------------------------------------
REP8 = {"awq-f16-hd64": ("tiny-awq", dict(hidden=512, n_heads=8, n_kv_heads=1, n_layers=1, max_seq_len=4096)),
        "dense-bf16-hd128": ("tiny-bf16", dict(hidden=512, n_heads=8, n_kv_heads=1, head_dim=128, n_layers=1, max_seq_len=4096)),
        # the issue's second override set as written (4 / 1 heads of 128: REP 4, inside the scalar kernel's 8 180): the same rows through the scalar kernel
        "dense-bf16-hd128-4-1": ("tiny-bf16", dict(hidden=512, n_heads=4, n_kv_heads=1, head_dim=128, n_layers=1, max_seq_len=4096))}
_CACHE = {}


def _rep8(device, key):
    if key not in _CACHE:
        preset, over = REP8[key]
        model = synth.make_llama(preset, **over)
        _CACHE[key] = (model, runtime.LoadedModel.from_synth(device, model))
    return _CACHE[key]


def _slots(tables, lens):
    return [tb[(n - 1) // BS] * BS + (n - 1) % BS for tb, n in zip(tables, lens)]


# ------------------------------------------------------------------------------------------------------------------------------------------
# 4. formerly refused: one eager step over rows of 3 063, 3 200 and 40 positions
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.watchdog(600)
@pytest.mark.parametrize("key", list(REP8))
def test_batch_step_beyond_the_scalar_limit(device, monkeypatch, key):
    """The parent commit returns BZ_E_UNSUPPORTED ("prefill attention: context 3200 too long for this kernel") for the two REP-8 models.  The same injected rows go
    into the pool (write_block), the oracle (kv_inject) and the float64 truth; one dominant row is planted in each long row.  Bars: the suite's split-KV bars
    (test_gpu_long_context.py)."""
    monkeypatch.delenv("BZ_ROWS_SPLIT_MIN", raising=False)
    model, lm = _rep8(device, key)
    cfg = model["config"]
    act, nkv, hd = cfg["act_dtype"], cfg["n_kv_heads"], cfg["head_dim"]
    rep = cfg["n_heads"] // nkv
    lens = [3063, 3200, 40]
    plan = runtime.rows_attn_plan(cfg["n_heads"], nkv, hd, RC.DT[act], 0, len(lens), max(lens))
    assert plan["kernel"] == (1 if rep == 8 else 0), plan
    om, tm, nl = orc_py.OrcLlama(model), npref.NpLlamaTruth(model), npref.NpLlama(model)
    pool = RC.Pool(device, 1, 1 + sum(-(-n // BS) for n in lens), nkv, hd, act, seed=4)
    rng = np.random.default_rng(4)
    bar = SPLIT_BARS[act]
    tables, want, truths = [], [], []
    for n in lens:
        P = n - 1                                     # the new token's position; rows 0 .. P - 1 are cached
        K, V = RC.background(rng, P, nkv, hd, act)
        sens = None
        if n > 100:
            q, _, _ = nl.qkv0(TOKEN, P)
            r = P - 700                               # in the slice before the last one of the split plan
            K[r], V[r] = RC.key_with_score(q, nkv, 16.0, act), RC.pattern(2, nkv, hd, act)
            tm.set_history([(K, V)])
            base = tm.step(TOKEN, P)
            keep = np.setdiff1d(np.arange(P), [r])
            tm.set_history([(K[keep], V[keep])])
            sens = RC.rel(tm.step(TOKEN, P), base)
            assert sens >= 20 * bar, "row of %d: removing the planted row moves the truth by only %.3e" % (n, sens)
        tb = pool.take(n)
        pool.write(0, tb, K, V)
        tables.append(tb)
        okv = om.new_kv(n + 1)
        try:
            orc_py.kv_inject(okv, 0, K, V)
            want.append(np.asarray(om.forward_kv([TOKEN], okv, P)).reshape(-1))
        finally:
            orc_py.lib().orc_kv_free(okv)
        tm.set_history([(K, V)])
        truths.append(np.asarray(tm.step(TOKEN, P)).reshape(-1))
    got = lm.forward_paged_batch([TOKEN] * len(lens), pool.kv, _slots(tables, lens), tables, lens).to_numpy()
    for i, n in enumerate(lens):
        go, gt, ot = RC.rel(got[i], want[i]), RC.rel(got[i], truths[i]), RC.rel(want[i], truths[i])
        msg = "%s row of %d: hip vs oracle %.3e (bar %.1e); to the f64 truth: hip %.3e, oracle %.3e" % (key, n, go, bar, gt, ot)
        print(msg)
        assert go <= bar, msg
        assert gt <= max(TRUTH_FACTOR * ot, FLOOR), msg


# ------------------------------------------------------------------------------------------------------------------------------------------
# 5. graph
# ------------------------------------------------------------------------------------------------------------------------------------------
def _seeded_pools(device, cfg, lens, per, n_pools, seed):
    """n_pools pools with the same injected rows 0 .. len - 2 per sequence -> (pools, tables)"""
    act, nkv, hd = cfg["act_dtype"], cfg["n_kv_heads"], cfg["head_dim"]
    pools = [RC.Pool(device, 1, 1 + len(lens) * per, nkv, hd, act, seed=seed) for _ in range(n_pools)]
    rng = np.random.default_rng(seed)
    tables = []
    for n in lens:
        K, V = RC.background(rng, n - 1, nkv, hd, act)
        K *= 8.0                                      # scores of a few units: the rows are not near-uniform
        K = orc_py.round_act(K, act)
        tbs = [p.take(per * BS) for p in pools]
        assert all(tb == tbs[0] for tb in tbs)
        for p in pools:
            p.write(0, tbs[0], K, V)
        tables.append(tbs[0])
    return pools, tables


@pytest.mark.parametrize("key", ["awq-f16-hd64", "dense-bf16-hd128"])
def test_graph_replays_equal_eager_beyond_the_limit(device, monkeypatch, key):
    """BatchDecodeGraph at capacity 3 328 (refused by the parent inside its capture), rows seeded at 3 063, 3 070 and 10; eight replays against the eager step,
    whose decision length is beyond the limit too"""
    monkeypatch.delenv("BZ_ROWS_SPLIT_MIN", raising=False)
    model, lm = _rep8(device, key)
    cfg = model["config"]
    per, lens0, steps = 3328 // BS, [3063, 3070, 10], 8
    (pe, pg), tables = _seeded_pools(device, cfg, lens0, per, 2, seed=5)
    toks, lens, eager, ids = [TOKEN, TOKEN + 1, TOKEN + 2], list(lens0), [], []
    for _ in range(steps):
        lg = lm.forward_paged_batch(toks, pe.kv, _slots(tables, lens), tables, lens).to_numpy()
        eager.append(lg)
        toks = [int(t) for t in lg.argmax(axis=1)]
        ids.append(toks)
        lens = [n + 1 for n in lens]
    g = runtime.BatchDecodeGraph(lm, pg.kv, 3, per)
    g.seed([TOKEN, TOKEN + 1, TOKEN + 2], lens0, tables)
    for i in range(steps):
        g.replay()
        if i in (0, 3, 7):
            got = g.read_logits()
            assert np.array_equal(got, eager[i]), (i, float(np.abs(got - eager[i]).max()))
        assert g.read_tokens(i).tolist() == ids[i], i
    with pytest.raises(L.BlazrHipError) as e:         # a sequence beyond the captured capacity is refused, not a fault
        g.seed([TOKEN, TOKEN, TOKEN], [3329, 10, 10], tables)
    assert e.value.code == L.E_INVALID and "3328" in str(e.value), str(e.value)


# ------------------------------------------------------------------------------------------------------------------------------------------
# 6. engine
# ------------------------------------------------------------------------------------------------------------------------------------------
def _engine(lm, prefix_cache=False):
    per = 3200 // BS
    return runtime.BatchEngine(lm, 3, 3 * per + 3, BS, 3200, 0, 2, False, None, prefix_cache)


def _drive(eng, reqs):
    ids = [eng.submit(**kw) for kw in reqs]
    res, steps, busy = {}, 0, True
    while busy:
        busy = eng.step()
        eng.collect(eng.poll(), res)
        steps += 1
        assert steps < 3000
    return [res[i][0] for i in ids], [res[i][1] for i in ids]


def _static(device, model, lm, prompts, steps, per):
    """tests/test_gpu_engine.py's loop through the existing API: forward_with_paged_kv_cache(prompt[:-1]), BatchDecodeGraph.seed(prompt[-1], len(prompt)), replays"""
    cfg = model["config"]
    nseq = len(prompts)
    pool = runtime.LayeredPagedKvCache(device, cfg["n_layers"], nseq * per, BS, cfg["n_kv_heads"], cfg["head_dim"], RC.DT[cfg["act_dtype"]])
    tables = [[i + nseq * j for j in range(per)] for i in range(nseq)]
    for p, tb in zip(prompts, tables):
        n = len(p) - 1
        lm.forward_with_paged_kv_cache(p[:n], pool, [tb[i // BS] * BS + i % BS for i in range(n)], tb, n, 0)
    g = runtime.BatchDecodeGraph(lm, pool, nseq, per)
    g.seed([int(p[-1]) for p in prompts], [len(p) for p in prompts], tables)
    for _ in range(steps):
        g.replay()
    out = np.stack([g.read_tokens(s) for s in range(steps)], axis=1)
    return [out[r].tolist() for r in range(nseq)]


@pytest.mark.watchdog(300)
@pytest.mark.parametrize("prefix_cache", [False, True], ids=["plain", "prefix-cache"])
def test_engine_with_a_long_request(device, monkeypatch, prefix_cache):
    """BatchEngine with max_seq_len = 3 200 (its creation is refused on the parent): a 3 070-token prompt beside two 20-token ones, greedy, 6 tokens each.  The two
    comparisons of tests/test_gpu_engine.py: each request among the others equals that request alone, and the static batch equals a BatchDecodeGraph driven
    by hand.  With the prefix cache the long prompt is submitted twice: once by itself, which publishes its blocks, and again (a hit: 191 shared blocks, 13
    tokens prefilled) among the others -- compared with the same second submission alone."""
    monkeypatch.delenv("BZ_ROWS_SPLIT_MIN", raising=False)
    model, lm = _rep8(device, "awq-f16-hd64")
    V = model["config"]["vocab"]
    long_p, a, b = synth.prompt_tokens(3070, V, seed=61), synth.prompt_tokens(20, V, seed=62), synth.prompt_tokens(20, V, seed=63)
    alone = []
    for p in (long_p, a, b):
        toks, fin = _drive(_engine(lm), [dict(prompt=p, max_tokens=6)])
        assert len(toks[0]) == 6 and fin == [0]
        alone.append(toks[0])
    reqs = [dict(prompt=p, max_tokens=6) for p in (long_p, a, b)]
    if not prefix_cache:
        toks, fin = _drive(_engine(lm), reqs)
        assert toks == alone and fin == [0, 0, 0]
        assert toks == _static(device, model, lm, [long_p, a, b], 6, 3200 // BS)
        return
    e1, e2 = _engine(lm, True), _engine(lm, True)
    for e in (e1, e2):
        toks, _ = _drive(e, reqs[:1])
        assert toks[0] == alone[0]                     # a miss: prefilled in one piece, as without the cache
    again, _ = _drive(e1, reqs[:1])                    # the second submission alone
    toks, fin = _drive(e2, reqs)                       # ... and among the others
    assert toks == [again[0], alone[1], alone[2]] and fin == [0, 0, 0]
    for e in (e1, e2):
        ps = e.prefix_stats()
        assert ps["hits"] == 1 and ps["cached_tokens"] == 3056 == ps["prompt_tokens_skipped"], ps


# ------------------------------------------------------------------------------------------------------------------------------------------
# 7. refusals
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_refused_where_neither_kernel_applies(device, monkeypatch):
    """an f32 cache (GGUF model) beyond the scalar kernel's 18 416 positions at REP 2: BZ_E_UNSUPPORTED naming the limit, from the plan and from the capture
    (before it begins); a head_dim-96 plan likewise."""
    monkeypatch.delenv("BZ_ROWS_SPLIT_MIN", raising=False)
    p = runtime.rows_attn_plan(4, 2, 64, L.F32, 0, 2, 19200)
    assert p["kernel"] == -1 and p["code"] == L.E_UNSUPPORTED and "18416" in p["error"], p
    p = runtime.rows_attn_plan(8, 2, 96, L.F16, 0, 2, 19200)
    assert p["kernel"] == -1 and p["code"] == L.E_UNSUPPORTED and str(p["scalar_limit"]) in p["error"], p
    model = synth.make_llama("tiny-q4km", n_layers=2, max_seq_len=20000)
    lm = runtime.LoadedModel.from_synth(device, model)
    cfg = model["config"]
    pool = runtime.LayeredPagedKvCache(device, 2, 8, BS, cfg["n_kv_heads"], cfg["head_dim"], L.F32)
    with pytest.raises(L.BlazrHipError) as e:
        runtime.BatchDecodeGraph(lm, pool, 2, 19200 // BS)
    assert e.value.code == L.E_UNSUPPORTED and "18416" in str(e.value) and "19200" in str(e.value), str(e.value)
