"""Batched device sampler on the GPU (bz_sample_batch.hip): every row of a batch against the single-row sampler (runtime.logits_to_token, the
kernels of bz_sample.hip) and against the oracle -- neither is code the batched sampler shares.

Against the single-row kernel a case must match exactly unless its decision margin (tests/batch_sampler_ref.py) is below 1e-6: both sides hold the
same p_i bits and differ only in how cumulative masses are accumulated (<= V * 2^-53 ~ 1.4e-11 at 128 k), so 1e-6 leaves room and excludes a case with
probability ~4e-6; at most 1 case in 1000 may be excluded.  Against the oracle the bar is the one test_gpu_ops.py grants the single-row kernel: at most
one disagreement per 120 (row, seed) pairs of one parameter set."""
import numpy as np
import pytest

from blazr_amd import _lib as L
from blazr_amd import runtime, synth

import batch_sampler_ref as R

pytestmark = pytest.mark.gpu

_SET_ROW_KEYS = ("history", "draw_index", "temperature", "top_k", "top_p", "min_p", "repeat_penalty", "frequency_penalty", "presence_penalty", "repeat_last_n", "seed")


def _single_row(device, row_logits, kw, history=None, draw_index=None):
    """The parent's path for one row: host penalty window + bz_logits_to_token with seed + draw index."""
    hist = kw["history"] if history is None else history
    draw = kw["draw_index"] if draw_index is None else draw_index
    ids, cnts = runtime.penalty_window(list(hist), kw["repeat_last_n"]) if R.penalties_active(kw) else ([], [])
    t = device.tensor(np.ascontiguousarray(row_logits, dtype=np.float32).reshape(1, -1))
    return int(runtime.logits_to_token(device, t, ids, cnts, repeat_penalty=kw["repeat_penalty"], frequency_penalty=kw["frequency_penalty"],
                                       presence_penalty=kw["presence_penalty"], temperature=kw["temperature"], top_k=kw["top_k"], top_p=kw["top_p"],
                                       min_p=kw["min_p"], seed=kw["seed"] + draw).to_numpy()[0])


def _batched(device, logits, rows):
    N, V = logits.shape
    s = runtime.BatchSampler(device, N, V)
    for r, kw in enumerate(rows):
        s.set_row(r, **{k: kw[k] for k in _SET_ROW_KEYS})
    return s.sample(device.tensor(logits)).to_numpy().tolist(), s


_RESULTS = {}


def _run_case(device, N, V):
    """(logits, rows, batched tokens, single-row tokens, margins) of one grid case, computed once."""
    if (N, V) not in _RESULTS:
        logits, rows = R.make_case(N, V, R.case_id(N, V))
        got, _ = _batched(device, logits, rows)
        single = [_single_row(device, logits[r], kw) for r, kw in enumerate(rows)]
        margins = [R.sample_row(logits[r], **kw)[1] for r, kw in enumerate(rows)]
        _RESULTS[(N, V)] = (logits, rows, got, single, margins)
    return _RESULTS[(N, V)]


@pytest.mark.parametrize("N,V", R.GRID)
def test_rows_equal_the_single_row_sampler(device, N, V):
    logits, rows, got, single, margins = _run_case(device, N, V)
    assert all(0 <= t < V for t in got)
    excluded = [r for r in range(N) if margins[r] < R.MARGIN]
    assert len(excluded) * 1000 <= N, excluded                       # the seeds were chosen on the CPU so that none is excluded
    bad = [(r, got[r], single[r], margins[r]) for r in range(N) if margins[r] >= R.MARGIN and got[r] != single[r]]
    assert not bad, bad


def test_rows_equal_the_oracle_per_parameter_set(device):
    count, bad = [0] * len(R.PSETS), [0] * len(R.PSETS)
    for N, V in R.GRID:
        logits, rows, got, _, _ = _run_case(device, N, V)
        cid = R.case_id(N, V)
        for r, kw in enumerate(rows):
            ps = (r + cid) % len(R.PSETS)
            count[ps] += 1
            bad[ps] += got[r] != R.oracle_row(logits[r], kw)
    for ps in range(len(R.PSETS)):
        assert count[ps] >= 120 and bad[ps] * 120 <= count[ps], (ps, bad, count)


def test_ties_and_degenerate_rows(device):
    cases = R.degenerate_cases()
    total = excluded = 0
    for name, (logits, rows) in cases.items():
        N, V = logits.shape
        got, sampler = _batched(device, logits, rows)
        assert all(0 <= t < V for t in got), (name, got)
        if name == "all_neg_inf":
            again = sampler.sample(device.tensor(cases["masked_90"][0])).to_numpy()      # the next call on the same device and handle succeeds
            assert all(0 <= t < V for t in again.tolist())
            continue
        for r, kw in enumerate(rows):
            want, margin = R.sample_row(logits[r], **kw)
            total += 1
            if margin < R.MARGIN:
                excluded += 1
                continue
            assert got[r] == _single_row(device, logits[r], kw), (name, r)
            assert got[r] == want, (name, r)
        if name == "masked_90":
            assert all(np.isfinite(logits[0][t]) for t in got)                           # a masked id is never drawn
        if name == "ties_straddle_top_k":
            assert set(got) <= {100, 2000, 7, 12, 40, 333} and len(set(got)) >= 3          # the kept set follows ascending id
        if name == "all_equal_top_k":
            assert max(got) < 700
        if name == "all_equal_top_p":
            assert max(got) < 1112                                                       # ceil(0.37 * 3001) ids kept, in ascending order
    assert excluded * 1000 <= total, (excluded, total)


def test_a_row_does_not_depend_on_its_place_or_its_neighbours(device):
    V = 1003
    rng = np.random.default_rng(12)
    row = (rng.standard_normal(V) * 2.5).astype(np.float32)
    kw = dict(R.PSETS[1]); kw.update(R.PENALTIES); kw["history"] = [5, 5, 9, V - 1, 77]; kw["draw_index"] = 0
    seeds = list(range(300, 350))
    outcomes = []
    for N, place in ((2, 0), (2, 1), (64, 0), (64, 63)):
        logits = (rng.standard_normal((N, V)) * 2.5).astype(np.float32)
        logits[place] = row
        s = runtime.BatchSampler(device, N, V)
        for r in range(N):
            if r != place:
                nb = dict(R.PSETS[int(rng.integers(0, len(R.PSETS)))]); nb.update(R.PENALTIES)
                s.set_row(r, history=rng.integers(0, V, size=int(rng.integers(0, 300))).tolist(), seed=int(rng.integers(0, 1 << 30)), **nb)
        t = device.tensor(logits)
        out = device.zeros((N,), L.I64)
        toks = []
        for seed in seeds:
            s.set_row(place, seed=seed, **kw)
            toks.append(int(s.sample(t, out).to_numpy()[place]))
        outcomes.append(toks)
    assert all(o == outcomes[0] for o in outcomes[1:]), outcomes
    assert len(set(outcomes[0])) > 3


def test_device_side_history_follows_the_host_loop(device):
    V, steps = 1003, 40
    rng = np.random.default_rng(31)
    logits = (rng.standard_normal((4, V)) * 2.0).astype(np.float32)
    base = dict(temperature=0.8, top_k=50, top_p=0.95, min_p=0.0, repeat_penalty=1.3, frequency_penalty=0.2, presence_penalty=0.1, draw_index=0)
    rows, hists = [], []
    for r, (last_n, hlen) in enumerate(((1, 300), (4, 300), (64, 240), (256, 250))):
        h = rng.integers(0, 40, size=hlen).tolist()                  # few distinct ids: counts above 1
        h[-3] = V + 5                                                # out of range: skipped
        h[5] = -2
        rows.append(dict(base, repeat_last_n=last_n, seed=900 + r))
        hists.append(h)
    s = runtime.BatchSampler(device, 4, V)
    for r in range(4):
        s.set_row(r, history=hists[r], **rows[r])
    t = device.tensor(logits)
    out = device.zeros((4,), L.I64)
    total = excluded = 0
    for step in range(steps):                                        # rows 2 and 3 cross slot 256 of the ring at steps 16 and 6; rows 0 and 1 start full
        got = s.sample(t, out).to_numpy().tolist()
        for r in range(4):
            kw = dict(rows[r], history=hists[r], draw_index=step)
            _, margin = R.sample_row(logits[r], **kw)
            total += 1
            if margin >= R.MARGIN:
                assert got[r] == _single_row(device, logits[r], kw), (step, r)
            else:
                excluded += 1
            hists[r].append(got[r])
    assert excluded * 1000 <= total, (excluded, total)


def _kv_dt(cfg):
    return {"f16": L.F16, "bf16": L.BF16, "f32": L.F32}[cfg["act_dtype"]]


@pytest.mark.parametrize("preset", ["tiny-awq", "tiny-bf16"])
def test_sampled_batch_graph(device, preset):
    model = synth.make_llama(preset)
    cfg = model["config"]
    V = cfg["vocab"]
    lm = runtime.LoadedModel.from_synth(device, model)
    nseq, bs, per, steps = 4, 16, 5, 24
    def fresh_pool():
        return runtime.LayeredPagedKvCache(device, cfg["n_layers"], nseq * per, bs, cfg["n_kv_heads"], cfg["head_dim"], _kv_dt(cfg))
    tables = [[i + nseq * j for j in range(per)] for i in range(nseq)]
    plens = [3 + (13 * i) % 30 for i in range(nseq)]
    prompts = [synth.prompt_tokens(n, V, seed=70 + i) for i, n in enumerate(plens)]

    def prefill(pool):
        first = []
        for p, tb in zip(prompts, tables):
            slots = [tb[i // bs] * bs + i % bs for i in range(len(p))]
            lg = lm.forward_with_paged_kv_cache(p, pool, slots, tb, len(p), 0).to_numpy()
            first.append(int(lg[0].argmax()))
        return first

    none = dict(repeat_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0, repeat_last_n=64)
    params = [dict(none, temperature=0.8, top_k=12, top_p=1.0, min_p=0.02, seed=211),
              dict(none, temperature=0.0, top_k=0, top_p=1.0, min_p=0.0, seed=0),
              dict(temperature=1.0, top_k=10, top_p=0.9, min_p=0.0, repeat_penalty=1.2, frequency_penalty=0.0, presence_penalty=0.0, repeat_last_n=16, seed=212),
              dict(temperature=1.3, top_k=8, top_p=1.0, min_p=0.05, repeat_penalty=1.0, frequency_penalty=0.3, presence_penalty=0.1, repeat_last_n=64, seed=213)]
    # A draw is within the margin of one of the two ends of its interval with probability 2e-6 x (candidates kept) / (kept mass): these models' rows are
    # nearly flat over 1024 ids, so an unfiltered row would be excluded about once in 500 draws.  Every sampled row keeps at most 12 candidates (top-k),
    # which puts the 72 sampled draws of one run at ~0.2 %; the step is deterministic, so the seeds below, which exclude none, keep doing so.
    swapped = dict(none, temperature=0.9, top_k=5, top_p=1.0, min_p=0.02, seed=99)

    with pytest.raises(L.BlazrHipError) as e:
        runtime.BatchDecodeGraph(lm, fresh_pool(), nseq, per, sampler=runtime.BatchSampler(device, nseq - 1, V))
    assert e.value.code == L.E_INVALID and "sampler" in str(e.value)
    with pytest.raises(L.BlazrHipError) as e:
        runtime.BatchDecodeGraph(lm, fresh_pool(), nseq, per, sampler=runtime.BatchSampler(device, nseq, V + 1))
    assert e.value.code == L.E_INVALID and "sampler" in str(e.value)

    pool = fresh_pool()
    first = prefill(pool)
    hists = [list(map(int, p)) + [first[i]] for i, p in enumerate(prompts)]
    draws = [0] * nseq
    sampler = runtime.BatchSampler(device, nseq, V)
    for r in range(nseq):
        sampler.set_row(r, history=hists[r], draw_index=0, **params[r])
    g = runtime.BatchDecodeGraph(lm, pool, nseq, per, sampler=sampler)
    g.seed(first, [n + 1 for n in plens], tables)
    total, excluded = 0, []
    fed = [list(first)]                                              # what every replay consumed
    for step in range(steps):
        g.replay()
        lg = g.read_logits()
        got = g.read_tokens(step).tolist()
        for r in range(nseq):
            kw = dict(params[r], history=hists[r], draw_index=draws[r])
            _, margin = R.sample_row(lg[r], **kw)
            total += 1
            if margin >= R.MARGIN:
                assert got[r] == _single_row(device, lg[r], kw), (step, r)
            else:
                excluded.append((step, r, margin, got[r]))
            hists[r].append(got[r]); draws[r] += 1
        fed.append(got)
        if step == 12:                                               # row 2 is handed to a new configuration: no recapture
            params[2] = swapped
            hists[2] = hists[2][-7:]
            draws[2] = 0
            sampler.set_row(2, history=hists[2], draw_index=0, **swapped)
    assert len(excluded) * 1000 <= total, (excluded, total)
    assert len({tuple(f) for f in fed}) > 1
    # the greedy row against an unsampled graph fed the same tokens: rows of the batched step do not see each other
    pool_b = fresh_pool()
    assert prefill(pool_b) == first
    g2 = runtime.BatchDecodeGraph(lm, pool_b, nseq, per)
    g2.seed(first, [n + 1 for n in plens], tables)
    for step in range(steps):
        g2.replay()
    assert [g2.read_tokens(s)[1] for s in range(steps)] == [fed[s + 1][1] for s in range(steps)]
    del g, g2


def test_draws_follow_the_softmax(device):
    rng = np.random.default_rng(4)
    V, N, calls, T = 48, 500, 12, 1.5
    row = rng.standard_normal(V).astype(np.float32)
    s = runtime.BatchSampler(device, N, V)
    for r in range(N):
        s.set_row(r, temperature=T, seed=1000 * r)                   # draw t of row r uses seed 1000 r + t: all distinct
    t = device.tensor(np.repeat(row[None, :], N, axis=0))
    out = device.zeros((N,), L.I64)
    counts = np.zeros(V)
    for _ in range(calls):
        np.add.at(counts, s.sample(t, out).to_numpy(), 1)
    p = np.exp((row - row.max()) / T)
    p /= p.sum()
    n = N * calls
    chi2 = float((((counts - n * p) ** 2) / (n * p)).sum())
    assert chi2 < 95.0, chi2                                         # 47 degrees of freedom: the bound of the single-row test


def test_refusals_name_their_cause(device):
    def refused(fn, *words):
        with pytest.raises(L.BlazrHipError) as e:
            fn()
        assert e.value.code == L.E_INVALID, str(e.value)
        assert all(w in str(e.value) for w in words), str(e.value)
    refused(lambda: runtime.BatchSampler(device, 0, 100), "N = 0")
    refused(lambda: runtime.BatchSampler(device, 513, 100), "N = 513")
    refused(lambda: runtime.BatchSampler(device, 4, 0), "V = 0")
    refused(lambda: runtime.BatchSampler(device, 4, (1 << 20) + 1), "V = 1048577")
    s = runtime.BatchSampler(device, 4, 100)
    refused(lambda: s.set_row(0, temperature=-0.5), "temperature")
    refused(lambda: s.set_row(0, temperature=float("nan")), "temperature")
    refused(lambda: s.set_row(0, temperature=1.0, repeat_penalty=1.1, repeat_last_n=0), "repeat_last_n = 0")
    refused(lambda: s.set_row(0, temperature=1.0, presence_penalty=0.1, repeat_last_n=257), "repeat_last_n = 257")
    refused(lambda: s.set_row(4, temperature=1.0), "row 4")
    s.set_row(0, temperature=1.0, repeat_last_n=0)                   # ignored while no penalty is active
    good, tok = device.zeros((4, 100)), device.zeros((4,), L.I64)
    refused(lambda: s.sample(device.zeros((4, 101)), tok), "logits")
    refused(lambda: s.sample(device.zeros((3, 100)), tok), "logits")
    refused(lambda: s.sample(device.zeros((4, 100), L.F16), tok), "logits")
    refused(lambda: s.sample(good, device.zeros((5,), L.I64)), "tokens_out")
    refused(lambda: s.sample(good, device.zeros((4,), L.I32)), "tokens_out")
    got = s.sample(good, tok).to_numpy().tolist()                    # after the refusals the handle still works: row 0 draws, rows 1-3 are greedy
    assert 0 <= got[0] < 100 and got[1:] == [0, 0, 0]
