"""Per-row grammars on the device (blazr_amd/csrc/bz_grammar.hip: k_grammar_mask_rows, k_grammar_advance_rows, the cursor) and inside the two captured
steps (bz_decode_batch_graph_capture_grammar, bz_decode_graph_capture(_paged)_grammar, bz_generate_grammar with use_graph = 1).  References: the Python
restatement tests/grammar_ref.py for masks and states, the single-row sampler for sampled picks (the margin rule of tests/test_gpu_batch_sampler.py), the eager
loops for the captured ones.  Masks, states, greedy tokens and untouched logits are compared exactly."""
import numpy as np
import pytest

import batch_sampler_ref as R
import grammar_ref as G
from blazr_amd import _lib as L
from blazr_amd import runtime, synth
from test_gpu_batch_sampler import _single_row
from test_gpu_grammar import _Stepper, _big_table, _bits, _model, _nasty_logits, _states_after_tokens
from test_gpu_llama import _kv_dt
from test_grammar_rows import LITERALS, REGULAR

pytestmark = pytest.mark.gpu

THIRD = 'root ::= word ( " " word )*\nword ::= "yes" | "no" | "maybe" | "0" [0-9]+'
FREE = runtime.GrammarCursor.FREE
_VOCABS = {}


def _vocab(V, seed):
    if (V, seed) not in _VOCABS:
        _VOCABS[(V, seed)] = G.synth_vocab(V, seed=seed)[0]
    return _VOCABS[(V, seed)]


def _dead_end(t):
    """a state without transitions: it admits the empty tokens and nothing else"""
    dead = np.nonzero((t < 0).all(axis=1))[0]
    assert len(dead)
    return int(dead[0])


def _rows_dfa(kind, vocab):
    """-> (GrammarDfa, table, the states rows are put in: starts, states some tokens in, a dead end)"""
    if kind == "literals":
        g = runtime.GrammarDfa(LITERALS)
        t, _ = g.table()
        states = _states_after_tokens(t, vocab, seed=5)
    elif kind == "global-table":
        t, a = _big_table(300)
        t[299] = -1                                                  # a dead end; transitions into it stay
        g = runtime.GrammarDfa(table=t, accepting=a)
        states = _states_after_tokens(t, vocab, seed=6)
    else:
        parts = [runtime.GrammarDfa(LITERALS), runtime.GrammarDfa(REGULAR, regular=True)]
        g, starts = runtime.GrammarDfa.concat(parts)
        t, _ = g.table()
        states = []
        for p, o in zip(parts, starts):                               # rows in both languages
            states += [o + s for s in _states_after_tokens(p.table()[0], vocab, seed=7, n=2)]
    assert len(states) >= 3
    return g, t, states + [_dead_end(t)]


@pytest.mark.parametrize("N", [1, 3, 9])
@pytest.mark.parametrize("V", [1000, 1025])
@pytest.mark.parametrize("kind", ["literals", "global-table", "concat"])
def test_mask_rows_equals_the_restatement_bit_for_bit(device, kind, V, N):
    vocab = _vocab(V, V + 1)
    g, t, states = _rows_dfa(kind, vocab)
    dg = g.to_device(device, vocab)
    assert dg.info()["lds_table"] == (kind == "literals")            # 118 states in LDS; 300 and 150 through L2
    cur = runtime.GrammarCursor(dg, N)
    pool = states + [FREE]
    masks = {s: G.token_mask(t, s, vocab) for s in states}
    empty = np.array([len(tok) == 0 for tok in vocab])
    assert np.array_equal(masks[states[-1]], empty)                  # the dead end admits exactly the empty tokens
    x = _nasty_logits(N, V, seed=N + V)
    # every rotation of the pool over the rows: each row visits each state (and FREE), and a permutation of the states permutes the result and nothing else
    for k in range(len(pool)):
        row_states = [pool[(k + r) % len(pool)] for r in range(N)]
        for r, s in enumerate(row_states):
            cur.set_row(r, s)
        want = x.copy()
        for r, s in enumerate(row_states):
            if s != FREE:
                want[r][~masks[s]] = -np.inf
        tx = device.tensor(x)
        cur.mask(tx)
        got = tx.to_numpy()
        assert np.array_equal(_bits(got), _bits(want)), (kind, V, N, k, int((_bits(got) != _bits(want)).sum()))
        st, rej = cur.read()
        assert st.tolist() == row_states and not rej.any()           # masking moves no state


def test_cursor_starts_at_the_grammars_state_and_checks_its_arguments(device):
    vocab = _vocab(1000, 2)
    g = runtime.GrammarDfa(LITERALS)
    g.advance(b"the ")
    dg = g.to_device(device, vocab)
    cur = runtime.GrammarCursor(dg, 3)
    st, rej = cur.read()
    assert st.tolist() == [g.current_state()] * 3 and rej.tolist() == [0, 0, 0]

    def refused(fn, *words):
        with pytest.raises(L.BlazrHipError) as e:
            fn()
        assert e.value.code == L.E_INVALID, str(e.value)
        assert all(w in str(e.value) for w in words), str(e.value)
    refused(lambda: runtime.GrammarCursor(dg, 0), "N = 0")
    refused(lambda: runtime.GrammarCursor(dg, 513), "N = 513")
    refused(lambda: cur.set_row(3, 0), "row 3")
    refused(lambda: cur.set_row(0, g.num_states()), "state %d" % g.num_states())
    refused(lambda: cur.set_row(0, 0xFFFFFFFE), "state")
    refused(lambda: cur.mask(device.zeros((3, 1001))), "logits")
    refused(lambda: cur.mask(device.zeros((2, 1000))), "logits")
    refused(lambda: cur.advance(device.zeros((2,), L.I64)), "tokens")
    refused(lambda: cur.advance(device.zeros((3,), L.I32)), "tokens")
    cur.set_row(1, FREE)
    assert cur.read()[0].tolist() == [g.current_state(), FREE, g.current_state()]


def test_advance_rows_follows_the_host_dfa(device):
    V = 1000
    vocab = _vocab(V, 12)
    parts = [runtime.GrammarDfa(LITERALS), runtime.GrammarDfa(REGULAR, regular=True)]
    g, starts = runtime.GrammarDfa.concat(parts)
    t, _ = g.table()
    dg = g.to_device(device, vocab)
    N = 6
    cur = runtime.GrammarCursor(dg, N)
    byte = lambda ch: vocab.index(ch)
    empty = [i for i, tok in enumerate(vocab) if not tok]
    long_tok = next(i for i, tok in enumerate(vocab) if len(tok) >= 64)
    # a token whose first byte the start of LITERALS takes and whose middle does not: part of it is walked, part rejected
    mid = next(i for i, tok in enumerate(vocab) if len(tok) >= 3 and t[starts[0], tok[0]] >= 0 and 0 < G.advance(t, starts[0], tok)[1] < len(tok)
               and G.advance(t, starts[0], tok[:2])[1] == 1)
    init = [starts[0], starts[1], starts[0], FREE, starts[1], starts[0]]
    for r, s in enumerate(init):
        cur.set_row(r, s)
    calls = [[byte(b"t"), byte(b"<"), mid, byte(b"t"), empty[0], V],                 # row 5: an id that is no token
             [byte(b"h"), byte(b"4"), empty[1], long_tok, long_tok, -1],
             [byte(b"e"), byte(b">"), byte(b"Q"), empty[0], byte(b"\""), byte(b"p")]]
    state, rej = list(init), [0] * N
    for toks in calls:
        cur.advance(device.tensor(np.asarray(toks, dtype=np.int64)))
        for r, tk in enumerate(toks):
            if state[r] != FREE and 0 <= tk < V:
                state[r], k = G.advance(t, state[r], vocab[tk])
                rej[r] += k
        st, rj = cur.read()
        assert st.tolist() == state and rj.tolist() == rej, (toks, st, rj, state, rej)
    assert state[0] == G.advance(t, starts[0], b"the")[0] and rej[0] == 0
    assert rej[2] >= 2 and rej[4] > 0 and state[3] == FREE and rej[3] == 0 and rej[5] == 0
    # set_row restarts a row's rejected count and leaves the other rows alone
    cur.set_row(2, starts[1])
    state[2], rej[2] = starts[1], 0
    st, rj = cur.read()
    assert st.tolist() == state and rj.tolist() == rej


# ---- the batched step -------------------------------------------------------------------------------------------------------------------------------------
def _argmax_to_buf(device, row):
    tl = device.tensor(np.ascontiguousarray(row, dtype=np.float32).reshape(1, -1))
    tok = device.zeros((1,), L.I64)
    L.check(L.lib().bz_argmax_to_buf(device.h, tl.h, 1, tl.shape[1], tok.h))
    return int(tok.to_numpy()[0])


@pytest.mark.parametrize("preset", ["tiny-awq", "tiny-bf16"])
def test_batch_graph_with_per_row_grammars(device, preset):
    model, lm = _model(device, preset)
    cfg = model["config"]
    V = cfg["vocab"]
    vocab = _vocab(V, 21)
    nseq, bs, per, steps = 4, 16, 5, 24
    parts = [runtime.GrammarDfa(LITERALS), runtime.GrammarDfa(REGULAR, regular=True), runtime.GrammarDfa(THIRD, regular=True)]
    cat, starts = runtime.GrammarDfa.concat(parts)
    t, _ = cat.table()
    dg = cat.to_device(device, vocab)

    def fresh_pool():
        return runtime.LayeredPagedKvCache(device, cfg["n_layers"], nseq * per, bs, cfg["n_kv_heads"], cfg["head_dim"], _kv_dt(cfg))
    tables = [[i + nseq * j for j in range(per)] for i in range(nseq)]
    plens = [3 + (13 * i) % 30 for i in range(nseq)]
    prompts = [synth.prompt_tokens(n, V, seed=70 + i) for i, n in enumerate(plens)]
    row_start = [starts[0], starts[1], FREE, FREE]                   # greedy + A, sampled + B, sampled + free, greedy + free

    def prefill(pool):
        """first token of every row from its prompt logits, masked for the constrained rows; -> (tokens, states after them)"""
        first, state = [], []
        for r, (p, tb) in enumerate(zip(prompts, tables)):
            slots = [tb[i // bs] * bs + i % bs for i in range(len(p))]
            lg = lm.forward_with_paged_kv_cache(p, pool, slots, tb, len(p), 0).to_numpy()[0]
            s = row_start[r]
            if s != FREE:
                lg = G.mask_logits(t, s, vocab, lg)
            tok = int(lg.argmax())
            if s != FREE:
                s, rej = G.advance(t, s, vocab[tok])
                assert rej == 0
            first.append(tok); state.append(s)
        return first, state

    none = dict(repeat_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0, repeat_last_n=64)
    greedy = dict(none, temperature=0.0, top_k=0, top_p=1.0, min_p=0.0, seed=0)
    # the sampled rows keep at most 12 candidates, as in test_sampled_batch_graph: 48 sampled draws put an excluded draw at ~0.1 % per run, the step is
    # deterministic, and these seeds exclude none
    params = [greedy, dict(none, temperature=0.8, top_k=12, top_p=1.0, min_p=0.02, seed=311), dict(none, temperature=1.0, top_k=10, top_p=0.9, min_p=0.0, seed=312), greedy]

    pool = fresh_pool()
    first, state = prefill(pool)
    cur = runtime.GrammarCursor(dg, nseq)
    for r in range(nseq):
        cur.set_row(r, state[r])
    hists = [list(map(int, p)) + [first[i]] for i, p in enumerate(prompts)]
    draws = [0] * nseq
    sampler = runtime.BatchSampler(device, nseq, V)
    for r in range(nseq):
        sampler.set_row(r, history=hists[r], draw_index=0, **params[r])
    g = runtime.BatchDecodeGraph(lm, pool, nseq, per, sampler=sampler, grammar=cur)
    g.seed(first, [n + 1 for n in plens], tables)
    total, excluded, fed = 0, [], [list(first)]
    admissible, free_ok = [], 0
    for step in range(steps):
        g.replay()                                                   # nothing from the host between replays but these reads
        lg = g.read_logits()
        got = g.read_tokens(step).tolist()
        for r in range(nseq):
            if state[r] == FREE:
                assert not np.isneginf(lg[r]).any(), (step, r)
            else:
                allowed = G.token_mask(t, state[r], vocab)
                assert np.array_equal(np.isneginf(lg[r]), ~allowed), (step, r, state[r])
                if r == 0:
                    admissible.append(allowed.mean())
            kw = dict(params[r], history=hists[r], draw_index=draws[r])
            _, margin = R.sample_row(lg[r], **kw)
            total += 1
            if margin >= R.MARGIN:
                assert got[r] == _single_row(device, lg[r], kw), (step, r)
            else:
                excluded.append((step, r, margin, got[r]))
            if state[r] != FREE:
                state[r], rej = G.advance(t, state[r], vocab[got[r]])
                assert rej == 0, (step, r, got[r])
            hists[r].append(got[r]); draws[r] += 1
        fed.append(got)
        if step == 12:                                               # row 1 is handed to a third grammar by set_row alone: no recapture
            cur.set_row(1, starts[2])
            state[1] = starts[2]
    print("excluded draws:", excluded, "of", total)
    assert len(excluded) * 1000 <= total, (excluded, total)
    st, rj = cur.read()
    assert st.tolist() == state and not rj.any()
    assert starts[2] <= state[1] and starts[0] <= state[0] < starts[1]
    # row 1's tokens after the hand-over are a viable prefix of the third grammar
    t3, a3 = parts[2].table()
    s3, rej3 = G.advance(t3, 0, b"".join(vocab[fed[s + 1][1]] for s in range(13, steps)))
    assert rej3 == 0 and s3 + starts[2] == state[1] and G.co_accessible(t3, a3)[s3]
    assert max(admissible) < 0.05, admissible                        # the constraint binds: under 5 % of the vocabulary is admissible on the greedy row

    # the free greedy row against a grammarless graph fed the same first tokens: rows do not see each other, and a FREE row is the row it always was
    pool_b = fresh_pool()
    prefill(pool_b)
    g2 = runtime.BatchDecodeGraph(lm, pool_b, nseq, per)
    g2.seed(first, [n + 1 for n in plens], tables)
    for step in range(steps):
        g2.replay()
    assert [int(g2.read_tokens(s)[3]) for s in range(steps)] == [fed[s + 1][3] for s in range(steps)]

    # a second capture without a sampler: every row greedy.  Against the eager batched step + mask_logits + bz_argmax_to_buf row by row
    pool_c, pool_d = fresh_pool(), fresh_pool()
    first_c, state_c = prefill(pool_c)
    assert prefill(pool_d)[0] == first_c == first
    cur_c = runtime.GrammarCursor(dg, nseq)
    for r in range(nseq):
        cur_c.set_row(r, state_c[r])
    g3 = runtime.BatchDecodeGraph(lm, pool_c, nseq, per, grammar=cur_c)
    g3.seed(first_c, [n + 1 for n in plens], tables)
    for step in range(steps):
        g3.replay()
    toks, lens, st_d = list(first_c), list(plens), list(state_c)
    one = cat.to_device(device, vocab)                               # the single-row mask path, put into each row's state in turn
    for step in range(steps):
        lens = [n + 1 for n in lens]
        slots = [tb[(n - 1) // bs] * bs + (n - 1) % bs for n, tb in zip(lens, tables)]
        lg = lm.forward_paged_batch(toks, pool_d, slots, tables, lens).to_numpy()
        nxt = []
        for r in range(nseq):
            if st_d[r] == FREE:
                nxt.append(_argmax_to_buf(device, lg[r]))
                continue
            if r == 0:                                               # what the row would pick unconstrained must mostly be inadmissible, or the comparison shows little
                free_ok += bool(G.token_mask(t, st_d[r], vocab)[int(lg[r].argmax())])
            one.set_state(st_d[r])
            tl = device.tensor(lg[r:r + 1])
            one.mask_logits(tl)
            nxt.append(_argmax_to_buf(device, tl.to_numpy()[0]))
            st_d[r], rej = G.advance(t, st_d[r], vocab[nxt[-1]])
            assert rej == 0
        assert g3.read_tokens(step).tolist() == nxt, step
        toks = nxt
    assert cur_c.read()[0].tolist() == st_d
    assert free_ok <= steps // 2, "the unconstrained argmax was admissible at %d of %d steps: the comparison would show little" % (free_ok, steps)
    del g, g2, g3


# ---- the single-sequence step --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("branch", ["contiguous", "paged"])
def test_single_graph_with_a_grammar_equals_the_eager_loop(device, branch):
    model, lm = _model(device, "tiny-awq")
    V = model["config"]["vocab"]
    vocab = _vocab(V, 21)
    prompt = synth.prompt_tokens(8, V)
    n_new = 17
    ex = runtime.Executor(lm)
    paged = branch == "paged"
    g = runtime.GrammarDfa(REGULAR, regular=True)
    t, _ = g.table()
    want = ex.generate(prompt, n_new, paged=paged, grammar=g, vocab_bytes=vocab).tolist()
    final = g.current_state()
    assert G.advance(t, 0, b"".join(vocab[k] for k in want)) == (final, 0) and len(want) == n_new
    # DecodeGraph(grammar=cursor): the first token from the masked prompt logits, then 16 replays without a host step
    g.reset()
    dg = g.to_device(device, vocab)
    st = _Stepper(device, model, lm, branch, len(prompt), n_new)
    logits = st.forward(prompt)
    dg.mask_logits(logits)
    tok0 = int(logits.to_numpy()[0].argmax())
    assert tok0 == want[0]
    s0, _ = G.advance(t, 0, vocab[tok0])
    cur = runtime.GrammarCursor(dg, 1)
    cur.set_row(0, s0)
    if paged:
        nblocks = st.pk.num_blocks
        graph = runtime.DecodeGraph(lm, st.pk, max_blocks=nblocks, grammar=cur)
        graph.set_block_table(list(range(nblocks)))
    else:
        graph = runtime.DecodeGraph(lm, st.kv, grammar=cur)
    graph.seed_next_token(tok0, len(prompt))
    for _ in range(n_new - 1):
        graph.replay()
    assert [graph.read_token(i) for i in range(n_new - 1)] == want[1:]
    before_last = G.advance(t, 0, b"".join(vocab[k] for k in want[:-1]))[0]
    assert np.array_equal(np.isneginf(graph.read_logits()), ~G.token_mask(t, before_last, vocab))      # read_logits returns the masked row
    sts, rej = cur.read()
    assert sts.tolist() == [final] and rej.tolist() == [0]
    del graph
    # generate(use_graph=True, grammar=...) takes the captured step: the eager tokens, g in the same final state
    g.reset()
    assert ex.generate(prompt, n_new, paged=paged, use_graph=True, grammar=g, vocab_bytes=vocab).tolist() == want
    assert g.current_state() == final
    # with an active penalty graph mode would ignore what the eager loop applies: the eager loop runs, and its tokens come back
    g.reset()
    pen = ex.generate(prompt, n_new, paged=paged, repeat_penalty=1.1, grammar=g, vocab_bytes=vocab).tolist()
    s_pen = g.current_state()
    g.reset()
    assert ex.generate(prompt, n_new, paged=paged, repeat_penalty=1.1, use_graph=True, grammar=g, vocab_bytes=vocab).tolist() == pen
    assert g.current_state() == s_pen


@pytest.mark.parametrize("branch", ["contiguous", "paged"])
def test_single_graph_with_a_grammar_crosses_into_the_split_kv_variant(device, branch):
    model = synth.make_llama("tiny-awq", max_seq_len=640)
    lm = runtime.LoadedModel.from_synth(device, model)
    V = model["config"]["vocab"]
    vocab = _vocab(V, 21)
    prompt = synth.prompt_tokens(508, V, seed=5)                      # replays at positions 508 .. 518: the split-KV variant takes over beyond 512
    ex = runtime.Executor(lm)
    g = runtime.GrammarDfa(REGULAR, regular=True)
    t, _ = g.table()
    want = ex.generate(prompt, 12, paged=branch == "paged", grammar=g, vocab_bytes=vocab).tolist()
    final = g.current_state()
    g.reset()
    got = ex.generate(prompt, 12, paged=branch == "paged", use_graph=True, grammar=g, vocab_bytes=vocab).tolist()
    assert got == want and g.current_state() == final
    state = 0
    for k in got:                                                     # every token admissible where it was picked
        assert G.token_mask(t, state, vocab)[k]
        state, rej = G.advance(t, state, vocab[k])
        assert rej == 0
    assert state == final


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------------
def test_captures_refuse_a_cursor_that_does_not_fit_and_name_it(device):
    model, lm = _model(device, "tiny-awq")
    cfg = model["config"]
    V = cfg["vocab"]
    g = runtime.GrammarDfa(LITERALS)
    dg = g.to_device(device, _vocab(V, 21))
    nseq, per = 4, 2

    def pool():
        return runtime.LayeredPagedKvCache(device, cfg["n_layers"], nseq * per, 16, cfg["n_kv_heads"], cfg["head_dim"], _kv_dt(cfg))

    def refused(fn, code, *words):
        with pytest.raises(L.BlazrHipError) as e:
            fn()
        assert e.value.code == code, str(e.value)
        assert all(w in str(e.value) for w in words), str(e.value)
    refused(lambda: runtime.BatchDecodeGraph(lm, pool(), nseq, per, grammar=runtime.GrammarCursor(dg, nseq - 1)), L.E_INVALID, "cursor", "N = 3")
    dg_v = g.to_device(device, _vocab(V + 1, 21))
    refused(lambda: runtime.BatchDecodeGraph(lm, pool(), nseq, per, grammar=runtime.GrammarCursor(dg_v, nseq)), L.E_INVALID, "cursor", "V = %d" % (V + 1))
    refused(lambda: runtime.BatchDecodeGraph(lm, pool(), nseq, per, sampler=runtime.BatchSampler(device, nseq - 1, V), grammar=runtime.GrammarCursor(dg, nseq)),
            L.E_INVALID, "sampler")
    other = runtime.Device(0)                                         # a second handle on the same GPU
    try:
        dg_o = g.to_device(other, _vocab(V, 21))
        cur_o = runtime.GrammarCursor(dg_o, nseq)
        refused(lambda: runtime.BatchDecodeGraph(lm, pool(), nseq, per, grammar=cur_o), L.E_INVALID, "cursor", "another device handle")
        cur_o1 = runtime.GrammarCursor(dg_o, 1)
        refused(lambda: runtime.DecodeGraph(lm, lm.new_kv_cache(32), grammar=cur_o1), L.E_INVALID, "cursor", "another device handle")
        del cur_o, cur_o1, dg_o
    finally:
        other.close()
    # the single-sequence step
    refused(lambda: runtime.DecodeGraph(lm, lm.new_kv_cache(32), grammar=runtime.GrammarCursor(dg, 2)), L.E_INVALID, "cursor", "N = 2")
    refused(lambda: runtime.DecodeGraph(lm, lm.new_kv_cache(32), grammar=runtime.GrammarCursor(dg_v, 1)), L.E_INVALID, "cursor", "V = %d" % (V + 1))
    refused(lambda: runtime.DecodeGraph(lm, pool(), max_blocks=2, grammar=runtime.GrammarCursor(dg, 2)), L.E_INVALID, "cursor", "N = 2")
    mmodel, mlm = _model(device, "tiny-mamba2")
    dg_m = g.to_device(device, _vocab(mmodel["config"]["vocab"], 21))
    refused(lambda: runtime.DecodeGraph(mlm, runtime.LayeredSsmState(mlm), grammar=runtime.GrammarCursor(dg_m, 1)), L.E_UNSUPPORTED, "llama family")
    cur = runtime.GrammarCursor(dg, 1)
    refused(lambda: cur.set_row(0, g.num_states()), L.E_INVALID, "state %d" % g.num_states())
    # after the refusals everything still works
    graph = runtime.DecodeGraph(lm, lm.new_kv_cache(32), grammar=cur)
    graph.seed_next_token(1, 0)
    graph.replay()
    assert G.token_mask(g.table()[0], 0, _vocab(V, 21))[graph.read_token(0)]
