"""Host side of per-row grammars (blazr_amd/csrc/bz_grammar.hip): bz_grammar_concat -- n DFAs as one table, a row's state alone deciding its language -- and
bz_grammar_advance_tokens, against the Python restatement in tests/grammar_ref.py.  No device is needed."""
import numpy as np
import pytest

import grammar_ref as G
from blazr_amd import _lib as L
from blazr_amd import runtime

LITERALS = 'root ::= "the quick brown fox jumps over the lazy dog" | "pack my box with five dozen liquor jugs" | "{\\"name\\": \\"Ada Lovelace\\", \\"age\\": 36}"'
REGULAR = 'root ::= item ( "," item )*\nitem ::= "<" [0-9] [0-9]? ">" | "\\"" name "\\""\nname ::= ( "Ada" | "item" [-_] [0-9] )+'


def _parts():
    return [runtime.GrammarDfa(LITERALS), runtime.GrammarDfa(REGULAR, regular=True), runtime.GrammarDfa('start ::= "no root rule"')]


def _walk(t, vocab, seed, depth):
    """a state `depth` admissible non-empty tokens in, and the bytes that lead there"""
    rng = np.random.RandomState(seed)
    s, text = 0, b""
    for _ in range(depth):
        ok = [i for i in np.nonzero(G.token_mask(t, s, vocab))[0] if vocab[i]]
        if not ok:
            break
        tok = vocab[ok[rng.randint(len(ok))]]
        s, rej = G.advance(t, s, tok)
        assert rej == 0
        text += tok
    return s, text


def test_concat_stacks_the_tables_and_keeps_every_language():
    parts = _parts()
    tabs = [p.table() for p in parts]
    assert tabs[2][0].shape == (1, 256)
    cat, starts = runtime.GrammarDfa.concat(parts)
    offs = np.concatenate([[0], np.cumsum([len(t) for t, _ in tabs])])
    assert starts == offs[:-1].tolist() and cat.num_states() == offs[-1] and cat.current_state() == starts[0]
    ct, ca = cat.table()
    for (t, a), o in zip(tabs, offs):
        assert np.array_equal(ct[o:o + len(t)], np.where(t >= 0, t + o, -1))
        assert np.array_equal(ca[o:o + len(t)], a)
    assert np.array_equal(ca, np.concatenate([a for _, a in tabs]))
    vocab, _ = G.synth_vocab(300, seed=4)
    for (t, a), o in zip(tabs, offs):
        for depth in (0, 2, 4):
            s, text = _walk(t, vocab, seed=depth, depth=depth)
            assert np.array_equal(G.token_mask(ct, o + s, vocab), G.token_mask(t, s, vocab))
    # through the library: the concatenation starts in grammar 0 and, walked along a sentence of it, keeps computing grammar 0's masks
    t0 = tabs[0][0]
    assert np.array_equal(cat.compute_token_mask(vocab), G.token_mask(t0, 0, vocab))
    s, text = _walk(t0, vocab, seed=9, depth=3)
    assert cat.advance(text) == 0 and cat.current_state() == starts[0] + s
    assert np.array_equal(cat.compute_token_mask(vocab), G.token_mask(t0, s, vocab))


def test_concat_blocks_do_not_reach_each_other():
    parts = _parts()
    cat, starts = runtime.GrammarDfa.concat(parts)
    ct, _ = cat.table()
    bounds = starts + [cat.num_states()]
    for i in range(len(parts)):
        blk = ct[bounds[i]:bounds[i + 1]]
        live = blk[blk >= 0]
        assert ((live >= bounds[i]) & (live < bounds[i + 1])).all()


def test_concat_refusals():
    t = np.full((33000, 256), -1, dtype=np.int32)
    a = np.zeros(33000, dtype=np.uint8)
    big = [runtime.GrammarDfa(table=t, accepting=a), runtime.GrammarDfa(table=t, accepting=a)]
    with pytest.raises(L.BlazrHipError) as e:
        runtime.GrammarDfa.concat(big)
    assert e.value.code == L.E_UNSUPPORTED and "66000" in str(e.value)
    with pytest.raises(L.BlazrHipError) as e:
        runtime.GrammarDfa.concat([])
    assert e.value.code == L.E_INVALID
    with pytest.raises(L.BlazrHipError) as e:
        runtime.GrammarDfa.concat([runtime.GrammarDfa(LITERALS), None])
    assert e.value.code == L.E_INVALID and "null" in str(e.value)
    # one grammar alone is itself
    one, starts = runtime.GrammarDfa.concat([runtime.GrammarDfa(LITERALS)])
    assert starts == [0] and np.array_equal(one.table()[0], runtime.GrammarDfa(LITERALS).table()[0])


def test_advance_tokens_equals_advance_over_the_joined_bytes():
    V = 1000
    vocab, eos = G.synth_vocab(V, seed=12)
    g = runtime.GrammarDfa(REGULAR, regular=True)
    t, _ = g.table()
    empty = [i for i, tok in enumerate(vocab) if not tok]
    long_tok = next(i for i, tok in enumerate(vocab) if len(tok) >= 64)
    byte = lambda ch: vocab.index(ch)
    # "<4>" "," then 'Z', which no state of this grammar takes: the state stays and one byte is counted; then the sentence goes on
    toks = [empty[0], byte(b"<"), byte(b"4"), byte(b">"), empty[1], byte(b","), byte(b"Z"), byte(b"<"), byte(b"7"), eos, long_tok]
    joined = b"".join(vocab[i] for i in toks)
    want_state, want_rej = G.advance(t, 0, joined)
    s_mid, rej_mid = G.advance(t, 0, b"<4>,Z")
    assert rej_mid == 1 and s_mid == G.advance(t, 0, b"<4>,")[0]
    assert g.advance_tokens(vocab, toks) == want_rej and g.current_state() == want_state
    assert want_rej >= 1 + 1                                  # the long token is not a sentence of this grammar either
    # in pieces, from the current state
    g.reset()
    r1 = g.advance_tokens(vocab, toks[:7])
    assert (g.current_state(), r1) == (s_mid, 1)
    r2 = g.advance_tokens(vocab, toks[7:])
    assert r1 + r2 == want_rej and g.current_state() == want_state
    assert g.advance_tokens(vocab, []) == 0 and g.current_state() == want_state


def test_advance_tokens_refuses_an_id_outside_the_vocabulary_and_leaves_the_state():
    V = 300
    vocab, _ = G.synth_vocab(V, seed=1)
    g = runtime.GrammarDfa(LITERALS)
    g.advance(b"the ")
    s = g.current_state()
    assert s != 0
    for bad in ([vocab.index(b"q"), V], [-1], [vocab.index(b"q"), vocab.index(b"u"), V + 7]):
        with pytest.raises(L.BlazrHipError) as e:
            g.advance_tokens(vocab, bad)
        assert e.value.code == L.E_INVALID and "vocabulary" in str(e.value)
        assert g.current_state() == s
    assert g.advance_tokens(vocab, [vocab.index(b"q"), vocab.index(b"u")]) == 0 and g.current_state() != s
