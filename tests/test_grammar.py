"""Host side of grammar-constrained decoding (blazr_amd/csrc/bz_grammar.hip), checked without a GPU.

Mode 0 (the reference's semantics) is compared table for table with tests/grammar_ref.py, a Python restatement of /root/reference/src/engine/grammar_parser.rs:47-190 and
/root/reference/src/engine/grammar.rs:165-277 under the canonical state numbering (breadth first, ascending byte), plus known answers derived by hand.
BZ_GRAMMAR_REGULAR is compared with hand-written `re` patterns: acceptance of every short string over a small alphabet and of seeded random strings, and prefix viability.
Every comparison is exact."""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import grammar_ref as G
from blazr_amd import _lib as L
from blazr_amd import runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compile_rc(text, flags=0):
    h = C.c_void_p()
    rc = L.lib().bz_grammar_compile(text.encode("utf-8") if isinstance(text, str) else text, flags, C.byref(h))
    msg = L.lib().bz_last_error().decode("utf-8", "replace") if rc != L.OK else ""
    if rc == L.OK:
        L.lib().bz_grammar_free(h)
    return rc, msg


# every branch and quirk of the reference's parser / compiler (grammar_parser.rs:47-190, grammar.rs:165-277)
MODE0 = {
    "two literals sharing a prefix": 'root ::= "yes" | "yet" | "no"',
    "class with ranges and singletons": 'root ::= [a-cxz0-9] "-" [_]',
    "reversed range (no transitions, still a state)": 'root ::= "a" [z-a] "b"',
    "rule reference = one byte of 0..=127": 'root ::= "<" value ">"\nvalue ::= "ignored"',
    "name* name+ name?": 'root ::= item* sep+ tail? "."',
    "negated class = one byte of 0..=127": 'root ::= "\\"" [^"] "\\""',
    "| inside a quoted string still splits": 'root ::= "a|b" | "c"',
    "each escape": 'root ::= "l\\n" "t\\t" "q\\"" "b\\\\" "other\\x41" "end\\',
    "comments and blank lines": '# a comment\n\n   # another\nroot ::= "x"   \n\n',
    "crlf line ends and tabs": 'root ::= "x"\t[ab]\r\nother ::= "y"\r\n',
    "two root rules: only the first": 'root ::= "first"\nroot ::= "second"',
    "no root rule": 'start ::= "abc"',
    "non-ASCII literal": 'root ::= "né€" | "n"',
    "non-ASCII class member (as u8)": 'root ::= [é€a] "!"',
    "class: dangling dash and ] as a range end": 'root ::= [a-] "x" ] "y"',
    "unterminated literal and class": 'root ::= "abc | [xy',
    "empty body and empty alternative": 'root ::= "a" | ',
    "::= inside the body": 'root ::= "a::=b"',
    "unicode blanks trimmed": '\u00a0root\u3000::=\u2003"a"\u00a0',
    "shared prefixes merge in the subset construction": 'root ::= "ab" [c-e] | "ab" "d" "!" | "a" any "z"',
}


@pytest.mark.parametrize("name", sorted(MODE0))
def test_mode0_equals_the_restatement(name):
    text = MODE0[name]
    want_t, want_a = G.compile_grammar_to_dfa(text)
    g = runtime.GrammarDfa(text)
    got_t, got_a = g.table()
    assert g.num_states() == len(want_t), name
    assert np.array_equal(got_a, want_a), name
    assert np.array_equal(got_t, want_t), name
    assert g.current_state() == 0


def test_mode0_errors_carry_the_references_messages():
    rc, msg = _compile_rc('root "a"')
    assert rc == L.E_INVALID and msg == "Invalid GBNF rule: root \"a\""
    with pytest.raises(G.GbnfError, match="Invalid GBNF rule: root \"a\""):
        G.compile_grammar_to_dfa('root "a"')
    for empty in ("", "\n\n", "# only a comment\n   \n"):
        rc, msg = _compile_rc(empty)
        assert rc == L.E_INVALID and msg == "No rules found in GBNF grammar", empty
        with pytest.raises(G.GbnfError, match="No rules found"):
            G.compile_grammar_to_dfa(empty)
    for flags in (0, L.GRAMMAR_REGULAR):
        assert _compile_rc(b'root ::= "\xff"', flags)[0] == L.E_INVALID       # not UTF-8: a Rust &str cannot hold it
    assert _compile_rc('root ::= "a"', 2)[0] == L.E_INVALID                   # unknown flag


def test_known_answers_by_hand():
    # root ::= "yes" | "no": 0 -n-> 1 -o-> 3(acc) ; 0 -y-> 2 -e-> 4 -s-> 5(acc); breadth first with ascending bytes ('n' < 'y') gives exactly these ids
    g = runtime.GrammarDfa('root ::= "yes" | "no"')
    t, a = g.table()
    assert g.num_states() == 6
    assert sorted(np.nonzero(t[0] >= 0)[0].tolist()) == [ord("n"), ord("y")]
    assert (t[0, ord("n")], t[0, ord("y")]) == (1, 2)
    assert (t[1, ord("o")], t[2, ord("e")], t[4, ord("s")]) == (3, 4, 5)
    assert a.tolist() == [0, 0, 0, 1, 0, 1]
    assert int((t >= 0).sum()) == 5
    for word, acc in ((b"yes", True), (b"no", True), (b"ye", False), (b"", False), (b"n", False)):
        g.reset()
        assert g.advance(word) == 0 and g.is_accepting() == acc, word
    # a class is ONE state whatever its width; a rule reference is one byte of 0..=127
    g = runtime.GrammarDfa('root ::= [0-9] digits')
    t, a = g.table()
    assert g.num_states() == 3 and a.tolist() == [0, 0, 1]
    assert np.nonzero(t[0] >= 0)[0].tolist() == list(range(48, 58)) and set(t[0, 48:58].tolist()) == {1}
    assert np.nonzero(t[1] >= 0)[0].tolist() == list(range(128)) and set(t[1, :128].tolist()) == {2}
    assert (t[2] >= 0).sum() == 0
    # no root rule: one state, no transitions, not accepting
    g = runtime.GrammarDfa('start ::= "abc"')
    t, a = g.table()
    assert g.num_states() == 1 and (t >= 0).sum() == 0 and a.tolist() == [0]
    # an empty alternative makes the start state accepting
    g = runtime.GrammarDfa('root ::= "a" | ')
    assert g.is_accepting() and g.num_states() == 2
    # '|' splits inside quotes: "a|b" is the alternatives `"a` and `b"`: literal a ; rule reference b, then an unterminated empty literal
    g = runtime.GrammarDfa('root ::= "a|b"')
    t, a = g.table()
    # NFA: 0 -a-> 1, 0 -(0..=127)-> 2, both accepting; DFA: {0}, {2} (reached first, by byte 0), {1,2} (by 'a')
    assert g.num_states() == 3 and a.tolist() == [0, 1, 1] and np.nonzero(t[0] >= 0)[0].tolist() == list(range(128))
    assert t[0, ord("a")] == 2 and set(np.delete(t[0, :128], ord("a")).tolist()) == {1} and (t[1:] >= 0).sum() == 0


# inputs on which the reference's sequence parser never returns (grammar_parser.rs:153-185): each must come back as BZ_E_UNSUPPORTED, and quickly
LOOPS = ['root ::= "a"*', 'root ::= [0-9]+', 'root ::= ( "a" )', 'root ::= "a" )', 'root ::= "a"?', 'root ::= item*+', 'root ::= a , b', 'root ::= "x"\nother ::= ( "y" )']

_CHILD = r"""
import ctypes as C, sys
sys.path.insert(0, %r)
from blazr_amd import _lib as L
h = C.c_void_p()
rc = L.lib().bz_grammar_compile(sys.argv[1].encode(), int(sys.argv[2]), C.byref(h))
print(rc)
print(L.lib().bz_last_error().decode())
"""


@pytest.mark.parametrize("text", LOOPS)
def test_mode0_inputs_that_loop_forever_in_the_reference_are_unsupported(text):
    with pytest.raises(G.RefLoops):
        G.compile_grammar_to_dfa(text)
    # in a child with a time limit: a parser loop that stops consuming shows as a failure, not as a stuck suite
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT, text, "0"], capture_output=True, text=True, timeout=20)
    assert r.returncode == 0, r.stderr
    rc, msg = r.stdout.split("\n")[:2]
    assert int(rc) == L.E_UNSUPPORTED, (text, r.stdout)
    assert "column" in msg and "line" in msg, msg


def test_mode0_non_ascii_outside_quotes_is_unsupported():
    rc, msg = _compile_rc('root ::= né')
    assert rc == L.E_UNSUPPORTED and "line 1 column 11" in msg       # the name `n` is taken, the é after it is not


# ---- BZ_GRAMMAR_REGULAR ------------------------------------------------------------------------------------------------------------------------------------
JSON_OBJ = 'root ::= "{" ws "\\"name\\"" ws ":" ws string ws "}"\nws ::= [ \t]*\nstring ::= "\\"" [^"]* "\\""\n'      # the class holds a blank and a real tab
REGULAR = [
    # (name, grammar, equivalent bytes pattern, alphabet for the exhaustive part, its max length)
    ("literal alternatives", 'root ::= "yes" | "no" | "yet"', rb"yes|no|yet", b"yesnot", 4),
    ("group with nested alternatives", 'root ::= "a" ( "b" | "c" ( "d" | "e" ) ) "f"', rb"a(b|c(d|e))f", b"abcdef", 5),
    ("postfix on a literal", 'root ::= "ab"* "c"+ "d"?', rb"(ab)*c+d?", b"abcd", 6),
    ("postfix on a class", 'root ::= [0-9]+ [a-b]* [xy]?', rb"[0-9]+[a-b]*[xy]?", b"09abx", 5),
    ("postfix on a group", 'root ::= ( "a" | "bc" )* ( "d" )+ ( "e" "f" )?', rb"(a|bc)*d+(ef)?", b"abcdef", 5),
    ("postfix on a rule reference", 'root ::= item* sep+ tail?\nitem ::= "a" | "b"\nsep ::= ","\ntail ::= "!"', rb"[ab]*,+!?", b"ab,!", 6),
    ("stacked postfix", 'root ::= "a"+? "b"*+', rb"(a+)?(b*)+", b"ab", 6),
    ("negated class", 'root ::= "<" [^<>]* ">"', rb"<[^<>]*>", b"<>a\xc3", 5),
    ("quotes and brackets before |", 'root ::= "a|b" | [|x] "c"', rb"a\|b|[|x]c", b"ab|xc", 4),
    ("rules inlined three deep", 'root ::= l1 "."\nl1 ::= "(" l2 ")" | l2\nl2 ::= l3 l3?\nl3 ::= [ab]', rb"(\([ab][ab]?\)|[ab][ab]?)\.", b"ab().", 6),
    ("flat json object", JSON_OBJ, rb'\{[ \t]*"name"[ \t]*:[ \t]*"[^"]*"[ \t]*\}', b'{}":nae \xe2', 3),
    ("optional group and empty alternative", 'root ::= ( "a" | ) "b" ( | "c" )', rb"a?bc?", b"abc", 4),
    ("escapes", 'root ::= "\\n" "\\t"* "\\\\" "\\""', rb'\n\t*\\"', b'\n\t\\"', 5),
    ("utf-8 literal under a star", 'root ::= "é"* "z"', "(é)*z".encode("utf-8"), "éz".encode("utf-8"), 6),
]
SEEDS = {"flat json object": [b'{"name":"x"}', b'{ "name" : "a b" }', b'{"name":""}', b'{"name":"\xe2\x82\xac"}', b'{"name":"a"b"}', b'{"name" "x"}', b'{"nam":"x"}']}


def _viable_and_accepting(t, a, s):
    """advance() over s from state 0 -> (no byte rejected, accepting at the end)"""
    state, rej = G.advance(t, 0, s)
    return rej == 0, bool(a[state]) and rej == 0


@pytest.mark.parametrize("case", REGULAR, ids=[c[0] for c in REGULAR])
def test_regular_agrees_with_re(case):
    name, text, pattern, alphabet, maxlen = case
    pat = re.compile(pattern, re.S)
    g = runtime.GrammarDfa(text, regular=True)
    t, a = g.table()
    live = G.co_accessible(t, a)
    assert live[1:].all(), "a state that cannot reach an accepting state survived"
    alphabet = sorted(set(alphabet))
    strings = [bytes(s) for n in range(maxlen + 1) for s in itertools.product(alphabet, repeat=n)]
    rng = np.random.RandomState(1234)
    for _ in range(300):
        strings.append(bytes(rng.choice(alphabet, size=rng.randint(1, 14)).tolist()))
    strings += SEEDS.get(name, [])
    assert len(strings) < 20000
    n_acc = 0
    for k, s in enumerate(strings):
        want = pat.fullmatch(s) is not None
        n_acc += want
        if k % 7 == 0 or want:                   # the library's own walk ...
            g.reset()
            rej = g.advance(s)
            assert (rej == 0 and g.is_accepting()) == want, (name, s)
        viable, acc = _viable_and_accepting(t, a, s)            # ... and the walk over the table read back, for every string
        assert acc == want, (name, s)
        # prefix viability: "no byte rejected" == "some accepted string extends this prefix" (decided on the table: the state reached can reach acceptance)
        state, rej = G.advance(t, 0, s)
        if rej == 0:
            assert live[state], (name, s)
        else:
            assert not want
    assert n_acc >= 1, "the case never accepts anything: the comparison would be vacuous"


def test_regular_viability_against_the_accepted_strings():
    """prefix viability without going through the table: over ALL strings up to a length, a prefix is viable iff it is a prefix of an accepted string of that set
    or the language has longer words through it -- for finite languages (no * or +) the two coincide exactly"""
    text, pat, alphabet = 'root ::= "a" ( "b" | "c" ( "d" | "e" ) ) "f" | "ab" [xy]? "g"', re.compile(rb"a(b|c(d|e))f|ab[xy]?g"), b"abcdefgxy"
    g = runtime.GrammarDfa(text, regular=True)
    accepted = [bytes(s) for n in range(5) for s in itertools.product(sorted(alphabet), repeat=n) if pat.fullmatch(bytes(s))]
    assert len(accepted) == 6
    prefixes = {w[:k] for w in accepted for k in range(len(w) + 1)}
    for n in range(5):
        for s in itertools.product(sorted(alphabet), repeat=n):
            s = bytes(s)
            g.reset()
            assert (g.advance(s) == 0) == (s in prefixes), s


@pytest.mark.parametrize("text,what", [
    ('root ::= "a" root | "b"', "recursive"),
    ('root ::= a\na ::= b\nb ::= "x" a?', "recursive"),
    ('root ::= "a" missing', "not defined"),
    ('start ::= "a"', "not defined"),
    ('root ::= ( "a" | "b"', "unbalanced"),
    ('root ::= "a" ) "b"', "unbalanced"),
    ('root ::= ( "a" ) )', "unbalanced"),
    ('root ::= "abc', "unterminated"),
    ('root ::= [é]', "non-ASCII"),
])
def test_regular_refuses_what_is_not_regular_or_not_well_formed(text, what):
    rc, msg = _compile_rc(text, L.GRAMMAR_REGULAR)
    assert rc == L.E_UNSUPPORTED and what in msg, (text, rc, msg)


def test_regular_refuses_more_than_65535_states():
    # (a|b)* a (a|b)^16 needs 2^17 DFA states
    text = 'root ::= [ab]* "a" ' + " ".join(["[ab]"] * 16)
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT, text, str(L.GRAMMAR_REGULAR)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert int(r.stdout.split("\n")[0]) == L.E_UNSUPPORTED and "65535" in r.stdout


def test_regular_a_recursive_rule_that_root_does_not_reach_is_fine():
    g = runtime.GrammarDfa('root ::= "a"\nloop ::= "x" loop', regular=True)
    assert g.num_states() == 2


# ---- advance / from_table / token_mask ------------------------------------------------------------------------------------------------------------------------
def test_advance_over_a_rejected_byte_keeps_the_state_and_goes_on():
    g = runtime.GrammarDfa('root ::= "yes" | "no"')
    assert g.advance(b"yXeZs") == 2 and g.is_accepting() and g.current_state() == 5      # X and Z rejected where they stood, y e s still walked
    assert g.advance(b"more") == 4 and g.current_state() == 5
    g.reset()
    assert g.current_state() == 0 and g.advance(b"") == 0


def test_from_table_round_trips_and_validates():
    rng = np.random.RandomState(3)
    n = 37
    t = rng.randint(-1, n, size=(n, 256)).astype(np.int32)
    a = (rng.rand(n) < 0.3).astype(np.uint8)
    g = runtime.GrammarDfa(table=t, accepting=a)
    t2, a2 = g.table()
    assert g.num_states() == n and np.array_equal(t, t2) and np.array_equal(a, a2)
    s, rej = G.advance(t, 0, b"hello, world")
    assert g.advance(b"hello, world") == rej and g.current_state() == s
    for bad in (n, n + 5, -2):
        tb = t.copy()
        tb[n - 1, 255] = bad
        with pytest.raises(L.BlazrHipError) as e:
            runtime.GrammarDfa(table=tb, accepting=a)
        assert e.value.code == L.E_INVALID
    h = C.c_void_p()
    assert L.lib().bz_grammar_from_table(0, t.ctypes.data, a.ctypes.data, C.byref(h)) == L.E_INVALID
    big = np.full((65536, 256), -1, dtype=np.int32)
    assert L.lib().bz_grammar_from_table(65536, big.ctypes.data, np.zeros(65536, np.uint8).ctypes.data, C.byref(h)) == L.E_UNSUPPORTED


def test_synthetic_vocabulary_is_what_the_issue_describes():
    for V in (1000, 1024, 32000, 128256):
        vocab, eos = G.synth_vocab(V, seed=5)
        assert len(vocab) == V and vocab[eos] == b"" and eos == V - 1
        assert [len(t) for t in vocab[:256]] == [1] * 256 and sorted(t[0] for t in vocab[:256]) == list(range(256))
        lens = np.array([len(t) for t in vocab])
        assert (lens == 0).sum() >= 3 and 4 <= ((lens >= 64) & (lens <= 300)).sum() <= 8
        merges = lens[(lens >= 2) & (lens <= 16)]
        assert len(merges) == V - 256 - 6 - 3 and np.median(merges) <= 5 and merges.max() <= 16
    assert G.synth_vocab(1000, seed=5)[0] == G.synth_vocab(1000, seed=5)[0] != G.synth_vocab(1000, seed=6)[0]


@pytest.mark.parametrize("V", [1000, 1024, 32000])
@pytest.mark.parametrize("text,regular", [('root ::= "{\\"name\\": \\"" [A-Za-z] any "\\", \\"age\\": " [0-9] "}" | "yes" | "no" | "the quick"', False),
                                          ('root ::= item ( "," item )*\nitem ::= "<" [0-9] [0-9]? ">" | "\\"" [^"]* "\\""', True)])
def test_token_mask_equals_the_restatement(V, text, regular):
    vocab, eos = G.synth_vocab(V, seed=V)
    g = runtime.GrammarDfa(text, regular=regular)
    t, a = g.table()
    if not regular:
        assert np.array_equal(t, G.compile_grammar_to_dfa(text)[0])
    packed = runtime.pack_vocab(vocab)
    # the start state and every state reachable within three tokens (breadth first over allowed tokens; bounded per level)
    seen, level = {0}, [0]
    for depth in range(4):
        nxt = []
        for s in level:
            gs = runtime.GrammarDfa(table=t, accepting=a)
            gs.advance(_witness(t, s))
            assert gs.current_state() == s
            got = gs.compute_token_mask(packed)
            want = G.token_mask(t, s, vocab)
            assert np.array_equal(got, want), (V, s)
            assert got[eos] and all(got[i] for i in range(V) if not vocab[i])
            if depth < 3:
                for i in np.nonzero(want)[0][:40]:
                    s2, rej = G.advance(t, s, vocab[i])
                    assert rej == 0
                    if s2 not in seen:
                        seen.add(s2)
                        nxt.append(s2)
        level = nxt[:12]
    assert len(seen) >= 4


def _witness(t, target):
    """a byte string that leads from state 0 to `target` (breadth first over the table)"""
    prev = {0: None}
    queue = [0]
    for s in queue:
        if s == target:
            break
        for b in range(256):
            n = int(t[s, b])
            if n >= 0 and n not in prev:
                prev[n] = (s, b)
                queue.append(n)
    out = []
    s = target
    while prev[s] is not None:
        s, b = prev[s]
        out.append(b)
    return bytes(reversed(out))


def test_token_mask_rejects_bad_vocabularies():
    g = runtime.GrammarDfa('root ::= "a"')
    out = np.zeros(4, np.uint8)
    flat = np.frombuffer(b"abc", dtype=np.uint8)
    for off in ([1, 1, 2, 3, 3], [0, 2, 1, 3, 3]):
        o = np.asarray(off, dtype=np.int64)
        assert L.lib().bz_grammar_token_mask(g.h, flat.ctypes.data, o.ctypes.data, 4, out.ctypes.data) == L.E_INVALID
    o = np.asarray([0, 1, 1, 2, 3], dtype=np.int64)
    assert L.lib().bz_grammar_token_mask(g.h, flat.ctypes.data, o.ctypes.data, 4, out.ctypes.data) == L.OK
    assert out.tolist() == [1, 1, 0, 0]
