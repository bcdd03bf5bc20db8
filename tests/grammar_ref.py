"""Checker of the grammar feature, shared by test_grammar.py (CPU) and test_gpu_grammar.py (GPU): a Python restatement of the reference's two Rust files
(/root/reference/src/engine/grammar_parser.rs:47-190 parse_gbnf / parse_gbnf_sequence, /root/reference/src/engine/grammar.rs:165-277
compile_grammar_to_dfa, :69-84 compute_token_mask, :142-158 mask_logits) and the seeded synthetic vocabulary both files use.  Nothing here calls the library.

The one deliberate difference from the Rust: its subset construction iterates a HashMap (arbitrary order); this one visits the bytes in ascending order, which is
the canonical numbering the library documents.  Where the Rust never returns (a character its sequence parser does not consume) this raises RefLoops."""
import numpy as np

# char::is_whitespace
_WS = set(chr(c) for c in [9, 10, 11, 12, 13, 32, 0x85, 0xA0, 0x1680, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000] + list(range(0x2000, 0x200B)))


class GbnfError(Exception):
    pass


class RefLoops(Exception):
    """the reference's parser would spin forever on this input"""


def _trim(s):
    b, e = 0, len(s)
    while b < e and s[b] in _WS:
        b += 1
    while e > b and s[e - 1] in _WS:
        e -= 1
    return s[b:e]


def _lines(text):
    parts = text.split("\n")
    if parts and parts[-1] == "":
        parts.pop()
    return [p[:-1] if p.endswith("\r") else p for p in parts]


def parse_gbnf_sequence(s):
    """-> list of ("lit", bytes) | ("class", [(start, end)]) | ("neg", ranges) | ("ref", name, modifier)"""
    out, i, n = [], 0, len(s)
    while i < n:
        c = s[i]
        if c == '"':
            i += 1
            lit = ""
            while i < n:
                ch = s[i]
                if ch == '"':
                    i += 1
                    break
                if ch == "\\":
                    i += 1
                    if i < n:
                        esc = s[i]
                        i += 1
                        lit += {"n": "\n", "t": "\t", '"': '"', "\\": "\\"}.get(esc, "\\" + esc)
                else:
                    lit += ch
                    i += 1
            out.append(("lit", lit.encode("utf-8")))
        elif c == "[":
            i += 1
            neg = i < n and s[i] == "^"
            if neg:
                i += 1
            ranges = []
            while i < n:
                ch = s[i]
                if ch == "]":
                    i += 1
                    break
                start = ord(ch) & 0xFF
                i += 1
                if i < n and s[i] == "-":
                    i += 1
                    if i < n:
                        ranges.append((start, ord(s[i]) & 0xFF))
                        i += 1
                else:
                    ranges.append((start, start))
            out.append(("neg" if neg else "class", ranges))
        elif c in " \t":
            i += 1
        else:
            name = ""
            while i < n and (s[i].isalnum() or s[i] in "-_"):
                name += s[i]
                i += 1
            if not name:
                raise RefLoops("%r at %d" % (c, i))
            mod = ""
            if i < n and s[i] in "*+?":
                mod = s[i]
                i += 1
            out.append(("ref", name, mod))
    return out


def parse_gbnf(text):
    rules = []
    for line in _lines(text):
        line = _trim(line)
        if not line or line.startswith("#"):
            continue
        parts = line.split("::=", 1)
        if len(parts) != 2:
            raise GbnfError("Invalid GBNF rule: " + line)
        name, body = _trim(parts[0]), _trim(parts[1])
        rules.append((name, [parse_gbnf_sequence(_trim(a)) for a in body.split("|")]))
    if not rules:
        raise GbnfError("No rules found in GBNF grammar")
    return rules


def compile_grammar_to_dfa(text):
    """-> (table int32 [n, 256] with -1 = none, accepting uint8 [n])"""
    rules = parse_gbnf(text)
    nfa = [dict()]
    nfa_acc = set()
    root = next((r for r in rules if r[0] == "root"), None)
    if root is not None:
        for alt in root[1]:
            cur = 0
            for el in alt:
                if el[0] == "lit":
                    for b in el[1]:
                        nfa.append(dict())
                        nfa[cur].setdefault(b, []).append(len(nfa) - 1)
                        cur = len(nfa) - 1
                else:
                    nfa.append(dict())
                    nxt = len(nfa) - 1
                    if el[0] == "class":
                        for (s, e) in el[1]:
                            for b in range(s, e + 1):
                                nfa[cur].setdefault(b, []).append(nxt)
                    else:
                        for b in range(128):
                            nfa[cur].setdefault(b, []).append(nxt)
                    cur = nxt
            nfa_acc.add(cur)
    return subset_construction(nfa, nfa_acc)


def subset_construction(nfa, nfa_acc):
    ids = {(0,): 0}
    queue = [(0,)]
    rows, acc = [], []
    q = 0
    while q < len(queue):
        cur = queue[q]
        acc.append(1 if any(s in nfa_acc for s in cur) else 0)
        row = [-1] * 256
        for b in range(256):
            t = set()
            for s in cur:
                t.update(nfa[s].get(b, ()))
            if not t:
                continue
            key = tuple(sorted(t))
            if key not in ids:
                ids[key] = len(queue)
                queue.append(key)
            row[b] = ids[key]
        rows.append(row)
        q += 1
    return np.asarray(rows, dtype=np.int32).reshape(-1, 256), np.asarray(acc, dtype=np.uint8)


# ---- walking a table ---------------------------------------------------------------------------------------------------------------------------------
def advance(table, state, data):
    """GrammarDfa::advance per byte as the generate loop uses it -> (state, rejected bytes)"""
    rej = 0
    for b in data:
        nx = int(table[state, b])
        if nx >= 0:
            state = nx
        else:
            rej += 1
    return state, rej


def token_mask(table, state, vocab):
    """compute_token_mask: vocab = list of bytes -> bool [V]"""
    out = np.zeros(len(vocab), dtype=bool)
    for i, tok in enumerate(vocab):
        s = state
        for b in tok:
            s = int(table[s, b])
            if s < 0:
                break
        out[i] = s >= 0
    return out


def mask_logits(table, state, vocab, logits):
    """mask_logits on a copy: disallowed -> -inf, everything else keeps its bits"""
    out = np.array(logits, dtype=np.float32, copy=True)
    out[~token_mask(table, state, vocab)] = -np.inf
    return out


def co_accessible(table, accepting):
    """states from which an accepting state can be reached"""
    n = len(table)
    live = np.array(accepting, dtype=bool)
    changed = True
    while changed:
        changed = False
        for s in range(n):
            if not live[s]:
                t = table[s]
                if live[t[t >= 0]].any():
                    live[s] = True
                    changed = True
    return live


# ---- the synthetic vocabulary ------------------------------------------------------------------------------------------------------------------------------
CORPUS = (b'{"name": "Ada Lovelace", "age": 36, "tags": ["math", "engine"], "ok": true} yes no maybe the quick brown fox jumps over the lazy dog; '
          b'pack my box with five dozen liquor jugs <12>,<7>,<40> abcabcabc 0123456789 item-1 item_2 "quoted \\" text" \t\n')


def synth_vocab(V, seed=0, corpus=CORPUS):
    """Seeded.  The 256 single bytes, then merges of 2..16 bytes whose length histogram falls off like a BPE vocabulary's (half of them substrings of `corpus`, half
    random bytes; duplicates allowed), a handful of tokens of 64..300 bytes, and at least three empty tokens: the last id (the EOS id) and two more.
    -> (list of bytes, eos_id)"""
    assert V >= 300
    rng = np.random.RandomState(seed)
    toks = [bytes([b]) for b in range(256)]
    n_long = 6
    n_empty = 3
    n_merge = V - 256 - n_long - n_empty
    lens = 2 + np.minimum(rng.geometric(0.3, size=n_merge) - 1, 14)      # 2..16, most mass on 2..6
    for ln in lens:
        if rng.rand() < 0.5:
            o = rng.randint(0, len(corpus) - ln)
            toks.append(corpus[o:o + ln])
        else:
            toks.append(rng.randint(0, 256, size=ln).astype(np.uint8).tobytes())
    for _ in range(n_long):
        ln = rng.randint(64, 301)
        reps = corpus * (ln // len(corpus) + 2)
        o = rng.randint(0, len(corpus))
        toks.append(reps[o:o + ln])
    body = toks[256:]
    order = rng.permutation(len(body))
    toks = toks[:256] + [body[k] for k in order]
    # empty tokens: two inside the merges' id range, one at the end (EOS)
    for pos in sorted(rng.choice(np.arange(256, len(toks)), size=n_empty - 1, replace=False)):
        toks.insert(int(pos), b"")
    toks.append(b"")
    assert len(toks) == V and sum(1 for t in toks if not t) >= 3
    return toks, V - 1
