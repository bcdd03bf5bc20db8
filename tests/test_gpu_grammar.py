"""Device side of grammar-constrained decoding: the mask kernel (k_grammar_mask, blazr_amd/csrc/bz_grammar.hip) against the Python restatement of the reference's
mask_logits (tests/grammar_ref.py; /root/reference/src/engine/grammar.rs:142-158) and against the library's own host checker bz_grammar_token_mask, and
bz_generate_grammar against a decode loop the test drives itself.  Every comparison is exact: masks, token ids, and untouched logits bit for bit."""
import ctypes as C

import numpy as np
import pytest

import grammar_ref as G
from blazr_amd import _lib as L
from blazr_amd import runtime, synth
from test_gpu_llama import _kv_dt

pytestmark = pytest.mark.gpu

LITERALS = 'root ::= "the quick brown fox jumps over the lazy dog" | "pack my box with five dozen liquor jugs" | "{\\"name\\": \\"Ada Lovelace\\", \\"age\\": 36}"'
REGULAR = 'root ::= item ( "," item )*\nitem ::= "<" [0-9] [0-9]? ">" | "\\"" name "\\""\nname ::= ( "Ada" | "item" [-_] [0-9] )+'


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _nasty_logits(rows, V, seed):
    """random logits salted with -inf, +inf, NaNs of several payloads, denormals and signed zeros"""
    rng = np.random.RandomState(seed)
    x = (rng.randn(rows, V) * 4).astype(np.float32)
    u = x.view(np.uint32)
    special = np.array([0xFF800000, 0x7F800000, 0x7FC00000, 0x7FC12345, 0xFFC00001, 0x7F800001, 0x00000001, 0x807FFFFF, 0x80000000, 0x00000000], dtype=np.uint32)
    idx = rng.choice(rows * V, size=min(rows * V // 5, 4000), replace=False)
    u.reshape(-1)[idx] = special[rng.randint(0, len(special), size=len(idx))]
    return x


def _big_table(n, seed=11):
    """a DFA too large for the LDS path: random walks over printable bytes, so that tokens survive several steps"""
    rng = np.random.RandomState(seed)
    t = np.full((n, 256), -1, dtype=np.int32)
    for b in list(range(32, 127)) + [9, 10, 0xC3, 0xA9]:
        keep = rng.rand(n) < 0.7
        t[keep, b] = rng.randint(0, n, size=int(keep.sum()))
    return t, (rng.rand(n) < 0.5).astype(np.uint8)


def _dfa(kind):
    if kind == "one-state":
        return runtime.GrammarDfa('start ::= "no root rule"')
    if kind == "literals":
        return runtime.GrammarDfa(LITERALS)
    if kind == "regular":
        return runtime.GrammarDfa(REGULAR, regular=True)
    t, a = _big_table(L.GRAMMAR_LDS_MAX_STATES + 172)
    return runtime.GrammarDfa(table=t, accepting=a)


def _states_after_tokens(t, vocab, seed, n=3, depth=5):
    """the start state and states reached after several allowed non-empty tokens"""
    rng = np.random.RandomState(seed)
    out = [0]
    for _ in range(n):
        s = 0
        for _ in range(depth):
            ok = [i for i in np.nonzero(G.token_mask(t, s, vocab))[0] if vocab[i]]
            if not ok:
                break
            s, rej = G.advance(t, s, vocab[ok[rng.randint(len(ok))]])
            assert rej == 0
        out.append(s)
    return sorted(set(out))


@pytest.mark.parametrize("V", [1000, 1024, 32000, 128256])
@pytest.mark.parametrize("kind", ["one-state", "literals", "regular", "global-table"])
def test_mask_kernel_equals_restatement_and_host_checker(device, V, kind):
    vocab, eos = G.synth_vocab(V, seed=V + 1)
    packed = runtime.pack_vocab(vocab)
    g = _dfa(kind)
    t, a = g.table()
    dg = g.to_device(device, packed)
    info = dg.info()
    assert info["num_states"] == len(t) and info["vocab"] == V
    # which table path runs is a documented threshold, reported by the handle
    assert info["lds_table"] == (len(t) <= L.GRAMMAR_LDS_MAX_STATES) and info["lds_table"] == (kind != "global-table")
    if kind in ("literals", "regular"):
        assert 24 <= len(t) <= L.GRAMMAR_LDS_MAX_STATES
    states = _states_after_tokens(t, vocab, seed=V) if V <= 32000 else [0, _states_after_tokens(t, vocab, seed=V, n=1)[-1]]
    for k, s in enumerate(states):
        want_mask = G.token_mask(t, s, vocab)
        gs = runtime.GrammarDfa(table=t, accepting=a)          # the host checker, put into state s
        gs.advance(_witness(t, s))
        assert gs.current_state() == s
        assert np.array_equal(gs.compute_token_mask(packed), want_mask), (kind, V, s)
        dg.set_state(s)
        for rows in ((1, 3) if k < 2 else (1,)):
            x = _nasty_logits(rows, V, seed=100 * k + rows)
            want = x.copy()
            want[-1][~want_mask] = -np.inf                      # mask_logits (grammar.rs:142-158): disallowed -> -inf, everything else keeps its bits
            # out of place: the input is untouched, the output is the input with the last row masked
            tin, tout = device.tensor(x), device.tensor(np.full_like(x, 7.0))
            dg.mask_logits(tin, out=tout)
            assert np.array_equal(_bits(tin.to_numpy()), _bits(x))
            got = tout.to_numpy()
            assert np.array_equal(_bits(got), _bits(want)), (kind, V, s, rows, int((_bits(got) != _bits(want)).sum()))
            # in place
            dg.mask_logits(tin)
            assert np.array_equal(_bits(tin.to_numpy()), _bits(want)), (kind, V, s, rows)


def _witness(t, target):
    prev, queue = {0: None}, [0]
    for s in queue:
        if s == target:
            break
        for b in np.nonzero(t[s] >= 0)[0]:
            n = int(t[s, b])
            if n not in prev:
                prev[n] = (s, int(b))
                queue.append(n)
    out, s = [], target
    while prev[s] is not None:
        s, b = prev[s]
        out.append(b)
    return bytes(reversed(out))


def test_mask_argument_checks(device):
    vocab, _ = G.synth_vocab(1000, seed=2)
    g = runtime.GrammarDfa(LITERALS)
    dg = g.to_device(device, vocab)
    x = device.zeros((1, 1024))
    with pytest.raises(L.BlazrHipError) as e:
        dg.mask_logits(x)                       # vocab != the uploaded V
    assert e.value.code == L.E_INVALID
    with pytest.raises(L.BlazrHipError) as e:
        dg.set_state(g.num_states())
    assert e.value.code == L.E_INVALID
    # to_device copies the current state of the host DFA
    g.advance(b"the ")
    assert g.to_device(device, vocab).info()["state"] == g.current_state() != 0


def test_a_state_that_admits_no_token(device):
    """The reference leaves this case undefined.  Here: exactly the empty tokens stay finite; without empty tokens the row is all -inf, bz_argmax_to_buf returns what it
    returns for any all -inf row, and the sampled path returns some id in [0, V) without an error."""
    V = 1000
    vocab, eos = G.synth_vocab(V, seed=9)
    g = runtime.GrammarDfa('root ::= "ok"')
    g.advance(b"ok")                                  # the final state: no transition leaves it
    assert g.is_accepting()
    x = np.random.RandomState(0).randn(1, V).astype(np.float32)
    got = g.to_device(device, vocab).mask_logits(device.tensor(x)).to_numpy()[0]
    empty = np.array([len(t) == 0 for t in vocab])
    assert empty.sum() >= 3 and np.array_equal(np.isfinite(got), empty) and np.array_equal(got[empty], x[0][empty]) and np.isneginf(got[~empty]).all()
    # a vocabulary without empty tokens
    full = [t if t else b"#" for t in vocab]
    tl = g.to_device(device, full).mask_logits(device.tensor(x))
    assert np.isneginf(tl.to_numpy()).all()
    ref = device.tensor(np.full((1, V), -np.inf, dtype=np.float32))
    tok, tok_ref = device.zeros((1,), L.I64), device.zeros((1,), L.I64)
    L.check(L.lib().bz_argmax_to_buf(device.h, tl.h, 1, V, tok.h))
    L.check(L.lib().bz_argmax_to_buf(device.h, ref.h, 1, V, tok_ref.h))
    assert int(tok.to_numpy()[0]) == int(tok_ref.to_numpy()[0])
    sampled = runtime.logits_to_token(device, tl, [], [], temperature=0.8, top_k=40, top_p=0.9, seed=5)
    assert 0 <= int(sampled.to_numpy()[0]) < V


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------------------
CASES = [("tiny-awq", "contiguous"), ("tiny-q4km", "contiguous"), ("tiny-mamba2", "ssm"), ("tiny-awq", "paged")]
_MODELS = {}


def _model(device, preset):
    if preset not in _MODELS:
        model = synth.make_mamba2(preset) if preset in synth.MAMBA_PRESETS else synth.make_llama(preset)
        _MODELS[preset] = (model, runtime.LoadedModel.from_synth(device, model))
    return _MODELS[preset]


class _Stepper:
    """forward passes driven from the test, the way bz_generate drives them: the prompt in one call, then one token at a time"""

    def __init__(self, device, model, lm, branch, n_prompt, n_new, block_size=16):
        cfg = model["config"]
        self.lm, self.branch, self.pos = lm, branch, 0
        if branch == "ssm":
            self.state = runtime.LayeredSsmState(lm)
        elif branch == "paged":
            nblocks = (n_prompt + n_new + block_size - 1) // block_size + 4
            self.pk = runtime.LayeredPagedKvCache(device, cfg["n_layers"], nblocks, block_size, cfg["n_kv_heads"], cfg["head_dim"], _kv_dt(cfg))
            self.pk.set_blocks(list(range(nblocks)))
        else:
            self.kv = lm.new_kv_cache(n_prompt + n_new + 1)

    def forward(self, toks):
        n = len(toks)
        if self.branch == "ssm":
            out = self.lm.forward_with_ssm_state(toks, self.state)
        elif self.branch == "paged":
            sm = self.pk.compute_slot_mapping(self.pos, n)
            self.pk.set_seq_len(self.pos + n)
            out = self.lm.forward_with_paged_kv_cache(toks, self.pk, sm, self.pk.block_table_device_format(), self.pos + n, self.pos)
        else:
            out = self.lm.forward_with_kv_cache(toks, self.kv, self.pos)
        self.pos += n
        return out


def _grammar(which):
    return runtime.GrammarDfa(LITERALS) if which == "literals" else runtime.GrammarDfa(REGULAR, regular=True)


@pytest.mark.parametrize("which", ["literals", "regular"])
@pytest.mark.parametrize("preset,branch", CASES, ids=["%s-%s" % c for c in CASES])
def test_generate_grammar_equals_a_test_driven_loop(device, preset, branch, which):
    model, lm = _model(device, preset)
    V = model["config"]["vocab"]
    vocab, eos = G.synth_vocab(V, seed=21)
    prompt = synth.prompt_tokens(8, V)
    n_new = 16
    g = _grammar(which)
    t, a = g.table()
    live = G.co_accessible(t, a)
    # the loop the test drives: forward -> logits to host -> numpy mask with the restatement -> argmax (lowest index on ties) -> advance
    st = _Stepper(device, model, lm, branch, len(prompt), n_new)
    logits = st.forward(prompt).to_numpy()[0]
    state, want, free_ok, text = 0, [], 0, b""
    for i in range(n_new):
        allowed = G.token_mask(t, state, vocab)
        assert allowed.mean() < 0.05, (i, state, allowed.mean())            # the constraint binds: under 5 % of the vocabulary is admissible
        free_ok += bool(allowed[int(np.argmax(logits))])
        tok = int(np.argmax(G.mask_logits(t, state, vocab, logits)))
        assert allowed[tok]
        want.append(tok)
        state, rej = G.advance(t, state, vocab[tok])
        assert rej == 0
        text += vocab[tok]
        if i + 1 < n_new:
            logits = st.forward([tok]).to_numpy()[0]
    assert free_ok <= n_new // 2, "the unconstrained argmax was admissible at %d of %d steps: the comparison would show little" % (free_ok, n_new)
    # the output is a viable prefix of the language (a model whose best admissible logit is an empty token may legitimately stay where it is)
    assert live[state] and G.advance(t, 0, text) == (state, 0)
    ex = runtime.Executor(lm)
    got = ex.generate(prompt, n_new, paged=branch == "paged", grammar=g, vocab_bytes=vocab)
    assert got.tolist() == want, (preset, branch, which)
    assert g.current_state() == state                                       # g is left in its final state ...
    # ... and used from its current state: a second call continues the same sentence
    more = ex.generate(np.concatenate([prompt, got]), 4, paged=branch == "paged", grammar=g, vocab_bytes=vocab)
    s2, rej = G.advance(t, state, b"".join(vocab[int(k)] for k in more))
    assert rej == 0 and g.current_state() == s2
    # use_graph = 1 with a grammar takes the eager loop
    g.reset()
    assert ex.generate(prompt, n_new, paged=branch == "paged", use_graph=True, grammar=g, vocab_bytes=vocab).tolist() == want
    # without a grammar nothing changes: bz_generate_grammar(g = NULL) is bz_generate
    free = ex.generate(prompt, n_new, paged=branch == "paged")
    out, stt = np.zeros(n_new, dtype=np.int64), L.GenStats()
    gc = L.GenConfig()
    gc.max_tokens, gc.repeat_penalty, gc.repeat_last_n, gc.top_p, gc.eos_id, gc.paged, gc.block_size, gc.dry_base, gc.dynatemp_exponent = n_new, 1.0, 64, 1.0, -1, int(branch == "paged"), 16, 2, 1.0
    p = np.ascontiguousarray(prompt, dtype=np.int64)
    L.check(L.lib().bz_generate_grammar(lm.h, p.ctypes.data, len(p), C.byref(gc), None, None, None, 0, out.ctypes.data, C.byref(stt)))
    assert out[:stt.n_generated].tolist() == free.tolist() != want


@pytest.mark.parametrize("preset,branch", CASES[:3], ids=["%s-%s" % c for c in CASES[:3]])
def test_generate_grammar_sampled_equals_mask_plus_logits_to_token(device, preset, branch):
    model, lm = _model(device, preset)
    V = model["config"]["vocab"]
    vocab, eos = G.synth_vocab(V, seed=21)
    prompt = synth.prompt_tokens(8, V)
    n_new, seed, kw = 16, 77, dict(temperature=0.9, top_k=50, top_p=0.95)
    g = _grammar("regular")
    t, a = g.table()
    dg = g.to_device(device, vocab)
    st = _Stepper(device, model, lm, branch, len(prompt), n_new)
    logits = st.forward(prompt)
    state, want = 0, []
    for i in range(n_new):
        dg.set_state(state)
        dg.mask_logits(logits)
        tok = int(runtime.logits_to_token(device, logits, [], [], seed=seed + i, **kw).to_numpy()[0])
        assert G.token_mask(t, state, vocab)[tok]
        want.append(tok)
        state, rej = G.advance(t, state, vocab[tok])
        assert rej == 0
        if i + 1 < n_new:
            logits = st.forward([tok])
    got = runtime.Executor(lm).generate(prompt, n_new, seed=seed, grammar=g, vocab_bytes=vocab, **kw)
    assert got.tolist() == want and g.current_state() == state


def test_generate_without_grammar_is_unchanged_across_the_existing_configurations(device):
    """the configurations of test_gpu_llama.py's generate tests, through bz_generate and through bz_generate_grammar(g = NULL)"""
    model, lm = _model(device, "tiny-awq")
    V = model["config"]["vocab"]
    p = np.ascontiguousarray(synth.prompt_tokens(12, V, seed=3), dtype=np.int64)
    ex = runtime.Executor(lm)
    for kw in (dict(), dict(use_graph=True), dict(paged=True), dict(paged=True, use_graph=True), dict(temperature=0.8, seed=3), dict(repeat_penalty=1.1),
               dict(temperature=0.7, dry_multiplier=0.8, typical_p=0.9, logit_bias={1: 1.0}, dynatemp_range=0.2), dict(mirostat_mode=2, temperature=0.8, seed=4)):
        a = ex.generate(p, 12, **kw)
        gc = L.GenConfig()
        gc.max_tokens, gc.temperature, gc.repeat_penalty, gc.repeat_last_n, gc.top_p, gc.eos_id, gc.block_size = 12, kw.get("temperature", 0.0), kw.get("repeat_penalty", 1.0), 64, 1.0, -1, 16
        gc.seed, gc.use_graph, gc.paged = kw.get("seed", 0), int(kw.get("use_graph", False)), int(kw.get("paged", False))
        gc.dry_multiplier, gc.dry_base, gc.typical_p, gc.dynatemp_range, gc.dynatemp_exponent = kw.get("dry_multiplier", 0.0), 2, kw.get("typical_p", 0.0), kw.get("dynatemp_range", 0.0), 1.0
        gc.mirostat_mode, gc.mirostat_tau, gc.mirostat_eta = kw.get("mirostat_mode", 0), 5.0, 0.1
        if "logit_bias" in kw:
            ids, vals = np.asarray([1], dtype=np.uint32), np.asarray([1.0], dtype=np.float32)
            gc.n_logit_bias, gc.logit_bias_ids, gc.logit_bias_vals = 1, ids.ctypes.data, vals.ctypes.data
        out, stt = np.zeros(12, dtype=np.int64), L.GenStats()
        L.check(L.lib().bz_generate_grammar(lm.h, p.ctypes.data, len(p), C.byref(gc), None, None, None, 0, out.ctypes.data, C.byref(stt)))
        assert out[:stt.n_generated].tolist() == a.tolist(), kw


def test_generate_grammar_with_host_side_options_and_mirostat(device):
    """DRY / typical before the mask, logit bias after it (sampling.rs:393-429): every token is admissible; Mirostat skips the mask but the DFA still advances"""
    model, lm = _model(device, "tiny-awq")
    V = model["config"]["vocab"]
    vocab, eos = G.synth_vocab(V, seed=21)
    prompt = synth.prompt_tokens(8, V)
    ex = runtime.Executor(lm)
    g = _grammar("regular")
    t, a = g.table()
    got = ex.generate(prompt, 12, temperature=0.8, seed=2, dry_multiplier=0.8, typical_p=0.95, logit_bias={5: 2.0, 40: -1.0}, dynatemp_range=0.2, grammar=g, vocab_bytes=vocab)
    state, rej = G.advance(t, 0, b"".join(vocab[int(k)] for k in got))
    assert len(got) == 12 and rej == 0 and g.current_state() == state
    g.reset()
    free = ex.generate(prompt, 12, temperature=0.8, seed=4, mirostat_mode=2)
    got = ex.generate(prompt, 12, temperature=0.8, seed=4, mirostat_mode=2, grammar=g, vocab_bytes=vocab)
    assert got.tolist() == free.tolist()
    state = 0
    for k in got:
        state, _ = G.advance(t, state, vocab[int(k)])
    assert g.current_state() == state
    with pytest.raises(L.BlazrHipError) as e:
        ex.generate(prompt, 4, grammar=g, vocab_bytes=vocab[:-1])
    assert e.value.code == L.E_INVALID
