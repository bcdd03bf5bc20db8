"""GPU: the pieces of speculative decoding -- the device accept rule (bz_spec_accept) against tests/spec_ref.py, and the verify forward (bz_forward_kv_verify), whose
rows must be the decode step's rows BIT FOR BIT: logits and K/V rows equal those of single-token bz_forward_kv calls, on the multi-row path (f16 int4 models: the
exact prompt rows + the multi-row lm_head, path 1) and on the token-by-token fallback (dense bf16, GGUF: path 0).  Every comparison is equality."""
import numpy as np
import pytest

import spec_ref
from blazr_amd import _lib as L
from blazr_amd import runtime, synth

pytestmark = pytest.mark.gpu

_MODELS = {}


def _model(device, preset, **over):
    key = (preset, tuple(sorted(over.items())))
    if key not in _MODELS:
        model = synth.make_llama(preset, **over)
        _MODELS[key] = (model["config"], runtime.LoadedModel.from_synth(device, model))
    return _MODELS[key]


def _argmax_to_buf(device, t_logits, rows, V):
    out = device.zeros((1,), L.I64)
    L.check(L.lib().bz_argmax_to_buf(device.h, t_logits.h, rows, V, out.h))
    return int(out.to_numpy()[0])


@pytest.mark.parametrize("V", [1024, 1003])
@pytest.mark.parametrize("R", [1, 2, 6, 8, 16])
def test_accept_record_is_the_reference_rule(device, R, V):
    rng = np.random.Generator(np.random.PCG64([R, V]))
    for shift in range(4):                      # every row takes each of the four row kinds once
        lg = rng.standard_normal((R, V)).astype(np.float32)
        for r in range(R):
            kind = (r + shift) % 4
            top = np.float32(lg[r].max() + 1.0)
            if kind == 1:                       # two equal maxima
                lg[r, [V // 3, V // 2]] = top
            elif kind == 2:                     # three, one at index 0 and one at V - 1
                lg[r, [0, V // 2, V - 1]] = top
            elif kind == 3:                     # nothing but -inf
                lg[r, :] = -np.inf
        am = spec_ref.row_argmax(lg)
        t_lg = device.tensor(lg)
        for r in range(R):
            assert _argmax_to_buf(device, t_lg, r + 1, V) == am[r], (r, shift)
        for n in range(R):                      # planted agreement: the draft follows the argmax for n rows, then leaves it
            draft = am[:R - 1].copy()
            if n < R - 1:
                draft[n] = (draft[n] + 1 + n) % V
                draft[n + 1:] = rng.integers(0, V, size=R - 2 - n)
            want = spec_ref.record(lg, draft)
            got = runtime.spec_accept(device, t_lg, draft)
            assert want[0] == n
            assert np.array_equal(got, want), (R, V, shift, n, got, want)


def _check_verify_rows(device, preset, over, expect_path, positions=(0, 5, 250), rows=(1, 2, 3, 7, 8, 9, 16)):
    cfg, lm = _model(device, preset, **over)
    nl, nkv, V = cfg["n_layers"], cfg["n_kv_heads"], cfg["vocab"]
    n_tok = max(positions) + max(rows)
    seq = [int(t) for t in synth.prompt_tokens(n_tok, V, seed=91)]
    kv_a, kv_b = lm.new_kv_cache(n_tok + 8), lm.new_kv_cache(n_tok + 8)
    # the reference, once: one single-token call per position on the second cache
    ref = np.stack([lm.forward_with_kv_cache([t], kv_b, i).to_numpy().reshape(-1) for i, t in enumerate(seq)])
    kvb = {(l, h, w): kv_b.read(l, h, w, n_tok) for l in range(nl) for h in range(nkv) for w in (0, 1)}
    filled = 0
    for P in sorted(positions):
        for i in range(filled, P):              # the same prefix in the first cache
            lm.forward_with_kv_cache([seq[i]], kv_a, i)
        filled = P
        for R in rows:
            n_acc, toks, path, lg = lm.forward_kv_verify(seq[P:P + R], kv_a, P)
            got = lg.to_numpy().reshape(R, -1)
            assert path == expect_path, (preset, P, R, path)
            assert np.array_equal(got, ref[P:P + R]), "%s P=%d R=%d: %d of %d logits differ" % (preset, P, R, int((got != ref[P:P + R]).sum()), got.size)
            for (l, h, w), b in kvb.items():
                a = kv_a.read(l, h, w, P + R)
                assert np.array_equal(a[P:], b[P:P + R]), (preset, P, R, l, h, w)
                assert np.array_equal(a[:P], b[:P]), (preset, P, R, l, h, w, "prefix rows changed")
            # the accept rule on these rows, and where the cache ends
            want = spec_ref.record(ref[P:P + R], seq[P + 1:P + R])
            assert n_acc == want[0] and np.array_equal(toks, want[1:2 + n_acc])
            assert kv_a.seq_len() == P + n_acc + 1


FAST = [("tiny-awq", dict(max_seq_len=512)), ("tiny-gptq", dict(max_seq_len=512)), ("llama3-8b-awq-2l", dict(vocab=4096)), ("llama3-8b-awq-2l", dict(vocab=1003))]


@pytest.mark.parametrize("preset,over", FAST, ids=["tiny-awq", "tiny-gptq", "8b-awq-2l-v4096", "8b-awq-2l-v1003"])
def test_verify_rows_are_the_decode_rows(device, preset, over):
    """P on both sides of the decode attention's 256-row chunk; R = 9 crosses the 8-row pass, R = 16 fills two"""
    _check_verify_rows(device, preset, over, 1)


FALLBACK = [("tiny-bf16", dict(max_seq_len=512), 0), ("tiny-q4km", dict(max_seq_len=512), 0), ("tiny-awq", dict(max_seq_len=512, sliding_window=8), 1)]


@pytest.mark.parametrize("preset,over,path", FALLBACK, ids=["tiny-bf16", "tiny-q4km", "tiny-awq-window8"])
def test_verify_rows_on_the_fallback_and_under_a_window(device, preset, over, path):
    _check_verify_rows(device, preset, over, path)


@pytest.mark.parametrize("preset,over", [("tiny-awq", {}), ("llama3-8b-awq-2l", dict(vocab=4096))], ids=["tiny-awq", "8b-awq-2l"])
def test_acceptance_by_construction(device, preset, over):
    """the verify rows are decode rows, so a draft that follows the plain greedy continuation g for a tokens and then leaves it is accepted for exactly a tokens"""
    cfg, lm = _model(device, preset, **over)
    V, n_p, i = cfg["vocab"], 9, 3
    prompt = [int(t) for t in synth.prompt_tokens(n_p, V, seed=92)]
    g = [int(t) for t in runtime.Executor(lm).generate(prompt, 16, temperature=0.0, repeat_penalty=1.0)]
    assert len(g) == 16
    kv = lm.new_kv_cache(64)
    lm.forward_with_kv_cache(prompt, kv, 0)                       # as bz_generate: the prompt in one call, then token by token
    for j in range(i):
        lm.forward_with_kv_cache([g[j]], kv, n_p + j)
    P = n_p + i
    for k in (5, 7):
        for a in range(k + 1):
            draft = g[i + 1:i + 1 + a] + [(t + 1) % V for t in g[i + 1 + a:i + 1 + k]]
            n_acc, toks, path, _ = lm.forward_kv_verify([g[i]] + draft, kv, P, want_logits=False)
            assert path == 1
            assert n_acc == a, (k, a, n_acc)
            assert toks.tolist() == g[i + 1:i + a + 2]
            assert kv.seq_len() == P + a + 1
            nxt = lm.forward_with_kv_cache([int(toks[-1])], kv, P + a + 1).to_numpy().reshape(-1)
            assert int(np.argmax(nxt)) == g[i + a + 2], (k, a)
