"""GPU: bz_generate_speculative.  Greedy speculative decoding must emit exactly the tokens plain greedy bz_generate emits, whatever the draft proposes (its verify rows
are the decode step's rows); the statistics must add up; what is not built is refused with the cause in bz_last_error()."""
import numpy as np
import pytest

from blazr_amd import _lib as L
from blazr_amd import runtime, synth

pytestmark = pytest.mark.gpu

N_PROMPT, N_GEN = 9, 48
_MODELS = {}


def _model(device, preset, maker=synth.make_llama, **over):
    key = (preset, tuple(sorted(over.items())))
    if key not in _MODELS:
        model = maker(preset, **over)
        _MODELS[key] = (model["config"], runtime.LoadedModel.from_synth(device, model))
    return _MODELS[key]


def _prompt(V):
    return [int(t) for t in synth.prompt_tokens(N_PROMPT, V, seed=93)]


def _plain(lm, prompt, n, **kw):
    ex = runtime.Executor(lm)
    out = ex.generate(prompt, n, temperature=0.0, repeat_penalty=1.0, **kw)
    return [int(t) for t in out], ex.last_stats


def _full_accept_iterations(n_gen, k, adaptive):
    """iterations of a run in which every proposal is accepted: k clipped so that no more than n_gen tokens are emitted"""
    n, it = 1, 0
    while n < n_gen:
        ke = min(k, n_gen - n - 1)
        n += ke + 1
        it += 1
        if adaptive and ke > 0:
            k = min(k + 1, 15)
    return it


TARGETS = {"tiny-awq": ("tiny-awq", {}), "8b-awq-2l": ("llama3-8b-awq-2l", dict(vocab=4096))}


def _draft(device, target_key, kind):
    V = 1024 if target_key == "tiny-awq" else 4096
    if kind == "self":                      # the target's own weights: a second handle for the tiny model, the target's handle itself for the wide one
        if target_key == "tiny-awq":
            return _model(device, "tiny-awq", seed=synth.BASE_SEED)[1]
        return _model(device, *TARGETS[target_key][:1], **TARGETS[target_key][1])[1]
    if kind == "other-seed":
        return _model(device, "tiny-awq", seed=0x5EED, vocab=V)[1]
    return _model(device, "tiny-bf16", vocab=V)[1]


@pytest.mark.parametrize("kind", ["self", "other-seed", "bf16"])
@pytest.mark.parametrize("target_key", ["tiny-awq", "8b-awq-2l"])
def test_greedy_speculative_equals_plain_greedy(device, target_key, kind):
    preset, over = TARGETS[target_key]
    cfg, lm = _model(device, preset, **over)
    draft = _draft(device, target_key, kind)
    prompt = _prompt(cfg["vocab"])
    want, _ = _plain(lm, prompt, N_GEN)
    assert len(want) == N_GEN
    for k in (1, 5, 7, 12):
        for adaptive in (False, True):
            sx = runtime.SpeculativeExecutor(lm, draft, num_speculative_tokens=k, adaptive_depth=adaptive)
            got = [int(t) for t in sx.generate(prompt, N_GEN)]
            ss, st = sx.last_spec_stats, sx.last_stats
            assert got == want, (target_key, kind, k, adaptive, ss)
            assert ss["verify_path"] == 1
            assert ss["accepted_tokens"] + ss["rejected_tokens"] == ss["drafted_tokens"]
            assert st["n_generated"] == N_GEN == 1 + ss["accepted_tokens"] + ss["iterations"]
            assert 1 <= ss["final_depth"] <= 15 and (adaptive or ss["final_depth"] == k)
            # the timings the plain loop reports (test_gpu_llama.py: test_generate_reports_the_reference_bench_timings), from the same stats function; the tokens one
            # iteration accepts share an arrival time, so an inter-token latency may be 0 here
            assert 0.0 < st["ttft_ms"] <= st["total_ms"]
            assert st["prefill_ms"] <= st["ttft_ms"] + 1e-6
            assert 0.0 <= st["itl_p50_ms"] <= st["itl_p99_ms"] <= st["itl_max_ms"]
            assert abs(st["decode_tok_per_s"] - (st["n_generated"] - 1) / ((st["total_ms"] - st["ttft_ms"]) / 1e3)) <= 1e-6 * st["decode_tok_per_s"]
            if kind == "self":                  # every proposal accepted: the two-token catch-up every iteration
                assert ss["rejected_tokens"] == 0
                assert ss["iterations"] == _full_accept_iterations(N_GEN, k, adaptive), (k, adaptive, ss)
            print("%s draft=%s k=%d adaptive=%d: %s" % (target_key, kind, k, adaptive, ss))


def test_dense_target_takes_the_fallback_and_still_equals_plain_greedy(device):
    cfg, lm = _model(device, "tiny-bf16")
    draft = _model(device, "tiny-bf16", seed=0x5EED)[1]
    prompt = _prompt(cfg["vocab"])
    want, _ = _plain(lm, prompt, N_GEN)
    for d in (lm, draft):
        sx = runtime.SpeculativeExecutor(lm, d, num_speculative_tokens=5)
        assert [int(t) for t in sx.generate(prompt, N_GEN)] == want
        assert sx.last_spec_stats["verify_path"] == 0
        assert sx.last_spec_stats["accepted_tokens"] + sx.last_spec_stats["rejected_tokens"] == sx.last_spec_stats["drafted_tokens"]


def test_stats_eos_max_tokens_and_the_end_of_the_context(device):
    cfg, lm = _model(device, "tiny-awq")
    other = _model(device, "tiny-awq", seed=0x5EED)[1]
    prompt = _prompt(cfg["vocab"])
    g, _ = _plain(lm, prompt, N_GEN)
    k = 5
    # EOS in the middle of an iteration (self-draft, k = 5: iterations emit g[1..6], g[7..12], ...): a token whose first occurrence is inside one
    mid = [i for i in range(2, N_GEN) if g[i] not in g[:i] and 1 <= (i - 1) % (k + 1) <= k - 1]
    assert mid, "no first occurrence strictly inside an iteration in %s" % g
    j = mid[-1]
    for d in (lm, other):
        sx = runtime.SpeculativeExecutor(lm, d, num_speculative_tokens=k)
        got = [int(t) for t in sx.generate(prompt, N_GEN, eos_id=g[j])]
        want, wst = _plain(lm, prompt, N_GEN, eos_id=g[j])
        assert want == g[:j + 1] and wst["finish_reason"] == 1
        assert got == want and sx.last_stats["finish_reason"] == 1 and sx.last_stats["n_generated"] == j + 1
        ss = sx.last_spec_stats
        assert ss["accepted_tokens"] + ss["rejected_tokens"] == ss["drafted_tokens"]
        assert j + 1 <= 1 + ss["accepted_tokens"] + ss["iterations"] <= j + 1 + k      # what the EOS clip removed: at most the rest of the last iteration
    for mt in (1, 2, k + 1, k + 2):
        for d in (lm, other):
            sx = runtime.SpeculativeExecutor(lm, d, num_speculative_tokens=k)
            got = [int(t) for t in sx.generate(prompt, mt)]
            ss = sx.last_spec_stats
            assert got == g[:mt] and sx.last_stats["finish_reason"] == 0 and sx.last_stats["n_generated"] == mt
            assert mt == 1 + ss["accepted_tokens"] + ss["iterations"] if mt > 1 else ss["iterations"] == 0
            assert ss["accepted_tokens"] + ss["rejected_tokens"] == ss["drafted_tokens"]
    # a run that ends exactly at max_seq_len (both models): 20 tokens fit behind the 9-token prompt
    cfg2, lm2 = _model(device, "tiny-awq", max_seq_len=N_PROMPT + 20)
    want, wst = _plain(lm2, prompt, 40)
    assert len(want) == 20 and want == g[:20]
    for kk in (5, 12):
        sx = runtime.SpeculativeExecutor(lm2, lm2, num_speculative_tokens=kk)
        got = [int(t) for t in sx.generate(prompt, 40)]
        assert got == want and sx.last_stats["finish_reason"] == 0 and sx.last_spec_stats["rejected_tokens"] == 0


def _refused(code, needle, fn):
    with pytest.raises(L.BlazrHipError) as e:
        fn()
    assert e.value.code == code, str(e.value)
    assert needle in str(e.value), str(e.value)


def test_refusals_name_their_cause(device):
    cfg, lm = _model(device, "tiny-awq")
    prompt = _prompt(cfg["vocab"])
    sx = runtime.SpeculativeExecutor(lm, lm)
    _refused(L.E_UNSUPPORTED, "temperature", lambda: sx.generate(prompt, 8, temperature=0.7))
    _refused(L.E_UNSUPPORTED, "repeat_penalty", lambda: sx.generate(prompt, 8, repeat_penalty=1.1))
    _refused(L.E_UNSUPPORTED, "paged", lambda: sx.generate(prompt, 8, paged=True))
    _refused(L.E_UNSUPPORTED, "DRY", lambda: sx.generate(prompt, 8, dry_multiplier=0.5))
    mamba = _model(device, "tiny-mamba2", maker=synth.make_mamba2)[1]
    dsv2 = _model(device, "tiny-dsv2", maker=synth.make_dsv2)[1]
    _refused(L.E_UNSUPPORTED, "Mamba2", lambda: runtime.SpeculativeExecutor(mamba, lm))
    _refused(L.E_UNSUPPORTED, "Mamba2", lambda: runtime.SpeculativeExecutor(lm, mamba))
    _refused(L.E_UNSUPPORTED, "DeepSeek-V2", lambda: runtime.SpeculativeExecutor(dsv2, lm))
    _refused(L.E_UNSUPPORTED, "DeepSeek-V2", lambda: runtime.SpeculativeExecutor(lm, dsv2))
    small = _model(device, "tiny-awq", vocab=1003)[1]
    _refused(L.E_INVALID, "vocabularies differ", lambda: runtime.SpeculativeExecutor(lm, small))
    _refused(L.E_INVALID, "num_speculative_tokens = 16", lambda: runtime.SpeculativeExecutor(lm, lm, num_speculative_tokens=16))
