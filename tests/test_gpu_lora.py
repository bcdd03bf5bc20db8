"""LoRA adapters in the single-sequence paths on the GPU, against tests/lora_ref.py (npref's numpy forwards with the adapter arithmetic of DESIGN.md
section 4 "LoRA"; the CPU oracle has no adapters).

Bars are the suite's own, as tests/test_gpu_swa.py takes them: relative L2 over the logits at most SPLIT_BARS[act] for 16-bit activations and BAR for f32
ones, no further from the float64 truth than TRUTH_FACTOR times the reference's own distance, batched rows against token-by-token rows at PATH_BAR (f32) or the
16-bit bar.

What makes the first test fail without the feature: the base model's logits are 0.18 .. 0.6 (f16 / bf16 models) and 2.7e-3 .. 0.28 (the f32 model) away from
the adapted reference on every row -- 10x to 27000x the bars (test_lora.py checks this on the references alone; the first test repeats it against the measured
base-model run)."""
import numpy as np
import pytest

from blazr_amd import _lib as L
from blazr_amd import runtime, synth
import lora_cases
import lora_ref
import npref

pytestmark = pytest.mark.gpu

SPLIT_BARS, TRUTH_FACTOR, FLOOR = {"f16": 1.5e-3, "bf16": 2.0 ** -7}, 1.25, 4e-6      # test_gpu_long_context.py
BAR, PATH_BAR = 1e-5, 2e-5                                                              # test_gpu_gguf_legacy.py
CASES = [(k, m) for k in lora_cases.MODELS for m in lora_cases.MASKS]


def _rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _bar(act):
    return BAR if act == "f32" else SPLIT_BARS[act]


def _tbt(lm, toks):
    kv = lm.new_kv_cache(len(toks) + 8)
    return np.stack([lm.forward_with_kv_cache([int(t)], kv, i).to_numpy().reshape(-1) for i, t in enumerate(toks)])


def _dev_adapter(device, ad):
    return runtime.LoraAdapter.from_arrays(device, ad["rank"], ad["alpha"], ad["pairs"], ad["use_rslora"])


def _loaded(device, key, mask, seeds=(1,), **table):
    """the case's model with a table over the mask and one adapter per seed registered as "a<seed>" """
    lm = runtime.LoadedModel.from_synth(device, lora_cases.model(key))
    lm.enable_lora(targets=lora_cases.MASKS[mask], **dict(dict(n_slots=4, max_rank=16), **table))
    for s in seeds:
        lm.load_lora(_dev_adapter(device, lora_cases.adapter(key, mask, s)), "a%d" % s)
    return lm


@pytest.mark.parametrize("key,mask", CASES)
def test_adapter_logits_match_the_reference(device, key, mask):
    act = lora_cases.model(key)["config"]["act_dtype"]
    toks, r = lora_cases.tokens(key), lora_cases.reference(key, mask)
    lm = _loaded(device, key, mask)
    lm.set_lora("a1")
    got = _tbt(lm, toks)
    lm.set_lora(None)
    base = _tbt(lm, toks)
    bar = _bar(act)
    go, gt, ot = _rel(got, r["ref"]), _rel(got, r["truth"]), _rel(r["ref"], r["truth"])
    worst = max(_rel(got[i], r["ref"][i]) for i in range(len(toks)))
    gaps = [_rel(base[i], r["ref"][i]) for i in range(len(toks))]
    print("%s / %s: hip vs ref %.3e (worst row %.3e, bar %.1e); vs truth %.3e, ref vs truth %.3e; base-model gap min %.3e median %.3e"
          % (key, mask, go, worst, bar, gt, ot, min(gaps), float(np.median(gaps))))
    # the test must not pass on the base model: every measured base row is at least 10 bars from the adapted reference, the median row 50
    assert min(gaps) >= 10 * bar and np.median(gaps) >= 50 * bar, (min(gaps), float(np.median(gaps)))
    assert worst <= bar, (worst, bar)
    assert gt <= max(TRUTH_FACTOR * ot, FLOOR), (gt, ot)


@pytest.mark.parametrize("key,mask", CASES)
def test_a_table_without_an_adapter_is_the_base_model(device, key, mask):
    """q,v keeps every fused launch and adds two: a row without an adapter is the model without a table, bit for bit.  All seven targets take attention and
    o_proj as two launches and the split MLP; their sums are the fused kernels' exact sums, so equality is required there as well (measured: 0 on all four
    models, the f32 one included -- tightened from PATH_BAR)"""
    toks = lora_cases.tokens(key)
    plain = _tbt(runtime.LoadedModel.from_synth(device, lora_cases.model(key)), toks)
    lm = _loaded(device, key, mask)
    got = _tbt(lm, toks)                      # nothing selected
    print("%s / %s: table without adapter vs no table %.3e" % (key, mask, _rel(got, plain)))
    assert np.array_equal(got, plain)
    lm.set_lora("a1")
    lm.set_lora(None)
    assert np.array_equal(_tbt(lm, toks), got)


@pytest.mark.parametrize("key,mask", CASES)
def test_prompt_rows_match_token_by_token(device, key, mask):
    """prompts run the rows form: 12 rows (the int4 model's exact rows are the decode step's bits) and 24 rows (the matrix cores) against the decode form"""
    cfg = lora_cases.model(key)["config"]
    act = cfg["act_dtype"]
    toks = [int(t) for t in synth.prompt_tokens(24, cfg["vocab"], seed=31)]
    lm = _loaded(device, key, mask)
    lm.set_lora("a1")
    tbt = _tbt(lm, toks)
    for n in (12, 24):
        kv = lm.new_kv_cache(n + 8)
        rows = lm.forward_with_kv_cache(toks[:n], kv, 0, all_logits=True).to_numpy()
        worst = max(_rel(rows[i], tbt[i]) for i in range(n))
        print("%s / %s: %d prompt rows vs token by token, worst row %.3e" % (key, mask, n, worst))
        assert worst <= (PATH_BAR if act == "f32" else SPLIT_BARS[act]), (n, worst)
        # a decode step on top of the prompt's cache continues the run
        nxt = lm.forward_with_kv_cache([toks[n % 7]], kv, n).to_numpy().reshape(-1)
        kv2 = lm.new_kv_cache(n + 8)
        for i, t in enumerate(toks[:n]):
            lm.forward_with_kv_cache([t], kv2, i)
        want = lm.forward_with_kv_cache([toks[n % 7]], kv2, n).to_numpy().reshape(-1)
        assert _rel(nxt, want) <= (PATH_BAR if act == "f32" else SPLIT_BARS[act])
    # and the base model's rows are far away: the rows form did something
    lm.set_lora(None)
    kv = lm.new_kv_cache(32)
    rows0 = lm.forward_with_kv_cache(toks, kv, 0, all_logits=True).to_numpy()
    assert min(_rel(rows0[i], tbt[i]) for i in range(24)) >= 10 * _bar(act)


def _greedy(lm, prompt, n_new):
    kv = lm.new_kv_cache(len(prompt) + n_new + 8)
    for i, t in enumerate(prompt):
        lg = lm.forward_with_kv_cache([int(t)], kv, i).to_numpy().reshape(-1)
    out = []
    for j in range(n_new):
        out.append(int(np.argmax(lg)))
        lg = lm.forward_with_kv_cache([out[-1]], kv, len(prompt) + j).to_numpy().reshape(-1)
    return out


@pytest.mark.parametrize("key,mask", [("tiny-awq", "qv"), ("tiny-awq", "all"), ("tiny-bf16", "all"), ("tiny-q4km", "qv")])
def test_generate_under_an_adapter(device, key, mask):
    cfg = lora_cases.model(key)["config"]
    lm = _loaded(device, key, mask)
    ex = runtime.Executor(lm)
    prompt, n_new = [int(t) for t in synth.prompt_tokens(6, cfg["vocab"], seed=41)], 10
    lm.set_lora("a1")
    steps = _greedy(lm, prompt, n_new)
    base = ex.generate(prompt, n_new, lora_adapter="a1")
    assert list(base) == steps
    for kw in (dict(use_graph=True), dict(paged=True, block_size=8), dict(paged=True, block_size=8, use_graph=True)):
        assert list(ex.generate(prompt, n_new, lora_adapter="a1", **kw)) == steps, kw
    none = list(ex.generate(prompt, n_new))                                     # the request's choice: no adapter
    lm.set_lora(None)
    assert none == _greedy(lm, prompt, n_new)
    if cfg["act_dtype"] != "f32":               # (the f32 model's greedy run repeats one token with and without the adapter: its logits tests carry the difference)
        assert none != steps
    with pytest.warns(UserWarning, match="not found in registry"):              # executor_generate.rs:54-57
        assert list(ex.generate(prompt, n_new, lora_adapter="nope")) == none


@pytest.mark.parametrize("key,mask", [("tiny-awq", "qv"), ("tiny-awq", "all"), ("tiny-q4km", "all")])
def test_a_captured_graph_follows_set_lora(device, key, mask):
    """one decode graph, captured with nothing selected, replayed under slot 0, then slot 1, then none: each segment continues as the eager run does"""
    cfg = lora_cases.model(key)["config"]
    lm = _loaded(device, key, mask, seeds=(1, 2))
    prompt = [int(t) for t in synth.prompt_tokens(6, cfg["vocab"], seed=42)]
    seg, order = 4, ["a1", "a2", None]

    # eager: the token fed at each step is the previous step's pick
    kv = lm.new_kv_cache(64)
    lm.set_lora(order[0])
    for i, t in enumerate(prompt):
        lg = lm.forward_with_kv_cache([t], kv, i).to_numpy().reshape(-1)
    first = int(np.argmax(lg))
    want, tok, pos = [], first, len(prompt)
    for name in order:
        lm.set_lora(name)
        for _ in range(seg):
            tok = int(np.argmax(lm.forward_with_kv_cache([tok], kv, pos).to_numpy().reshape(-1)))
            want.append(tok)
            pos += 1
    # graph
    lm.set_lora(None)
    kv2 = lm.new_kv_cache(64)
    g = runtime.DecodeGraph(lm, kv2)              # captured before anything is selected
    lm.set_lora(order[0])
    for i, t in enumerate(prompt):
        lm.forward_with_kv_cache([t], kv2, i)
    g.seed_next_token(first, len(prompt))
    got = []
    for name in order:
        lm.set_lora(name)
        for _ in range(seg):
            g.replay()
    got = [g.read_token(i) for i in range(seg * len(order))]
    assert got == want, (got, want)
    # the three segments differ from a run under one setting throughout: the switch mattered
    if cfg["act_dtype"] != "f32":
        lm.set_lora(order[0])
        assert _greedy(lm, prompt, seg * len(order) + 1)[1:] != want


def test_8b_width_qv_keeps_the_fused_launches(device):
    """llama3-8b-awq-2l, mask q,v, r = 16: the step still shows the fused attention + o_proj and the fused MLP, plus two lora launches per layer"""
    model = synth.make_llama("llama3-8b-awq-2l", vocab=2048)
    cfg = model["config"]
    ad = lora_cases.make_adapter(cfg, ("q", "v"), rank=16, alpha=32.0, seed=5)
    lm = runtime.LoadedModel.from_synth(device, model)
    lm.enable_lora(n_slots=2, max_rank=16, targets=("q", "v"))
    lm.load_lora(_dev_adapter(device, ad), "a")
    lm.set_lora("a")
    toks = [int(t) for t in synth.prompt_tokens(3, cfg["vocab"], seed=51)]
    got = _tbt(lm, toks)
    ref = lora_ref.run(lora_ref.LoraLlama(model, ad), toks)
    base = lora_ref.run(npref.NpLlama(model), toks)
    worst, gap = max(_rel(got[i], ref[i]) for i in range(3)), min(_rel(base[i], ref[i]) for i in range(3))
    print("8B width q,v r=16: hip vs ref worst row %.3e (bar %.1e), base-model gap %.3e" % (worst, SPLIT_BARS["f16"], gap))
    assert gap >= 10 * SPLIT_BARS["f16"]
    assert worst <= SPLIT_BARS["f16"]
    kv = lm.new_kv_cache(16)
    recs = {r["name"]: r for r in lm.profile_step(kv, toks[0], 0, iters=1)}
    print(sorted((n, r["launches"]) for n, r in recs.items()))
    assert any(n.startswith("attn+o_proj") for n in recs) and any(n.startswith("mlp_q4g") for n in recs), sorted(recs)
    assert recs["lora_shrink"]["launches"] == cfg["n_layers"] and recs["lora_expand"]["launches"] == cfg["n_layers"]
    assert recs["lora_shrink"]["algo_bytes"] == cfg["n_layers"] * 2 * 16 * cfg["hidden"] * 2        # the adapter bytes read: A of q and v


def test_refusals(device):
    for make, preset in ((synth.make_mamba_config, "tiny-mamba2"), (synth.make_dsv2_config, "tiny-dsv2")):
        other = runtime.LoadedModel.from_synth_streamed(device, make(preset))
        with pytest.raises(L.BlazrHipError) as e:
            other.enable_lora()
        assert e.value.code == L.E_UNSUPPORTED and "Llama family" in str(e.value), str(e.value)
    model = lora_cases.model("tiny-awq")
    cfg = model["config"]
    lm = runtime.LoadedModel.from_synth(device, model)
    with pytest.raises(L.BlazrHipError) as e:
        lm.load_lora(_dev_adapter(device, lora_cases.adapter("tiny-awq", "qv")), "a")            # no table yet
    assert e.value.code == L.E_INVALID
    lm.enable_lora(n_slots=2, max_rank=8, targets=("q", "v"))
    with pytest.raises(L.BlazrHipError) as e:
        lm.enable_lora()                                                                           # a second table
    assert e.value.code == L.E_INVALID
    with pytest.raises(L.BlazrHipError) as e:                                                      # a target outside the mask
        lm.load_lora(_dev_adapter(device, lora_cases.make_adapter(cfg, ("q", "o"))), "a")
    assert e.value.code == L.E_INVALID and "o_proj" in str(e.value) and "outside the table's targets" in str(e.value), str(e.value)
    with pytest.raises(L.BlazrHipError) as e:                                                      # above max_rank
        lm.load_lora(_dev_adapter(device, lora_cases.make_adapter(cfg, ("q",), rank=12)), "a")
    assert e.value.code == L.E_INVALID and "rank 12" in str(e.value) and "max_rank is 8" in str(e.value), str(e.value)
    wide = lora_cases.make_adapter(synth.make_config("tiny-awq", hidden=512), ("q",))             # another model's shapes
    with pytest.raises(L.BlazrHipError) as e:
        lm.load_lora(_dev_adapter(device, wide), "a")
    assert e.value.code == L.E_INVALID and "512 input features" in str(e.value) and "takes 256" in str(e.value), str(e.value)
    assert lm.list_loras() == []
    a = _dev_adapter(device, lora_cases.adapter("tiny-awq", "qv"))
    assert lm.load_lora(a, "a") == 0 and lm.list_loras() == ["a"]
    assert L.lib().bz_lora_free(a.h) == L.E_INVALID                                               # attached
    lm.set_lora("a")
    with pytest.raises(L.BlazrHipError) as e:
        lm.unload_lora("a")                                                                        # the current adapter
    assert e.value.code == L.E_INVALID and "current adapter" in str(e.value)
    lm.set_lora(None)
    assert lm.unload_lora("a") is True and lm.unload_lora("a") is False and lm.list_loras() == []
    # an insert under an existing name replaces it
    lm.load_lora(a, "x")
    lm.load_lora(_dev_adapter(device, lora_cases.adapter("tiny-awq", "qv", 2)), "x")
    assert lm.list_loras() == ["x"]
    # speculative decoding refuses a model with a table
    draft = runtime.LoadedModel.from_synth(device, model)
    with pytest.raises(L.BlazrHipError) as e:
        runtime.SpeculativeExecutor(lm, draft)
    assert e.value.code == L.E_UNSUPPORTED and "LoRA table" in str(e.value)
    with pytest.raises(L.BlazrHipError):
        runtime.SpeculativeExecutor(draft, lm)


def test_load_lora_from_a_peft_directory(device, tmp_path):
    """bz_lora_load end to end: the directory a PEFT save leaves (its real key prefix included) gives the logits of the same adapter built from arrays"""
    key, mask = "tiny-awq", "qv"
    ad = lora_cases.adapter(key, mask)
    d = lora_cases.write_peft_dir(str(tmp_path / "peft"), ad, prefix="base_model.model.")        # base_model.model.model.layers.N...
    toks = lora_cases.tokens(key)[:4]
    lm = _loaded(device, key, mask)
    lm.load_lora(d, "disk")
    lm.set_lora("a1")
    want = _tbt(lm, toks)
    lm.set_lora("disk")
    assert np.array_equal(_tbt(lm, toks), want)
    assert _rel(want, lora_cases.reference(key, mask)["ref"][:4]) <= SPLIT_BARS["f16"]


def test_bz_run_with_lora(device, tmp_path):
    """tools/bz_run.cpp --lora: single-sequence modes run under the first adapter; --requests hands request i adapter i mod (n + 1), 0 = none"""
    import os
    import subprocess
    import ckpt_writer as W
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "blazr_amd", "bz-run")
    assert os.path.exists(exe), "bz-run was not built (python -c 'import __graft_entry__ as g; g.build()')"
    key, mask = "tiny-awq", "qv"
    model = lora_cases.model(key)
    os.makedirs(str(tmp_path / "ckpt"))
    W.write_hf_checkpoint(str(tmp_path / "ckpt"), model)
    dirs = [lora_cases.write_peft_dir(str(tmp_path / ("peft%d" % s)), lora_cases.adapter(key, mask, s)) for s in (1, 2)]
    lm = _loaded(device, key, mask, seeds=(1, 2))
    ex = runtime.Executor(lm)
    p = [int(t) for t in synth.prompt_tokens(9, 1024, seed=31)]
    want = {name: [int(t) for t in ex.generate(p, 12, lora_adapter=name)] for name in (None, "a1", "a2")}
    lora_args = ["--lora", dirs[0], "--lora", dirs[1]]
    for extra in ([], ["--graphs"]):
        r = subprocess.run([exe, str(tmp_path / "ckpt"), "--prompt", ",".join(map(str, p)), "--max-tokens", "12"] + lora_args + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert [int(t) for t in r.stdout.strip().split(",")] == want["a1"], (extra, r.stdout)
    req = tmp_path / "requests.txt"
    req.write_text("".join("12;%s\n" % ",".join(map(str, p)) for _ in range(3)))
    r = subprocess.run([exe, str(tmp_path / "ckpt"), "--requests", str(req), "--rows", "4"] + lora_args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = [[int(t) for t in line.split(",")] for line in r.stdout.strip().splitlines()]
    assert got == [want[None], want["a1"], want["a2"]], got
    r = subprocess.run([exe, str(tmp_path / "ckpt"), "--prompt", "1,2", "--lora", dirs[0], "--lora-targets", "q"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "outside the table's targets" in r.stderr, r.stderr
