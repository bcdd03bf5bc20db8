"""Sliding-window attention on the GPU, against tests/swa_ref.py (npref's numpy forwards with the window mask; the CPU oracle has no window).

Bars are the suite's own.  A windowed run is compared with the rounded numpy reference the way test_gpu_long_context.py compares the split-KV
path with the oracle -- relative L2 over the logits at most SPLIT_BARS[act] for 16-bit activations, and no further from the float64 truth than
TRUTH_FACTOR times the reference's own distance -- and, for f32 activations, at test_gpu_gguf_legacy.py's BAR; batched prompt rows against
token-by-token rows at PATH_BAR.  The numpy reference is not the oracle (f32 matmuls, not the oracle's exact sums), so 16-bit runs get the
bar of the path whose sums are not the oracle's either.  Each comparison is made on the rows at positions >= W stacked into one vector.

What makes the first test fail without the feature: at positions >= W the full-attention logits are 0.14 .. 1.3 (relative L2) away from the
windowed reference in these models (measured on the references alone: npref.NpLlama against swa_ref.SwaLlama), 10x .. 700x the bars.
"""
import os

import numpy as np
import pytest

from blazr_amd import _lib as L
from blazr_amd import runtime, synth
import swa_ref

pytestmark = pytest.mark.gpu

SPLIT_BARS, TRUTH_FACTOR, FLOOR = {"f16": 1.5e-3, "bf16": 2.0 ** -7}, 1.25, 4e-6      # test_gpu_long_context.py
BAR, PATH_BAR = 1e-5, 2e-5                                                              # test_gpu_gguf_legacy.py
_DT = {"f16": L.F16, "bf16": L.BF16, "f32": L.F32}

MODELS = {
    "awq-w8": ("tiny-awq", dict(sliding_window=8), 56),                                 # f16 int4, head_dim 64
    "bf16-w16": ("tiny-bf16", dict(sliding_window=16), 56),                             # bf16 dense
    "q4km-w24": ("tiny-q4km", dict(n_layers=2, sliding_window=24), 56),                 # GGUF blocks, f32 activations and cache
    "awq-hd128-w24": ("tiny-awq", dict(head_dim=128, sliding_window=24, max_seq_len=512), 300),          # head_dim 128: the window passes the first 256-position chunk
    "q4km-hd128-w24": ("tiny-q4km", dict(n_layers=2, head_dim=128, sliding_window=24, max_seq_len=512), 300),
    "awq-w8-pattern2": ("tiny-awq", dict(sliding_window=8, sliding_window_pattern=2), 56),   # Gemma2 style: layer 0 windowed, layer 1 global
}


def _rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _bar(act):
    return BAR if act == "f32" else SPLIT_BARS[act]


def _pair(device, key):
    """(windowed model dict, its LoadedModel, the same weights loaded with W = 0, context)"""
    preset, over, ctx = MODELS[key]
    model = synth.make_llama(preset, **over)
    plain = dict(model, config={k: v for k, v in model["config"].items() if not k.startswith("sliding_window")})
    return model, runtime.LoadedModel.from_synth(device, model), runtime.LoadedModel.from_synth(device, plain), ctx


def _tbt(lm, toks):
    kv = lm.new_kv_cache(len(toks) + 8)
    return np.stack([lm.forward_with_kv_cache([int(t)], kv, i).to_numpy().reshape(-1) for i, t in enumerate(toks)])


@pytest.mark.watchdog(600)
@pytest.mark.parametrize("key", list(MODELS))
def test_window_logits_match_the_reference(device, key):
    model, lm, lm0, ctx = _pair(device, key)
    cfg = model["config"]
    W, act = cfg["sliding_window"], cfg["act_dtype"]
    assert lm.c.sliding_window == W
    toks = synth.prompt_tokens(ctx, cfg["vocab"], seed=11)
    got, full = _tbt(lm, toks), _tbt(lm0, toks)
    ref, truth = swa_ref.run(swa_ref.SwaLlama(model), toks), swa_ref.run(swa_ref.SwaTruth(model), toks)
    bar = _bar(act)
    go, gt, ot = _rel(got[W:], ref[W:]), _rel(got[W:], truth[W:]), _rel(ref[W:], truth[W:])
    gaps = [_rel(full[i], ref[i]) for i in range(W, ctx)]
    print("%s: hip vs ref %.3e (bar %.1e); vs truth %.3e, ref vs truth %.3e; full-attention gap min %.3e median %.3e"
          % (key, go, bar, gt, ot, min(gaps), float(np.median(gaps))))
    # positions < W see every key: the same bits as the same weights without a window
    assert np.array_equal(got[:W], full[:W])
    # the test must not pass on full attention: every row past the window is at least 10 bars from the windowed reference, the median row 50
    assert min(gaps) >= 10 * bar and np.median(gaps) >= 50 * bar, (min(gaps), np.median(gaps))
    assert go <= bar, (go, bar)
    assert gt <= max(TRUTH_FACTOR * ot, FLOOR), (gt, ot)


@pytest.mark.watchdog(600)
@pytest.mark.parametrize("key", ["awq-w8", "bf16-w16", "q4km-w24"])
def test_paths_agree_under_a_window(device, key):
    model, lm, _, _ = _pair(device, key)
    cfg = model["config"]
    W, act, nkv, hd = cfg["sliding_window"], cfg["act_dtype"], cfg["n_kv_heads"], cfg["head_dim"]
    ctx = 48
    toks = [int(t) for t in synth.prompt_tokens(ctx, cfg["vocab"], seed=12)]
    tbt = _tbt(lm, toks)
    # ---- prompt rows.  16 rows of the int4 model are the exact rows (bit-identical to the decode step, as without a window); longer prompts and the
    # other models take the matrix cores: f32 models at PATH_BAR, 16-bit ones at the 16-bit logit bar
    kv = lm.new_kv_cache(ctx + 8)
    if key == "awq-w8":
        rows = lm.forward_with_kv_cache(toks[:16], kv, 0, all_logits=True).to_numpy()
        assert np.array_equal(rows, tbt[:16])
        kv = lm.new_kv_cache(ctx + 8)
    rows = lm.forward_with_kv_cache(toks, kv, 0, all_logits=True).to_numpy()
    worst = max(_rel(rows[i], tbt[i]) for i in range(ctx))
    print("%s: prompt rows vs token-by-token, worst row %.3e" % (key, worst))
    assert worst <= (PATH_BAR if act == "f32" else SPLIT_BARS[act]), worst
    # a decode step on top of the prompt's cache continues the token-by-token run
    nxt = lm.forward_with_kv_cache([toks[0]], kv, ctx).to_numpy().reshape(-1)
    kv2 = lm.new_kv_cache(ctx + 8)
    for i, t in enumerate(toks):
        lm.forward_with_kv_cache([t], kv2, i)
    want = lm.forward_with_kv_cache([toks[0]], kv2, ctx).to_numpy().reshape(-1)
    assert _rel(nxt, want) <= (PATH_BAR if act == "f32" else SPLIT_BARS[act])
    # ---- paged cache, blocks out of order: the decode kernels' sums do not depend on where a row lives
    bs, nb = 8, (ctx + 7) // 8 + 2
    cache = runtime.LayeredPagedKvCache(device, cfg["n_layers"], nb + 4, bs, nkv, hd, _DT[act])
    cache.set_blocks(list(np.random.default_rng(5).permutation(nb + 4)[:nb].astype(int)))
    bt = cache.block_table_device_format()
    paged = np.stack([lm.forward_with_paged_kv_cache([t], cache, cache.compute_slot_mapping(i, 1), bt, i + 1, i).to_numpy().reshape(-1) for i, t in enumerate(toks)])
    if act == "f32":
        assert max(_rel(paged[i], tbt[i]) for i in range(ctx)) <= BAR
    else:
        assert np.array_equal(paged, tbt)
    # ---- pieces: embed -> layers -> head is forward_kv
    kv3 = lm.new_kv_cache(ctx + 8)
    for i, t in enumerate(toks[:W + 6]):
        h = lm.forward_embed([t])
        h, pm = lm.forward_layers_range(h, None, kv3, 0, cfg["n_layers"], i)
        assert np.array_equal(lm.forward_head(h, pm).to_numpy().reshape(-1), tbt[i]), i
    # ---- a decode batch of three sequences whose lengths straddle the window: each row against its own token-by-token step
    lens = [W - 3, W + 1, ctx - 1]
    caches_bt, slots = [], []
    cache2 = runtime.LayeredPagedKvCache(device, cfg["n_layers"], 3 * nb, bs, nkv, hd, _DT[act])
    for s, n in enumerate(lens):
        blocks = list(range(s * nb, (s + 1) * nb))[::-1]
        cache2.set_blocks(blocks)
        if n > 1:
            for i, t in enumerate(toks[:n - 1]):
                lm.forward_with_paged_kv_cache([t], cache2, cache2.compute_slot_mapping(i, 1), blocks, i + 1, i)
        caches_bt.append(blocks)
        slots.append(cache2.compute_slot_mapping(n - 1, 1)[0])
    out = lm.forward_paged_batch([toks[n - 1] for n in lens], cache2, slots, caches_bt, lens).to_numpy()
    for s, n in enumerate(lens):
        r = _rel(out[s], tbt[n - 1])
        print("%s: batch row of length %d vs its own step %.3e" % (key, n, r))
        assert r <= (PATH_BAR if act == "f32" else SPLIT_BARS[act]), (n, r)
    # ---- generate: eager, graph, paged and paged graph produce the greedy tokens of the token-by-token logits
    prompt, n_new = toks[:W + 4], 12
    ex = runtime.Executor(lm)
    base = ex.generate(prompt, n_new)
    kv4 = lm.new_kv_cache(len(prompt) + n_new + 8)
    for i, t in enumerate(prompt):
        lg = lm.forward_with_kv_cache([t], kv4, i).to_numpy().reshape(-1)
    steps = []
    for j in range(n_new):
        steps.append(int(np.argmax(lg)))
        lg = lm.forward_with_kv_cache([steps[-1]], kv4, len(prompt) + j).to_numpy().reshape(-1)
    assert list(base) == steps
    for kw in (dict(use_graph=True), dict(paged=True, block_size=8), dict(paged=True, block_size=8, use_graph=True)):
        assert list(ex.generate(prompt, n_new, **kw)) == list(base), kw


@pytest.mark.watchdog(600)
def test_split_kv_under_a_window(device, monkeypatch):
    """BZ_SPLIT_MIN is read per call: at 16, a window of 24 keys keeps a 60-position context on the split-KV pair (slices over [lo, len)), a window
    of 8 sends it back to the single-pass kernel, and the same weights without a window split as they always did"""
    monkeypatch.setenv("BZ_SPLIT_MIN", "16")
    ctx = 60
    out = {}
    for W in (24, 8, 0):
        over = dict(head_dim=128, sliding_window=W) if W else dict(head_dim=128)
        model = synth.make_llama("tiny-awq", **over)
        lm = runtime.LoadedModel.from_synth(device, model)
        toks = synth.prompt_tokens(ctx, model["config"]["vocab"], seed=13)
        kv = lm.new_kv_cache(ctx + 8)
        got = np.stack([lm.forward_with_kv_cache([int(t)], kv, i).to_numpy().reshape(-1) for i, t in enumerate(toks)])
        labels = {r["name"] for r in lm.profile_step(kv, int(toks[0]), ctx, iters=1)}
        out[W] = labels
        if W:
            ref = swa_ref.run(swa_ref.SwaLlama(model), toks)
            go = _rel(got[W:], ref[W:])
            print("split-KV W=%d: labels %s; hip vs ref %.3e" % (W, sorted(l for l in labels if "attn" in l), go))
            assert go <= SPLIT_BARS["f16"], (W, go)
    assert any(l.startswith("attn_split") for l in out[24]) and any(l.startswith("attn_merge") for l in out[24]), out[24]
    assert not any(l.startswith("attn_split") for l in out[8]), out[8]
    assert any(l.startswith("attn_split") for l in out[0]), out[0]


@pytest.mark.parametrize("act", ["f16", "f32"])
@pytest.mark.parametrize("length", [5, 24, 25, 70, 300])
def test_attn_decode_op_under_a_window(device, act, length):
    """bz_attn_decode / bz_paged_attn_decode of a windowed layer against a float64 softmax over the last W rows"""
    W = 24
    preset, over = ("tiny-awq", dict()) if act == "f16" else ("tiny-q4km", dict(n_layers=2))
    model = synth.make_llama(preset, sliding_window=W, sliding_window_pattern=2, max_seq_len=512, **over)      # layer 0 windowed, layer 1 global
    lm = runtime.LoadedModel.from_synth(device, model)
    cfg = model["config"]
    nq, nkv, hd = cfg["n_heads"], cfg["n_kv_heads"], cfg["head_dim"]
    rng = np.random.default_rng(length)
    R = (lambda x: x.astype(np.float16).astype(np.float32)) if act == "f16" else (lambda x: x)
    K, V = R(rng.standard_normal((length, nkv, hd)).astype(np.float32)), R(rng.standard_normal((length, nkv, hd)).astype(np.float32))
    q = R(rng.standard_normal((nq, hd)).astype(np.float32))
    kv = runtime.LayeredKvCache(device, cfg["n_layers"], 1, nkv, 8, cfg["max_seq_len"], hd, _DT[act])
    for layer in (0, 1):
        for p in range(length):
            tk, tv = device.tensor(K[p]), device.tensor(V[p])
            L.check(L.lib().bz_kv_insert(lm.h, kv.h, layer, p, tk.h, tv.h))
    tq = device.tensor(q)
    for layer, w in ((0, W), (1, 0)):
        out = device.zeros((nq, hd))
        L.check(L.lib().bz_attn_decode(lm.h, tq.h, kv.h, layer, length, out.h))
        want = swa_ref.attn_decode(q, K, V, w)
        tol = (2 ** -9 if act == "f16" else 2 ** -20) * max(np.abs(want).max(), 1e-3)        # test_gpu_ops.py's f16 bar; f32: a few ulps of the largest output
        assert np.abs(out.to_numpy() - want).max() <= tol, (layer, float(np.abs(out.to_numpy() - want).max()), tol)
        if w and length > w:
            assert np.abs(swa_ref.attn_decode(q, K, V, 0) - want).max() > 20 * tol      # the full-attention answer is far outside the tolerance


def test_window_refused_outside_the_llama_family(device):
    for make, preset in ((synth.make_mamba_config, "tiny-mamba2"), (synth.make_dsv2_config, "tiny-dsv2")):
        cfg = dict(make(preset), sliding_window=16)
        with pytest.raises(L.BlazrHipError) as e:
            runtime.LoadedModel(device, cfg)
        assert e.value.code == L.E_UNSUPPORTED and "sliding_window" in str(e.value), str(e.value)
        runtime.LoadedModel(device, make(preset))       # the same config without a window is accepted
