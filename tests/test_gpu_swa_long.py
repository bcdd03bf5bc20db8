"""Sliding-window attention at the sizes where the window leaves the first tile / chunk / slice: several split-KV slices laid over [lo, len) with lo
off the slice grid, the single-pass kernels walking several 256-position chunks from the chunk that holds lo, prompts of hundreds of rows (from
position 0 and on top of a cache) through the MFMA and the scalar prompt kernels, a prompt longer than the scalar kernel's score buffer allowed
before, and the decode graphs (single sequence: eager == graph bit for bit across the split threshold; batched: sequences crossing W on the device).

Bars: windowed logits against the rounded numpy reference at test_gpu_long_context.py's SPLIT_BARS, as in test_gpu_swa.py.  16-bit prompt rows
against token-by-token rows: the suite's bar for that comparison is test_gpu_llama.py's _check_logits (relative L2 REL x 2 for the tiny fixtures:
2e-3 f16, 2^-6 bf16); these tests hold the rows to the tighter 1.5e-3 / 2^-7.  f32 rows: test_gpu_gguf_legacy.py's PATH_BAR.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from blazr_amd import runtime, synth
import swa_ref
from test_gpu_swa import SPLIT_BARS, PATH_BAR, _DT, _rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain(model):
    return dict(model, config={k: v for k, v in model["config"].items() if not k.startswith("sliding_window")})


def _tbt(lm, toks, kv=None, pos0=0):
    kv = kv or lm.new_kv_cache(pos0 + len(toks) + 8)
    return np.stack([lm.forward_with_kv_cache([int(t)], kv, pos0 + i).to_numpy().reshape(-1) for i, t in enumerate(toks)])


# ---- decode: several slices / several chunks ----------------------------------------------------------------------------------------------------
@pytest.mark.watchdog(900)
@pytest.mark.parametrize("preset", ["tiny-awq", "tiny-bf16"])          # int4: merge fused with o_proj; dense: the plain merge
@pytest.mark.parametrize("split_min", [256, 1 << 20])                   # split-KV pair / single-pass kernel forced
def test_window_over_several_slices_and_chunks(device, monkeypatch, preset, split_min):
    """W = 300 at contexts up to 800: the window spans three 128-position slices (or two 256-position chunks) whose first position is not on
    the slice / chunk grid, and moves with every step"""
    monkeypatch.setenv("BZ_SPLIT_MIN", str(split_min))                   # read per call
    W, ctx = 300, 800
    model = synth.make_llama(preset, head_dim=128, sliding_window=W, max_seq_len=1024)
    cfg = model["config"]
    act = cfg["act_dtype"]
    lm, lm0 = runtime.LoadedModel.from_synth(device, model), runtime.LoadedModel.from_synth(device, _plain(model))
    toks = synth.prompt_tokens(ctx, cfg["vocab"], seed=21)
    kv = lm.new_kv_cache(ctx + 8)
    got = _tbt(lm, toks, kv)
    labels = {r["name"] for r in lm.profile_step(kv, int(toks[0]), ctx, iters=1)}
    if split_min == 256:
        assert any(l.startswith("attn_split") for l in labels) and any(l.startswith("attn_merge") for l in labels), labels
    else:
        assert not any(l.startswith("attn_split") for l in labels), labels
    ref = swa_ref.run(swa_ref.SwaLlama(model), toks)
    full = _tbt(lm0, toks[:W + 200])
    go = _rel(got[W:], ref[W:])
    gaps = [_rel(full[i], ref[i]) for i in range(W + 100, W + 200)]
    print("%s split_min %d: labels %s; hip vs ref %.3e (bar %.1e); full-attention gap min %.3e" % (preset, split_min, sorted(l for l in labels if "attn" in l), go, SPLIT_BARS[act], min(gaps)))
    assert np.array_equal(got[:W], full[:W])
    assert min(gaps) >= 10 * SPLIT_BARS[act], min(gaps)
    assert go <= SPLIT_BARS[act], go
    # a slice / chunk that starts one position off would show at single steps, not only in the stacked vector: the worst row as well
    worst = max(_rel(got[i], ref[i]) for i in range(W, ctx))
    assert worst <= 2 * SPLIT_BARS[act], worst


@pytest.mark.watchdog(900)
@pytest.mark.parametrize("seed_pos", [250, 700])                        # 250: the replays cross BZ_SPLIT_MIN = 256 and W = 300; 700: lo moves through a slice boundary
def test_decode_graph_equals_eager_under_a_window(device, monkeypatch, seed_pos):
    monkeypatch.setenv("BZ_SPLIT_MIN", "256")
    W, steps = 300, 70
    model = synth.make_llama("tiny-awq", head_dim=128, sliding_window=W, max_seq_len=1024)
    cfg = model["config"]
    lm = runtime.LoadedModel.from_synth(device, model)
    toks = synth.prompt_tokens(seed_pos + 1, cfg["vocab"], seed=22)
    caches = [lm.new_kv_cache(1024) for _ in range(2)]
    for kv in caches:                                                    # the same prompt rows in both caches
        lm.forward_with_kv_cache(toks[:seed_pos], kv, 0)
    eager, tok = [], int(toks[seed_pos])
    for i in range(steps):
        lg = lm.forward_with_kv_cache([tok], caches[0], seed_pos + i).to_numpy().reshape(-1)
        eager.append(lg)
        tok = int(lg.argmax())
    g = runtime.DecodeGraph(lm, caches[1])
    g.seed_next_token(int(toks[seed_pos]), seed_pos)
    for i in range(steps):
        g.replay()
        got = g.read_logits()
        assert np.array_equal(got, eager[i]), (seed_pos, i, float(np.abs(got - eager[i]).max()))
    # and the eager run is the windowed model's: its last step against the reference fed the same tokens
    seq = [int(t) for t in toks[:seed_pos + 1]] + [int(e.argmax()) for e in eager[:-1]]
    ref = swa_ref.run(swa_ref.SwaLlama(model), seq)
    # (the cache rows came from the prompt kernels: the 16-bit prompt-vs-decode bar applies)
    assert _rel(eager[-1], ref[-1]) <= SPLIT_BARS["f16"], _rel(eager[-1], ref[-1])


def test_paged_decode_graph_equals_eager_under_a_window(device):
    W, seed_pos, steps, bs = 8, 5, 30, 8
    model = synth.make_llama("tiny-awq", sliding_window=W)
    cfg = model["config"]
    lm = runtime.LoadedModel.from_synth(device, model)
    toks = [int(t) for t in synth.prompt_tokens(seed_pos + 1, cfg["vocab"], seed=23)]
    nb = 6
    pools = [runtime.LayeredPagedKvCache(device, cfg["n_layers"], nb + 2, bs, cfg["n_kv_heads"], cfg["head_dim"], _DT["f16"]) for _ in range(2)]
    blocks = [5, 2, 7, 0, 3, 6]
    for pk in pools:
        pk.set_blocks(blocks)
        for i, t in enumerate(toks[:seed_pos]):
            lm.forward_with_paged_kv_cache([t], pk, pk.compute_slot_mapping(i, 1), blocks, i + 1, i)
    eager, tok = [], toks[seed_pos]
    for i in range(steps):
        p = seed_pos + i
        lg = lm.forward_with_paged_kv_cache([tok], pools[0], pools[0].compute_slot_mapping(p, 1), blocks, p + 1, p).to_numpy().reshape(-1)
        eager.append(lg)
        tok = int(lg.argmax())
    pools[1].set_seq_len(seed_pos)
    g = runtime.DecodeGraph(lm, pools[1], max_blocks=nb)
    g.set_block_table(blocks)
    g.seed_next_token(toks[seed_pos], seed_pos)
    for i in range(steps):
        g.replay()
        assert np.array_equal(g.read_logits(), eager[i]), i
    seq = toks[:seed_pos + 1] + [int(e.argmax()) for e in eager[:-1]]
    ref = swa_ref.run(swa_ref.SwaLlama(model), seq)
    assert _rel(np.stack(eager[W:]), ref[seed_pos + W:]) <= SPLIT_BARS["f16"]


# ---- prompts --------------------------------------------------------------------------------------------------------------------------------------
PROMPT_MODELS = {
    "awq-hd64": ("tiny-awq", dict(sliding_window=24, max_seq_len=512)),                       # f16, MFMA prompt attention, head_dim 64
    "awq-hd128": ("tiny-awq", dict(head_dim=128, sliding_window=24, max_seq_len=512)),        # head_dim 128
    "bf16": ("tiny-bf16", dict(sliding_window=24, max_seq_len=512)),
    "q4km": ("tiny-q4km", dict(n_layers=2, sliding_window=24, max_seq_len=512)),              # f32: the scalar prompt kernel, exact sums
}


@pytest.mark.watchdog(600)
@pytest.mark.parametrize("key", list(PROMPT_MODELS))
def test_long_prompts_under_a_window(device, key):
    """300 prompt rows with W = 24: five key tiles, most of them wholly below a query tile's windows (not loaded), the rest entered by waves whose
    later queries see none of a tile's keys; once from position 0 and once as 200 rows on top of 100 cached positions"""
    preset, over = PROMPT_MODELS[key]
    model = synth.make_llama(preset, **over)
    cfg = model["config"]
    W, act, n = cfg["sliding_window"], cfg["act_dtype"], 300
    bar = PATH_BAR if act == "f32" else SPLIT_BARS[act]
    lm, lm0 = runtime.LoadedModel.from_synth(device, model), runtime.LoadedModel.from_synth(device, _plain(model))
    toks = [int(t) for t in synth.prompt_tokens(n, cfg["vocab"], seed=24)]
    tbt = _tbt(lm, toks)
    rows = lm.forward_with_kv_cache(toks, lm.new_kv_cache(n + 8), 0, all_logits=True).to_numpy()
    worst = max(_rel(rows[i], tbt[i]) for i in range(n))
    rows0 = lm0.forward_with_kv_cache(toks, lm0.new_kv_cache(n + 8), 0, all_logits=True).to_numpy()
    gap = min(_rel(rows0[i], tbt[i]) for i in range(W + 40, n))
    kv = lm.new_kv_cache(n + 8)
    _tbt(lm, toks[:100], kv)
    top = lm.forward_with_kv_cache(toks[100:], kv, 100, all_logits=True).to_numpy()
    worst_top = max(_rel(top[i], tbt[100 + i]) for i in range(n - 100))
    nxt = lm.forward_with_kv_cache([toks[0]], kv, n).to_numpy().reshape(-1)          # the rows the prompt left in the cache serve the next decode step
    kv2 = lm.new_kv_cache(n + 8)
    _tbt(lm, toks, kv2)
    want = lm.forward_with_kv_cache([toks[0]], kv2, n).to_numpy().reshape(-1)
    print("%s: prompt rows vs token-by-token worst %.3e, on a cache %.3e, next step %.3e (bar %.1e); full-attention prompt rows at least %.3e away"
          % (key, worst, worst_top, _rel(nxt, want), bar, gap))
    assert gap >= 10 * bar, gap
    assert worst <= bar, worst
    assert worst_top <= bar, worst_top
    assert _rel(nxt, want) <= bar


_CHILD = r"""
import sys
import numpy as np
from blazr_amd import runtime, synth
n, W = int(sys.argv[2]), int(sys.argv[3])
model = synth.make_llama("tiny-q4km", n_layers=2, sliding_window=W, max_seq_len=n + 64)
dev = runtime.Device(0)
lm = runtime.LoadedModel.from_synth(dev, model)
toks = [int(t) for t in synth.prompt_tokens(n, model["config"]["vocab"], seed=25)]
kv = lm.new_kv_cache(n + 8)
print("MARK prompt", file=sys.stderr, flush=True)
rows = lm.forward_with_kv_cache(toks, kv, 0, all_logits=True).to_numpy()
print("MARK steps", file=sys.stderr, flush=True)
kv2 = lm.new_kv_cache(n + 8)
tail = []
for i, t in enumerate(toks):
    lg = lm.forward_with_kv_cache([t], kv2, i)
    if i % 997 == 0 or i >= n - 64:
        tail.append((i, lg.to_numpy().reshape(-1)))
idx = np.array([i for i, _ in tail])
np.savez(sys.argv[1], idx=idx, rows=rows[idx], steps=np.stack([r for _, r in tail]))
del kv, kv2, lm
dev.close()
"""


@pytest.mark.watchdog(900)
def test_prompt_longer_than_the_old_score_buffer(tmp_path):
    """The scalar prompt kernel (f32 models) keeps a row's scores in LDS: [group][context] floats before, 160 KiB at ~16 300 positions of this model,
    beyond which the prompt ran token by token.  With W = 24 a row has 24 scores: a 17 000-token prompt takes the batched path (trace line
    'prefill:') and its rows are the token-by-token rows at PATH_BAR.  A fresh process: BZ_TRACE is read once."""
    n, W = 17000, 24
    cfg = synth.make_config("tiny-q4km")
    rep, hd = cfg["n_heads"] // cfg["n_kv_heads"], cfg["head_dim"]
    old_smem = (8 * rep + (256 // (hd // 8)) * rep * hd) * 8 + rep * n * 4 + 64          # bzk_pf_attn_smem with the whole context, exact sums
    assert old_smem > 160 * 1024, old_smem
    out = str(tmp_path / "rows.npz")
    env = dict(os.environ, BZ_TRACE="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-c", _CHILD, out, str(n), str(W)], env=env, capture_output=True, text=True, timeout=640, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    err = r.stderr
    prompt_part = err[err.index("MARK prompt"):err.index("MARK steps")]
    assert "[bz] prefill: S=%d position=0" % n in prompt_part, prompt_part[:500]
    z = np.load(out)
    worst = max(_rel(a, b) for a, b in zip(z["rows"], z["steps"]))
    print("prompt of %d rows, W = %d: %d rows compared, worst %.3e (bar %.1e)" % (n, W, len(z["idx"]), worst, PATH_BAR))
    assert len(z["idx"]) >= 80 and worst <= PATH_BAR, worst


# ---- batched decode graph -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.watchdog(600)
@pytest.mark.parametrize("preset,nseq", [("tiny-awq", 10), ("tiny-bf16", 3)])             # 10 sequences share the prompt-row kernels, 3 run one by one
def test_batched_decode_graph_under_a_window(device, preset, nseq):
    """sequences of 3 .. 29 positions decode 24 steps in one graph with W = 16: every one crosses W (or starts past it) while the positions move on
    the device.  Graph == eager batch bit for bit; the eager batch rows are the windowed model's (reference fed the same ids)."""
    W = 16
    model = synth.make_llama(preset, sliding_window=W)
    cfg = model["config"]
    act = cfg["act_dtype"]
    lm = runtime.LoadedModel.from_synth(device, model)
    bs, per, steps = 16, 5, 24

    def fresh_pool():
        return runtime.LayeredPagedKvCache(device, cfg["n_layers"], nseq * per, bs, cfg["n_kv_heads"], cfg["head_dim"], _DT[act])
    tables = [[i + nseq * j for j in range(per)] for i in range(nseq)]
    plens = [3 + (13 * i) % 27 for i in range(nseq)]
    prompts = [[int(t) for t in synth.prompt_tokens(n, cfg["vocab"], seed=80 + i)] for i, n in enumerate(plens)]

    def prefill(pool):
        first = []
        for p, tb in zip(prompts, tables):
            for i, t in enumerate(p):
                lg = lm.forward_with_paged_kv_cache([t], pool, [tb[i // bs] * bs + i % bs], tb, i + 1, i).to_numpy()
            first.append(int(lg[0].argmax()))
        return first

    pool_a = fresh_pool()
    toks = prefill(pool_a)
    first = list(toks)
    lens = list(plens)
    eager_ids, eager_logits = [], []
    for _ in range(steps):
        lens = [n + 1 for n in lens]
        slots = [tb[(n - 1) // bs] * bs + (n - 1) % bs for n, tb in zip(lens, tables)]
        lg = lm.forward_paged_batch(toks, pool_a, slots, tables, lens).to_numpy()
        toks = [int(r.argmax()) for r in lg]
        eager_ids.append(list(toks)); eager_logits.append(lg)
    pool_b = fresh_pool()
    assert prefill(pool_b) == first
    g = runtime.BatchDecodeGraph(lm, pool_b, nseq, per)
    g.seed(first, [n + 1 for n in plens], tables)
    for s in range(steps):
        g.replay()
        if s in (0, 7, 13, steps - 1):
            assert np.array_equal(g.read_logits(), eager_logits[s]), "graph step %d differs from the eager batched step" % s
    for s in range(steps):
        assert g.read_tokens(s).tolist() == eager_ids[s], s
    worst = 0.0
    for i in range(nseq):
        seq = prompts[i] + [first[i]] + [eager_ids[s][i] for s in range(steps - 1)]
        ref = swa_ref.run(swa_ref.SwaLlama(model), seq)
        mine = np.stack([eager_logits[s][i] for s in range(steps)])
        want = ref[plens[i]:plens[i] + steps]
        keep = [s for s in range(steps) if plens[i] + s >= W]               # rows past the window
        worst = max(worst, _rel(mine[keep], want[keep]))
    print("%s x %d: batched rows past W vs reference, worst sequence %.3e (bar %.1e)" % (preset, nseq, worst, SPLIT_BARS[act]))
    assert worst <= SPLIT_BARS[act], worst
