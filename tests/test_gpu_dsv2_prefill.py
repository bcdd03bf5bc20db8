"""The DeepSeek-V2 prompt path (dsv2_prefill, blazr_amd/csrc/bz_host.hip) against the oracle: configuration variants, routing extremes, a prompt
across the 512-row chunk, the paged latent cache, and every prompt-MLA kernel regime over long injected contexts.

Every prompt here has more than BZ_EXACT_PREFILL_MAX (16) rows, so an eligible model takes the batched path: k_mla_append_rows, the prompt MLA
kernels (k_mla_attn_tile<4|8> or k_mla_attn<BATCH>), the MoE row pipeline (route -> plan -> gather -> grouped GEMM -> combine) and the shared-slot
sum (k_acc_rows).  Which path ran is shown, not assumed: each case also feeds the same tokens one at a time through the decode step.  The MFMA
f32 sums of the batched path are not the exact sums of the decode kernels, so an eligible model's batched rows differ from its token-by-token
rows somewhere (where every rounding of a chunk happens to agree, the library's BZ_TRACE line shows the path instead); a model
dsv2_prefill_eligible turns away falls back to the decode step, and its rows are those rows bit for bit.

Bars (as tests/test_gpu_workloads.py): bar = REL[act] x 1.25 for bf16 activations, REL[act] otherwise, on the per-row relative L2 -- median <= bar,
90th percentile <= 2 x bar, rows beyond 4 x bar <= max(1, 3 % of the rows).  A router near-tie can legitimately give one row another expert, hence
the distribution; where routing cannot flip (no MoE layer, a zero router, top_k == n_experts) _check_logits over all rows applies as well.
"""
import json
import os
import re
import subprocess
import sys
import time
from types import SimpleNamespace

import numpy as np
import pytest

from blazr_amd import _lib as L
from blazr_amd import runtime, synth
from oracle import orc_py
import npref
from test_gpu_dsv2 import _YARN
from test_gpu_llama import REL, _check_logits

pytestmark = pytest.mark.gpu

LAT = {"bf16": 2 ** -7, "f16": 2 ** -10, "f32": 1e-5}      # one rounding unit of a latent-cache value (relative to the largest)


def _bar(act):
    return REL[act] * (1.25 if act == "bf16" else 1.0)


def _rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _check_rows(name, got, want, act):
    """the per-row distribution bars; prints median, p90, max and the far-row count"""
    got = np.asarray(got, np.float64).reshape(len(want), -1)
    want = np.asarray(want, np.float64).reshape(len(want), -1)
    per = np.linalg.norm(got - want, axis=1) / np.maximum(np.linalg.norm(want, axis=1), 1e-30)
    bar = _bar(act)
    far = int((per > 4 * bar).sum())
    med, p90 = float(np.median(per)), float(np.quantile(per, 0.9))
    print("%s: %d rows vs the oracle, relative L2 per row median %.3e, p90 %.3e, max %.3e (bar %.2e), rows beyond 4x the bar: %d"
          % (name, len(per), med, p90, per.max(), bar, far))
    assert med <= bar, (name, med, bar)
    assert p90 <= 2 * bar, (name, p90, bar)
    assert far <= max(1, 0.03 * len(per)), (name, far, np.nonzero(per > 4 * bar)[0].tolist())


def _stepped(lm, tokens, kv, pos0):
    """the same tokens one at a time through the decode step"""
    return np.stack([lm.forward_with_kv_cache([int(t)], kv, pos0 + i).to_numpy().reshape(-1) for i, t in enumerate(tokens)])


_TRACE_CHILD = r"""
import json, sys
from blazr_amd import runtime, synth
over, chunks = eval(sys.argv[1]), json.loads(sys.argv[2])
model = synth.make_dsv2("tiny-dsv2", **over)
dev = runtime.Device(0)
lm = runtime.LoadedModel.from_synth(dev, model)
kv = lm.new_kv_cache(sum(len(t) for t, _ in chunks) + 8)
for toks, pos in chunks:
    lm.forward_with_kv_cache(toks, kv, pos, all_logits=True)
dev.close()
"""


def _traced_prefill_calls(over, chunks):
    """the chunks [(tokens, position)] of a tiny-dsv2 variant, run in a child process with BZ_TRACE set: (S, position) of every dsv2_prefill call"""
    e = dict(os.environ)
    e["BZ_TRACE"] = "1"
    e["PYTHONPATH"] = os.path.dirname(os.path.dirname(os.path.abspath(__file__))) + os.pathsep + e.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", _TRACE_CHILD, repr(over), json.dumps([[[int(t) for t in toks], pos] for toks, pos in chunks])],
                       env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return [(int(a), int(b)) for a, b in re.findall(r"\[bz\] dsv2_prefill: S=(\d+) position=(\d+)", r.stderr)]


def _check_path(name, batched, stepped, eligible, at=None, trace=None):
    """eligible: the batched rows differ from the token-by-token rows somewhere -- or, where every rounding happened to agree, the library's
    trace shows dsv2_prefill running the chunk at = (S, position).  Ineligible: the rows are the token-by-token rows bit for bit."""
    same = np.array_equal(batched, stepped)
    if eligible and same and trace is not None:
        calls = trace()
        print("%s: rows equal the token-by-token rows bit for bit; dsv2_prefill calls traced (S, position): %s" % (name, calls))
        assert at in calls, "%s: the batched path did not run (traced calls %s)" % (name, calls)
        return
    print("%s: %s path (rows %s the token-by-token rows)" % (name, "fallback" if same else "batched", "equal" if same else "differ from"))
    if eligible:
        assert not same, "%s: the rows are the token-by-token rows bit for bit -- the batched path did not run" % name
    else:
        assert same, "%s: ineligible for dsv2_prefill, yet the rows differ from the token-by-token rows (max |d| %g)" % (
            name, float(np.abs(batched - stepped).max()))


def _check_latents(name, kv, okc, n_layers, pos0, n, act):
    olat = orc_py.mla_rows(okc)
    for layer in range(n_layers):
        g = kv.read(layer, 0, 0, pos0 + n)[pos0:]
        o = olat[layer, pos0:pos0 + n]
        err = float(np.abs(g - o).max())
        assert err <= 2 * LAT[act] * np.abs(o).max(), (name, layer, err, float(np.abs(o).max()))


# ------------------------------------------------------------------------------------------------------------------------------------------
# 1 + 5. configuration variants on the batched path (and the float64 truth for the eligible non-YaRN ones)
# ------------------------------------------------------------------------------------------------------------------------------------------
S1, S2, N_DEC = 37, 21, 4
# tie_embeddings: the tied lm_head is the dense embedding itself (one LK_ROWS part, direct f32 output), which dsv2_prefill_eligible accepts
ELIGIBLE = [({}, "default"), (dict(n_shared=0), "no-shared"), (dict(n_shared=1), "one-shared"), (dict(n_shared=3), "three-shared"),
            (dict(first_dense=0, n_layers=2), "all-moe"), (dict(top_k=8), "topk-all"), (dict(n_experts=0, first_dense=3), "dense-only"),
            (dict(norm_topk=True, routed_scale=2.0), "norm-topk-scaled"), (dict(rope_scaling=_YARN), "yarn-mscale"),
            (dict(kv_lora_rank=64, nope_dim=32, v_dim=128, rope_dim=16), "odd-mla-dims"), (dict(act_dtype="f16"), "f16"),
            (dict(tie_embeddings=True), "tied-embeddings")]
# q_lora_rank > 0, a moe_inter that is not a multiple of 64, f32 activations: dsv2_prefill_eligible sends these to the decode step
INELIGIBLE = [(dict(q_lora_rank=96), "q-lora"), (dict(moe_inter=96), "moe-inter-96"), (dict(act_dtype="f32"), "f32")]
VARIANTS = [(o, n, True) for o, n in ELIGIBLE] + [(o, n, False) for o, n in INELIGIBLE]


def _no_flip(cfg):
    """routing cannot flip: no MoE layer, or every expert selected"""
    return cfg["n_experts"] == 0 or cfg["first_dense"] >= cfg["n_layers"] or cfg["top_k"] == cfg["n_experts"]


@pytest.mark.watchdog(300)
@pytest.mark.parametrize("over,name,eligible", VARIANTS, ids=[v[1] for v in VARIANTS])
def test_config_variants_on_the_prompt_path(device, over, name, eligible):
    """a 37-token prompt, a 21-token chunk behind it, then decode steps over the cache the prompt path wrote: every row against the oracle,
    the latent rows of the first chunk against the oracle's, and (eligible, non-YaRN) the rows against the float64 truth"""
    model = synth.make_dsv2("tiny-dsv2", **over)
    cfg = model["config"]
    act = cfg["act_dtype"]
    lm, om = runtime.LoadedModel.from_synth(device, model), orc_py.OrcDsv2(model)
    p1 = synth.prompt_tokens(S1, cfg["vocab"], seed=17)
    p2 = synth.prompt_tokens(S2, cfg["vocab"], seed=18)
    cap = S1 + S2 + N_DEC + 4
    kv, kv2, okc = lm.new_kv_cache(cap), lm.new_kv_cache(cap), om.new_cache(cap)
    try:
        g1 = lm.forward_with_kv_cache(p1, kv, 0, all_logits=True).to_numpy()
        o1 = om.forward(p1, okc, 0, all_logits=True).copy()
        _check_latents(name, kv, okc, cfg["n_layers"], 0, S1, act)
        g2 = lm.forward_with_kv_cache(p2, kv, S1, all_logits=True).to_numpy()
        o2 = om.forward(p2, okc, S1, all_logits=True).copy()
        _check_latents(name + " second chunk", kv, okc, cfg["n_layers"], S1, S2, act)
        G, O = np.concatenate([g1, g2]), np.concatenate([o1, o2])
        T = _stepped(lm, list(p1) + list(p2), kv2, 0)
        trace = lambda: _traced_prefill_calls(over, [(p1, 0), (p2, S1)])
        _check_path(name + " first chunk", g1, T[:S1], eligible, (S1, 0), trace)
        _check_path(name + " second chunk", g2, T[S1:], eligible, (S2, S1), trace)
        _check_rows(name, G, O, act)
        if _no_flip(cfg):
            _check_logits(G, O, act)
        tok = int(o2[-1].argmax())
        for i in range(N_DEC):      # the decode step reads the latents the prompt path wrote
            lo = om.forward([tok], okc, S1 + S2 + i).copy()
            _check_logits(lm.forward_with_kv_cache([tok], kv, S1 + S2 + i).to_numpy(), lo, act)
            tok = int(lo[0].argmax())
    finally:
        orc_py.lib().orc_mla_cache_free(okc)
    if not eligible or "rope_scaling" in over:       # npref.NpDsv2 has no YaRN
        return
    # 5. the unrounded float64 truth: the prompt-path rows no further from it than the oracle's own (1.25x on L2, 1.5x on the max-norm, as
    #    test_parity_truth.py::test_dsv2_full_width_against_the_unrounded_truth).  Only rows whose truth routing gap is below 1e-3 (relative) are left out.
    tm = npref.NpDsv2(model, truth=True)
    TR = np.stack([tm.step(int(t), i) for i, t in enumerate(list(p1) + list(p2))])
    gaps = tm.routing_gaps()
    keep = np.ones(len(TR), bool) if gaps.size == 0 else gaps.min(axis=1) >= 1e-3
    if not keep.all():
        print("%s: rows left out of the truth comparison (routing gap < 1e-3): %s" % (name, [(int(i), float(gaps[i].min())) for i in np.nonzero(~keep)[0]]))
    Gk, Ok, Tk = G[keep].astype(np.float64), O[keep].astype(np.float64), TR[keep]
    nT = np.linalg.norm(Tk)
    g2_, o2_ = np.linalg.norm(Gk - Tk) / nT, np.linalg.norm(Ok - Tk) / nT
    gm, omx = np.abs(Gk - Tk).max() / np.abs(Tk).max(), np.abs(Ok - Tk).max() / np.abs(Tk).max()
    msg = "%s (%d rows): relative L2 to the f64 truth: hip %.3e, oracle %.3e; max-norm: hip %.3e, oracle %.3e" % (name, int(keep.sum()), g2_, o2_, gm, omx)
    print(msg)
    assert g2_ <= 1.25 * o2_ and gm <= 1.5 * omx, msg


# ------------------------------------------------------------------------------------------------------------------------------------------
# 2 + 3. routing extremes and a prompt across the 512-row chunk (600 rows: dsv2_prefill's chunks of 512 + 88)
# ------------------------------------------------------------------------------------------------------------------------------------------
S_LONG, S_TAIL = 600, 30


@pytest.mark.watchdog(600)
@pytest.mark.parametrize("case", ["zero-router", "topk-all", "plain"])
def test_600_row_prompts(device, case):
    """zero-router: every router logit is exactly 0, and ties pick the lowest index, so every token takes experts 0..k-1 with weight 1/E and the
    other experts get zero rows (a grouped GEMM with maxc = 600; 600 x top_k entries through k_moe_plan_rows).  topk-all: every expert gets every
    row.  plain: the tiny model as it is, with a 30-token chunk behind the 600 rows.  Every row against the oracle."""
    model = synth.make_dsv2("tiny-dsv2", max_seq_len=1024, **(dict(top_k=8) if case == "topk-all" else {}))
    cfg = model["config"]
    act = cfg["act_dtype"]
    if case == "zero-router":
        for lay in model["layers"]:
            if lay["is_moe"]:
                lay["router"]["weight"] = np.zeros_like(lay["router"]["weight"])
    lm, om = runtime.LoadedModel.from_synth(device, model), orc_py.OrcDsv2(model)
    p = synth.prompt_tokens(S_LONG, cfg["vocab"], seed=23)
    tail = synth.prompt_tokens(S_TAIL, cfg["vocab"], seed=24) if case == "plain" else []
    cap = S_LONG + S_TAIL + 8
    kv, kv2, okc = lm.new_kv_cache(cap), lm.new_kv_cache(cap), om.new_cache(cap)
    try:
        G = lm.forward_with_kv_cache(p, kv, 0, all_logits=True).to_numpy()
        O = om.forward(p, okc, 0, all_logits=True).copy()
        _check_latents(case, kv, okc, cfg["n_layers"], 0, S_LONG, act)
        T = _stepped(lm, list(p) + list(tail), kv2, 0)
        _check_path(case + " 600 rows", G, T[:S_LONG], True)
        _check_rows(case + " 600 rows", G, O, act)
        if case != "plain":
            _check_logits(G, O, act)
        if case == "plain":
            g2 = lm.forward_with_kv_cache(tail, kv, S_LONG, all_logits=True).to_numpy()
            o2 = om.forward(tail, okc, S_LONG, all_logits=True).copy()
            _check_path("chunk at 600", g2, T[S_LONG:], True)
            _check_rows("chunk at 600", g2, o2, act)
            _check_latents("chunk at 600", kv, okc, cfg["n_layers"], S_LONG, S_TAIL, act)
    finally:
        orc_py.lib().orc_mla_cache_free(okc)


# ------------------------------------------------------------------------------------------------------------------------------------------
# 3. the paged latent cache on the batched path
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs", [4, 16])
def test_paged_batched_prompt_equals_contiguous(device, bs):
    """a 37-token prompt and a 21-token chunk through dsv2_prefill over a scattered block table, then decode steps == the contiguous cache, bit for bit"""
    model = synth.make_dsv2("tiny-dsv2")
    cfg = model["config"]
    lm = runtime.LoadedModel.from_synth(device, model)
    W = cfg["kv_lora_rank"] + cfg["rope_dim"]
    p1 = synth.prompt_tokens(S1, cfg["vocab"], seed=4)
    p2 = synth.prompt_tokens(S2, cfg["vocab"], seed=5)
    n_tot = S1 + S2 + 6
    kv = lm.new_kv_cache(n_tot)
    a1 = lm.forward_with_kv_cache(p1, kv, 0, all_logits=True).to_numpy()
    a2 = lm.forward_with_kv_cache(p2, kv, S1, all_logits=True).to_numpy()
    _check_path("paged bs %d" % bs, np.concatenate([a1, a2]), _stepped(lm, list(p1) + list(p2), lm.new_kv_cache(n_tot), 0), True)
    nb = (n_tot + bs - 1) // bs + 3
    pk = runtime.LayeredPagedKvCache(device, cfg["n_layers"], nb, bs, 1, W, lm.c.act_dtype)
    pk.set_blocks([int(b) for b in np.random.default_rng(bs).permutation(nb)])
    bt = pk.block_table_device_format()
    pk.set_seq_len(S1)
    b1 = lm.forward_with_paged_kv_cache(p1, pk, pk.compute_slot_mapping(0, S1), bt, S1, 0, all_logits=True).to_numpy()
    pk.set_seq_len(S1 + S2)
    b2 = lm.forward_with_paged_kv_cache(p2, pk, pk.compute_slot_mapping(S1, S2), bt, S1 + S2, S1, all_logits=True).to_numpy()
    assert np.array_equal(a1, b1) and np.array_equal(a2, b2)
    tok = int(a2[-1].argmax())
    for i in range(6):
        n = S1 + S2 + i + 1
        pk.set_seq_len(n)
        x = lm.forward_with_kv_cache([tok], kv, n - 1).to_numpy()
        y = lm.forward_with_paged_kv_cache([tok], pk, pk.compute_slot_mapping(n - 1, 1), bt, n, n - 1).to_numpy()
        assert np.array_equal(x, y), i
        tok = int(x[0].argmax())


# ------------------------------------------------------------------------------------------------------------------------------------------
# 4. a 24-token chunk over long injected latent contexts: every mla_tile_tt regime at DeepSeek-V2-Lite MLA widths
# ------------------------------------------------------------------------------------------------------------------------------------------
LONG_N = 24
LONG_MAX = 32000
# Restated from bz_kernels.hip / bz_host.hip at rank 512, nope 128, rope 64, v 128, with LS = (P + 24 + 3) & ~3:
#   mla_tile_smem(TT, LS) = TT (nope + rope + rank + 4 rank + 8 + LS) 4 + 64 = TT (2760 + LS) 4 + 64 bytes;
#   mla_tile_tt: TT = 4 while that is <= 64 KiB (LS <= 1332), else TT = 8 while <= 160 KiB (LS <= 2358: LS is a multiple of 4, so P + 24 <= 2356),
#   else TT = 4 while <= 160 KiB (LS <= 7476), else 0: the (head, token) kernel k_mla_attn<BATCH>.
#   dsv2_prefill_eligible probes bzk_mla_smem of the decode kernel (16 waves, no split): (18 rank + 2 rope + nope + 16 + P + 24) 4 + 64 <= 160 KiB,
#   i.e. P + 24 <= 31456; past that the chunk runs token by token on the decode step.
LONG_CASES = [(1000, "tile TT=4"), (1336, "tile TT=8"), (2000, "tile TT=8"), (5000, "tile TT=4"), (12000, "head-token"), (31456, "head-token"),
              (LONG_MAX, "fallback")]


def _regime(total, rank=512, nope=128, rope=64):
    if (rank * 18 + rope * 2 + nope + 16 + total) * 4 + 64 > 160 * 1024:
        return "fallback"
    LS = (total + 3) & ~3
    sm = lambda TT: TT * (nope + rope + rank + 4 * rank + 8 + LS) * 4 + 64
    if sm(4) <= 64 * 1024:
        return "tile TT=4"
    if sm(8) <= 160 * 1024:
        return "tile TT=8"
    return "tile TT=4" if sm(4) <= 160 * 1024 else "head-token"


def test_long_context_regime_table():
    """the stated limits of the table above (a CPU check of the restatement itself)"""
    for total, want in ((1332, "tile TT=4"), (1333, "tile TT=8"), (2356, "tile TT=8"), (2357, "tile TT=4"), (7476, "tile TT=4"),
                        (7477, "head-token"), (31456, "head-token"), (31457, "fallback")):
        assert _regime(total) == want, (total, _regime(total), want)


@pytest.fixture(scope="module")
def long_ctx(device):
    """1-layer dense model at V2-Lite MLA widths; LONG_MAX - 24 latent rows injected into the GPU cache (the oracle's are set per test).  Rows 100 and 101
    are planted at +-64x a background row, so one of the two scores is high for every head."""
    model = synth.make_dsv2("deepseek-v2-lite", n_layers=1, vocab=1024, inter=512, n_experts=0, first_dense=1, max_seq_len=32768)
    cfg = model["config"]
    W = cfg["kv_lora_rank"] + cfg["rope_dim"]
    lm, om = runtime.LoadedModel.from_synth(device, model), orc_py.OrcDsv2(model)
    top = LONG_MAX - LONG_N
    kv, okc = lm.new_kv_cache(LONG_MAX + 8), om.new_cache(LONG_MAX + 8)
    rng = np.random.default_rng(7)
    X = orc_py.round_act(rng.standard_normal((top, W)).astype(np.float32) * 0.5, cfg["act_dtype"])
    X[100] = orc_py.round_act(X[100] * 64, cfg["act_dtype"])
    X[101] = -X[100]
    tk, tv = device.zeros((1, W)), device.zeros((1, W))

    def inject(lo, hi):
        for q in range(lo, min(hi, top)):
            tk.copy_from(X[q])
            L.check(L.lib().bz_kv_insert(lm.h, kv.h, 0, q, tk.h, tv.h))

    t0 = time.time()
    inject(0, top)
    print("injected %d latent rows in %.1f s" % (top, time.time() - t0))
    assert np.array_equal(kv.read(0, 0, 0, top), X)
    yield SimpleNamespace(model=model, cfg=cfg, lm=lm, om=om, kv=kv, okc=okc, X=X, inject=inject)
    orc_py.lib().orc_mla_cache_free(okc)


@pytest.mark.watchdog(300)
@pytest.mark.parametrize("total,regime", LONG_CASES, ids=["ctx%d" % t for t, _ in LONG_CASES])
def test_prompt_chunk_over_long_injected_context(long_ctx, total, regime):
    """a 24-token chunk at position P = total - 24 over P injected latents: every row against the oracle, the 24 latent rows it appended against
    the oracle's, and the path (batched, or the token-by-token fallback past eligibility) against the decode step"""
    c = long_ctx
    act = c.cfg["act_dtype"]
    bar = _bar(act)
    P = total - LONG_N
    assert _regime(total) == regime, (total, _regime(total))
    print("context %d (P = %d): %s" % (total, P, regime))
    lat = orc_py.mla_rows(c.okc)
    lat[0, :P] = c.X[:P]
    p = synth.prompt_tokens(LONG_N, c.cfg["vocab"], seed=P)
    try:
        # the planted rows must matter to the oracle's first row: a kernel that skipped far positions would then fail
        c.okc.contents.seq_len = P
        o = np.asarray(c.om.forward([int(p[0])], c.okc, P)).reshape(-1).copy()
        lat[0, 100:102] = c.X[102:104]
        c.okc.contents.seq_len = P
        o_drop = np.asarray(c.om.forward([int(p[0])], c.okc, P)).reshape(-1).copy()
        lat[0, 100:102] = c.X[100:102]
        sens = _rel(o_drop, o)
        print("context %d: planted-row sensitivity %.3e (20x bar %.3e)" % (total, sens, 20 * bar))
        assert sens >= 20 * bar, (total, sens)
        c.okc.contents.seq_len = P
        want = c.om.forward(p, c.okc, P, all_logits=True).copy()
        got = c.lm.forward_with_kv_cache(p, c.kv, P, all_logits=True).to_numpy()
        _check_latents("context %d" % total, c.kv, c.okc, 1, P, LONG_N, act)
        # token by token over the same cache: decode step P + i writes row P + i before it reads rows 0 .. P + i, so this is a fresh cache's result
        T = _stepped(c.lm, p, c.kv, P)
        _check_path("context %d" % total, got, T, regime != "fallback")
        _check_rows("context %d" % total, got, want, act)
        _check_logits(got, want, act, factor=1.25 if act == "bf16" else 1.0)
    finally:
        c.inject(P, total)
