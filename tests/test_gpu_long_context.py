"""Long-context attention, against the CPU oracle and an unrounded float64 truth, at the contexts the served configs run (up to 20 000 positions).

Running the oracle over an L-token prompt costs O(L^2), so the caches are INJECTED instead: the same rows (exactly representable in the cache
dtype) go into the GPU cache through bz_kv_insert, into the oracle's orc_kv and into npref.NpLlamaTruth's history, and one decode step at
position P then costs O(P) everywhere.

Random caches cannot catch a dropped or doubled row: softmax over thousands of random keys is nearly uniform, so one row moves the output by
~1/L, under every bar.  The 1-layer models here make the roped query at P a function of the token alone (npref computes it), so each planted
key is chosen from that query with a set score margin, and each planted row carries a V pattern of its own.  Every planted case first proves
on the CPU that the truth moves by at least 20x the bar of its path when the planted row is removed.

Bars are the suite's own: exact single-launch paths 1e-4 relative L2 against the oracle (test_gpu_workloads.py); split-KV 1.5e-3 against the
oracle for f16 activations (2^-7, the suite's bf16 logit bar, for bf16) and, in addition, no further from the truth than 1.25x the oracle's
distance (test_gpu_parity_truth.py).
"""
import numpy as np
import pytest

from blazr_amd import _lib as L
from blazr_amd import runtime, synth
from oracle import orc_py
import npref

pytestmark = pytest.mark.gpu

# split-KV: 1.5e-3 for f16 activations (test_gpu_workloads.py); bf16 activations keep the suite's bf16 logit bar, 2^-7 (test_gpu_llama.py REL)
EXACT_BAR, SPLIT_BARS, TRUTH_FACTOR, FLOOR = 1e-4, {"f16": 1.5e-3, "bf16": 2.0 ** -7}, 1.25, 4e-6
TOKEN = 5
_DT = {"f16": L.F16, "bf16": L.BF16, "f32": L.F32}


def _rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _labels(lm, kv, P):
    return {r["name"] for r in lm.profile_step(kv, TOKEN, P, iters=1)}


def _spl(ctx):
    """positions per split-KV slice for a context of ctx positions (128, doubled until at most 128 slices)"""
    spl = 128
    while -(-ctx // spl) > 128:
        spl *= 2
    return spl


class Injected:
    """one model with the same cached rows in the GPU cache, the oracle's cache and the float64 truth's history"""

    def __init__(self, device, model, rows, seed=0, capacity=None):
        self.dev, self.model, self.cfg = device, model, model["config"]
        c = self.cfg
        self.act, self.nkv, self.hd = c["act_dtype"], c["n_kv_heads"], c["head_dim"]
        self.lm, self.om, self.tm = runtime.LoadedModel.from_synth(device, model), orc_py.OrcLlama(model), npref.NpLlamaTruth(model)
        self.np = npref.NpLlama(model)
        rng = np.random.default_rng(seed)
        R = lambda x: orc_py.round_act(x, self.act)
        self.K = R(rng.standard_normal((rows, self.nkv, self.hd)).astype(np.float32) * 0.05)
        self.V = R(rng.standard_normal((rows, self.nkv, self.hd)).astype(np.float32))
        # a small initial capacity: kv_grow re-allocates the cache many times on the way to `rows`
        self.kv = runtime.LayeredKvCache(device, 1, 1, self.nkv, 16, c["max_seq_len"], self.hd, _DT[self.act])
        self.okv = self.om.new_kv(capacity or rows + 1)
        self.tk, self.tv = device.zeros((self.nkv, self.hd)), device.zeros((self.nkv, self.hd))
        for p in range(rows):
            self._put(p)
        orc_py.kv_inject(self.okv, 0, self.K, self.V)

    def close(self):
        orc_py.lib().orc_kv_free(self.okv)

    def _put(self, p):
        self.tk.copy_from(self.K[p])
        self.tv.copy_from(self.V[p])
        L.check(L.lib().bz_kv_insert(self.lm.h, self.kv.h, 0, p, self.tk.h, self.tv.h))

    def set_rows(self, rows, K, V):
        """overwrite cached rows in all three caches"""
        ok, ov = orc_py.kv_rows(self.okv)
        for p, k, v in zip(rows, K, V):
            self.K[p], self.V[p] = k, v
            self._put(p)
            ok[0, :, p], ov[0, :, p] = k, v

    def step(self, P):
        """one decode step at P over rows 0..P-1: GPU, oracle and truth logits.  Row P is the step's own; both implementations overwrite it,
        and the next step at any P' > P sees the injected row again (restored here)."""
        g = self.lm.forward_with_kv_cache([TOKEN], self.kv, P).to_numpy().reshape(-1)
        o = np.asarray(self.om.forward_kv([TOKEN], self.okv, P)).reshape(-1)
        t = self.truth(P)
        self.set_rows([P], self.K[P:P + 1].copy(), self.V[P:P + 1].copy())
        return g, o, t

    def truth(self, P, drop=()):
        keep = np.setdiff1d(np.arange(P), np.asarray(drop, dtype=np.int64))
        self.tm.set_history([(self.K[keep], self.V[keep])])
        return self.tm.step(TOKEN, P)

    def query(self, P):
        q, _, _ = self.np.qkv0(TOKEN, P)
        return q.reshape(self.nkv, -1, self.hd)          # [kv head][group][head_dim]

    def key_with_score(self, P, score):
        """one key per kv head whose score against EVERY query head of its group at P is at least `score` (background scores are ~N(0, small))"""
        q = self.query(P)
        u = q.sum(axis=1)
        u = u / np.linalg.norm(u, axis=1, keepdims=True)
        s = np.einsum("ghd,gd->gh", q, u).min(axis=1) / np.sqrt(self.hd)
        assert (s > 0).all(), "a query head points away from its group's mean: no key scores high for all of them"
        return orc_py.round_act(u * (1.001 * score / s)[:, None], self.act)

    def margin(self, P, rows):
        """smallest gap, over all query heads, between the best of `rows` and the best of every other cached row"""
        q = self.query(P)
        sc = np.einsum("ghd,tgd->ght", q.astype(np.float64), self.K[:P].astype(np.float64)) / np.sqrt(self.hd)
        mask = np.zeros(P, bool)
        mask[rows] = True
        return float((sc[..., mask].max(axis=-1) - sc[..., ~mask].max(axis=-1)).min())

    def pattern(self, j):
        """a V row of its own for planted row j: large, and orthogonal-ish to every other pattern"""
        d = np.arange(self.hd)
        v = 4.0 * np.sign(np.cos((j + 1) * 0.7 * d + j)) * (1.0 + (d % (j + 3) == 0))
        return orc_py.round_act(np.broadcast_to(v, (self.nkv, self.hd)).astype(np.float32), self.act)


def _check(name, g, o, t, bar, split, sens):
    go = _rel(g, o)
    msg = "%s: hip vs oracle %.3e (bar %.1e)" % (name, go, bar)
    if split:
        gt, ot = _rel(g, t), _rel(o, t)
        msg += "; relative L2 to the f64 truth: hip %.3e, oracle %.3e" % (gt, ot)
    msg += "; planted-row sensitivity %.3e (%.0fx the bar)" % (sens, sens / bar) if sens is not None else ""
    print(msg)
    assert go <= bar, msg
    if split:
        assert gt <= max(TRUTH_FACTOR * ot, FLOOR), msg


def _cases(inj, P, split):
    """planted constructions at context P + 1; yields (name, rows, K, V, sensitivity rows)"""
    ctx = P + 1
    if split:                 # the slice edges of the split plan, the first row of the last slice
        spl = _spl(ctx)
        edges = {spl - 1, spl, ((ctx - 1) // spl) * spl}
    else:                     # single-launch kernels: 128-row chunks (k_attn2 / k_attn2f) and 256-row tiles (k_attn_decode)
        edges = {127, 128, 255, 256}
    spots = sorted(({0, P - 1} | edges) & set(range(P)))
    for j, r in enumerate(spots):
        yield "dominant row %d" % r, [r], [inj.key_with_score(P, 16.0)], [inj.pattern(j)], [r]
    a, b = 0, max(spots)
    if a != b:
        k = inj.key_with_score(P, 16.0)
        yield "two equal rows %d and %d" % (a, b), [a, b], [k, k], [inj.pattern(1), inj.pattern(2)], [a]
    yield "margin 120 at row %d" % (P // 2), [P // 2], [inj.key_with_score(P, 120.0)], [inj.pattern(3)], [P // 2]
    # (margin >= 110 for every query head: every other slice's weight exp(m_s - M) underflows to exactly 0 -- checked below)


def _run_form(device, preset, over, contexts, split_above, fused_labels, long_labels, seed=0):
    top = max(contexts)
    model = synth.make_llama(preset, n_layers=1, max_seq_len=top + 16, **over)
    inj = Injected(device, model, top, seed=seed)
    try:
        for h in range(inj.nkv):     # the injected rows survived every kv_grow, byte for byte
            assert np.array_equal(inj.kv.read(0, h, 0, top), inj.K[:, h]) and np.array_equal(inj.kv.read(0, h, 1, top), inj.V[:, h])
        for ctx in contexts:
            P = ctx - 1
            split = ctx > split_above
            labels = _labels(inj.lm, inj.kv, P)
            inj.set_rows([P], inj.K[P:P + 1].copy(), inj.V[P:P + 1].copy())
            want, notwant = long_labels if ctx > 512 else fused_labels
            assert want <= labels and not (notwant & labels), (ctx, labels)
            bar = SPLIT_BARS[inj.act] if split else EXACT_BAR
            for name, rows, K, V, drop in _cases(inj, P, split):
                old = (inj.K[rows].copy(), inj.V[rows].copy())
                inj.set_rows(rows, K, V)
                if name.startswith("margin"):
                    assert inj.margin(P, rows) >= 110, (ctx, inj.margin(P, rows))
                base = inj.truth(P)
                sens = _rel(inj.truth(P, drop), base)
                assert sens >= 20 * bar, "%s at %d: removing the planted row moves the truth by only %.3e" % (name, ctx, sens)
                g, o, t = inj.step(P)
                _check("%s ctx %d %s" % (preset, ctx, name), g, o, t, bar, split, sens)
                inj.set_rows(rows, *old)
            # all keys equal: the output is the mean of V (plus the step's own row); the first and the last slice carry V patterns of their own, 64x the
            # others' (which share the last one's pattern), so a dropped or doubled slice moves it
            spl = _spl(ctx) if split else 128
            oldK = inj.K[:P].copy()
            oldV = inj.V[:P].copy()
            sl = np.arange(P) // spl
            w = np.where(sl == 0, 64.0, np.where(sl == sl[-1], 64.0 * spl / (sl == sl[-1]).sum(), 1.0)).astype(np.float32)   # (equal slice totals)
            Ve = orc_py.round_act(oldV * 0.25 + w[:, None, None] * np.where((sl == 0)[:, None, None], inj.pattern(5)[None], inj.pattern(6)[None]), inj.act)
            inj.set_rows(range(P), np.zeros_like(oldK), Ve)
            base = inj.truth(P)
            lastslice = list(range(((P - 1) // spl) * spl, P))
            sens = min(_rel(inj.truth(P, range(spl)), base), _rel(inj.truth(P, lastslice), base))
            assert sens >= 20 * bar, "all keys equal at %d: dropping a slice moves the truth by only %.3e" % (ctx, sens)
            g, o, t = inj.step(P)
            _check("%s ctx %d all keys equal" % (preset, ctx), g, o, t, bar, split, sens)
            inj.set_rows(range(P), oldK, oldV)
    finally:
        inj.close()


SPLIT = ({"attn_split", "attn_merge+o_proj"}, {"attn+o_proj", "attn_merge", "attn_decode"})
FUSED = ({"attn+o_proj"}, {"attn_split", "attn_merge", "attn_merge+o_proj", "attn_decode"})


@pytest.mark.watchdog(900)
def test_int4_f16_cache_head_dim_128(device):
    """Llama-3-8B heads (32 q / 8 kv, hd 128), AWQ, f16 cache: fused attention + o_proj up to 512, split-KV + attn_merge+o_proj above; 128-position
    slices up to 16 384, 256-position slices at 16 385 and 20 000"""
    _run_form(device, "llama3-8b-awq-2l", dict(hidden=2048, inter=1024, vocab=1024), [512, 513, 2049, 8192, 16384, 16385, 20000], 512, FUSED, SPLIT)


@pytest.mark.watchdog(600)
@pytest.mark.parametrize("nkv", [8, 4, 2, 1], ids=["rep1", "rep2", "rep4", "rep8"])
def test_bf16_dense_head_dim_128_split_and_unfused_merge(device, nkv):
    long = ({"attn_split", "attn_merge"}, {"attn_merge+o_proj", "attn+o_proj<dense>", "attn_decode"})
    _run_form(device, "tiny-bf16", dict(n_heads=8, n_kv_heads=nkv, head_dim=128), [513, 4097, 16385], 512, long, long, seed=nkv)


@pytest.mark.watchdog(600)
def test_bf16_head_dim_64_standalone_beyond_512(device):
    """Llama-3.2-1B heads (32 q / 8 kv, hd 64): fused attn+o_proj<dense> up to 512, the standalone single-launch k_attn2<..., 64> above (no split form)"""
    fused = ({"attn+o_proj<dense>"}, {"attn_split", "attn_merge", "attn_decode"})
    long = ({"attn_decode"}, {"attn_split", "attn_merge", "attn+o_proj<dense>"})
    _run_form(device, "llama3.2-1b-bf16", dict(hidden=512, inter=512, vocab=1024), [512, 513, 4096, 8192], 1 << 30, fused, long)


@pytest.mark.watchdog(600)
def test_f32_cache_head_dim_128_k_attn2f(device):
    """Mistral heads (32 q / 8 kv, hd 128), Q4_K_M, f32 cache: attn+o_proj<q4_K> up to 512, the standalone k_attn2f above"""
    fused = ({"attn+o_proj<q4_K>"}, {"attn_split", "attn_merge", "attn_decode"})
    long = ({"attn_decode"}, {"attn_split", "attn_merge", "attn+o_proj<q4_K>"})
    _run_form(device, "mistral-7b-q4km", dict(hidden=1024, inter=1024, vocab=1024), [512, 513, 4096, 8192], 1 << 30, fused, long)


@pytest.mark.watchdog(600)
def test_f32_cache_head_dim_64_generic_kernel(device):
    """GGUF at head_dim 64 (tiny-q4km): the generic k_attn_decode<64, F32>, 256-row tiles; no fused or split form at any context"""
    only = ({"attn_decode"}, {"attn_split", "attn_merge", "attn+o_proj<q4_K>", "attn+o_proj"})
    _run_form(device, "tiny-q4km", {}, [255, 256, 257, 4096], 1 << 30, only, only)


# ------------------------------------------------------------------------------------------------------------------------------------------
# graph replay == eager, bit for bit, with the split variant captured for a capacity above 16 384
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.watchdog(600)
@pytest.mark.parametrize("cap", [8192, 20480])
def test_graph_replay_equals_eager_bit_for_bit(device, cap):
    """the long-context graph variant is captured with a grid for `cap` positions; the eager step sizes its grid for position + 1.  Both must
    slice the live context the same way: their f32 merges then agree bit for bit."""
    model = synth.make_llama("llama3-8b-awq-2l", n_layers=1, hidden=2048, inter=1024, vocab=1024, max_seq_len=cap)
    cfg = model["config"]
    lm = runtime.LoadedModel.from_synth(device, model)
    rng = np.random.default_rng(3)
    seed_pos, steps = 600, 20
    K = orc_py.round_act(rng.standard_normal((seed_pos, cfg["n_kv_heads"], 128)).astype(np.float32), "f16")
    V = orc_py.round_act(rng.standard_normal((seed_pos, cfg["n_kv_heads"], 128)).astype(np.float32), "f16")
    caches = [runtime.LayeredKvCache(device, 1, 1, cfg["n_kv_heads"], cap, cap, 128, L.F16) for _ in range(2)]
    tk, tv = device.zeros((cfg["n_kv_heads"], 128)), device.zeros((cfg["n_kv_heads"], 128))
    for kv in caches:
        for p in range(seed_pos):
            tk.copy_from(K[p])
            tv.copy_from(V[p])
            L.check(L.lib().bz_kv_insert(lm.h, kv.h, 0, p, tk.h, tv.h))
    eager, tok = [], TOKEN
    for i in range(steps):
        lg = lm.forward_with_kv_cache([tok], caches[0], seed_pos + i).to_numpy().reshape(-1)
        eager.append(lg)
        tok = int(lg.argmax())
    g = runtime.DecodeGraph(lm, caches[1])
    g.seed_next_token(TOKEN, seed_pos)
    for i in range(steps):
        g.replay()
        got = g.read_logits()
        assert np.array_equal(got, eager[i]), (cap, i, float(np.abs(got - eager[i]).max()))


# ------------------------------------------------------------------------------------------------------------------------------------------
# paged == contiguous over a long batched prompt
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.watchdog(600)
@pytest.mark.parametrize("n", [4096, 16385])
def test_paged_equals_contiguous_long_prompt(device, n):
    """the batched prompt path through a scattered block table is bit-identical to the contiguous cache, and so is the decode step after it
    (split-KV at these contexts)"""
    model = synth.make_llama("tiny-bf16", n_heads=8, n_kv_heads=2, head_dim=128, n_layers=1, max_seq_len=n + 16)
    cfg = model["config"]
    lm = runtime.LoadedModel.from_synth(device, model)
    p = synth.prompt_tokens(n, cfg["vocab"], seed=n)
    bs = 16
    nb = (n + 1 + bs - 1) // bs
    kv = runtime.LayeredKvCache(device, 1, 1, 2, n + 1, cfg["max_seq_len"], 128, L.BF16)
    pk = runtime.LayeredPagedKvCache(device, 1, nb + 3, bs, 2, 128, L.BF16)
    blocks = list(np.random.default_rng(n).permutation(nb + 3)[:nb])
    pk.set_blocks(blocks)
    a = lm.forward_with_kv_cache(p, kv, 0).to_numpy()
    pk.set_seq_len(n)
    b = lm.forward_with_paged_kv_cache(p, pk, pk.compute_slot_mapping(0, n), blocks, n, 0).to_numpy()
    assert np.array_equal(a, b)
    tok = int(a.reshape(-1).argmax())
    a2 = lm.forward_with_kv_cache([tok], kv, n).to_numpy()
    pk.set_seq_len(n + 1)
    b2 = lm.forward_with_paged_kv_cache([tok], pk, pk.compute_slot_mapping(n, 1), blocks, n + 1, n).to_numpy()
    assert np.array_equal(a2, b2)


# ------------------------------------------------------------------------------------------------------------------------------------------
# prompt chunks at large offsets over injected caches
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.watchdog(600)
@pytest.mark.parametrize("pos0", [4000, 8150])
def test_prompt_chunk_at_large_offset_mfma(device, pos0):
    """S = 40 rows through the batched prompt path (MFMA flash attention) after pos0 injected rows: every row against the oracle at the suite's
    prompt bar (test_gpu_llama.py: relative L2 2x 2^-7 for the tiny bf16 fixtures, max-norm 3x that)"""
    model = synth.make_llama("tiny-bf16", n_heads=8, n_kv_heads=2, head_dim=128, n_layers=1, max_seq_len=8192 + 64)
    inj = Injected(device, model, pos0, seed=pos0, capacity=pos0 + 40)
    try:
        p = synth.prompt_tokens(40, model["config"]["vocab"], seed=1)
        got = inj.lm.forward_with_kv_cache(p, inj.kv, pos0, all_logits=True).to_numpy()
        want = inj.om.forward_kv(p, inj.okv, pos0, all_logits=True)
        rel = 2 * 2.0 ** -7
        for i in range(40):
            e = _rel(got[i], want[i])
            assert e <= rel, (pos0, i, e)
            assert np.abs(got[i] - want[i]).max() <= 3 * rel * np.abs(want[i]).max(), (pos0, i)
    finally:
        inj.close()


@pytest.mark.watchdog(600)
@pytest.mark.parametrize("pos0", [4000, 8150])
def test_prompt_chunk_at_large_offset_exact_rows(device, monkeypatch, pos0):
    """S = 12 on an f16 int4 model (the exact prompt rows): every row against the oracle at the exact bar, and equal bit for bit to the decode
    step's row at the same position.  The comparison holds the decode on its single-launch attention (BZ_SPLIT_MIN out of reach): the exact
    prompt attention carries the oracle's exactly rounded sums, as that kernel does, while the split-KV decode merges f32 partials and rounds
    differently.  At 8 150 the exact prompt attention cannot hold the context's scores in LDS, and the chunk runs on the decode step instead."""
    monkeypatch.setenv("BZ_SPLIT_MIN", str(1 << 30))
    model = synth.make_llama("llama3-8b-awq-2l", n_layers=1, hidden=2048, inter=1024, vocab=1024, max_seq_len=8192 + 64)
    inj = Injected(device, model, pos0, seed=pos0, capacity=pos0 + 12)
    try:
        p = synth.prompt_tokens(12, model["config"]["vocab"], seed=2)
        rows = inj.lm.forward_with_kv_cache(p, inj.kv, pos0, all_logits=True).to_numpy()
        want = inj.om.forward_kv(p, inj.okv, pos0, all_logits=True)
        kv2 = runtime.LayeredKvCache(device, 1, 1, inj.nkv, 16, model["config"]["max_seq_len"], 128, L.F16)
        for q in range(pos0):
            inj.tk.copy_from(inj.K[q])
            inj.tv.copy_from(inj.V[q])
            L.check(L.lib().bz_kv_insert(inj.lm.h, kv2.h, 0, q, inj.tk.h, inj.tv.h))
        for i, t in enumerate(p):
            dec = inj.lm.forward_with_kv_cache([int(t)], kv2, pos0 + i).to_numpy().reshape(-1)
            assert _rel(rows[i], want[i]) <= EXACT_BAR, (pos0, i, _rel(rows[i], want[i]))
            assert np.array_equal(rows[i], dec), (pos0, i, float(np.abs(rows[i] - dec).max()))
    finally:
        inj.close()


# ------------------------------------------------------------------------------------------------------------------------------------------
# MLA exact decode (DeepSeek-V2) over injected latent caches
# ------------------------------------------------------------------------------------------------------------------------------------------
MLA_LABELS = {"mla_scores<exact>", "mla_weights<exact>", "mla_merge<exact>"}


@pytest.mark.watchdog(900)
@pytest.mark.parametrize("max_len", [8192, 20000])
@pytest.mark.parametrize("preset,over", [("tiny-dsv2", {}), ("deepseek-v2-lite", dict(vocab=1024))], ids=["tiny-dsv2", "v2-lite-widths"])
def test_mla_exact_decode_long_context(device, preset, over, max_len):
    """1-layer DeepSeek-V2 models: the latent rows of a real 4-token prompt read back equal to the oracle's (the layout injection relies on), then
    decode steps at contexts 650, 4 096 and 8 191 over injected latents: the exact three-launch MLA (8 slices sized from max_seq_len) against
    the oracle at the exact bar.  Two rows planted with latents +-64x a background row's move the oracle's logits by more than 20x that bar.
    (A decode step ends with the oracle's own row P and seq_len P + 1; the next, longer context re-injects every row before P.)"""
    model = synth.make_dsv2(preset, n_layers=1, max_seq_len=max_len, **over)
    cfg = model["config"]
    W = cfg["kv_lora_rank"] + cfg["rope_dim"]
    lm, om = runtime.LoadedModel.from_synth(device, model), orc_py.OrcDsv2(model)
    top = 8191
    kv, okc = lm.new_kv_cache(16), om.new_cache(top + 1)
    try:
        p = synth.prompt_tokens(4, cfg["vocab"], seed=3)
        for i, t in enumerate(p):
            lm.forward_with_kv_cache([int(t)], kv, i)
            om.forward([int(t)], okc, i)
        lat = orc_py.mla_rows(okc)
        assert np.array_equal(kv.read(0, 0, 0, 4), lat[0, :4])
        rng = np.random.default_rng(7)
        X = orc_py.round_act(rng.standard_normal((top, W)).astype(np.float32) * 0.5, cfg["act_dtype"])
        X[100] = orc_py.round_act(X[100] * 64, cfg["act_dtype"])      # +x and -x: one of the two scores high for every head
        X[101] = -X[100]
        tk, tv = device.zeros((1, W)), device.zeros((1, W))
        for q in range(top):
            tk.copy_from(X[q])
            L.check(L.lib().bz_kv_insert(lm.h, kv.h, 0, q, tk.h, tv.h))
        assert np.array_equal(kv.read(0, 0, 0, top), X)
        for ctx in (650, 4096, 8191):
            P = ctx - 1
            labels = {r["name"] for r in lm.profile_step(kv, TOKEN, P, iters=1)}
            assert MLA_LABELS <= labels, (ctx, labels)
            tk.copy_from(X[P])
            L.check(L.lib().bz_kv_insert(lm.h, kv.h, 0, P, tk.h, tv.h))
            lat[0, :P] = X[:P]
            okc.contents.seq_len = P
            g = lm.forward_with_kv_cache([TOKEN], kv, P).to_numpy().reshape(-1)
            o = np.asarray(om.forward([TOKEN], okc, P)).reshape(-1)
            lat[0, 100:102] = X[102:104]
            o_drop = np.asarray(om.forward([TOKEN], okc, P)).reshape(-1)
            lat[0, 100:102] = X[100:102]
            sens = _rel(o_drop, o)
            print("%s max_seq_len %d ctx %d: hip vs oracle %.3e (bar %.1e); planted-row sensitivity %.3e" % (preset, max_len, ctx, _rel(g, o), EXACT_BAR, sens))
            assert sens >= 20 * EXACT_BAR, (ctx, sens)
            assert _rel(g, o) <= EXACT_BAR, (ctx, _rel(g, o))
            tk.copy_from(X[P])
            L.check(L.lib().bz_kv_insert(lm.h, kv.h, 0, P, tk.h, tv.h))
    finally:
        orc_py.lib().orc_mla_cache_free(okc)


# ------------------------------------------------------------------------------------------------------------------------------------------
# RoPE tables at 131 072 positions
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rs", [None, dict(type="llama3", factor=32.0, low_freq_factor=1.0, high_freq_factor=4.0, original_max_position_embeddings=8192),
                                dict(type="yarn", factor=4.0, original_max_position_embeddings=32768)], ids=["none", "llama3", "yarn"])
def test_rope_tables_at_131072_positions(device, rs):
    """the product's tables equal the oracle's and npref's bit for bit (all three form the angle as an f32 product, as HF does)"""
    model = synth.make_llama("tiny-awq", n_layers=1, head_dim=128, n_heads=2, n_kv_heads=2, max_seq_len=131072, rope_scaling=rs, rope_theta=500000.0)
    cfg = model["config"]
    cos, sin = runtime.LoadedModel.from_synth(device, model).rope_caches()
    rc = orc_py.RopeCfg()
    orc_py._rope_cfg(cfg, rc)
    rc.head_dim, rc.max_pos = cfg["head_dim"], cfg["max_seq_len"]
    wc, ws = np.empty_like(cos), np.empty_like(sin)
    orc_py.lib().orc_rope_tables(orc_py.C.byref(rc), wc.ctypes.data_as(orc_py.C.c_void_p), ws.ctypes.data_as(orc_py.C.c_void_p))
    nc, ns = npref.rope_tables(cfg)
    assert cos.shape == (131072, 64)
    assert np.array_equal(cos, wc) and np.array_equal(sin, ws)
    assert np.array_equal(cos, nc) and np.array_equal(sin, ns)
