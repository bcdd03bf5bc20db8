"""The model shapes real checkpoints have, not only powers of two: tests/irregular_cases.py through the C ABI against the CPU oracle.

Every other Llama-family fixture of the suite has hidden 256 / 2048 / 4096 / 8192, a GQA group of 1 / 2 / 4 / 8 and a vocabulary that is a multiple of
64; the dispatch code sends everything else to fallbacks (or to fast paths at odd tile counts) that no test had reached.  Here: GQA groups of 3 / 6 / 7
(single-launch attention at every context, prompts token by token, decode batches sequence by sequence), widths 384 / 768 / 896 with 5 / 7 / 11 groups
or superblocks along K and 6 / 12 / 20 / 22 column tiles along N, ragged vocabularies (1001 / 1003 / 1027 rows through the row GEMV, the fused argmax,
the MFMA prompt GEMM and the batched-decode head), and the head_dims that are not built (refused at bz_model_finalize).

What each case launched in one decode step at position 8, and at position 269 under BZ_SPLIT_MIN=4: profiles/step_census.json holds the kernel names and
launch counts bz_profile_step reported on an MI355X (scripts/step_census.py takes the record), tests/test_step_plan.py holds the layer plan to them without a
device (awq-g3, bf16-g3-hd64, bf16-g2-w768, gptq-g6, q4km-g3 and q8_0-g7 by name), and tests/test_gpu_step_plan.py holds a loaded model's step to its plan.
`test_kernels_each_case_reached` prints the names (with launch counts, under `-s`) and asserts the entries the reasoning above depends on: no fused
attention + o_proj / MLP launch on the shapes those kernels are not built for (hidden 384 / 768 / 896), the slim SILU GEMV on q4km-g3's down projection.  With
BZ_SPLIT_MIN=4 at position 269 the rep-3 cases still report `attn_decode`, and bf16-g2-w768 reports `attn_split` + `attn_merge` in its place
(test_long_context_token_by_token).

Tolerances are the suite's own: logits at 2 x REL[act] (test_gpu_llama.py TINY: the rule for narrow fixtures), op-level bounds as in tests/test_gpu_ops.py /
test_gpu_llama.py, ids bit-exact on the oracle's fair prefix.
"""
import ctypes as C

import numpy as np
import pytest

from blazr_amd import _lib as L
from blazr_amd import runtime, synth
from oracle import orc_py
import irregular_cases as ic
import npref
from fullwidth_cases import OrcRun
from test_gpu_llama import TINY, _check_logits, _fair_prefix, _kv_dt

pytestmark = pytest.mark.gpu

ALL = list(ic.CASES)
_MODELS, _ORC = {}, {}


def _model(device, name):
    """(synth model, LoadedModel, OrcLlama) of a case, built once per session"""
    if name not in _MODELS:
        m = ic.make(name)
        _MODELS[name] = (m, runtime.LoadedModel.from_synth(device, m), orc_py.OrcLlama(m))
    return _MODELS[name]


def _orc(key, fn):
    """oracle results are computed once and shared by the tests that need them"""
    if key not in _ORC:
        _ORC[key] = fn()
    return _ORC[key]


def _kv(device, cfg, cap=16):
    return runtime.LayeredKvCache(device, cfg["n_layers"], 1, cfg["n_kv_heads"], cap, cfg["max_seq_len"], cfg["head_dim"], _kv_dt(cfg))


class _GpuRun:
    """fullwidth_cases.GpuRun's interface over the session's LoadedModel of a case: GpuRun itself loads and repacks the model again on every use, and
    teacher_forced needs the ids up front while test (a) takes each next id from the oracle's row, so neither is used as it is"""

    def __init__(self, device, lm, cfg):
        self.lm, self.kv, self.pos = lm, _kv(device, cfg), 0

    def forward(self, toks, all_logits=False):
        toks = [int(t) for t in toks]
        out = self.lm.forward_with_kv_cache(toks, self.kv, self.pos, all_logits=all_logits)
        self.pos += len(toks)
        return out.to_numpy()


def _labels(lm, kv, tok, pos):
    return {r["name"] for r in lm.profile_step(kv, tok, pos, iters=1)}


@pytest.fixture
def split_min(monkeypatch):
    def _set(n):
        monkeypatch.setenv("BZ_SPLIT_MIN", str(n))      # read per call
    return _set


# ---------------------------------------------------------------------------------------------------------
# (a) logits at the bar
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_logits_prefill_and_decode_at_the_bar(device, name):
    """the protocol of test_gpu_fullwidth.py: a 6-token prompt (token by token: the decode kernels), 8 teacher-forced steps, a 20-token second chunk
    (the batched prompt path where the shape has one: bf16-g2-w768, awq-g4-w768; token by token for the odd groups), one more step -- every row of
    logits at 2 x REL[act], the suite's rule for narrow fixtures (test_gpu_llama.py:21-23)"""
    model, lm, _ = _model(device, name)
    cfg = model["config"]
    act = cfg["act_dtype"]
    g, o = _GpuRun(device, lm, cfg), OrcRun("llama", model, cap=64)
    p = synth.prompt_tokens(6, cfg["vocab"], seed=2)
    want, got = o.forward(p, all_logits=True), g.forward(p, all_logits=True)
    assert got.shape == want.shape == (6, cfg["vocab"])
    _check_logits(got, want, act, factor=TINY)
    tok = int(want[-1].argmax())
    for _ in range(8):
        lo, lg = o.forward([tok]), g.forward([tok])
        _check_logits(lg.reshape(-1), lo.reshape(-1), act, factor=TINY)
        tok = int(lo.reshape(-1).argmax())
    p2 = synth.prompt_tokens(20, cfg["vocab"], seed=9)
    _check_logits(g.forward(p2, all_logits=True), o.forward(p2, all_logits=True), act, factor=TINY)
    lo, lg = o.forward([tok]), g.forward([tok])
    _check_logits(lg.reshape(-1), lo.reshape(-1), act, factor=TINY)
    orc_py.lib().orc_kv_free(o.state)


# ---------------------------------------------------------------------------------------------------------
# (b) greedy ids
# ---------------------------------------------------------------------------------------------------------
def _fair_prompt(om, vocab, plen, ntok, need, seeds):
    """first prompt seed whose oracle run has no near-tie in its first `need` steps (deterministic): (prompt, oracle ids, fair prefix)"""
    n = 0
    for seed in seeds:
        p = synth.prompt_tokens(plen, vocab, seed=seed)
        want, trace = om.generate(p, ntok, trace=True)
        n = _fair_prefix(trace)
        if n >= need:
            break
    assert n >= need, "no prompt seed gives a fair fixture"
    return p, want, n


@pytest.mark.parametrize("mode", ["eager", "graph", "paged", "paged-graph"])
@pytest.mark.parametrize("name", ALL)
def test_greedy_ids(device, name, mode):
    model, lm, om = _model(device, name)
    p, want, n = _orc(("ids", name), lambda: _fair_prompt(om, model["config"]["vocab"], 12, 24, 8, range(3, 40)))
    got = runtime.Executor(lm).generate(p, 24, use_graph="graph" in mode, paged="paged" in mode)
    assert got[:n].tolist() == want[:n].tolist(), (name, mode, got.tolist(), want.tolist(), n)
    assert len(got) == len(want)


# ---------------------------------------------------------------------------------------------------------
# (c) long context on shapes the split kernels do not take
# ---------------------------------------------------------------------------------------------------------
# bf16-g3-hd64: k_attn2<head_dim 64> at rep 3 across its 256-row chunk; bf16-g2-w768 takes the split path: the control
LONG = ["bf16-g3-hd128", "awq-g3", "q4km-g3", "bf16-g3-hd64", "bf16-g2-w768"]
LONG_ROWS = (0, 1, 17, 127, 128, 129, 255, 256, 257, 269)


@pytest.mark.parametrize("name", LONG)
def test_long_context_token_by_token(device, split_min, name):
    """270 positions token by token with the split threshold at 4: across the 128-position slice boundary of the split-KV kernels and the 256-row chunk of
    k_attn2 / k_attn2f.  The rep-3 shapes must stay on the single-launch attention (`attn_decode`, never `attn_split` / `attn_merge`); the rep-2 control
    must take `attn_split` -- asserted by kernel name, so that neither half passes because its path was skipped"""
    model, lm, om = _model(device, name)
    cfg = model["config"]
    split_min(4)
    n = 270
    p = synth.prompt_tokens(n, cfg["vocab"], seed=5)

    def oracle_rows():
        okv = om.new_kv(n)
        w = np.asarray(om.forward_kv(p, okv, 0, all_logits=True))[list(LONG_ROWS)].copy()
        orc_py.lib().orc_kv_free(okv)
        return w
    want = _orc(("long", name), oracle_rows)
    kv = _kv(device, cfg, 8)
    for i in range(n):
        lg = lm.forward_with_kv_cache([int(p[i])], kv, i)
        if i in LONG_ROWS:
            _check_logits(lg.to_numpy()[0], want[LONG_ROWS.index(i)], cfg["act_dtype"], factor=TINY)
    labels = _labels(lm, kv, int(p[-1]), n - 1)
    if name in ic.ODD_GROUP:
        assert "attn_decode" in labels and not any(l.startswith(("attn_split", "attn_merge")) for l in labels), (name, sorted(labels))
    else:
        assert "attn_split" in labels and any(l.startswith("attn_merge") for l in labels) and "attn_decode" not in labels, (name, sorted(labels))


@pytest.mark.parametrize("mode", ["graph", "paged-graph"])
@pytest.mark.parametrize("name", LONG)
def test_long_context_generate_modes_agree(device, split_min, name, mode):
    """9 + 40 tokens in graph and paged-graph mode under the setting of the token-by-token test, BZ_SPLIT_MIN=4: every replayed step is beyond the threshold, and
    a captured graph sizes its grid for the capacity, so a rep-3 model must still replay the single-launch attention.  Ids equal the eager ids with the
    threshold out of reach, on the oracle's fair prefix.  (A replayed graph cannot be profiled by kernel name: that the control's steps beyond the threshold
    launch `attn_split` is asserted in test_long_context_token_by_token; here the control shows that the two attention paths agree in ids)"""
    model, lm, om = _model(device, name)
    p, _, k = _orc(("long-ids", name), lambda: _fair_prompt(om, model["config"]["vocab"], 9, 40, 16, range(3, 60)))
    ex = runtime.Executor(lm)

    def eager():
        split_min(100000)
        return ex.generate(p, 40, use_graph=False)
    base = _orc(("long-eager", name), eager)
    split_min(4)
    got = ex.generate(p, 40, use_graph=True, paged="paged" in mode)
    assert got[:k].tolist() == base[:k].tolist(), (name, mode, got.tolist(), base.tolist(), k)


# ---------------------------------------------------------------------------------------------------------
# (d) which kernels each case reached
# ---------------------------------------------------------------------------------------------------------
NO_FUSED_LAUNCH = ["bf16-g3-hd64", "bf16-g3-hd128", "awq-g3", "q4km-g3"]     # the cases the issue lists as "refused"


@pytest.mark.parametrize("name", ALL)
def test_kernels_each_case_reached(device, name):
    model, lm, _ = _model(device, name)
    cfg = model["config"]
    p = synth.prompt_tokens(8, cfg["vocab"], seed=2)
    kv = _kv(device, cfg)
    for i, t in enumerate(p):
        lm.forward_with_kv_cache([int(t)], kv, i)
    prof = lm.profile_step(kv, 5, 8, iters=1)
    labels = {r["name"] for r in prof}
    print("%s: %s" % (name, ", ".join("%s x%d" % (r["name"], r["launches"]) for r in sorted(prof, key=lambda r: r["name"]))))
    if name in NO_FUSED_LAUNCH:
        assert not any(l.startswith(("attn+o_proj", "attn_merge+o_proj", "mlp_")) for l in labels), (name, sorted(labels))
        assert "attn_decode" in labels, (name, sorted(labels))
    if name in ic.ODD_GROUP:
        assert not any(l.startswith(("attn_split", "attn_merge")) for l in labels), (name, sorted(labels))
    if name == "q4km-g3":
        # down projection: Q4_K in layer 0, Q6_K in layer 1 (the Q4_K_M rule), both on the slim kernel's SILU form at 5 superblocks; q/k/v and gate/up
        # (K = 768: no slim NORM instantiation) on the generic kernel
        assert {"gemv_q4_K<slim>", "gemv_q6_K<slim>"} <= labels and "gemv_q4_K" in labels, sorted(labels)
    if name in ("awq-g3", "awq-g7", "awq-g4-w768", "gptq-g6"):
        assert any(l.startswith("gemv_q4g") for l in labels) and not any("slim" in l for l in labels), (name, sorted(labels))
    if name == "q8_0-g7":
        assert "gemv_q8_0" in labels, sorted(labels)


# ---------------------------------------------------------------------------------------------------------
# (e) batched decode
# ---------------------------------------------------------------------------------------------------------
def _batch_fixture(cfg, nseq, per, bs=16):
    tables = [[i + nseq * j for j in range(per)] for i in range(nseq)]            # interleaved physical blocks
    plens = [3 + (11 * i) % 40 for i in range(nseq)]                              # unequal lengths
    prompts = [synth.prompt_tokens(n, cfg["vocab"], seed=40 + i) for i, n in enumerate(plens)]
    return tables, plens, prompts


@pytest.mark.parametrize("name,nseq", [("awq-g3", 3), ("bf16-g3-hd64", 10), ("bf16-g2-w768", 3), ("bf16-g2-w768", 10), ("awq-g4-w768", 10), ("q4km-g3", 3)])
def test_batched_paged_decode_matches_per_sequence_oracle(device, name, nseq):
    """the protocol of test_gpu_llama.py::test_batched_paged_decode_matches_per_sequence_oracle.  Odd groups run the batch sequence by sequence; bf16-g2-w768
    and awq-g4-w768 take the weight-sharing multi-row step (8-row passes at 3 sequences, the MFMA GEMMs at 10) at 12 / 20 / 22 column tiles and a ragged head"""
    model, lm, om = _model(device, name)
    cfg = model["config"]
    bs, per = 16, 4
    pool = runtime.LayeredPagedKvCache(device, cfg["n_layers"], nseq * per, bs, cfg["n_kv_heads"], cfg["head_dim"], _kv_dt(cfg))
    tables, plens, prompts = _batch_fixture(cfg, nseq, per)
    okvs, toks, lens = [], [], []
    for p, tb in zip(prompts, tables):
        slots = [tb[i // bs] * bs + i % bs for i in range(len(p))]
        lg = lm.forward_with_paged_kv_cache(p, pool, slots, tb, len(p), 0).to_numpy()
        okv = om.new_kv(64)
        lo = om.forward_kv(p, okv, 0)
        _check_logits(lg, lo, cfg["act_dtype"])
        okvs.append(okv); toks.append(int(lo[0].argmax())); lens.append(len(p))
    for step in range(5):
        lens = [n + 1 for n in lens]
        slots = [tb[(n - 1) // bs] * bs + (n - 1) % bs for n, tb in zip(lens, tables)]
        got = lm.forward_paged_batch(toks, pool, slots, [tb[:(n + bs - 1) // bs] for n, tb in zip(lens, tables)], lens).to_numpy()
        nxt = []
        for i in range(nseq):
            lo = om.forward_kv([toks[i]], okvs[i], lens[i] - 1)
            _check_logits(got[i:i + 1], lo, cfg["act_dtype"])
            nxt.append(int(lo[0].argmax()))
        toks = nxt
    for okv in okvs:
        orc_py.lib().orc_kv_free(okv)


@pytest.mark.parametrize("name,nseq", [("bf16-g3-hd64", 4), ("awq-g3", 4), ("q4km-g3", 3), ("bf16-g2-w768", 4), ("bf16-g2-w768", 10), ("awq-g4-w768", 4),
                                       ("awq-g4-w768", 10)])
def test_batched_decode_graph(device, name, nseq):
    """bz_decode_batch_graph_capture: a model whose group the multi-row step is not built for either is refused with BZ_E_UNSUPPORTED or replays to the eager
    batch's logits; bf16-g2-w768 and awq-g4-w768 MUST capture (the capture needs prefill_eligible: the same predicate sends their decode batches and prompts to
    the multi-row pipeline, so a shape that quietly fell back to per-sequence execution fails here), and their replays equal the eager batched step bit for bit
    (logits and the device-side argmax over 1003 / 1001 rows)"""
    model, lm, _ = _model(device, name)
    cfg = model["config"]
    bs, per, steps = 16, 4, 6
    tables, plens, prompts = _batch_fixture(cfg, nseq, per)

    def fresh_pool():
        return runtime.LayeredPagedKvCache(device, cfg["n_layers"], nseq * per, bs, cfg["n_kv_heads"], cfg["head_dim"], _kv_dt(cfg))

    def prefill(pool):
        first = []
        for p, tb in zip(prompts, tables):
            slots = [tb[i // bs] * bs + i % bs for i in range(len(p))]
            first.append(int(lm.forward_with_paged_kv_cache(p, pool, slots, tb, len(p), 0).to_numpy()[0].argmax()))
        return first
    pool_b = fresh_pool()
    try:
        g = runtime.BatchDecodeGraph(lm, pool_b, nseq, per)
    except L.BlazrHipError as e:
        assert name in ic.ODD_GROUP, (name, str(e))
        assert e.code == L.E_UNSUPPORTED, str(e)
        return
    pool_a = fresh_pool()
    toks, lens = prefill(pool_a), list(plens)
    eager_ids, eager_logits = [], []
    for _ in range(steps):
        lens = [n + 1 for n in lens]
        slots = [tb[(n - 1) // bs] * bs + (n - 1) % bs for n, tb in zip(lens, tables)]
        lg = lm.forward_paged_batch(toks, pool_a, slots, tables, lens).to_numpy()
        toks = [int(r.argmax()) for r in lg]
        eager_ids.append(list(toks)); eager_logits.append(lg)
    first = prefill(pool_b)
    g.seed(first, [n + 1 for n in plens], tables)
    for s in range(steps):
        g.replay()
        assert np.array_equal(g.read_logits(), eager_logits[s]), "graph step %d differs from the eager batched step" % s
    for s in range(steps):
        assert g.read_tokens(s).tolist() == eager_ids[s], s


# ---------------------------------------------------------------------------------------------------------
# (f) op level, layer 1 of every case
# ---------------------------------------------------------------------------------------------------------
def _names(i):
    p = "model.layers.%d." % i
    return {"q": p + "self_attn.q_proj.weight", "k": p + "self_attn.k_proj.weight", "v": p + "self_attn.v_proj.weight",
            "o": p + "self_attn.o_proj.weight", "gate": p + "mlp.gate_proj.weight", "up": p + "mlp.up_proj.weight",
            "down": p + "mlp.down_proj.weight"}


@pytest.mark.parametrize("name", ALL)
def test_dequant_bit_exact(device, name):
    """the load-time repack at 3 / 5 / 7 / 11 groups or superblocks along K and 6 .. 22 column tiles along N is lossless"""
    model, lm, _ = _model(device, name)
    for short, wname in _names(1).items():
        want = orc_py.OrcLinear(model["layers"][1][short]).dequant()
        got = lm.dequant(wname)
        assert got.shape == want.shape and np.array_equal(got, want), (name, short, float(np.abs(got - want).max()))
    if not model["config"].get("tie_embeddings"):
        assert np.array_equal(lm.dequant("lm_head.weight"), orc_py.OrcLinear(model["lm_head"]).dequant()), name


@pytest.mark.parametrize("short", ["q", "k", "o", "gate", "down"])
@pytest.mark.parametrize("name", ALL)
def test_matmul_vs_oracle(device, name, short):
    """the decode GEMV of each projection (generic k_gemv_q4g / k_gemv_gq with choose_sbw on odd superblock counts / k_gemv_rows2 balancing a matrix that is
    no power of two) against the oracle's linear.  Tolerances: those of test_gpu_ops.py::test_quant_matmul_vs_oracle (int4, f16 inputs: 2e-6) and
    test_gguf_matmul_vs_oracle (block formats, f32 inputs: 3e-6); dense 16-bit weights carry exact sums on both sides and take the int4 bound"""
    model, lm, _ = _model(device, name)
    spec = model["layers"][1][short]
    gguf = spec["kind"] == "gguf"
    rng = np.random.default_rng(6 if gguf else 5)
    x = rng.standard_normal((3, spec["K"])).astype(np.float32)
    if not gguf:
        x = orc_py.round_act(x, model["config"]["act_dtype"])
    x[1] *= 50.0 if gguf else 37.0          # large dynamic range
    x[2, ::5 if gguf else 7] = 0.0
    want = orc_py.OrcLinear(spec).forward(x)
    got = lm.quant_matmul(_names(1)[short], x)
    tol = (3e-6 if gguf else 2e-6) * np.abs(want).max() + 1e-7
    assert got.shape == want.shape and np.abs(got - want).max() <= tol, (name, short, float(np.abs(got - want).max()), tol)


@pytest.mark.parametrize("S", [9, 33, 130])
def test_prefill_matmul_ragged_and_odd_tiles(device, S):
    """the MFMA prompt GEMMs as test_gpu_llama.py::test_prefill_matmul_mfma / _q4g_mfma check theirs: the ragged dense head [1003, 768] (15 full column
    tiles of 64 and one of 43 rows) and awq-g4-w768's gate [1280, 768] (20 column tiles, 3 k-steps of 256)"""
    rng = np.random.default_rng(500 + S)
    for name, wname, spec_of, dt in (("bf16-g3-hd128", "lm_head.weight", lambda m: m["lm_head"], "bf16"),
                                     ("awq-g4-w768", "model.layers.0.mlp.gate_proj.weight", lambda m: m["layers"][0]["gate"], "f16")):
        model, lm, _ = _model(device, name)
        W = npref.dequant(spec_of(model)).astype(np.float64)
        N, K = W.shape
        assert (N, K) == ((1003, 768) if dt == "bf16" else (1280, 768))
        x = rng.standard_normal((S, K)).astype(np.float32)
        tx, ty = device.tensor(x), device.tensor(np.full((S + 1, N), 7.0, np.float32))     # one guard row behind the output
        L.check(L.lib().bz_prefill_matmul(lm.h, wname.encode(), tx.h, S, ty.h))
        want = orc_py.round_act(x, dt).astype(np.float64) @ W.T
        got = ty.to_numpy()
        assert np.all(got[S] == 7.0), (name, S, "the GEMM wrote behind its last row")
        assert np.abs(got[:S] - want).max() <= 3e-6 * np.abs(want).max(), (name, S, float(np.abs(got[:S] - want).max()), float(np.abs(want).max()))


ATTN_FIXTURES = ["bf16-g3-hd64", "bf16-g3-hd128", "awq-g3", "awq-g7", "gptq-g6", "q4km-g3", "q8_0-g7"]     # groups of 3 / 6 / 7
# one step of the activation grid at the top of the range, twice (test_kv_insert_and_attention: 2^-9 for f16 = 2 x 2^-10); f32 rows are not rounded to a coarser
# grid, what remains there is the order of the f32 normalisation: 8 x 2^-23
ATTN_TOL = {"f16": 2.0 ** -9, "bf16": 2.0 ** -6, "f32": 2.0 ** -20}


@pytest.mark.parametrize("name", ATTN_FIXTURES)
def test_kv_insert_and_attention(device, name):
    """bz_kv_insert + bz_attn_decode against orc_attn_decode at lengths 1, 63, 64, 65, 257, `kvh = hq / rep` with rep 3 / 6 / 7: the asserts of
    test_gpu_ops.py::test_kv_insert_and_attention.  The op-level entry passes a finished q (no RoPE row), so the kernels reached are k_attn2<head_dim 128> for
    bf16-g3-hd128 and awq-g3 (256-row chunks) and the one-thread-per-position k_attn_decode for the rest (head_dim 64, and every f32 cache).  k_attn2<64> and
    k_attn2f at an odd group beyond 256 rows are reached end to end, by test_long_context_token_by_token (bf16-g3-hd64, q4km-g3)"""
    model, lm, _ = _model(device, name)
    cfg = model["config"]
    act, nq, nkv, hd = cfg["act_dtype"], cfg["n_heads"], cfg["n_kv_heads"], cfg["head_dim"]
    rep = nq // nkv
    assert rep in (3, 6, 7)
    total = 257
    rng = np.random.default_rng(total + rep)
    kv = _kv(device, cfg, 8)                                           # grows on demand
    K = orc_py.round_act(rng.standard_normal((total, nkv, hd)).astype(np.float32), act)
    V = orc_py.round_act(rng.standard_normal((total, nkv, hd)).astype(np.float32), act)
    tk, tv = device.zeros((nkv, hd)), device.zeros((nkv, hd))
    for p in range(total):
        tk.copy_from(K[p]); tv.copy_from(V[p])
        L.check(L.lib().bz_kv_insert(lm.h, kv.h, 1, p, tk.h, tv.h))
    for h in range(nkv):   # byte-exact round trip through the cache
        assert np.array_equal(kv.read(1, h, 0, total), K[:, h]) and np.array_equal(kv.read(1, h, 1, total), V[:, h])
    for length in (1, 63, 64, 65, 257):
        q = orc_py.round_act(rng.standard_normal((nq, hd)).astype(np.float32), act)
        out, tq = device.zeros((nq, hd)), device.tensor(q)
        L.check(L.lib().bz_attn_decode(lm.h, tq.h, kv.h, 1, length, out.h))
        want = np.empty((nq, hd), np.float32)
        for h in range(nkv):
            kc, vc = np.ascontiguousarray(K[:length, h]), np.ascontiguousarray(V[:length, h])
            qq = np.ascontiguousarray(q[h * rep:(h + 1) * rep])
            o = np.empty((rep, hd), np.float32)
            orc_py.lib().orc_attn_decode(qq.ctypes.data_as(C.c_void_p), rep, hd, kc.ctypes.data_as(C.c_void_p), vc.ctypes.data_as(C.c_void_p),
                                         hd, length, 1.0 / np.sqrt(hd), o.ctypes.data_as(C.c_void_p))
            want[h * rep:(h + 1) * rep] = o
        want = orc_py.round_act(want, act)
        err = float(np.abs(out.to_numpy() - want).max())
        assert err <= ATTN_TOL[act] * max(float(np.abs(want).max()), 1e-3), (name, length, err)


# ---------------------------------------------------------------------------------------------------------
# (g) ragged argmax
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,V", [(2, 1003), (1, 1027)])
def test_argmax_over_a_ragged_vocabulary(device, rows, V):
    """bz_argmax_to_buf on a vocabulary that is no multiple of 64: the maximum at V - 1, at 1000, and an exact tie between V - 1 and 5 (the lowest index wins, as
    test_gpu_ops.py::test_logits_to_token_greedy_and_penalties pins).  The row in front carries a larger value at an index the last row must not see"""
    rng = np.random.default_rng(V)
    base = rng.standard_normal((rows, V)).astype(np.float32)
    if rows > 1:
        base[0, 77] = 100.0
    top = float(base[-1].max()) + 1.0
    for hot, want in (([V - 1], V - 1), ([1000], 1000), ([V - 1, 5], 5)):
        x = base.copy()
        x[-1, hot] = top
        t, tok = device.tensor(x), device.zeros((1,), L.I64)
        L.check(L.lib().bz_argmax_to_buf(device.h, t.h, rows, V, tok.h))
        assert int(tok.to_numpy()[0]) == want == int(np.argmax(x[-1])), (rows, V, hot)


def test_graph_replay_argmax_over_the_ragged_head(device):
    """the fused argmax of the lm_head launch (bzk_argmax_partials / bzk_argmax_final inside the captured step) on bf16-g3-hd64's 1003 rows: after every replay
    read_token equals np.argmax(read_logits).  A second model whose LAST head row is three times the row the first model picked must pick V - 1: the
    ragged tail of the last workgroup takes part in the argmax"""
    model, lm, _ = _model(device, "bf16-g3-hd64")
    cfg = model["config"]
    V = cfg["vocab"]
    p = synth.prompt_tokens(7, V, seed=21)

    def run(lm_, replays):
        kv = _kv(device, cfg)
        tok = int(lm_.forward_with_kv_cache(p, kv, 0).to_numpy()[0].argmax())
        g = runtime.DecodeGraph(lm_, kv)
        g.seed_next_token(tok, len(p))
        picks = []
        for s in range(replays):
            g.replay()
            lg = g.read_logits()
            assert g.read_token(s) == int(np.argmax(lg)), (s, g.read_token(s), int(np.argmax(lg)))
            picks.append((g.read_token(s), float(lg.max())))
        return picks
    picks = run(lm, 6)
    j, top = picks[0]
    assert top > 0.0 and j != V - 1
    m2 = dict(model, lm_head=dict(model["lm_head"], weight=model["lm_head"]["weight"].copy()))
    w = synth.bf16_bits_to_f32(m2["lm_head"]["weight"][j])
    m2["lm_head"]["weight"][V - 1] = synth.f32_to_bf16_bits(3.0 * w)
    assert run(runtime.LoadedModel.from_synth(device, m2), 1)[0][0] == V - 1


# ---------------------------------------------------------------------------------------------------------
# (h) shapes that are not built
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd", [96, 256])
def test_head_dims_that_are_not_built_are_refused_at_finalize(device, hd):
    """a Llama-arch model with head_dim 96 (Phi-3) or 256 (Gemma2) loaded and then failed in bzk_attn_decode at the first forward, after the q/k/v launches;
    bz_model_finalize refuses it now, naming head_dim, so nothing is launched for a model that cannot run"""
    model = synth.make_llama("tiny-bf16", head_dim=hd)
    with pytest.raises(L.BlazrHipError) as e:
        runtime.LoadedModel.from_synth(device, model)
    assert e.value.code == L.E_UNSUPPORTED and "head_dim" in str(e.value) and str(hd) in str(e.value), str(e.value)


def test_block_format_linear_with_half_a_superblock_is_refused(device):
    """the issue's q8_0-g7 outline (14q / 2kv x 64): o_proj K = 896 = 3.5 superblocks of 256.  Refused when the tensor is added, naming K (the loadable
    28q / 4kv form of the same group is the q8_0-g7 of every test above)"""
    preset, over = ic.Q8_0_G7_NOT_LOADABLE
    with pytest.raises(L.BlazrHipError) as e:
        runtime.LoadedModel.from_synth(device, synth.make_llama(preset, **over))
    assert e.value.code == L.E_UNSUPPORTED and "K=896" in str(e.value), str(e.value)
