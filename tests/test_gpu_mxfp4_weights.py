"""MXFP4 weights on the device: read-back of every code under the scale codes at the edges, the refusals, the decode GEMV and the W4A16 GEMM against
float64, whole models against the CPU oracle on the exact f32 restatement (tests/mxfp4_cases.py restate_f32), the structural identities of the step, decode
batches and the request engine, and checkpoints loaded from disk."""
import json
import os
import subprocess

import numpy as np
import pytest

import mxfp4_cases as M
from blazr_amd import _lib as L
from blazr_amd import runtime, synth
from oracle import orc_py
from test_gpu_engine import _drive
from test_gpu_llama import TINY, _check_logits, _fair_prefix, _kv_dt

pytestmark = pytest.mark.gpu

DOWN = "model.layers.0.mlp.down_proj.weight"
_PTR = lambda a: a.ctypes.data_as(orc_py.C.c_void_p)


def _op_model(device, spec, act="bf16"):
    """the smallest Llama-family model whose down_proj is the [N, K] linear `spec` (hidden N, inter K, one layer, one head); everything else dense"""
    N, K = spec["N"], spec["K"]
    cfg = dict(arch="llama", hidden=N, n_layers=1, n_heads=1, n_kv_heads=1, head_dim=64, inter=K, vocab=64, rms_eps=1e-5, rope_theta=10000.0,
               act_dtype=act, quant="none", max_seq_len=64, tie_embeddings=True)
    model = synth.make_llama(cfg)
    model["layers"][0]["down"] = spec
    return runtime.LoadedModel.from_synth(device, model)


def _ulp(v, act):
    """one rounding interval of the activation dtype at |v|"""
    a = np.maximum(np.abs(np.asarray(v, dtype=np.float64)), 1e-300)
    e = np.floor(np.log2(a))
    if act == "f16":
        return np.exp2(np.maximum(e, -14.0) - 10.0)
    return np.exp2(np.maximum(e, -126.0) - 7.0)


# ---- 1. bz_dequant on every code ----------------------------------------------------------------------------------------------------------
def test_dequant_reads_back_every_code(device):
    """[64, 1024], the smallest shape the call admits that has two tiles per row: every block pairs all sixteen codes in both nibble positions (an even and an
    odd element each), under the scale codes {0, 1, 104, 115, 127, 140, 252} -- f32 subnormals at the low end, 6 . 2^125 at the high.  Pins the nibble order,
    the expansion and the tile layout (row r of a group of four, block b of a tile of sixteen)."""
    N, K = 64, 1024
    rng = np.random.default_rng(4)
    codes = np.empty((N, K), np.uint8)
    for n in range(N):
        for b in range(K // 32):
            blk = np.concatenate([rng.permutation(16), rng.permutation(16)]).astype(np.uint8)
            if (n + b) % 2:
                blk = np.roll(blk, 1)                    # every code meets an even and an odd position over the rows
            codes[n, 32 * b:32 * b + 32] = blk
    pool = np.array([0, 1, 104, 115, 127, 140, 252], np.uint8)
    scale = pool[(np.arange(N)[:, None] * 3 + np.arange(K // 32)[None, :]) % 7]
    for c in range(16):
        assert ((codes[:, 0::2] == c).any() and (codes[:, 1::2] == c).any())
    assert set(scale.reshape(-1).tolist()) == set(pool.tolist())
    spec = M.spec_of(codes, scale)
    lm = _op_model(device, spec)
    got = lm.dequant(DOWN)
    want = M.weight_f64(spec).astype(np.float32)
    assert np.array_equal(want.astype(np.float64), M.weight_f64(spec))
    assert np.array_equal(got, want)
    assert np.array_equal(np.signbit(got), np.signbit(want))          # -0 reads back as -0
    res, per_tok = lm.weight_bytes()
    assert per_tok >= N * (K // 2 + K // 32) and res >= N * (K // 2 + K // 32)     # K/2 + K/32 bytes per row (the other linears and the head come on top)


# ---- 2. refusals -----------------------------------------------------------------------------------------------------------------------------
def _add(lm, name, N, K, w, s, b=None):
    w, s = np.ascontiguousarray(w, np.uint8), np.ascontiguousarray(s, np.uint8)
    rc = L.lib().bz_model_add_mxfp4(lm.h, name.encode(), N, K, _PTR(w), _PTR(s), None if b is None else _PTR(np.ascontiguousarray(b, np.float32)))
    return rc, L.lib().bz_last_error().decode()


@pytest.mark.parametrize("case", ["N%64", "K%64", "scale-255", "scale-253"])
def test_add_mxfp4_refusals_name_the_tensor(device, case):
    lm = runtime.LoadedModel(device, synth.make_config("tiny-mxfp4"))
    name = "model.layers.0.mlp.down_proj.weight"
    N, K = (96, 128) if case == "N%64" else (128, 96) if case == "K%64" else (128, 128)
    w = np.zeros((N, K // 2), np.uint8)
    s = np.full((N, K // 32), 120, np.uint8)
    want = L.E_UNSUPPORTED
    if case == "scale-255":
        s[100, 3] = 255
        want = L.E_INVALID
    elif case == "scale-253":
        s[N - 1, K // 32 - 1] = 253
    rc, msg = _add(lm, name, N, K, w, s)
    assert rc == want and name in msg, (rc, msg)
    rc, _ = _add(lm, name, 128, 128, np.zeros((128, 64), np.uint8), np.full((128, 4), 252, np.uint8))      # nothing was kept of the refused tensor; 252 is admitted
    assert rc == L.OK


@pytest.mark.parametrize("arch", ["mamba2", "deepseek2"])
def test_mxfp4_tensors_outside_the_llama_family_are_refused_at_finalize(device, arch):
    cfg = synth.make_mamba_config("tiny-mamba2") if arch == "mamba2" else synth.make_dsv2_config("tiny-dsv2")
    lm = runtime.LoadedModel(device, cfg)
    name = "backbone.layers.0.mixer.out_proj.weight" if arch == "mamba2" else "model.layers.0.self_attn.o_proj.weight"
    rc, _ = _add(lm, name, 256, 512, np.zeros((256, 256), np.uint8), np.full((256, 16), 127, np.uint8))
    assert rc == L.OK
    rc = L.lib().bz_model_finalize(lm.h)
    msg = L.lib().bz_last_error().decode()
    assert rc == L.E_UNSUPPORTED and name in msg, (rc, msg)


# ---- 3. the decode kernel against float64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["bf16", "f16"])
@pytest.mark.parametrize("N,K", M.GEMV_SHAPES)
def test_quant_matmul_is_the_rounded_float64_product(device, N, K, act):
    """Bar (the exact GEMVs' op bar): every output within one rounding interval of the activation dtype of R_act(f32(float64 value) + b), at most 1 % of
    the outputs not identical.  Weights: e2m1_encode of N(0, 0.02).  k_gemv_mx4 has the direct form only (no split-K form exists to force)."""
    rng = np.random.default_rng(N + K)
    x = synth._repr(rng.standard_normal((2, K)).astype(np.float32), act)
    base = M.quantised(N, K, N * 7 + K)
    w64 = M.weight_f64(base)
    for bias in (None, synth._repr(rng.standard_normal(N).astype(np.float32), act)):
        spec = dict(base, bias=bias)
        lm = _op_model(device, spec, act)
        got = lm.quant_matmul(DOWN, x)
        ref = (x.astype(np.float64) @ w64.T).astype(np.float32)
        if bias is not None:
            ref = ref + bias
        want, gr = orc_py.round_act(ref, act), orc_py.round_act(got, act)
        diff = np.abs(gr.astype(np.float64) - want.astype(np.float64))
        nd = int((gr != want).sum())
        print("gemv_mx4 [%d, %d] %s bias=%s: %d of %d outputs differ, max %.3g intervals" % (N, K, act, bias is not None, nd, want.size, float((diff / _ulp(want, act)).max())))
        assert (diff <= _ulp(want, act)).all()
        assert nd <= want.size // 100


# ---- 4. the GEMM against float64 --------------------------------------------------------------------------------------------------------------
_GEMM = {}
WIDE_SHAPE = (192, 704)


def _gemm_models(device, N, K, act):
    """models of one shape and dtype, built once: the dense 16-bit tensor holding W (the parent commit's GEMM, the yardstick) and the same W as MXFP4 under
    the scale codes 115 .. 121 (2^-12 .. 2^-6: every value exact in f16 and in bf16); for WIDE_SHAPE also an MXFP4 tensor whose every row mixes the scale
    codes 97 .. 127 (2^-30 .. 2^0), most of which f16 cannot hold"""
    if (N, K, act) not in _GEMM:
        rng = np.random.default_rng(N + 3 * K)
        codes = rng.integers(0, 16, size=(N, K), dtype=np.uint8)
        narrow = M.spec_of(codes, rng.integers(115, 122, size=(N, K // 32), dtype=np.uint8))
        wd = M.weight_f64(narrow).astype(np.float32)
        assert np.array_equal(synth._repr(wd, "bf16"), wd) and np.array_equal(synth._repr(wd, "f16"), wd)      # exact in both 16-bit dtypes: the same matrix
        dense = dict(kind="dense", N=N, K=K, weight=synth._store(wd, act))
        wide = None
        if (N, K) == WIDE_SHAPE:
            sc = np.stack([rng.permutation(np.arange(97, 128))[:K // 32] for _ in range(N)]).astype(np.uint8)
            sc[:, 0], sc[:, 1] = 127, 97                                                                      # every row holds both ends
            wide = M.spec_of(codes, sc)
        _GEMM[(N, K, act)] = (_op_model(device, dense, act), _op_model(device, narrow, act), narrow, None if wide is None else _op_model(device, wide, act), wide)
    return _GEMM[(N, K, act)]


def _prefill_matmul(device, lm, x, N):
    tx, ty = device.tensor(x), device.zeros((x.shape[0], N))
    L.check(L.lib().bz_prefill_matmul(lm.h, DOWN.encode(), tx.h, x.shape[0], ty.h))
    return ty.to_numpy().astype(np.float64)


def _err(got, x64, w64):
    return float((np.abs(got - x64 @ w64.T) / (np.abs(x64) @ np.abs(w64).T)).max())


@pytest.mark.parametrize("act", ["bf16", "f16"])
@pytest.mark.parametrize("S", M.GEMM_ROWS)
@pytest.mark.parametrize("N,K", M.GEMM_SHAPES)
def test_prefill_matmul_stays_within_twice_the_dense_gemm_error(device, N, K, S, act):
    """No tolerance fixed in advance: the parent's bz_prefill_matmul on the dense 16-bit tensor holding the same W sets it.  Largest element error against
    float64, normalised by sum_k |x_k| |W_nk|; the MXFP4 GEMM stays within 2 x that.  On WIDE_SHAPE the wide-range tensor is held to the same yardstick."""
    ld, ln, narrow, lw, wide = _gemm_models(device, N, K, act)
    x = synth._repr(np.random.default_rng(S * 1000 + N).standard_normal((S, K)).astype(np.float32), act)
    x64 = x.astype(np.float64)
    e_dense = _err(_prefill_matmul(device, ld, x, N), x64, M.weight_f64(narrow))
    e_mx4 = _err(_prefill_matmul(device, ln, x, N), x64, M.weight_f64(narrow))
    e_wide = _err(_prefill_matmul(device, lw, x, N), x64, M.weight_f64(wide)) if lw is not None else 0.0
    print("gemm_mx4w %s S=%d [%d, %d]: dense %.3e, mxfp4 %.3e, mxfp4 wide-range %.3e" % (act, S, N, K, e_dense, e_mx4, e_wide))
    assert e_dense > 0.0
    assert e_mx4 <= 2.0 * e_dense
    assert e_wide <= 2.0 * e_dense


# ---- 5. whole model, decode, against the oracle on the restatement ---------------------------------------------------------------------------
_MODELS = {}


def _pair(device, name):
    if name not in _MODELS:
        model = M.make(name)
        _MODELS[name] = (model, runtime.LoadedModel.from_synth(device, model), orc_py.OrcLlama(M.restate_f32(model)))
    return _MODELS[name]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize("name", list(M.MODELS))
def test_mxfp4_llama_decode_is_the_oracle_on_the_restatement(device, name):
    """The protocol and bar of test_fp8_llama_decode_is_the_oracle_on_the_restatement: a prompt of 12 tokens (short prompts stay on the decode kernels), then 12
    teacher-forced steps; at most 1 logit in 10 000 differing, relative L2 <= 1e-5, greedy ids equal over the fair prefix."""
    model, lm, om = _pair(device, name)
    cfg = model["config"]
    p = [int(t) for t in synth.prompt_tokens(12, cfg["vocab"], seed=51)]
    kv = runtime.LayeredKvCache(device, cfg["n_layers"], 1, cfg["n_kv_heads"], 32, cfg["max_seq_len"], cfg["head_dim"], _kv_dt(cfg))
    okv = om.new_kv(32)
    got = [lm.forward_with_kv_cache(p, kv, 0, all_logits=True).to_numpy().reshape(12, -1)]
    want = [om.forward_kv(p, okv, 0, all_logits=True).reshape(12, -1)]
    tok = int(want[0][-1].argmax())
    ids_got, ids_want = [], []
    for i in range(12):
        got.append(lm.forward_with_kv_cache([tok], kv, 12 + i).to_numpy().reshape(1, -1))
        want.append(om.forward_kv([tok], okv, 12 + i).reshape(1, -1))
        ids_got.append(int(got[-1][0].argmax())); ids_want.append(int(want[-1][0].argmax()))
        tok = ids_want[-1]
    orc_py.lib().orc_kv_free(okv)
    got, want = np.concatenate(got), np.concatenate(want)
    ndiff, rel = int((got != want).sum()), _rel(got, want)
    print("%s: %d of %d logits differ, rel L2 %.2e" % (name, ndiff, got.size, rel))
    hard = (1e-3 if cfg["act_dtype"] == "f16" else 1.25 * 2.0 ** -7) * (2.0 if cfg["hidden"] == 256 else 1.0)
    assert rel <= hard
    n = _fair_prefix(want[12:])
    assert ids_got[:n] == ids_want[:n]
    assert ndiff <= got.size // 10000 and rel <= 1e-5


# ---- 6. structure -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny-mxfp4-bf16", "tiny-mxfp4-f16"])
def test_graph_eager_paged_and_pieces_are_the_same_bits(device, name):
    model, lm, _ = _pair(device, name)
    cfg = model["config"]
    p = synth.prompt_tokens(12, cfg["vocab"], seed=8)
    mk = lambda: runtime.LayeredKvCache(device, cfg["n_layers"], 1, cfg["n_kv_heads"], 32, cfg["max_seq_len"], cfg["head_dim"], _kv_dt(cfg))
    # eager: prompt, then 6 greedy steps
    kv = mk()
    mono = lm.forward_with_kv_cache(p, kv, 0, all_logits=True).to_numpy()
    toks, eager = [int(mono[-1].argmax())], []
    for i in range(6):
        eager.append(lm.forward_with_kv_cache([toks[-1]], kv, 12 + i).to_numpy()[0])
        toks.append(int(eager[-1].argmax()))
    # pieces: head(layers(embed(x))), the layer range split in two
    kv2 = mk()
    h = lm.forward_embed(p)
    h, pm = lm.forward_layers_range(h, None, kv2, 0, 1, 0)
    h, pm = lm.forward_layers_range(h, pm, kv2, 1, cfg["n_layers"], 0)
    assert np.array_equal(mono, lm.forward_head(h, pm, all_logits=True).to_numpy())
    # graph: the captured step over the cache the eager prompt filled
    kv3 = mk()
    lm.forward_with_kv_cache(p, kv3, 0)
    g = runtime.DecodeGraph(lm, kv3)
    g.seed_next_token(toks[0], 12)
    for i in range(6):
        g.replay()
        assert np.array_equal(g.read_logits(), eager[i]), i
        assert g.read_token(i) == toks[i + 1]
    # paged: scattered blocks of 4, prompt and steps, eager and captured
    pk = runtime.LayeredPagedKvCache(device, cfg["n_layers"], 9, 4, cfg["n_kv_heads"], cfg["head_dim"], _kv_dt(cfg))
    pk.set_blocks([7, 2, 5, 0, 8, 3, 1])
    pk.set_seq_len(12)
    b = lm.forward_with_paged_kv_cache(p, pk, pk.compute_slot_mapping(0, 12), pk.block_table_device_format(), 12, 0, all_logits=True).to_numpy()
    assert np.array_equal(mono, b)
    for i in range(3):
        pk.set_seq_len(13 + i)
        lg = lm.forward_with_paged_kv_cache([toks[i]], pk, pk.compute_slot_mapping(12 + i, 1), pk.block_table_device_format(), 13 + i, 12 + i).to_numpy()[0]
        assert np.array_equal(lg, eager[i]), i
    ex = runtime.Executor(lm)
    runs = [ex.generate(p, 12, use_graph=gr, paged=pg).tolist() for gr in (False, True) for pg in (False, True)]
    assert runs[0] == runs[1] == runs[2] == runs[3] and runs[0][:7] == toks


@pytest.mark.parametrize("name", list(M.MODELS))
def test_prompt_of_40_rows_takes_the_batched_path(device, name):
    """40 rows > BZ_EXACT_PREFILL_MAX: route ROWS -- the W4A16 GEMMs and the MFMA attention; every row within the MFMA-prompt bar of DESIGN 5 (1e-3 f16,
    1.25 2^-7 bf16, twice that at hidden 256) against the oracle restatement"""
    model, lm, om = _pair(device, name)
    cfg = model["config"]
    tr = runtime.prompt_traits(lm)
    assert tr.proj_16 and tr.any_dense
    assert runtime.prompt_plan(tr, L.PLAN_PROMPT, 40, 40, _kv_dt(cfg))["route"] == L.ROUTE_ROWS
    assert runtime.prompt_plan(tr, L.PLAN_DECODE_BATCH, 4, 40, _kv_dt(cfg))["route"] == L.ROUTE_ROWS
    p = synth.prompt_tokens(40, cfg["vocab"], seed=13)
    kv = runtime.LayeredKvCache(device, cfg["n_layers"], 1, cfg["n_kv_heads"], 64, cfg["max_seq_len"], cfg["head_dim"], _kv_dt(cfg))
    okv = om.new_kv(64)
    got, want = lm.forward_with_kv_cache(p, kv, 0, all_logits=True).to_numpy(), om.forward_kv(p, okv, 0, all_logits=True)
    hard = (1e-3 if cfg["act_dtype"] == "f16" else 1.25 * 2.0 ** -7) * (TINY if cfg["hidden"] == 256 else 1.0)
    worst = max(_rel(got[r], want[r]) for r in range(40))
    print("%s: 40-row prompt, worst row rel L2 %.3e (bar %.3e)" % (name, worst, hard))
    assert worst <= hard
    # the decode steps that follow read the cache the batched rows wrote
    tok = int(want[-1].argmax())
    for i in range(3):
        lg, lo = lm.forward_with_kv_cache([tok], kv, 40 + i).to_numpy(), om.forward_kv([tok], okv, 40 + i)
        assert _rel(lg, lo) <= hard
        tok = int(lo[0].argmax())
    orc_py.lib().orc_kv_free(okv)
    # and the profile of a step names the new kernel
    names = [k["name"] for k in lm.profile_step(kv, 1, 43)]
    assert sum(n.startswith("gemv_mx4") for n in names) >= 3, names       # q/k/v and gate/up (norm), o_proj (plain), down_proj (silu)


def test_four_row_paged_batch_matches_the_per_sequence_oracle(device):
    model, lm, om = _pair(device, "tiny-mxfp4-bf16")
    cfg = model["config"]
    nseq, bs, per = 4, 16, 4
    pool = runtime.LayeredPagedKvCache(device, cfg["n_layers"], nseq * per, bs, cfg["n_kv_heads"], cfg["head_dim"], _kv_dt(cfg))
    tables = [[i + nseq * j for j in range(per)] for i in range(nseq)]
    prompts = [synth.prompt_tokens(3 + (11 * i) % 40, cfg["vocab"], seed=40 + i) for i in range(nseq)]
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


def test_engine_run_gives_each_request_its_own_greedy_tokens(device):
    """tests/test_gpu_engine.py's protocol: 4 rows, 6 requests of 8 tokens coming and going; every request's tokens equal those of its alone run on an engine of
    the same configuration, and the oracle restatement's on the fair prefix."""
    model, lm, om = _pair(device, "tiny-mxfp4-bf16")
    V = model["config"]["vocab"]
    prompts = [synth.prompt_tokens(3 + (13 * i) % 30, V, seed=70 + i) for i in range(6)]
    mk = lambda: runtime.BatchEngine(lm, 4, 4 * 5 + 4, 16, 80, 0, 2, False)
    ids, res, _ = _drive(mk(), [(0 if i < 4 else 2 + i, dict(prompt=p, max_tokens=8)) for i, p in enumerate(prompts)])
    for i, rid in enumerate(ids):
        (aid,), ares, _ = _drive(mk(), [(0, dict(prompt=prompts[i], max_tokens=8))])
        assert res[rid]["tokens"] == ares[aid]["tokens"] and len(res[rid]["tokens"]) == 8 and res[rid]["reason"] == 0, i
        want, trace = om.generate(prompts[i], 8, trace=True)
        n = _fair_prefix(trace)
        assert res[rid]["tokens"][:n] == want[:n].tolist(), (i, n)


# ---- 7. checkpoints ---------------------------------------------------------------------------------------------------------------------------
def _logits(device, lm, cfg, p):
    kv = runtime.LayeredKvCache(device, cfg["n_layers"], 1, cfg["n_kv_heads"], 32, cfg["max_seq_len"], cfg["head_dim"], _kv_dt(cfg))
    out = [lm.forward_with_kv_cache(p, kv, 0, all_logits=True).to_numpy()]
    tok = int(out[0][-1].argmax())
    for i in range(4):
        out.append(lm.forward_with_kv_cache([tok], kv, len(p) + i).to_numpy())
        tok = int(out[-1][0].argmax())
    return np.concatenate(out)


@pytest.mark.parametrize("bias", [False, True], ids=["plain", "bias"])
def test_checkpoint_round_trip(device, tmp_path, bias):
    """a Quark-style directory: U8 weights and scales, lm_head on the exclude list (untied, 16-bit), FP4 activations in input_tensors (ignored)"""
    model = synth.make_llama("tiny-mxfp4", tie_embeddings=False, bias=bias)
    cfg = model["config"]
    assert (model["layers"][0]["q"]["bias"] is not None) == bias
    M.write_mxfp4_checkpoint(str(tmp_path), model)
    a, b = runtime.load_model(device, str(tmp_path)), runtime.LoadedModel.from_synth(device, model)
    assert a.c.act_dtype == L.BF16
    p = synth.prompt_tokens(12, cfg["vocab"], seed=5)
    assert np.array_equal(_logits(device, a, cfg, p), _logits(device, b, cfg, p))
    assert a.weight_bytes() == b.weight_bytes()


def test_loader_refusals_on_files(device, tmp_path):
    model = synth.make_llama("tiny-mxfp4", tie_embeddings=False)
    # the config branch: every refusal names its field
    for name, qc, field in M.loader_refusals():
        d = tmp_path / name
        M.write_mxfp4_checkpoint(str(d), model, quant_config=qc)
        with pytest.raises(L.BlazrHipError) as ex:
            runtime.load_model(device, str(d))
        assert ex.value.code == L.E_UNSUPPORTED and field in str(ex.value), (name, str(ex.value))
    # the tensor branch: a scale tensor of the wrong shape, and a weight without its scales, name the layer
    good = tmp_path / "good"
    M.write_mxfp4_checkpoint(str(good), model)
    cfgj = open(str(good / "config.json")).read()
    base = "model.layers.0.mlp.down_proj"
    for case, edit in (("scale-shape", lambda t: t.__setitem__(base + ".weight_scale", np.full((256, 8), 120, np.uint8))),
                       ("no-scale", lambda t: t.pop(base + ".weight_scale")),
                       ("scale-255", lambda t: t.__setitem__(base + ".weight_scale", np.full((256, 16), 255, np.uint8)))):
        t = {base + ".weight": np.zeros((256, 256), np.uint8), base + ".weight_scale": np.full((256, 16), 120, np.uint8)}
        edit(t)
        d = tmp_path / case
        d.mkdir()
        M.write_safetensors(str(d / "model.safetensors"), t)
        (d / "config.json").write_text(cfgj)
        with pytest.raises(L.BlazrHipError) as ex:
            runtime.load_model(device, str(d))
        assert ex.value.code == L.E_INVALID and base in str(ex.value), (case, str(ex.value))


# ---- 8. bz-run -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graphs", [False, True])
def test_bz_run_prints_the_oracle_restatements_ids(device, tmp_path, graphs):
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "blazr_amd", "bz-run")
    assert os.path.exists(exe), "bz-run was not built (python -c 'import __graft_entry__ as g; g.build()')"
    model = synth.make_llama("tiny-mxfp4", tie_embeddings=False)
    M.write_mxfp4_checkpoint(str(tmp_path), model)
    want, trace = orc_py.OrcLlama(M.restate_f32(model)).generate([1, 2, 3], 16, trace=True)
    n = _fair_prefix(trace)
    r = subprocess.run([exe, str(tmp_path), "--prompt", "1,2,3", "--max-tokens", "16"] + (["--graphs"] if graphs else []), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in r.stdout.strip().split("\n")[-1].replace(",", " ").split()]
    assert n >= 4 and got[:n] == want[:n].tolist() and len(got) == 16, (r.stdout, want.tolist(), n)
