"""FP8 (E4M3) weights on the device: read-back of every code, the refusals, the decode GEMV and the W8A16 GEMM against float64, whole models against the
CPU oracle on the exact f32 restatement (tests/fp8_cases.py restate_f32), the structural identities of the step, decode batches and the request engine, and
checkpoints loaded from disk."""
import os
import subprocess

import numpy as np
import pytest

import fp8_cases as F
from blazr_amd import _lib as L
from blazr_amd import runtime, synth
from oracle import orc_py
from test_gpu_engine import _drive
from test_gpu_llama import REL, TINY, _check_logits, _fair_prefix, _kv_dt

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


def _fp8_spec(N, K, scale, bias=None, codes=None, seed=0):
    return dict(kind="fp8", N=N, K=K, weight=F.random_codes(N, K, seed) if codes is None else codes, scale=np.asarray(scale, np.float32), bias=bias)


def _ulp(v, act):
    """one rounding interval of the activation dtype at |v|"""
    a = np.maximum(np.abs(np.asarray(v, dtype=np.float64)), 1e-300)
    e = np.floor(np.log2(a))
    if act == "f16":
        return np.exp2(np.maximum(e, -14.0) - 10.0)
    return np.exp2(np.maximum(e, -126.0) - 7.0)


# ---- 1. bz_dequant on every code ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy", ["channel", "tensor"])
def test_dequant_reads_back_every_code(device, strategy):
    N, K = 64, 256
    codes = F.random_codes(N, K, 11)
    codes[0, :254] = F.FINITE_CODES                 # the first row runs through 0x00 .. 0xFF minus the two NaN codes
    codes[1, :254] = F.FINITE_CODES[::-1]
    scale = F.bf16_scales(N, 12) if strategy == "channel" else F.bf16_scales(1, 13)
    lm = _op_model(device, _fp8_spec(N, K, scale, codes=codes))
    got = lm.dequant(DOWN)
    s64 = scale.astype(np.float64)
    want = (F.TABLE[codes].astype(np.float64) * (s64[:, None] if strategy == "channel" else s64[0])).astype(np.float32)      # f32(s . e4m3(q)), one rounding
    assert np.array_equal(got, want)
    assert np.array_equal(np.signbit(got[0, :254]), np.signbit(want[0, :254]))          # -0 reads back as -0
    res, per_tok = lm.weight_bytes()
    assert per_tok >= N * K + 4 * N                                                      # one byte per weight plus the scales


# ---- 2. refusals -----------------------------------------------------------------------------------------------------------------------------
def _add(lm, name, N, K, w, s, b=None):
    w, s = np.ascontiguousarray(w, np.uint8), np.ascontiguousarray(s, np.float32)
    rc = L.lib().bz_model_add_fp8(lm.h, name.encode(), N, K, _PTR(w), _PTR(s), s.size, None if b is None else _PTR(np.ascontiguousarray(b, np.float32)))
    return rc, L.lib().bz_last_error().decode()


@pytest.mark.parametrize("case", ["N%64", "K%64", "n_scale", "scale-inf", "scale-nan", "nan-code-7f", "nan-code-ff"])
def test_add_fp8_refusals_name_the_tensor(device, case):
    lm = runtime.LoadedModel(device, synth.make_config("tiny-fp8"))
    name = "model.layers.0.mlp.down_proj.weight"
    N, K = (96, 128) if case == "N%64" else (128, 96) if case == "K%64" else (128, 128)
    w = np.zeros((N, K), np.uint8)
    s = np.full(N, 2.0 ** -8, np.float32)
    want = L.E_INVALID
    if case in ("N%64", "K%64"):
        want = L.E_UNSUPPORTED
    elif case == "n_scale":
        s = s[:2]
    elif case == "scale-inf":
        s[5] = np.inf
    elif case == "scale-nan":
        s[7] = np.nan
    elif case == "nan-code-7f":
        w[100, 17] = 0x7F
    elif case == "nan-code-ff":
        w[N - 1, K - 1] = 0xFF
    rc, msg = _add(lm, name, N, K, w, s)
    assert rc == want and name in msg, (rc, msg)
    rc, _ = _add(lm, name, 128, 128, np.zeros((128, 128), np.uint8), np.full(128, 2.0 ** -8, np.float32))      # nothing was kept of the refused tensor
    assert rc == L.OK


@pytest.mark.parametrize("arch", ["mamba2", "deepseek2"])
def test_fp8_tensors_outside_the_llama_family_are_refused_at_finalize(device, arch):
    cfg = synth.make_mamba_config("tiny-mamba2") if arch == "mamba2" else synth.make_dsv2_config("tiny-dsv2")
    lm = runtime.LoadedModel(device, cfg)
    name = "backbone.layers.0.mixer.out_proj.weight" if arch == "mamba2" else "model.layers.0.self_attn.o_proj.weight"
    rc, _ = _add(lm, name, 256, 512, np.zeros((256, 512), np.uint8), np.ones(1, np.float32))
    assert rc == L.OK
    rc = L.lib().bz_model_finalize(lm.h)
    msg = L.lib().bz_last_error().decode()
    assert rc == L.E_UNSUPPORTED and name in msg, (rc, msg)


# ---- 3. the decode kernel against float64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["bf16", "f16"])
@pytest.mark.parametrize("N,K", F.GEMV_SHAPES)
def test_quant_matmul_is_the_rounded_float64_product(device, N, K, act):
    """Bar (the exact GEMVs' op bar): every output within one rounding interval of the activation dtype of R_act(f32(float64 value) + b), at most 1 % of
    the outputs not identical.  (256, 4096) and (64, 14336) run the split-K form, the others the direct one."""
    assert (F.choose_sk(N, K) > 1) == ((N, K) in ((256, 4096), (64, 14336)))
    rng = np.random.default_rng(N + K)
    x = synth._repr(rng.standard_normal((2, K)).astype(np.float32), act)
    for bias in (None, synth._repr(rng.standard_normal(N).astype(np.float32), act)):
        for scale in (F.bf16_scales(N, K), F.bf16_scales(1, K + 1)):
            spec = _fp8_spec(N, K, scale, bias=bias, seed=N * 7 + K)
            lm = _op_model(device, spec, act)
            got = lm.quant_matmul(DOWN, x)
            ref = (x.astype(np.float64) @ F.weight_f64(spec).T).astype(np.float32)
            if bias is not None:
                ref = ref + bias
            want, gr = orc_py.round_act(ref, act), orc_py.round_act(got, act)
            diff = np.abs(gr.astype(np.float64) - want.astype(np.float64))
            nd = int((gr != want).sum())
            print("gemv_f8 [%d, %d] %s bias=%s scales=%d: %d of %d outputs differ, max %.3g intervals" % (N, K, act, bias is not None, scale.size, nd, want.size, float((diff / _ulp(want, act)).max())))
            assert (diff <= _ulp(want, act)).all()
            assert nd <= want.size // 100


# ---- 4. the GEMM against float64 --------------------------------------------------------------------------------------------------------------
_GEMM = {}


def _gemm_models(device, N, K):
    """three models of one shape, built once: the dense bf16 tensor 2^e . e4m3(q) (the parent commit's GEMM), the same matrix as FP8 with the power-of-two
    scales, and the same bytes under general scales"""
    if (N, K) not in _GEMM:
        codes = F.random_codes(N, K, N + 3 * K)
        p2, gen = F.pow2_scales(N, N + K), F.bf16_scales(N, N + K + 1)
        wd = (F.TABLE[codes] * p2[:, None]).astype(np.float32)
        assert np.array_equal(synth._repr(wd, "bf16"), wd)                               # exact in bf16: the same matrix
        dense = dict(kind="dense", N=N, K=K, weight=synth._store(wd, "bf16"))
        sp, sg = _fp8_spec(N, K, p2, codes=codes), _fp8_spec(N, K, gen, codes=codes)
        _GEMM[(N, K)] = (_op_model(device, dense), _op_model(device, sp), _op_model(device, sg), sp, sg)
    return _GEMM[(N, K)]


def _prefill_matmul(device, lm, x, N):
    tx, ty = device.tensor(x), device.zeros((x.shape[0], N))
    L.check(L.lib().bz_prefill_matmul(lm.h, DOWN.encode(), tx.h, x.shape[0], ty.h))
    return ty.to_numpy().astype(np.float64)


@pytest.mark.parametrize("S", F.GEMM_ROWS)
@pytest.mark.parametrize("N,K", F.GEMM_SHAPES)
def test_prefill_matmul_stays_within_twice_the_dense_gemm_error(device, N, K, S):
    """No tolerance fixed in advance: the parent's bz_prefill_matmul on the dense bf16 tensor 2^e . e4m3(q) sets it.  Largest element error against float64,
    normalised by sum_k |x_k| |W_nk|; the FP8 GEMM with the same power-of-two scales and with general scales stays within 2 x that."""
    ld, lp, lg, sp, sg = _gemm_models(device, N, K)
    x = synth._repr(np.random.default_rng(S * 1000 + N).standard_normal((S, K)).astype(np.float32), "bf16")
    x64 = x.astype(np.float64)

    def err(got, w64):
        return float((np.abs(got - x64 @ w64.T) / (np.abs(x64) @ np.abs(w64).T)).max())

    e_dense = err(_prefill_matmul(device, ld, x, N), F.weight_f64(sp))
    e_pow2 = err(_prefill_matmul(device, lp, x, N), F.weight_f64(sp))
    e_gen = err(_prefill_matmul(device, lg, x, N), F.weight_f64(sg))
    print("gemm_f8w S=%d [%d, %d]: dense %.3e, fp8 pow2 %.3e, fp8 general %.3e" % (S, N, K, e_dense, e_pow2, e_gen))
    assert e_dense > 0.0
    assert e_pow2 <= 2.0 * e_dense and e_gen <= 2.0 * e_dense


# ---- 5. whole model, decode, against the oracle on the restatement ---------------------------------------------------------------------------
_MODELS = {}


def _pair(device, name):
    if name not in _MODELS:
        model = F.make(name)
        _MODELS[name] = (model, runtime.LoadedModel.from_synth(device, model), orc_py.OrcLlama(F.restate_f32(model)))
    return _MODELS[name]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize("name", list(F.MODELS))
def test_fp8_llama_decode_is_the_oracle_on_the_restatement(device, name):
    """Prompt of 12 tokens (short prompts stay on the decode kernels), then 12 steps.  The kernels carry exact sums and apply the scale once to the finished
    sum, which is the oracle's dense f32 linear on s . e4m3(q): held to the dense bar of test_dense_16bit_llama_is_the_oracle_bit_for_bit (at most 1 logit in
    10 000 differing, relative L2 <= 1e-5) -- inside the hard bar of DESIGN 5 (1e-3 f16 / 1.25 2^-7 bf16, twice that at hidden 256) by orders."""
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
@pytest.mark.parametrize("name", ["tiny-fp8-channel-bf16", "tiny-fp8-tensor-f16"])
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


def test_forced_split_k_step_is_the_direct_step(device, monkeypatch):
    """The tiny fixtures' rows are too short for the split rule, so the split-K form of k_gemv_f8 (unscaled partials in the ring, the finish in the launch, the
    row-block counters, the zeroing duty) is forced at finalize (BZ_F8_SPLITK) and must give the direct form's tokens and -- every row's sum being exact --
    logits, eager and captured."""
    model = F.make("fp8-g2-w768")
    cfg = model["config"]
    p = synth.prompt_tokens(9, cfg["vocab"], seed=21)
    out = {}
    for sk in ("0", "2", "3"):
        monkeypatch.setenv("BZ_F8_SPLITK", sk)
        lm = runtime.LoadedModel.from_synth(device, model)
        kv = runtime.LayeredKvCache(device, cfg["n_layers"], 1, cfg["n_kv_heads"], 32, cfg["max_seq_len"], cfg["head_dim"], _kv_dt(cfg))
        lg = lm.forward_with_kv_cache(p, kv, 0, all_logits=True).to_numpy()
        ex = runtime.Executor(lm)
        a, b, c = (ex.generate(p, 16, use_graph=True).tolist(), ex.generate(p, 16, use_graph=True).tolist(), ex.generate(p, 16, use_graph=False).tolist())
        assert a == b == c
        out[sk] = (lg, a)
    for sk in ("2", "3"):
        nd = int((out[sk][0] != out["0"][0]).sum())
        print("split %s vs direct: %d of %d logits differ" % (sk, nd, out["0"][0].size))
        assert nd <= out["0"][0].size // 10000 and out[sk][1] == out["0"][1]


@pytest.mark.parametrize("name", ["tiny-fp8-channel-bf16", "fp8-g2-w768"])
def test_prompt_of_40_rows_takes_the_batched_path(device, name):
    """40 rows > BZ_EXACT_PREFILL_MAX: the W8A16 GEMMs and the MFMA attention; every row within the MFMA-prompt bar of DESIGN 5 against the oracle restatement"""
    model, lm, om = _pair(device, name)
    cfg = model["config"]
    p = synth.prompt_tokens(40, cfg["vocab"], seed=13)
    kv = runtime.LayeredKvCache(device, cfg["n_layers"], 1, cfg["n_kv_heads"], 64, cfg["max_seq_len"], cfg["head_dim"], _kv_dt(cfg))
    okv = om.new_kv(64)
    got, want = lm.forward_with_kv_cache(p, kv, 0, all_logits=True).to_numpy(), om.forward_kv(p, okv, 0, all_logits=True)
    factor = TINY if cfg["hidden"] == 256 else 1.0
    for r in range(40):
        _check_logits(got[r:r + 1], want[r:r + 1], cfg["act_dtype"], factor)
    # the decode steps that follow read the cache the batched rows wrote
    tok = int(want[-1].argmax())
    for i in range(3):
        lg, lo = lm.forward_with_kv_cache([tok], kv, 40 + i).to_numpy(), om.forward_kv([tok], okv, 40 + i)
        _check_logits(lg, lo, cfg["act_dtype"], factor)
        tok = int(lo[0].argmax())
    orc_py.lib().orc_kv_free(okv)
    # and the profile of a step names the new kernel
    names = [k["name"] for k in lm.profile_step(kv, 1, 43)]
    assert sum(n.startswith("gemv_f8") for n in names) >= 3, names       # q/k/v and gate/up (norm), o_proj (plain), down_proj (silu)


def test_four_row_paged_batch_matches_the_per_sequence_oracle(device):
    model, lm, om = _pair(device, "tiny-fp8-channel-bf16")
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
    the same configuration (same kernels at the same N, a row depends on nothing in the other rows), and the oracle restatement's on the fair prefix."""
    model, lm, om = _pair(device, "tiny-fp8-channel-bf16")
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


@pytest.mark.parametrize("form,with_qc", [("compressed-tensors", True), ("fp8", True), ("fp8", False)], ids=["compressed-tensors", "fp8", "dtype-alone"])
def test_checkpoint_round_trip(device, tmp_path, form, with_qc):
    """compressed-tensors: channel scales as BF16 [N,1], lm_head on the ignore list, an input_scale beside every weight (ignored); "fp8": per-tensor F32 []
    scales; and the same file without a quantization_config (detected from the F8_E4M3 weight with its scale beside it).  Untied 16-bit lm_head."""
    name = "tiny-fp8-channel-bf16" if form == "compressed-tensors" else "tiny-fp8-tensor-bf16"
    preset, over = F.MODELS[name]
    model = synth.make_llama(preset, tie_embeddings=False, **over)
    cfg = model["config"]
    F.write_fp8_checkpoint(str(tmp_path), model, form, with_quant_config=with_qc)
    a, b = runtime.load_model(device, str(tmp_path)), runtime.LoadedModel.from_synth(device, model)
    assert a.c.act_dtype == L.BF16
    p = synth.prompt_tokens(12, cfg["vocab"], seed=5)
    assert np.array_equal(_logits(device, a, cfg, p), _logits(device, b, cfg, p))
    assert a.weight_bytes() == b.weight_bytes()


def test_loader_refusals(device, tmp_path):
    model = synth.make_llama("tiny-fp8", tie_embeddings=False)
    d = tmp_path / "inv"
    F.write_fp8_checkpoint(str(d), model, "compressed-tensors")
    # a block-scaled file ships .weight_scale_inv
    import json
    hdr = F.write_safetensors
    t = {"model.layers.0.mlp.down_proj.weight": F.F8(np.zeros((256, 512), np.uint8)), "model.layers.0.mlp.down_proj.weight_scale_inv": np.ones((2, 4), np.float32)}
    e = tmp_path / "blk"
    e.mkdir()
    hdr(str(e / "model.safetensors"), t)
    json.dump(json.load(open(str(d / "config.json"))), open(str(e / "config.json"), "w"))
    with pytest.raises(L.BlazrHipError) as ex:
        runtime.load_model(device, str(e))
    assert ex.value.code == L.E_UNSUPPORTED and "weight_scale_inv" in str(ex.value)
    # E5M2 is not read
    raw = open(str(d / "model.safetensors"), "rb").read()
    f = tmp_path / "e5m2"
    f.mkdir()
    (f / "model.safetensors").write_bytes(raw.replace(b"F8_E4M3", b"F8_E5M2"))
    json.dump(json.load(open(str(d / "config.json"))), open(str(f / "config.json"), "w"))
    with pytest.raises(L.BlazrHipError) as ex:
        runtime.load_model(device, str(f))
    assert ex.value.code == L.E_UNSUPPORTED and "F8_E5M2" in str(ex.value)


@pytest.mark.parametrize("graphs", [False, True])
def test_bz_run_prints_the_oracle_restatements_ids(device, tmp_path, graphs):
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "blazr_amd", "bz-run")
    assert os.path.exists(exe), "bz-run was not built (python -c 'import __graft_entry__ as g; g.build()')"
    model = synth.make_llama("tiny-fp8", tie_embeddings=False)
    F.write_fp8_checkpoint(str(tmp_path), model, "compressed-tensors")
    want, trace = orc_py.OrcLlama(F.restate_f32(model)).generate([1, 2, 3], 16, trace=True)
    n = _fair_prefix(trace)
    r = subprocess.run([exe, str(tmp_path), "--prompt", "1,2,3", "--max-tokens", "16"] + (["--graphs"] if graphs else []), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in r.stdout.strip().split("\n")[-1].replace(",", " ").split()]
    assert n >= 4 and got[:n] == want[:n].tolist() and len(got) == 16, (r.stdout, want.tolist(), n)
