"""GPU parity, op level: every kernel of the hot path against the CPU oracle, through the C-ABI.

Bars: bit-exact for integer/byte work (repack -> dequant round trip, KV insert/read, argmax ids);
fp tolerances are written at each assert.  The oracle is the checker only (see oracle/orc.h).
"""
import ctypes as C

import numpy as np
import pytest

from blazr_amd import _lib as L
from blazr_amd import runtime, synth
from oracle import orc_py

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiny_awq(device):
    model = synth.make_llama("tiny-awq")
    return model, runtime.LoadedModel.from_synth(device, model), orc_py.OrcLlama(model)


@pytest.fixture(scope="module")
def tiny_gptq(device):
    model = synth.make_llama("tiny-gptq", act_order=True, bias=True)
    return model, runtime.LoadedModel.from_synth(device, model), orc_py.OrcLlama(model)


@pytest.fixture(scope="module")
def tiny_q4km(device):
    model = synth.make_llama("tiny-q4km")
    return model, runtime.LoadedModel.from_synth(device, model), orc_py.OrcLlama(model)


@pytest.fixture(scope="module")
def tiny_q80(device):
    model = synth.make_llama("tiny-q8_0")
    return model, runtime.LoadedModel.from_synth(device, model), orc_py.OrcLlama(model)


def _names(i=0):
    p = "model.layers.%d." % i
    return {"q": p + "self_attn.q_proj.weight", "k": p + "self_attn.k_proj.weight", "v": p + "self_attn.v_proj.weight",
            "o": p + "self_attn.o_proj.weight", "gate": p + "mlp.gate_proj.weight", "up": p + "mlp.up_proj.weight",
            "down": p + "mlp.down_proj.weight"}


@pytest.mark.parametrize("fix", ["tiny_awq", "tiny_gptq"])
def test_repack_dequant_bit_exact(fix, request):
    """load-time repack (AWQ nibble order awq.rs:29-32 / GPTQ sequential + act-order) is lossless: dequantising the
    REPACKED HBM layout reproduces the oracle's dequant of the original tensors bit for bit."""
    model, lm, _ = request.getfixturevalue(fix)
    for short, name in _names(1).items():
        want = orc_py.OrcLinear(model["layers"][1][short]).dequant()
        got = lm.dequant(name)
        assert np.array_equal(got, want), (fix, short, np.abs(got - want).max())


@pytest.mark.parametrize("fix", ["tiny_q4km", "tiny_q80"])
def test_gguf_repack_dequant_bit_exact(fix, request):
    """GGML Q8_0 / Q4_K / Q6_K blocks -> kernel layout is lossless: dequantising the repacked HBM layout equals the
    oracle's ggml dequant of the raw blocks bit for bit (layer 0 of Q4_K_M carries Q6_K attn_v / ffn_down)."""
    model, lm, _ = request.getfixturevalue(fix)
    seen = set()
    for layer in (0, 1, 3):
        if layer >= model["config"]["n_layers"]:
            continue
        for short, name in _names(layer).items():
            spec = model["layers"][layer][short]
            seen.add(spec["ggml_type"])
            want = orc_py.OrcLinear(spec).dequant()
            got = lm.dequant(name)
            assert np.array_equal(got, want), (fix, layer, short, spec["ggml_type"], np.abs(got - want).max())
    want = orc_py.OrcLinear(model["lm_head"]).dequant()
    assert np.array_equal(lm.dequant("lm_head.weight"), want)
    assert seen == ({8} if fix == "tiny_q80" else {12, 14})


@pytest.mark.parametrize("fix", ["tiny_q4km", "tiny_q80"])
@pytest.mark.parametrize("short", ["q", "v", "gate", "down"])
def test_gguf_matmul_vs_oracle(fix, short, request):
    model, lm, _ = request.getfixturevalue(fix)
    spec = model["layers"][0][short]
    rng = np.random.default_rng(6)
    x = rng.standard_normal((3, spec["K"])).astype(np.float32)
    x[1] *= 50.0
    x[2, ::5] = 0.0
    want = orc_py.OrcLinear(spec).forward(x)
    got = lm.quant_matmul(_names(0)[short], x)
    # f32 activations through the 24-bit (per 32-k chunk) fixed-point split: |err| <= 2^-23 * chunk max per term
    tol = 3e-6 * np.abs(want).max() + 1e-7
    assert np.abs(got - want).max() <= tol, (np.abs(got - want).max(), tol)


@pytest.mark.parametrize("fix", ["tiny_awq", "tiny_gptq"])
@pytest.mark.parametrize("short", ["q", "k", "o", "gate", "down"])
def test_quant_matmul_vs_oracle(fix, short, request):
    model, lm, _ = request.getfixturevalue(fix)
    spec = model["layers"][0][short]
    rng = np.random.default_rng(5)
    x = rng.standard_normal((3, spec["K"])).astype(np.float16).astype(np.float32)
    x[1] *= 37.0          # large dynamic range
    x[2, ::7] = 0.0
    want = orc_py.OrcLinear(spec).forward(x)
    got = lm.quant_matmul(_names(0)[short], x)
    # the sums are exact (eight signed-nibble planes of the activation codes, integer group sums, doubles across groups); what is left is the op's accumulator grid:
    # f32 results take the 2^-32 fixed point, one rounding per workgroup, where the model's f16 steps take 2^-44
    tol = 2e-6 * np.abs(want).max() + 1e-7
    assert np.abs(got - want).max() <= tol, (np.abs(got - want).max(), tol)


@pytest.mark.parametrize("width,short", [("h2048", "o"), ("h2048", "down"), ("h4096", "k")])
def test_quant_matmul_bias_after_the_rounded_sum(device, width, short):
    """a biased GPTQ linear at real width, f16-exact inputs: |got - (RN32(exact sum) + bias)| <= 1 f32 ulp of the result (the bias is added in f32 to the
    sum's one rounding; the op's 2^-32 accumulator units leave no room for equality -- tests/test_gpu_linear_bias.py holds the f16 steps to that)"""
    import bias_cases as bc
    model = bc.make_model(width)
    spec = model["layers"][0][short]
    spec["bias"] = (np.random.default_rng(8).standard_normal(spec["N"]).astype(np.float32) * 0.01).astype(np.float16).astype(np.float32)
    lm = runtime.LoadedModel.from_synth(device, model)
    x = np.random.default_rng(5).standard_normal((3, spec["K"])).astype(np.float16).astype(np.float32)
    x[1] *= 8.0           # (a power of two: still f16 values)
    x[2, ::7] = 0.0
    got = lm.quant_matmul(_names(0)[short], x)
    worst = 0.0
    for r in range(3):
        want = bc.rn32(bc.exact_sums(dict(spec, bias=None), x[r])) + spec["bias"]
        assert np.array_equal(want, orc_py.OrcLinear(spec).forward(x[r])[0])
        ulps = np.abs(got[r].astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
        print("%s %s row %d: max |got - want| = %.3g f32 ulps of the result, %d of %d elements off" % (width, short, r, ulps.max(), int((ulps > 0).sum()), ulps.size))
        worst = max(worst, float(ulps.max()))
    assert worst <= 1.0, worst


def test_quant_matmul_edge_inputs(tiny_awq):
    model, lm, _ = tiny_awq
    spec = model["layers"][0]["gate"]
    name = _names(0)["gate"]
    K = spec["K"]
    ol = orc_py.OrcLinear(spec)
    for x in (np.zeros(K, np.float32), np.full(K, 65504.0, np.float32), np.full(K, -6.1e-5, np.float32),
              np.eye(1, K, 5, dtype=np.float32)[0] * 3.0):
        want = ol.forward(x)[0]
        got = lm.quant_matmul(name, x)[0]
        assert np.abs(got - want).max() <= 2e-6 * max(np.abs(want).max(), 1e-30) + 1e-12


def test_rms_norm(device):
    rng = np.random.default_rng(1)
    for act, adt in (("f16", L.F16), ("bf16", L.BF16), ("f32", L.F32)):
        n = 384
        x = orc_py.round_act(rng.standard_normal((2, n)).astype(np.float32) * 3, act)
        p = orc_py.round_act(rng.standard_normal((2, n)).astype(np.float32), act)
        w = orc_py.round_act(1 + 0.1 * rng.standard_normal(n).astype(np.float32), act)
        y, ho = device.zeros((2, n)), device.zeros((2, n))
        tx, tp, tw = device.tensor(x), device.tensor(p), device.tensor(w)   # keep the handles alive across the call
        L.check(L.lib().bz_rms_norm(device.h, tx.h, tp.h, tw.h, 2, n, 1e-5, adt, y.h, ho.h))
        h = orc_py.round_act(x + p, act)
        want = np.empty_like(h)
        for r in range(2):
            orc_py.lib().orc_rms_norm(h[r].ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), n, 1e-5, orc_py._DT[act],
                                      want[r].ctypes.data_as(C.c_void_p))
        assert np.array_equal(ho.to_numpy(), h)
        ulp = {"f16": 2 ** -10, "bf16": 2 ** -7, "f32": 1e-6}[act]
        assert np.abs(y.to_numpy() - want).max() <= ulp * np.abs(want).max()


def test_rope_tables_and_apply(tiny_awq, device):
    model, lm, om = tiny_awq
    cfg = model["config"]
    cos, sin = lm.rope_caches()
    rc = orc_py.RopeCfg()
    rc.head_dim, rc.max_pos, rc.theta, rc.scaling_type = cfg["head_dim"], cfg["max_seq_len"], cfg["rope_theta"], 0
    rc.factor, rc.low_freq_factor, rc.high_freq_factor, rc.original_max_pos = 1.0, 1.0, 4.0, 8192
    wc = np.empty_like(cos)
    ws = np.empty_like(sin)
    orc_py.lib().orc_rope_tables(C.byref(rc), wc.ctypes.data_as(C.c_void_p), ws.ctypes.data_as(C.c_void_p))
    assert np.array_equal(cos, wc) and np.array_equal(sin, ws)
    rng = np.random.default_rng(2)
    S, nh, hd = 3, cfg["n_heads"], cfg["head_dim"]
    x = rng.standard_normal((S, nh, hd)).astype(np.float16).astype(np.float32)
    t = device.tensor(x)
    L.check(L.lib().bz_rope(lm.h, t.h, S, nh, 11))
    want = x.copy()
    for s in range(S):
        for h in range(nh):
            v = want[s, h]
            orc_py.lib().orc_rope_apply(v.ctypes.data_as(C.c_void_p), hd, hd, wc[11 + s].ctypes.data_as(C.c_void_p),
                                        ws[11 + s].ctypes.data_as(C.c_void_p), 0)
    want = orc_py.round_act(want, "f16")
    assert np.abs(t.to_numpy() - want).max() <= 2 ** -10 * np.abs(want).max()


def test_silu_mul(device):
    rng = np.random.default_rng(3)
    g = (rng.standard_normal(1000) * 4).astype(np.float16).astype(np.float32)
    u = rng.standard_normal(1000).astype(np.float16).astype(np.float32)
    y = device.zeros((1000,))
    tg, tu = device.tensor(g), device.tensor(u)
    L.check(L.lib().bz_silu_mul(device.h, tg.h, tu.h, 1000, L.F16, y.h))
    want = orc_py.round_act(orc_py.round_act(g / (1 + np.exp(-g)), "f16") * u, "f16")
    assert np.abs(y.to_numpy() - want).max() <= 2 ** -9 * np.abs(want).max()


@pytest.mark.parametrize("length", [1, 2, 63, 64, 65, 200])
def test_kv_insert_and_attention(tiny_awq, device, length):
    model, lm, _ = tiny_awq
    cfg = model["config"]
    nq, nkv, hd = cfg["n_heads"], cfg["n_kv_heads"], cfg["head_dim"]
    rng = np.random.default_rng(length)
    kv = runtime.LayeredKvCache(device, cfg["n_layers"], 1, nkv, 8, cfg["max_seq_len"], hd, L.F16)  # grows on demand
    K = rng.standard_normal((length, nkv, hd)).astype(np.float16).astype(np.float32)
    V = rng.standard_normal((length, nkv, hd)).astype(np.float16).astype(np.float32)
    for p in range(length):
        tk, tv = device.tensor(K[p]), device.tensor(V[p])
        L.check(L.lib().bz_kv_insert(lm.h, kv.h, 1, p, tk.h, tv.h))
    for h in range(nkv):   # byte-exact round trip through the f16 cache
        assert np.array_equal(kv.read(1, h, 0, length), K[:, h])
        assert np.array_equal(kv.read(1, h, 1, length), V[:, h])
    q = rng.standard_normal((nq, hd)).astype(np.float16).astype(np.float32)
    out = device.zeros((nq, hd))
    tq = device.tensor(q)
    L.check(L.lib().bz_attn_decode(lm.h, tq.h, kv.h, 1, length, out.h))
    rep = nq // nkv
    want = np.empty((nq, hd), np.float32)
    for h in range(nkv):
        kc = np.ascontiguousarray(K[:, h])
        vc = np.ascontiguousarray(V[:, h])
        qq = np.ascontiguousarray(q[h * rep:(h + 1) * rep])
        o = np.empty((rep, hd), np.float32)
        orc_py.lib().orc_attn_decode(qq.ctypes.data_as(C.c_void_p), rep, hd, kc.ctypes.data_as(C.c_void_p), vc.ctypes.data_as(C.c_void_p),
                                     hd, length, 1.0 / np.sqrt(hd), o.ctypes.data_as(C.c_void_p))
        want[h * rep:(h + 1) * rep] = o
    want = orc_py.round_act(want, "f16")
    assert np.abs(out.to_numpy() - want).max() <= 2 ** -9 * max(np.abs(want).max(), 1e-3)


def test_logits_to_token_greedy_and_penalties(device):
    rng = np.random.default_rng(9)
    V = 5000
    logits = rng.standard_normal((2, V)).astype(np.float32)
    logits[1, 100] = logits[1, 4000] = logits[1].max() + 1.0      # exact tie: lowest index wins
    t = device.tensor(logits)
    tok = runtime.logits_to_token(device, t, [], []).to_numpy()[0]
    assert tok == 100
    # penalties (llama.cpp sign rule; unpinned in the reference, see oracle/orc_ops.c)
    hist = [100, 100, 4000, 7, 7, 7]
    ids, cnts = runtime.penalty_window(hist, 64)
    got = runtime.logits_to_token(device, t, ids, cnts, repeat_penalty=1.3, frequency_penalty=0.2, presence_penalty=0.1).to_numpy()[0]
    want = orc_py.lib().orc_logits_to_token(np.ascontiguousarray(logits[1]).ctypes.data_as(C.c_void_p), V, ids.ctypes.data_as(C.c_void_p),
                                            cnts.ctypes.data_as(C.c_void_p), len(ids), 1.3, 0.2, 0.1, 0.0, 0, 1.0, 0.0, 0)
    assert got == want
    with pytest.raises(L.BlazrHipError):
        runtime.logits_to_token(device, t, [], [], temperature=-1.0)


def _orc_sample(row, ids, cnts, rp, fp, pp, temp, top_k, top_p, min_p, seed):
    ids = np.asarray(ids, dtype=np.int64)
    cnts = np.asarray(cnts, dtype=np.int32)
    return orc_py.lib().orc_logits_to_token(np.ascontiguousarray(row).ctypes.data_as(C.c_void_p), len(row), ids.ctypes.data_as(C.c_void_p),
                                            cnts.ctypes.data_as(C.c_void_p), len(ids), rp, fp, pp, temp, top_k, top_p, min_p, seed)


@pytest.mark.parametrize("temp,top_k,top_p,min_p", [(1.0, 0, 1.0, 0.0), (0.7, 40, 0.9, 0.05), (1.3, 0, 0.8, 0.0), (0.5, 5, 1.0, 0.0), (1.0, 0, 1.0, 0.2)])
def test_logits_to_token_sampling_matches_oracle(device, temp, top_k, top_p, min_p):
    # temperature -> top-k -> top-p -> min-p -> seeded draw; the RNG and the order of the filters are this build's (boostr's are not
    # visible: parity unpinned), fixed in oracle/orc_ops.c.  Token ids must agree seed by seed.
    rng = np.random.default_rng(21)
    V = 32000
    row = (rng.standard_normal(V) * 2.5).astype(np.float32)
    t = device.tensor(row.reshape(1, V))
    hist = [5, 5, 9, 31999]
    ids, cnts = runtime.penalty_window(hist, 64)
    bad = 0
    for seed in range(120):
        got = int(runtime.logits_to_token(device, t, ids, cnts, repeat_penalty=1.1, frequency_penalty=0.1, presence_penalty=0.05, temperature=temp,
                                          top_k=top_k, top_p=top_p, min_p=min_p, seed=seed).to_numpy()[0])
        want = _orc_sample(row, ids, cnts, 1.1, 0.1, 0.05, temp, top_k, top_p, min_p, seed)
        bad += got != want
    assert bad <= 1, "%d of 120 seeds disagree" % bad    # expf differs by an ulp between host and device: a draw can land on a boundary


def test_logits_to_token_sampling_properties(device):
    rng = np.random.default_rng(4)
    V = 48
    row = rng.standard_normal(V).astype(np.float32)
    t = device.tensor(row.reshape(1, V))
    amax = int(row.argmax())
    # degenerate filters reduce to argmax
    for kw in (dict(top_k=1), dict(top_p=1e-6), dict(min_p=1.0)):
        for seed in (0, 1, 2):
            assert int(runtime.logits_to_token(device, t, [], [], temperature=0.9, seed=seed, **kw).to_numpy()[0]) == amax
    # unfiltered draws follow softmax(logits / T): chi-square over 6000 seeds, 47 degrees of freedom (99.9 % quantile 82.7)
    T = 1.5
    p = np.exp((row - row.max()) / T)
    p /= p.sum()
    n = 6000
    counts = np.zeros(V)
    for seed in range(n):
        counts[int(runtime.logits_to_token(device, t, [], [], temperature=T, seed=seed).to_numpy()[0])] += 1
    chi2 = float((((counts - n * p) ** 2) / (n * p)).sum())
    assert chi2 < 95.0, chi2
    # top-k support: only the k most likely ids are ever drawn
    top5 = set(np.argsort(-row)[:5].tolist())
    drawn = {int(runtime.logits_to_token(device, t, [], [], temperature=2.0, top_k=5, seed=s).to_numpy()[0]) for s in range(300)}
    assert drawn <= top5 and len(drawn) >= 4


def test_error_paths(device, tiny_awq):
    model, lm, _ = tiny_awq
    with pytest.raises(L.BlazrHipError) as e:
        lm.quant_matmul("model.layers.0.self_attn.q_proj.weight", np.zeros((1, 8), np.float32))
    assert e.value.code == L.E_INVALID
    za, zb = device.zeros((1, 256)), device.zeros((1, 256))
    with pytest.raises(L.BlazrHipError) as e:
        L.check(L.lib().bz_quant_matmul(lm.h, b"nope.weight", za.h, 1, zb.h))
    assert e.value.code == L.E_NOTFOUND
    bad = runtime.LoadedModel(device, model["config"])
    with pytest.raises(L.BlazrHipError):
        bad.finalize()    # nothing added
    kv = runtime.LayeredKvCache(device, 2, 1, 2, 4, 16, 64, L.F16)
    with pytest.raises(L.BlazrHipError):
        lm.forward_with_kv_cache([1, 2, 3], kv, 15)   # position + S > max_seq_len of the cache


def test_full_size_repack_and_gemv_properties(device):
    """BASELINE-size matrix (Llama-3-8B gate_proj, 14336 x 4096 AWQ): size-independent properties instead of an element-wise oracle run.
    (1) repack -> dequant round trip equals the oracle's dequant bit for bit; (2) a GEMV with a one-hot x returns that column of the
    dequantised matrix to the last f32 bit or the one next to it (1.0 splits exactly into the int8 planes); (3) linearity on inputs whose products are exact:
    W(e_i + e_j) == W e_i + W e_j within one f32 rounding."""
    spec = synth.awq_linear("model.layers.0.mlp.gate_proj", 14336, 4096, 128)
    # a model handle is only the container here: the matrix is registered as the q_proj of a 1-layer config of matching width
    model = synth.make_llama("tiny-awq", hidden=4096, n_layers=1, n_heads=112, n_kv_heads=8, head_dim=128, inter=256, vocab=512)
    model["layers"][0]["q"] = dict(spec, N=14336)
    lm = runtime.LoadedModel.from_synth(device, model)
    name = "model.layers.0.self_attn.q_proj.weight"
    W = orc_py.OrcLinear(spec).dequant()
    assert np.array_equal(lm.dequant(name), W)
    rng = np.random.default_rng(2)
    ks = rng.integers(0, 4096, size=4)
    x = np.zeros((5, 4096), np.float32)
    for r, k in enumerate(ks):
        x[r, k] = 1.0
    x[4, ks[0]] = x[4, ks[1]] = 1.0
    y = lm.quant_matmul(name, x)
    for r, k in enumerate(ks):      # (q*1 - z*1) * s evaluated as q*s' - z*s' in the kernel: one f32 rounding of difference at most
        assert np.abs(y[r] - W[:, k]).max() <= 2 ** -22 * np.abs(W[:, k]).max(), r
    assert np.abs(y[4] - (W[:, ks[0]] + W[:, ks[1]])).max() <= 2 ** -23 * np.abs(W).max() * 2


def test_tuning_entry_points_run_and_reject_bad_arguments(device):
    """bz_tune_gemv / bz_tune_rows / bz_tune_mlp / bz_probe_hbm_read (the per-kernel timing aids behind scripts/tune_*.py and bench.py's measured peak): one
    short call each returns a plausible time, a bad shape is an error code, not a fault"""
    us = C.c_double()
    L.check(L.lib().bz_tune_rows(device.h, 256, 1024, L.BF16, 1, 0, 2, 2, C.byref(us)))
    assert 0.5 < us.value < 1e4
    L.check(L.lib().bz_tune_gemv(device.h, 512, 1024, 2, 1, 2, 2, 0, C.byref(us)))
    assert 0.5 < us.value < 1e4
    L.check(L.lib().bz_tune_mlp(device.h, 2048, 1024, 2, 2, 0, C.byref(us), None))
    assert 0.5 < us.value < 1e4
    gbs = C.c_double()
    L.check(L.lib().bz_probe_hbm_read(device.h, 64 << 20, 2, C.byref(gbs)))
    assert 100.0 < gbs.value < 9000.0
    assert L.lib().bz_tune_rows(device.h, 256, 1001, L.BF16, 1, 0, 2, 2, C.byref(us)) != 0      # K not a multiple of 8
    assert L.lib().bz_tune_mlp(device.h, 1000, 1024, 2, 2, 0, C.byref(us), None) != 0          # hidden size the fused kernel is not built for
    assert L.lib().bz_tune_gemv(device.h, 512, 1024, 2, 1, 2, 2, 16, C.byref(us)) != 0        # flag bit other than 8 (the prefetch depth)
    stamps = (C.c_longlong * 512)()
    assert L.lib().bz_tune_mlp(device.h, 2048, 1024, 2, 2, 0, C.byref(us), stamps) != 0        # stamps_out must be NULL
