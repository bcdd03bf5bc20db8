"""NVFP4 weights on the device: read-back of every code under scale bytes from both ends of E4M3, the decode GEMV and the W4A16 GEMM against float64, whole
models against the CPU oracle on the exact f32 restatement (tests/nvfp4_cases.py restate_f32), and checkpoints loaded from disk."""
import numpy as np
import pytest

import nvfp4_cases as M
from blazr_amd import _lib as L
from blazr_amd import runtime, synth
from oracle import orc_py
from test_gpu_llama import TINY, _fair_prefix, _kv_dt
from test_gpu_mxfp4_weights import DOWN, _logits, _op_model, _prefill_matmul, _rel, _ulp      # the op-model builder and the measures of the MXFP4 suite

pytestmark = pytest.mark.gpu


def _random_spec(N, K, seed, global_scale, bias=None):
    r = np.random.default_rng(seed)
    return M.spec_of(r.integers(0, 16, size=(N, K), dtype=np.uint8), r.integers(0x28, 0x48, size=(N, K // 16), dtype=np.uint8), global_scale, bias)


def test_dequant_reads_back_every_code_and_scale(device):
    """[64, 64]: every group of 16 walks all sixteen codes (rotated by row, so each meets an even and an odd nibble), under the scale bytes 0, the subnormals
    1 .. 7, normals of every mantissa and 0x7E (448), with the global scale 2^5: the result is weight_f64 exactly.  Pins the nibble order, the group -> scale
    byte pairing inside a piece and the tile layout."""
    N, K = 64, 64
    codes = (np.arange(K)[None, :] + np.arange(N)[:, None]).astype(np.uint8) % 16
    pool = np.array([0, 1, 2, 3, 4, 5, 6, 7, 0x08, 0x2B, 0x39, 0x3C, 0x46, 0x55, 0x77, 0x7E], np.uint8)
    scale = pool[(np.arange(N)[:, None] * 5 + np.arange(K // 16)[None, :]) % 16]
    assert set(scale.reshape(-1).tolist()) == set(pool.tolist())
    spec = M.spec_of(codes, scale, 32.0)
    got = _op_model(device, spec).dequant(DOWN)
    want = M.weight_f64(spec)
    assert np.array_equal(got.astype(np.float64), want) and np.array_equal(np.signbit(got), np.signbit(want))


@pytest.mark.parametrize("act", ["bf16", "f16"])
@pytest.mark.parametrize("N,K", M.GEMV_SHAPES)
def test_quant_matmul_is_the_rounded_float64_product(device, N, K, act):
    """Bar (the exact GEMVs' op bar, as the MXFP4 suite states it): every output within one rounding interval of the activation dtype of
    R_act(f32(float64 value) + b), at most 1 % of the outputs not identical.  The global scale 1000 makes r a general f32; (192, 704) carries a bias."""
    rng = np.random.default_rng(N + K)
    x = synth._repr(rng.standard_normal((2, K)).astype(np.float32), act)
    bias = synth._repr(rng.standard_normal(N).astype(np.float32), act) if (N, K) == (192, 704) else None
    spec = _random_spec(N, K, N * 7 + K, 1000.0, bias)
    got = _op_model(device, spec, act).quant_matmul(DOWN, x)
    ref = (x.astype(np.float64) @ M.weight_f64(spec).T).astype(np.float32)
    if bias is not None:
        ref = ref + bias
    want, gr = orc_py.round_act(ref, act), orc_py.round_act(got, act)
    diff = np.abs(gr.astype(np.float64) - want.astype(np.float64))
    nd = int((gr != want).sum())
    print("gemv_nv4 [%d, %d] %s: %d of %d outputs differ, max %.3g intervals" % (N, K, act, nd, want.size, float((diff / _ulp(want, act)).max())))
    assert (diff <= _ulp(want, act)).all()
    assert nd <= want.size // 100


_GEMM = {}


def _gemm_models(device, N, K, act):
    """built once per shape and dtype: an NVFP4 tensor under a power-of-two global scale (so W is exact in both 16-bit dtypes) and the dense 16-bit tensor
    holding the same W -- the dense GEMM on it is the yardstick"""
    if (N, K, act) not in _GEMM:
        spec = _random_spec(N, K, N + 3 * K, 128.0)
        wd = M.weight_f64(spec).astype(np.float32)
        assert np.array_equal(synth._repr(wd, "bf16"), wd) and np.array_equal(synth._repr(wd, "f16"), wd)
        dense = dict(kind="dense", N=N, K=K, weight=synth._store(wd, act))
        _GEMM[(N, K, act)] = (_op_model(device, dense, act), _op_model(device, spec, act), M.weight_f64(spec))
    return _GEMM[(N, K, act)]


@pytest.mark.parametrize("act", ["bf16", "f16"])
@pytest.mark.parametrize("S", M.GEMM_ROWS)
@pytest.mark.parametrize("N,K", M.GEMM_SHAPES)
def test_prefill_matmul_stays_within_twice_the_dense_gemm_error(device, N, K, S, act):
    """The yardstick and bar of the MXFP4 suite's test of this name: largest element error against float64, normalised by sum_k |x_k| |W_nk|, within 2 x what
    bz_prefill_matmul gives on the dense 16-bit tensor holding the same W.  The scaled fragments are exact, so the ratio sits near 1."""
    ld, ln, w64 = _gemm_models(device, N, K, act)
    x = synth._repr(np.random.default_rng(S * 1000 + N).standard_normal((S, K)).astype(np.float32), act)
    x64 = x.astype(np.float64)
    err = lambda got: float((np.abs(got - x64 @ w64.T) / (np.abs(x64) @ np.abs(w64).T)).max())
    e_dense, e_nv4 = err(_prefill_matmul(device, ld, x, N)), err(_prefill_matmul(device, ln, x, N))
    print("gemm_nv4w %s S=%d [%d, %d]: dense %.3e, nvfp4 %.3e, ratio %.3f" % (act, S, N, K, e_dense, e_nv4, e_nv4 / e_dense))
    assert e_dense > 0.0
    assert e_nv4 <= 2.0 * e_dense


_MODELS = {}


def _pair(device, name):
    if name not in _MODELS:
        model = M.make(name)
        _MODELS[name] = (model, runtime.LoadedModel.from_synth(device, model), orc_py.OrcLlama(M.restate_f32(model)))
    return _MODELS[name]


@pytest.mark.parametrize("name", list(M.MODELS))
def test_nvfp4_llama_decode_is_the_oracle_on_the_restatement(device, name):
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
    n = _fair_prefix(want[12:])
    assert ids_got[:n] == ids_want[:n]
    assert ndiff <= got.size // 10000 and rel <= 1e-5


@pytest.mark.parametrize("name", list(M.MODELS))
def test_prompt_of_40_rows_takes_the_batched_path(device, name):
    """40 rows > BZ_EXACT_PREFILL_MAX: route ROWS -- the W4A16 GEMMs and the MFMA attention; every row within the MFMA-prompt bar of DESIGN 5 (1e-3 f16,
    1.25 2^-7 bf16, twice that at hidden 256) against the oracle restatement"""
    model, lm, om = _pair(device, name)
    cfg = model["config"]
    tr = runtime.prompt_traits(lm)
    assert tr.proj_16 and tr.any_dense
    assert runtime.prompt_plan(tr, L.PLAN_PROMPT, 40, 40, _kv_dt(cfg))["route"] == L.ROUTE_ROWS
    p = synth.prompt_tokens(40, cfg["vocab"], seed=13)
    kv = runtime.LayeredKvCache(device, cfg["n_layers"], 1, cfg["n_kv_heads"], 64, cfg["max_seq_len"], cfg["head_dim"], _kv_dt(cfg))
    okv = om.new_kv(64)
    got, want = lm.forward_with_kv_cache(p, kv, 0, all_logits=True).to_numpy(), om.forward_kv(p, okv, 0, all_logits=True)
    orc_py.lib().orc_kv_free(okv)
    hard = (1e-3 if cfg["act_dtype"] == "f16" else 1.25 * 2.0 ** -7) * (TINY if cfg["hidden"] == 256 else 1.0)
    worst = max(_rel(got[r], want[r]) for r in range(40))
    print("%s: 40-row prompt, worst row rel L2 %.3e (bar %.3e)" % (name, worst, hard))
    assert worst <= hard


@pytest.mark.parametrize("bias", [False, True], ids=["plain", "bias"])
def test_checkpoint_round_trip(device, tmp_path, bias):
    """a compressed-tensors directory: packed U8 weights, F8_E4M3 group scales, F32 global scales, lm_head on the ignore list (untied, 16-bit), the input
    global scales ignored; the loaded model gives the bits of the one added tensor by tensor"""
    model = synth.make_llama("tiny-nvfp4", tie_embeddings=False, bias=bias)
    cfg = model["config"]
    assert (model["layers"][0]["q"]["bias"] is not None) == bias
    M.write_nvfp4_checkpoint(str(tmp_path), model)
    a, b = runtime.load_model(device, str(tmp_path)), runtime.LoadedModel.from_synth(device, model)
    assert a.c.act_dtype == L.BF16
    p = synth.prompt_tokens(12, cfg["vocab"], seed=5)
    assert np.array_equal(_logits(device, a, cfg, p), _logits(device, b, cfg, p))
    assert a.weight_bytes() == b.weight_bytes()


def test_loader_refuses_a_nan_scale_byte_by_tensor_name(device, tmp_path):
    model = synth.make_llama("tiny-nvfp4", tie_embeddings=False)
    model["layers"][1]["down"]["scale"][7, 3] = 0x7F
    M.write_nvfp4_checkpoint(str(tmp_path), model)
    with pytest.raises(L.BlazrHipError) as ex:
        runtime.load_model(device, str(tmp_path))
    assert ex.value.code == L.E_INVALID and "model.layers.1.mlp.down_proj.weight" in str(ex.value), str(ex.value)
