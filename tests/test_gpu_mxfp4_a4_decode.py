"""MXFP4 W4A4 decode (bz_model_set_mxfp4_activations mode 3): k_gemv_mx4a4's operand layout on identity rows, the GEMV against float64 under the dense 16-bit
GEMM's own error, and whole single-token steps against the numpy reference that quantises every linear's input."""
import numpy as np
import pytest

import mxfp4_cases as M
import npref
from blazr_amd import _lib as L
from blazr_amd import runtime, synth
from test_gpu_mxfp4_a4 import NpLlamaA4, _prompt, _xq64
from test_gpu_mxfp4_weights import DOWN, WIDE_SHAPE, _err, _gemm_models, _op_model, _pair, _prefill_matmul, _rel

pytestmark = pytest.mark.gpu


def _a4_gemv(lm, x):
    lm.set_mxfp4_activations(3)
    try:
        return lm.quant_matmul(DOWN, x).astype(np.float64)
    finally:
        lm.set_mxfp4_activations(0)


@pytest.mark.parametrize("factor", [1.0, 1.5])
@pytest.mark.parametrize("K", [64, 192, 1024])
def test_identity_rows_read_back_every_weight(device, K, factor):
    """x = factor . e_k quantises to one code (4 or 6 under 2^-2), so row k of the result is factor . W[:, k] exactly: the lane -> (row, block) map, the scale
    byte, the nibble order and the order of the waves' partial sums; K = 1024 crosses a 512-k tile and gives every wave a slice"""
    rng = np.random.default_rng(K)
    codes = np.concatenate([np.concatenate([rng.permutation(16), rng.permutation(16)]) for _ in range(64 * K // 32)]).astype(np.uint8).reshape(64, K)
    codes[1::2] = np.roll(codes[1::2], 1, axis=1)                  # every code meets an even and an odd position
    spec = M.spec_of(codes, rng.integers(115, 122, size=(64, K // 32), dtype=np.uint8))
    got = _a4_gemv(_op_model(device, spec), factor * np.eye(K, dtype=np.float32))
    assert np.array_equal(got, factor * M.weight_f64(spec).T)


@pytest.mark.parametrize("act", ["bf16", "f16"])
@pytest.mark.parametrize("N,K,wide", [(N, K, False) for N, K in M.GEMV_SHAPES] + [WIDE_SHAPE + (True,)])
def test_a4_gemv_stays_within_twice_the_dense_gemm_error(device, N, K, wide, act):
    """The yardstick of test_a4_matmul_stays_within_twice_the_dense_gemm_error on 9 single rows: largest |got - xq W^T| / (|xq| |W|^T), xq the device quantiser's
    rows (held to encode_ref there), against 2 x the same measure of the dense 16-bit GEMM on the same W and rows.  `wide`: the tensor whose every row mixes the
    scale codes 97 .. 127.  The narrow tensor of that shape is run with a bias as well."""
    ld, ln, narrow, lw, wspec = _gemm_models(device, N, K, act)
    lm, spec = (lw, wspec) if wide else (ln, narrow)
    x = synth._repr(np.random.default_rng(9000 + N).standard_normal((9, K)).astype(np.float32), act)
    xq, w64 = _xq64(*lm.mxfp4_quant_rows(x)), M.weight_f64(spec)
    e_dense = _err(_prefill_matmul(device, ld, x, N), x.astype(np.float64), M.weight_f64(narrow))
    e_a4 = _err(_a4_gemv(lm, x), xq, w64)
    e_bias = 0.0
    if (N, K) == WIDE_SHAPE and not wide:
        bias = synth._repr(np.random.default_rng(N).standard_normal(N).astype(np.float32), act)
        got = _a4_gemv(_op_model(device, dict(spec, bias=bias), act), x[:2])
        want = (xq[:2] @ w64.T).astype(np.float32) + bias                                  # the kernel's order: one rounding to f32, then the bias in f32
        e_bias = float((np.abs(got - want.astype(np.float64)) / (np.abs(xq[:2]) @ np.abs(w64).T)).max())
    print("gemv_mx4a4 %s [%d, %d] wide=%s: dense %.3e, a4 %.3e, a4 biased %.3e" % (act, N, K, wide, e_dense, e_a4, e_bias))
    assert e_dense > 0.0
    assert e_a4 <= 2.0 * e_dense
    assert e_bias <= 2.0 * e_dense


@pytest.mark.parametrize("name", ["tiny-mxfp4-bf16", "tiny-mxfp4-f16"])
def test_single_token_steps_are_the_a4_reference(device, name):
    """12 steps under mode 3: rel L2 (device, numpy A4) <= 1/2 rel L2 (numpy A16, numpy A4), test_prompt_of_40_rows_is_the_a4_reference's bar; the steps differ
    from mode 1's (they changed path), the captured step gives the eager ids, mode 0 brings the mode-off bits back and mode 2 stays refused"""
    model, lm, _ = _pair(device, name)
    cfg = model["config"]
    p = [int(t) for t in synth.prompt_tokens(12, cfg["vocab"], seed=13)]
    a16, a4 = npref.NpLlama(M.restate_f32(model)), NpLlamaA4(M.restate_f32(model))
    ref16, ref4 = np.stack([a16.step(t, i) for i, t in enumerate(p)]), np.stack([a4.step(t, i) for i, t in enumerate(p)])
    effect = _rel(ref16, ref4)
    assert effect > 0.0
    off = _prompt(device, lm, cfg, p, 1)
    try:
        lm.set_mxfp4_activations(1)
        one = _prompt(device, lm, cfg, p, 1)
        lm.set_mxfp4_activations(3)
        got = _prompt(device, lm, cfg, p, 1)
        ex = runtime.Executor(lm)
        ids = [ex.generate(p, 8, use_graph=g).tolist() for g in (False, True)]
        assert L.lib().bz_model_set_mxfp4_activations(lm.h, 2) == L.E_INVALID
    finally:
        lm.set_mxfp4_activations(0)
    print("%s: device A4 steps to numpy A4 %.3e, numpy A16 to numpy A4 %.3e" % (name, _rel(got, ref4), effect))
    assert _rel(got, ref4) <= 0.5 * effect
    assert np.array_equal(one, off) and not np.array_equal(got, one)
    assert ids[0] == ids[1]
    assert np.array_equal(_prompt(device, lm, cfg, p, 1), off)
