"""MXFP4 with FP4 activations (W4A4, bz_model_set_mxfp4_activations): the activation quantiser bit for bit against tests/mxfp4_cases.py encode_ref, the
operand layout of the block-scaled FP4 MFMA on identity inputs, the GEMM against float64 under the dense 16-bit GEMM's own error, whole prompts against a
numpy reference that quantises every linear's input, and the switch."""
import numpy as np
import pytest

import mxfp4_cases as M
import npref
from blazr_amd import _lib as L
from blazr_amd import runtime, synth
from test_gpu_llama import _kv_dt
from test_gpu_mxfp4_weights import DOWN, WIDE_SHAPE, _err, _gemm_models, _op_model, _pair, _prefill_matmul, _rel

pytestmark = pytest.mark.gpu


def _xq64(codes, scales):
    """float64 value of quantised rows (codes packed [S, K/2], scales [S, K/32])"""
    return M.E2M1[M.unpack(codes)].astype(np.float64) * np.repeat(M.E8M0[scales], 32, axis=1)


def _a4_matmul(device, lm, x, N):
    lm.set_mxfp4_activations(1)
    try:
        return _prefill_matmul(device, lm, x, N)
    finally:
        lm.set_mxfp4_activations(0)


@pytest.mark.parametrize("act", ["bf16", "f16"])
@pytest.mark.parametrize("K", [64, 704])
def test_quantiser_is_encode_ref_bit_for_bit(device, K, act):
    """5 rows of N(0, 1) with planted blocks: all zero; every E2M1 midpoint under an amax of 6 (ties to the even significand); equal magnitudes 1.25 (a tie at 5
    under the block's own scale); 7.9 beside 7 (both saturate); 21 binades in one block; a block of 16-bit subnormals only; and -0 and a subnormal inside an
    ordinary block."""
    tiny = 2.0 ** -24 if act == "f16" else 2.0 ** -133          # the smallest subnormal of the dtype
    x = np.random.default_rng(K).standard_normal((5, K)).astype(np.float32)
    sign = np.where(np.arange(32) % 3 == 0, -1.0, 1.0)
    x[0, :32] = 0.0
    x[0, 32:64] = sign * np.resize([6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0], 32) * 2.0 ** -3
    x[1, :32] = sign * 1.25 * 2.0 ** 5
    x[1, 32:64] = sign * np.resize([7.9, 7.0, 2.5, 0.3], 32) * 2.0 ** -6
    x[2, :32] = sign * 2.0 ** -np.resize(np.arange(21.0), 32)
    x[2, 32:64] = sign * tiny * np.resize([1.0, 3.0, 5.0, 7.0], 32)
    x[3, 5], x[3, 6] = -0.0, tiny
    x = synth._repr(x, act)
    assert np.signbit(x[3, 5]) and x[3, 6] == np.float32(tiny) and x[2, 33] != 0.0
    codes, scales = M.encode_ref(x)
    c2, s2 = synth.e2m1_encode(x)
    assert np.array_equal(codes, c2) and np.array_equal(scales, s2)
    got_c, got_s = _op_model(device, M.quantised(64, 64, 1), act).mxfp4_quant_rows(x)
    assert np.array_equal(got_s, scales)
    assert np.array_equal(got_c, M.pack(codes))


@pytest.mark.parametrize("factor", [1.0, 1.5])
@pytest.mark.parametrize("K", [64, 192])
def test_identity_rows_read_back_every_weight(device, K, factor):
    """x = factor . I quantises to one code (4 or 6 under 2^-2) per row, so the product is factor . W exactly: which k a lane's block covers, the scale byte
    and its op_sel, and the nibble order of A against B, for every lane position and both tile heights (S = K = 64: TM 1, 192: TM 2)"""
    rng = np.random.default_rng(K)
    codes = np.concatenate([np.concatenate([rng.permutation(16), rng.permutation(16)]) for _ in range(64 * K // 32)]).astype(np.uint8).reshape(64, K)
    codes[1::2] = np.roll(codes[1::2], 1, axis=1)                  # every code meets an even and an odd position
    spec = M.spec_of(codes, rng.integers(115, 122, size=(64, K // 32), dtype=np.uint8))
    got = _a4_matmul(device, _op_model(device, spec), factor * np.eye(K, dtype=np.float32), 64)
    assert np.array_equal(got, factor * M.weight_f64(spec).T)


@pytest.mark.parametrize("act", ["bf16", "f16"])
@pytest.mark.parametrize("S", M.GEMM_ROWS)
@pytest.mark.parametrize("N,K", M.GEMM_SHAPES)
def test_a4_matmul_stays_within_twice_the_dense_gemm_error(device, N, K, S, act):
    """The yardstick of test_prefill_matmul_stays_within_twice_the_dense_gemm_error, with the device's own quantised rows (held to encode_ref above) as the
    input: largest |got - xq W^T| / (|xq| |W|^T) against 2 x the dense 16-bit GEMM's figure on the same W.  The wide-range tensor (scales 2^-30 .. 2^0 in every
    row) on WIDE_SHAPE is what decides whether the f32 accumulation of the instruction needs a fold.

    Measured on an MI355X: the narrow tensor's error is 0 in all 24 cases (dense 1.9e-8 .. 7.0e-8); the wide-range tensor 1.06 x .. 1.87 x the dense figure (the
    closest: bf16 S=64, 5.45e-8 against 2 x 2.92e-8).  It decided more than a fold: a running f32 C missed the bar in three cases (up to 2.47 x) and so did C folded
    into doubles every 256 k, so the kernel gives every MFMA one block and a zero C and sums the blocks in double."""
    ld, ln, narrow, lw, wide = _gemm_models(device, N, K, act)
    x = synth._repr(np.random.default_rng(S * 1000 + N).standard_normal((S, K)).astype(np.float32), act)
    xq = _xq64(*ln.mxfp4_quant_rows(x))
    e_dense = _err(_prefill_matmul(device, ld, x, N), x.astype(np.float64), M.weight_f64(narrow))
    e_a4 = _err(_a4_matmul(device, ln, x, N), xq, M.weight_f64(narrow))
    e_wide = _err(_a4_matmul(device, lw, x, N), xq, M.weight_f64(wide)) if lw is not None else 0.0
    print("gemm_mx4a4 %s S=%d [%d, %d]: dense %.3e, a4 %.3e, a4 wide-range %.3e" % (act, S, N, K, e_dense, e_a4, e_wide))
    assert e_dense > 0.0
    assert e_a4 <= 2.0 * e_dense
    assert e_wide <= 2.0 * e_dense


class NpLlamaA4(npref.NpLlama):
    """every linear's input through the MX quantiser first (encode_ref); the projections of one input share its quantised value"""
    _seen = (None, None)

    def _lin(self, l, name, x):
        if self._seen[0] is not x:
            codes, scales = M.encode_ref(x[None, :])
            self._seen = (x, (M.E2M1[codes[0]].astype(np.float64) * np.repeat(M.E8M0[scales[0]], 32)).astype(np.float32))
        return super()._lin(l, name, self._seen[1])


def _prompt(device, lm, cfg, p, rows):
    """logits of every position; rows at a time"""
    kv = runtime.LayeredKvCache(device, cfg["n_layers"], 1, cfg["n_kv_heads"], 64, cfg["max_seq_len"], cfg["head_dim"], _kv_dt(cfg))
    return np.concatenate([lm.forward_with_kv_cache(p[i:i + rows], kv, i, all_logits=True).to_numpy().reshape(rows, -1) for i in range(0, len(p), rows)])


@pytest.mark.parametrize("name", ["tiny-mxfp4-bf16", "tiny-mxfp4-f16"])
def test_prompt_of_40_rows_is_the_a4_reference(device, name):
    """rel L2 (device A4, numpy A4) <= 1/2 rel L2 (numpy A16, numpy A4): the feature's own effect is the yardstick -- an element near an FP4 tie may round
    differently on the two sides (a few percent of that effect), a linear left on 16-bit activations or a wrong scale is as large as the effect itself"""
    model, lm, _ = _pair(device, name)
    cfg = model["config"]
    p = [int(t) for t in synth.prompt_tokens(40, cfg["vocab"], seed=13)]
    a16, a4 = npref.NpLlama(M.restate_f32(model)), NpLlamaA4(M.restate_f32(model))
    ref16, ref4 = np.stack([a16.step(t, i) for i, t in enumerate(p)]), np.stack([a4.step(t, i) for i, t in enumerate(p)])
    effect = _rel(ref16, ref4)
    assert effect > 0.0
    lm.set_mxfp4_activations(1)
    try:
        got = _prompt(device, lm, cfg, p, 40)
        steps = _prompt(device, lm, cfg, p[:12], 1) if name == "tiny-mxfp4-bf16" else None
    finally:
        lm.set_mxfp4_activations(0)
    print("%s: device A4 to numpy A4 %.3e, numpy A16 to numpy A4 %.3e" % (name, _rel(got, ref4), effect))
    assert _rel(got, ref4) <= 0.5 * effect
    if steps is not None:                                      # single-token steps keep 16-bit activations: the bits of the mode-off run
        assert np.array_equal(steps, _prompt(device, lm, cfg, p[:12], 1))


def test_setter_refusals_and_the_way_back(device):
    dense = runtime.LoadedModel.from_synth(device, synth.make_llama("tiny-bf16"))
    assert L.lib().bz_model_set_mxfp4_activations(dense.h, 1) == L.E_UNSUPPORTED
    model, lm, _ = _pair(device, "tiny-mxfp4-bf16")
    assert L.lib().bz_model_set_mxfp4_activations(lm.h, 2) == L.E_INVALID
    cfg = model["config"]
    p = [int(t) for t in synth.prompt_tokens(40, cfg["vocab"], seed=13)]
    off = _prompt(device, lm, cfg, p, 40)
    lm.set_mxfp4_activations(1)
    on = _prompt(device, lm, cfg, p, 40)
    lm.set_mxfp4_activations(0)
    assert not np.array_equal(on, off)
    assert np.array_equal(_prompt(device, lm, cfg, p, 40), off)
