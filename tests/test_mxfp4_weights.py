"""MXFP4 weight checkpoints, the parts that need no GPU: the quantiser against an independent restatement, the packing, the exact f32 restatement the CPU
oracle runs, checkpoint detection and refusals from config.json, the on-disk form, the decode step's plan, the ABI symbol."""
import json

import numpy as np
import pytest

from blazr_amd import _lib as L
from blazr_amd import runtime, synth
from oracle import orc_py
import mxfp4_cases as M
import step_plan_cases as S


def test_tables():
    assert np.array_equal(synth.e2m1_table(), M.E2M1) and np.signbit(synth.e2m1_table()[8]) and synth.e2m1_table()[8] == 0.0
    t = synth.e8m0_table()
    assert np.array_equal(t[:255], M.E8M0[:255]) and np.isnan(t[255]) and t[127] == 1.0 and t[0] == 2.0 ** -127


def test_e2m1_encode_on_every_f16_value_up_to_8():
    """every f16 value in [-8, 8] (subnormals, both zeros, every tie of the E2M1 grid), one value per block beside a fixed maximum, under three block maxima:
    the shared exponent comes from the maximum, so the same value meets the grid at three scales, saturation (|v| > 6 at exponent 0) included"""
    bits = np.arange(1 << 16, dtype=np.uint16)
    v = bits.view(np.float16).astype(np.float32)
    v = v[np.isfinite(v) & (np.abs(v) <= 8.0)]
    for top in (4.0, 7.5, 31.0):      # floor(log2) - 2 = 0, 0, 2
        w = np.zeros((v.size, 32), np.float32)
        w[:, 0] = v
        w[:, 1] = top
        got_c, got_s = synth.e2m1_encode(w)
        want_c, want_s = M.encode_ref(w[::37])             # the slow restatement on a stride of the rows ...
        assert np.array_equal(got_c[::37], want_c) and np.array_equal(got_s[::37], want_s)
        # ... and on every row the defining property: no other E2M1 value is nearer, and a tie went to the even significand
        sc = M.E8M0[got_s[:, 0]]
        a = np.minimum(np.abs(v.astype(np.float64)) / sc, 6.0)
        mags = M.E2M1[:8].astype(np.float64)
        d = np.abs(a[:, None] - mags[None, :])
        m = got_c[:, 0] & 7
        chosen = d[np.arange(v.size), m]
        assert (chosen == d.min(axis=1)).all()
        tie = (d == d.min(axis=1)[:, None]).sum(axis=1) == 2
        assert ((m[tie] & 1) == 0).all() and tie.any()
        assert np.array_equal(got_c[:, 0] >> 3, np.signbit(v).astype(np.uint8))


def test_e2m1_encode_at_binade_edges():
    """blocks whose maximum sits on, just under and just over a power of two: the shared exponent steps exactly at the edge; an all-zero block takes code 127;
    huge and tiny maxima clamp to the admitted codes"""
    rows = []
    for e in (-20, -7, -1, 0, 1, 5):
        for f in (np.nextafter(np.float32(1.0), np.float32(0.0)), np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0)), np.float32(1.5), np.float32(1.75)):
            blk = (np.random.default_rng(e + 40).uniform(-1, 1, 32) * 2.0 ** e).astype(np.float32) * np.float32(0.9)
            blk[5] = -f * np.float32(2.0 ** e)
            rows.append(blk)
    rows.append(np.zeros(32, np.float32))
    rows.append(np.full(32, 3e38, np.float32))
    rows.append(np.full(32, 1e-45, np.float32))
    w = np.stack(rows)
    got_c, got_s = synth.e2m1_encode(w)
    want_c, want_s = M.encode_ref(w)
    assert np.array_equal(got_c, want_c) and np.array_equal(got_s, want_s)
    assert got_s[-3, 0] == 127 and got_s[-2, 0] == 127 + 127 - 2 and got_s[-1, 0] == 0
    assert got_s[1, 0] == got_s[0, 0] + 1                 # 2^e (1 - ulp) and 2^e: one binade apart
    assert int(got_s.max()) <= M.MAX_SCALE_CODE
    # the quantised weights stay near the input: half the widest grid gap (2, between 4 and 6) in units of the block's scale, or the saturation of a
    # block maximum in (6, 8) at 6 -- under 2 either way
    spec = M.spec_of(got_c, got_s)
    err = np.abs(M.weight_f64(spec)[:-3] - w[:-3].astype(np.float64))
    assert (err < 2.0 * np.repeat(M.E8M0[got_s[:-3]], 32, axis=1)).all()


def test_pack_unpack_round_trip():
    codes = np.random.default_rng(1).integers(0, 16, size=(64, 128), dtype=np.uint8)
    p = synth.mxfp4_pack(codes)
    assert p.shape == (64, 64) and p[3, 5] == (codes[3, 10] | (codes[3, 11] << 4))          # the LOW nibble is the even element
    assert np.array_equal(synth.mxfp4_unpack(p), codes) and np.array_equal(M.unpack(p), codes) and np.array_equal(M.pack(codes), p)


def test_restate_f32_is_exact_for_every_admitted_scale_code():
    """all sixteen codes under every scale code 0 .. 252: 2^(s - 127) e2m1 is an f32 (subnormal at the low end), and the oracle's dense linear on it is the
    float64 product"""
    codes = np.tile(np.arange(16, dtype=np.uint8), (64, 253 * 2))                              # [64, 253 * 32]
    scale = np.tile(np.arange(253, dtype=np.uint8), (64, 1))
    spec = M.spec_of(codes, scale)
    d = M.restate_linear(spec)
    assert d["kind"] == "dense" and d["weight"].dtype == np.float32
    assert np.array_equal(d["weight"].astype(np.float64), M.weight_f64(spec)) and np.isfinite(d["weight"]).all()
    assert d["weight"][0, 252 * 32 + 7] == np.float32(6.0 * 2.0 ** 125) and d["weight"][0, 1] == np.float32(2.0 ** -128)
    with pytest.raises(AssertionError):
        M.restate_linear(M.spec_of(codes[:, :32], np.full((64, 1), 254, np.uint8)))              # 6 . 2^127 is not an f32
    lin = synth.mxfp4_linear("model.layers.0.mlp.down_proj", 128, 704, bias=True)
    assert lin["weight"].shape == (128, 352) and lin["scale"].shape == (128, 22) and lin["weight"].dtype == np.uint8
    r = M.restate_linear(lin)
    x = synth._repr(np.random.default_rng(5).standard_normal((3, 704)).astype(np.float32), "bf16")
    want = (x.astype(np.float64) @ M.weight_f64(lin).T).astype(np.float32) + r["bias"]
    assert np.array_equal(orc_py.OrcLinear(r).forward(x), want)


def test_restate_f32_covers_every_linear_of_a_model():
    m = M.make("tiny-mxfp4-bf16")
    r = M.restate_f32(m)
    assert {lay[k]["kind"] for lay in m["layers"] for k in M.LINEARS} == {"mxfp4"}
    assert all(lay[k]["kind"] == "dense" and lay[k]["weight"].dtype == np.float32 for lay in r["layers"] for k in M.LINEARS)
    for a, b in (("tiny-mxfp4", "tiny-fp8"), ("llama3.1-8b-mxfp4", "llama3.1-8b-fp8")):
        pa, pb = synth.PRESETS[a], synth.PRESETS[b]
        assert all(pa[k] == pb[k] for k in ("hidden", "n_layers", "n_heads", "n_kv_heads", "head_dim", "inter", "vocab", "act_dtype", "tie_embeddings"))
    assert M.make("mxfp4-g2-w768")["config"]["inter"] == 1408


BASE = dict(model_type="llama", vocab_size=1024, hidden_size=256, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, intermediate_size=512,
            torch_dtype="bfloat16")


def test_config_detection_quark_mxfp4():
    """Without the feature the quant method reads 0 (None)."""
    c, q = runtime.config_from_hf_json(json.dumps(dict(BASE, quantization_config=M.quantization_config())))
    assert q["quant_method"] == "mxfp4" and q["group_size"] == 32 and c.act_dtype == L.BF16      # the checkpoint keeps its torch_dtype
    qi = L.QuantInfo(); cc = L.ModelConfig()
    L.check(L.lib().bz_config_from_hf_json(json.dumps(dict(BASE, torch_dtype="float16", quantization_config=M.quantization_config())).encode(), L.C.byref(cc), L.C.byref(qi)))
    assert qi.quant_method == 4 and cc.act_dtype == L.F16
    _, q = runtime.config_from_hf_json(json.dumps(dict(BASE, quantization_config=dict(quant_method="fp8", activation_scheme="dynamic"))))
    assert q["quant_method"] == "fp8"                                                             # the existing routes are as they were


@pytest.mark.parametrize("name,qc,field", M.loader_refusals(), ids=[r[0] for r in M.loader_refusals()])
def test_config_refusals_name_the_field(name, qc, field):
    with pytest.raises(L.BlazrHipError) as e:
        runtime.config_from_hf_json(json.dumps(dict(BASE, quantization_config=qc)))
    assert e.value.code == L.E_UNSUPPORTED and field in str(e.value), str(e.value)


def test_checkpoint_on_disk_as_the_loader_reads_it(tmp_path):
    m = M.make("tiny-mxfp4-bf16")
    M.write_mxfp4_checkpoint(str(tmp_path), m)
    d = runtime.safetensors_describe(str(tmp_path))["tensors"]
    w, s = d["model.layers.1.mlp.down_proj.weight"], d["model.layers.1.mlp.down_proj.weight_scale"]
    assert w["dtype"] == "U8" and w["shape"] == [256, 256] and w["bytes"] == 256 * 256
    assert s["dtype"] == "U8" and s["shape"] == [256, 16] and s["bytes"] == 256 * 16
    assert d["model.embed_tokens.weight"]["dtype"] == "BF16"
    _, q = runtime.config_from_hf_json(open(str(tmp_path / "config.json")).read())
    assert q["quant_method"] == "mxfp4"


def test_layer_plan_of_an_mxfp4_layer():
    """all five linears on k_gemv_mx4, plain attention + a separate o_proj launch (short and long), the split MLP -- as an FP8 layer's plan reads"""
    for H, I, nq, nkv, hd in ((4096, 14336, 32, 8, 128), (256, 512, 4, 2, 64)):
        def f(N, K):
            return S.fused(S.lin(L.LIN_MX4, N, K, wdt=L.U8 if hasattr(L, "U8") else 0), fix_out=0)
        t = S.llama_traits(L.BF16, H, I, nq, nkv, hd, f((nq + 2 * nkv) * hd, H), f(H, nq * hd), f(2 * I, H), f(H, I))
        for kv in (L.BF16, L.F16):
            p = runtime.layer_plan(t, kv)
            assert p["qkv"][0] == p["o"][0] == p["gateup"][0] == p["down"][0] == L.GEMV_MX4 and L.GEMV_MX4 == 9 and L.LIN_MX4 == 12
            assert p["qkv"][1] == L.GEMV_NONE and not p["qkv_mix"] and not p["gateup_mix"]
            assert p["attn_short"] == L.ATTN_PLAIN and p["attn_long"] in (L.ATTN_PLAIN, L.ATTN_SPLIT) and p["mlp"] == L.MLP_SPLIT
        # the same layer as FP8 differs in the GEMV form alone
        g = S.one_kind_layer(L.LIN_F8, H, I, nq, nkv, hd, act=L.BF16)
        for F in (g.qkv, g.o, g.gateup, g.down):
            F.fix_out = 0
        a, b = runtime.layer_plan(t, L.BF16), runtime.layer_plan(g, L.BF16)
        assert all(a[k] == b[k] for k in ("attn_short", "attn_long", "attn_kernel", "mlp", "qkv_mix", "gateup_mix"))


def test_abi_symbol_is_exported():
    """Without the feature the symbol is missing."""
    assert "bz_model_add_mxfp4" in L.SYMBOLS
    assert hasattr(L.lib(), "bz_model_add_mxfp4")
    assert L.lib().bz_abi_version() == 4


def test_bytes_per_token_counts_four_and_a_quarter_bits():
    cfg4, cfg16 = synth.make_config("llama3.1-8b-mxfp4"), synth.make_config("llama3.1-8b-mxfp4", quant="none")
    b4, b16 = synth.algorithmic_bytes_per_token(cfg4), synth.algorithmic_bytes_per_token(cfg16)
    head = cfg4["vocab"] * cfg4["hidden"] * 2
    assert abs((b4 - head) / (b16 - head) - 4.25 / 16) < 1e-3
