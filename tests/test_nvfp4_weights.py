"""NVFP4 weight checkpoints, the parts that need no GPU: detection and refusals from config.json, the ABI symbol, the decode step's plan, and the exactness
claim the prompt GEMM rests on (plain numpy: the one test here that does not need the feature)."""
import json

import numpy as np
import pytest

from blazr_amd import _lib as L
from blazr_amd import runtime, synth
import nvfp4_cases as M
import step_plan_cases as S

BASE = dict(model_type="llama", vocab_size=1024, hidden_size=256, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, intermediate_size=512)


@pytest.mark.parametrize("td,act", [("bfloat16", L.BF16), ("float16", L.F16)])
def test_config_detection(td, act):
    c, q = runtime.config_from_hf_json(json.dumps(dict(BASE, torch_dtype=td, quantization_config=M.quantization_config())))
    assert q["quant_method"] == "nvfp4" and q["group_size"] == 16 and c.act_dtype == act      # the checkpoint keeps its torch_dtype


@pytest.mark.parametrize("over,field", [(dict(group_size=32), "weights.group_size"), (dict(strategy="group"), "weights.strategy"), (dict(num_bits=8), "weights.num_bits"),
                                        (dict(type="int"), "weights.type")], ids=["group_size", "strategy", "num_bits", "type"])
def test_config_refusals_name_the_field(over, field):
    with pytest.raises(L.BlazrHipError) as e:
        runtime.config_from_hf_json(json.dumps(dict(BASE, torch_dtype="bfloat16", quantization_config=M.quantization_config(**over))))
    assert e.value.code == L.E_UNSUPPORTED and field in str(e.value), str(e.value)


def test_abi_symbol_is_exported_and_the_version_stays():
    assert "bz_model_add_nvfp4" in L.SYMBOLS and hasattr(L.lib(), "bz_model_add_nvfp4")
    assert L.lib().bz_abi_version() == 4


def test_layer_plan_of_an_nvfp4_layer():
    """all five linears on k_gemv_nv4, plain attention + a separate o_proj launch, the split MLP -- as an MXFP4 layer's plan reads"""
    assert L.GEMV_NV4 == 11 and L.LIN_NV4 == 14
    for H, I, nq, nkv, hd in ((4096, 14336, 32, 8, 128), (256, 512, 4, 2, 64)):
        f = lambda N, K: S.fused(S.lin(L.LIN_NV4, N, K, wdt=L.U8), fix_out=0)
        t = S.llama_traits(L.BF16, H, I, nq, nkv, hd, f((nq + 2 * nkv) * hd, H), f(H, nq * hd), f(2 * I, H), f(H, I))
        for kv in (L.BF16, L.F16):
            p = runtime.layer_plan(t, kv)
            assert p["qkv"][0] == p["o"][0] == p["gateup"][0] == p["down"][0] == L.GEMV_NV4
            assert p["qkv"][1] == L.GEMV_NONE and p["attn_short"] == L.ATTN_PLAIN and p["mlp"] == L.MLP_SPLIT


def test_scaled_weights_are_exact_in_both_16_bit_dtypes():
    """e2m1 . e4m3 over the 15 nonzero E2M1 codes and every finite non-negative E4M3 code survives f16 and bf16 unchanged: what k_gemm_nv4w's fragments hold"""
    e2 = M.E2M1[1:].astype(np.float64)                       # codes 1 .. 15 (code 8 is -0)
    p = (e2[:, None] * M.E4M3[None, :0x7F]).astype(np.float32)
    assert p.shape == (15, 127)
    assert np.array_equal(p.astype(np.float16).astype(np.float32), p) and np.array_equal(synth._repr(p, "bf16"), p)
    nz = np.abs(p[p != 0])
    assert nz.max() == 2688.0 and nz.min() == 2.0 ** -10
