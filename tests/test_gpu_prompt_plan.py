"""The traits bz_model_finalize records of real (synthetic) models, field by field against hand-written expectations, and the route anchors of
tests/test_prompt_plan.py through bz_prompt_plan(traits, NULL, ...): the process's own switches, which must be unset here.  No forward pass."""
import os

import pytest

from blazr_amd import _lib as L, runtime, synth

pytestmark = pytest.mark.gpu
SWITCHES = ("BZ_PREFILL_MIN", "BZ_NO_MFMA_PREFILL", "BZ_NO_GGUF_PREFILL", "BZ_EXACT_PREFILL", "BZ_EXACT_PREFILL_MAX", "BZ_EXACT_I8_MAX", "BZ_NO_PF_ATTN_MFMA")
STEPS, ROWS, DSV2, MAMBA = L.ROUTE_STEPS, L.ROUTE_ROWS, L.ROUTE_DSV2, L.ROUTE_MAMBA

TINY_LLAMA = dict(arch=L.ARCH_LLAMA, hidden=256, inter=512, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=64, rep=2, sliding_window=0, shapes_ok=1)
DENSE16 = dict(TINY_LLAMA, act_dtype=L.BF16, proj_16=1, any_dense=1, exact_cap=0, gq_all=0, head_rows=1, head_gemm=1, spec_head=0)     # tied bf16 head
TINY_DSV2 = dict(arch=L.ARCH_DEEPSEEK2, hidden=256, n_heads=4, mla_q_lora_rank=0, mla_rope_dim=32, mla_nope_dim=64, ds_dims_ok=1, head_rows=1, head_gemm=1)
CASES = {
    # every projection int4 without act-order with K in {256, 512} (multiples of 128: the integer-MFMA form too), dense f16 lm_head of K = 256
    "tiny-awq": (synth.make_llama, {}, dict(TINY_LLAMA, act_dtype=L.F16, proj_16=1, any_dense=0, exact_cap=2, gq_all=0, head_rows=1, head_gemm=1, spec_head=1)),
    "tiny-gptq": (synth.make_llama, dict(act_order=True), dict(TINY_LLAMA, act_dtype=L.F16, proj_16=0, any_dense=0, exact_cap=0, gq_all=0, head_rows=1, head_gemm=1,
                                                               spec_head=1)),
    "tiny-bf16": (synth.make_llama, {}, DENSE16),
    "tiny-fp8": (synth.make_llama, {}, DENSE16),
    # Q4_K / Q6_K parts, K 256 and 512; the widest fused linear is gate|up: 1024 x 3 x 256; Q6_K lm_head (fixed-point output)
    "tiny-q4km": (synth.make_llama, {}, dict(TINY_LLAMA, n_layers=8, act_dtype=L.F32, proj_16=0, any_dense=0, exact_cap=0, gq_all=1, gq_max_k=512, gq_max_n3k=1024 * 3 * 256,
                                             head_rows=0, head_gemm=0, spec_head=0)),
    "tiny-dsv2": (synth.make_dsv2, {}, dict(TINY_DSV2, act_dtype=L.BF16, n_layers=3, mla_kv_lora_rank=128, mla_v_dim=64, ds_weights_act=1)),
    "tiny-dsv2-f32": (synth.make_dsv2, {}, dict(TINY_DSV2, act_dtype=L.F32, n_layers=2, mla_kv_lora_rank=64, mla_v_dim=32)),
    "tiny-mamba2": (synth.make_mamba2, {}, dict(arch=L.ARCH_MAMBA2, act_dtype=L.BF16, hidden=256, n_layers=3, ssm_scan_ok=1, ssm_groups_ok=1, ssm_proj_ok=1, head_rows=1,
                                                head_gemm=1)),
}


def _traits(device, preset, over=None):
    make, base, _ = CASES[preset]
    return runtime.prompt_traits(runtime.LoadedModel.from_synth(device, make(preset, **dict(base, **(over or {})))))


def _route(t, kind, rows, total_len=None, kv=None):
    return runtime.prompt_plan(t, kind, rows, total_len or rows, t.act_dtype if kv is None else kv)


@pytest.fixture(autouse=True)
def _switches_unset():
    assert not [s for s in SWITCHES if s in os.environ], "the route switches are read once per process: run this module without them"


@pytest.mark.parametrize("preset", sorted(CASES))
def test_traits_and_anchors(device, preset):
    t = _traits(device, preset)
    got = {k: getattr(t, k) for k in CASES[preset][2]}
    print(preset, {n: getattr(t, n) for n, _ in L.PromptTraits._fields_})
    assert got == CASES[preset][2]
    P, B, V = L.PLAN_PROMPT, L.PLAN_DECODE_BATCH, L.PLAN_VERIFY
    if preset == "tiny-awq":
        assert _route(t, P, 16) == dict(route=ROWS, exact=1, attn=L.PF_ATTN_SCALAR_EXACT, head=L.HEAD_GEMV_ROWS, chunk=2048)
        assert _route(t, P, 17) == dict(route=ROWS, exact=0, attn=L.PF_ATTN_MFMA, head=L.HEAD_GEMM, chunk=2048)
        assert _route(t, V, 16, 56) == dict(route=ROWS, exact=1, attn=L.PF_ATTN_SCALAR_EXACT, head=L.HEAD_SPEC, chunk=2048)
        assert _route(t, B, 2, 100) == dict(route=ROWS, exact=0, attn=L.PF_ATTN_ROWS, head=L.HEAD_GEMM, chunk=512)
        assert _route(t, P, 7)["route"] == STEPS
    elif preset == "tiny-gptq":
        assert _route(t, B, 2, 100)["route"] == STEPS and _route(t, P, 40)["route"] == STEPS and _route(t, V, 4, 44)["route"] == STEPS
    elif preset in ("tiny-bf16", "tiny-fp8"):
        assert _route(t, P, 16)["route"] == STEPS and _route(t, P, 17)["route"] == ROWS and _route(t, V, 16, 56)["route"] == STEPS
        assert _route(t, B, 2, 100)["route"] == ROWS
    elif preset == "tiny-q4km":
        assert _route(t, P, 8) == dict(route=ROWS, exact=0, attn=L.PF_ATTN_SCALAR_EXACT, head=L.HEAD_STEP, chunk=2048)
        assert _route(t, P, 7)["route"] == STEPS and _route(t, P, 17000)["route"] == STEPS
    elif preset == "tiny-dsv2":
        assert _route(t, P, 13)["route"] == STEPS and _route(t, P, 16)["route"] == STEPS
        assert _route(t, P, 17) == dict(route=DSV2, exact=0, attn=L.PF_ATTN_NONE, head=L.HEAD_GEMM, chunk=512)
    elif preset == "tiny-dsv2-f32":
        assert _route(t, P, 17)["route"] == STEPS and _route(t, P, 200)["route"] == STEPS
    else:
        assert _route(t, P, 16)["route"] == STEPS
        assert _route(t, P, 17) == dict(route=MAMBA, exact=0, attn=L.PF_ATTN_NONE, head=L.HEAD_GEMV_ROWS, chunk=512)


def test_window_and_q_lora_variants(device):
    """a window of 24 keys on every layer admits the 17 000-row prompt of tiny-q4km; a q-lora DeepSeek-V2 model never batches"""
    t = _traits(device, "tiny-q4km", dict(sliding_window=24, max_seq_len=17024))
    assert t.sliding_window == 24 and _route(t, L.PLAN_PROMPT, 17000)["route"] == ROWS
    t = _traits(device, "tiny-dsv2", dict(q_lora_rank=96))
    assert t.mla_q_lora_rank == 96 and _route(t, L.PLAN_PROMPT, 17)["route"] == STEPS
