"""Which path a prompt, a decode batch or a speculative verify takes (bz_prompt_plan, bz_route.hip) against its Python restatement (tests/prompt_plan_ref.py),
field for field, over hand-built traits and explicit switches.  No device is needed."""
import itertools
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prompt_plan_ref as R  # noqa: E402
from blazr_amd import _lib as L, runtime  # noqa: E402

assert (R.F32, R.F16, R.BF16) == (L.F32, L.F16, L.BF16) and (R.LLAMA, R.MAMBA2, R.DEEPSEEK2) == (L.ARCH_LLAMA, L.ARCH_MAMBA2, L.ARCH_DEEPSEEK2)
STEPS, ROWS, DSV2, MAMBA = L.ROUTE_STEPS, L.ROUTE_ROWS, L.ROUTE_DSV2, L.ROUTE_MAMBA
FIELDS = [n for n, _ in L.PromptTraits._fields_]


def traits(**kw):
    """a traits dict with every field (0 unless given); rep follows the heads"""
    t = dict.fromkeys(FIELDS, 0)
    t.update(kw)
    if t["n_kv_heads"]:
        t["rep"] = t["n_heads"] // t["n_kv_heads"]
    return t


def c_traits(t):
    return L.PromptTraits(**t)


def llama(act, nq=4, nkv=2, hd=64, layers=2, **kw):
    return traits(arch=L.ARCH_LLAMA, act_dtype=act, hidden=256, inter=512, n_layers=layers, n_heads=nq, n_kv_heads=nkv, head_dim=hd, shapes_ok=1, **kw)


HEAD16 = dict(head_rows=1, head_gemm=1)
FAMILIES = {
    # f16 int4 without act-order (tiny-awq: every projection has the integer-MFMA form too), and one whose K is no multiple of 128 somewhere
    "awq": llama(L.F16, proj_16=1, exact_cap=2, spec_head=1, **HEAD16),
    "awq-cap1": llama(L.F16, proj_16=1, exact_cap=1, spec_head=1, **HEAD16),
    "awq-8b-heads": llama(L.F16, nq=32, nkv=8, hd=128, layers=4, proj_16=1, exact_cap=2, spec_head=1, **HEAD16),
    "gptq-act-order": llama(L.F16, spec_head=1, **HEAD16),
    "bf16": llama(L.BF16, proj_16=1, any_dense=1, **HEAD16),
    "f16-dense": llama(L.F16, proj_16=1, any_dense=1, spec_head=1, **HEAD16),
    "fp8": llama(L.BF16, proj_16=1, any_dense=1, **HEAD16),
    "fp8-head": llama(L.BF16, proj_16=1, any_dense=1),                               # an fp8 lm_head: fixed-point output, no 16-bit GEMM
    "awq-head-k": llama(L.F16, proj_16=1, exact_cap=2, spec_head=1, head_rows=1),     # a head whose K is no multiple of 64
    "q4km": llama(L.F32, layers=8, gq_all=1, gq_max_k=512, gq_max_n3k=1024 * 3 * 256),
    "q4km-dense-head": llama(L.F32, gq_all=1, gq_max_k=512, gq_max_n3k=1024 * 3 * 256, **HEAD16),
    "gguf-wide": llama(L.F32, gq_all=1, gq_max_k=1 << 20, gq_max_n3k=1 << 32),
    "gguf-long-k": llama(L.F32, gq_all=1, gq_max_k=800000, gq_max_n3k=1 << 30),        # 2048 rows x 3 K pass 2^32, 1024 rows do not
    "gguf-biased": llama(L.F32, gq_max_k=512, gq_max_n3k=1024 * 3 * 256),
    "mixed-parts": llama(L.F16, spec_head=1, **HEAD16),                               # q/k/v in two formats: no single-part projection, not all block formats
    "hd96": dict(llama(L.F16, nq=6, nkv=2, hd=96, proj_16=1, exact_cap=2, spec_head=1, **HEAD16), shapes_ok=0),
    "hd32": llama(L.F16, nq=8, nkv=2, hd=32, proj_16=1, exact_cap=2, spec_head=1, **HEAD16),      # no MFMA attention at this head_dim: the plain scalar kernel
    "swa-all": llama(L.F16, proj_16=1, exact_cap=2, spec_head=1, sliding_window=24, **HEAD16),
    "swa-pattern-hit": llama(L.F16, layers=4, proj_16=1, exact_cap=2, spec_head=1, sliding_window=24, sliding_window_pattern=2, **HEAD16),
    "swa-pattern-miss": llama(L.F16, layers=3, proj_16=1, exact_cap=2, spec_head=1, sliding_window=24, sliding_window_pattern=4, **HEAD16),
    "swa-q4km": llama(L.F32, layers=8, gq_all=1, gq_max_k=512, gq_max_n3k=1024 * 3 * 256, sliding_window=24),
    "swa-wide": llama(L.F16, proj_16=1, exact_cap=2, spec_head=1, sliding_window=17000, **HEAD16),
    "dsv2": traits(arch=L.ARCH_DEEPSEEK2, act_dtype=L.BF16, hidden=256, n_layers=3, n_heads=4, mla_kv_lora_rank=128, mla_rope_dim=32, mla_nope_dim=64, mla_v_dim=64,
                   ds_dims_ok=1, ds_weights_act=1, **HEAD16),
    "dsv2-odd-v": traits(arch=L.ARCH_DEEPSEEK2, act_dtype=L.F16, hidden=256, n_layers=3, n_heads=4, mla_kv_lora_rank=512, mla_rope_dim=64, mla_nope_dim=128, mla_v_dim=72,
                         ds_dims_ok=1, ds_weights_act=1, head_rows=1),
    "dsv2-f32": traits(arch=L.ARCH_DEEPSEEK2, act_dtype=L.F32, hidden=256, n_layers=2, n_heads=4, mla_kv_lora_rank=64, mla_rope_dim=32, mla_nope_dim=64, mla_v_dim=32,
                       ds_dims_ok=1, ds_weights_act=1, **HEAD16),
    "dsv2-q-lora": traits(arch=L.ARCH_DEEPSEEK2, act_dtype=L.BF16, hidden=256, n_layers=3, n_heads=4, mla_q_lora_rank=96, mla_kv_lora_rank=128, mla_rope_dim=32,
                          mla_nope_dim=64, mla_v_dim=64, ds_dims_ok=1, ds_weights_act=1, **HEAD16),
    "dsv2-moe-inter": traits(arch=L.ARCH_DEEPSEEK2, act_dtype=L.BF16, hidden=256, n_layers=3, n_heads=4, mla_kv_lora_rank=128, mla_rope_dim=32, mla_nope_dim=64,
                             mla_v_dim=64, ds_weights_act=1, **HEAD16),
    "mamba2": traits(arch=L.ARCH_MAMBA2, act_dtype=L.BF16, hidden=256, n_layers=3, ssm_scan_ok=1, ssm_groups_ok=1, ssm_proj_ok=1, **HEAD16),
    "mamba2-k": traits(arch=L.ARCH_MAMBA2, act_dtype=L.BF16, hidden=200, n_layers=3, ssm_scan_ok=1, ssm_groups_ok=1, **HEAD16),
    "mamba2-f32": traits(arch=L.ARCH_MAMBA2, act_dtype=L.F32, hidden=256, n_layers=2, ssm_scan_ok=1, ssm_groups_ok=1, ssm_proj_ok=1, **HEAD16),
}
ROWS_SWEEP = [1, 7, 8, 16, 17, 40, 70, 2049]
SWITCHES = {
    "default": {}, "exact0": dict(exact=0), "exact1": dict(exact=1), "exact2": dict(exact=2), "exact-max0": dict(exact_max=0), "exact-max32": dict(exact_max=32),
    "i8-max128": dict(exact_i8_max=128), "prefill-min4": dict(prefill_min=4), "no-mfma": dict(no_mfma_prefill=1), "no-gguf": dict(no_gguf_prefill=1),
    "exact0-min4": dict(exact=0, prefill_min=4), "max32-i8-128": dict(exact_max=32, exact_i8_max=128),
}


def c_plan(ct, sw, kind, rows, total_len, kv_dtype):
    return runtime.prompt_plan(ct, kind, rows, total_len, kv_dtype, L.PromptSwitches(**dict(R.DEFAULT_SWITCHES, **sw)))


def context_edges(t):
    """at and one past every LDS limit that can decide for these traits, each also as a window's worth of keys"""
    if t["arch"] == L.ARCH_DEEPSEEK2:
        lim = R.mla_limit(t["mla_kv_lora_rank"], t["mla_rope_dim"], t["mla_nope_dim"], t["mla_v_dim"])
        assert R.mla_lds(t["mla_kv_lora_rank"], t["mla_rope_dim"], t["mla_nope_dim"], t["mla_v_dim"], lim) <= R.LDS < \
            R.mla_lds(t["mla_kv_lora_rank"], t["mla_rope_dim"], t["mla_nope_dim"], t["mla_v_dim"], lim + 1)
        return [lim, lim + 1]
    if t["arch"] != L.ARCH_LLAMA or not t["shapes_ok"]:
        return [4096]
    out = []
    for exact in (False, True):
        lim = R.scalar_attn_limit(t["n_heads"], t["n_kv_heads"], t["head_dim"], exact)
        assert R.scalar_attn_lds(t["n_heads"], t["n_kv_heads"], t["head_dim"], lim, exact) <= R.LDS < R.scalar_attn_lds(t["n_heads"], t["n_kv_heads"], t["head_dim"], lim + 1, exact)
        out += [lim, lim + 1]
    return out


def test_limits_restated():
    """the scalar kernel's limits as tests/test_rows_attn_plan.py documents them (plain sums), and the exact kernel's below them"""
    assert [R.scalar_attn_limit(rep * 2, 2, 128, False) for rep in (1, 2, 4, 8)] == [38888, 18416, 8180, 3062]
    assert R.scalar_attn_limit(4, 2, 64, False) == 18416 and R.scalar_attn_limit(4, 2, 64, True) == 16360
    assert R.scalar_attn_limit(32, 8, 128, True) == 6124          # (32 + 16 x 4 x 128) 8 + 16 len + 64 <= 160 KiB
    assert R.mla_limit(512, 64, 128, 128) == 31456          # DeepSeek-V2-Lite: (18 x 512 + 128 + 128 + 16 + len) 4 + 64 <= 160 KiB


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_sweep_against_the_restatement(family):
    t = FAMILIES[family]
    ct = c_traits(t)
    n = 0
    for (swn, sw), kind, rows in itertools.product(SWITCHES.items(), (L.PLAN_PROMPT, L.PLAN_DECODE_BATCH, L.PLAN_VERIFY), ROWS_SWEEP):
        for total_len in sorted({rows, rows + 40, 2048 + rows} | {e for e in context_edges(t) if e >= rows}):
            for kv_dtype in ((t["act_dtype"], L.F16) if t["arch"] == L.ARCH_DEEPSEEK2 else (t["act_dtype"],)):
                got, want = c_plan(ct, sw, kind, rows, total_len, kv_dtype), R.plan(t, sw, kind, rows, total_len, kv_dtype)
                assert got == want, (family, swn, kind, rows, total_len, kv_dtype, got, want)
                n += 1
    assert n >= 12 * 3 * 8 * 3


def test_routes_all_occur():
    """the sweep is not vacuous: every route, exact mode, attention form and head occurs in it"""
    seen = {k: set() for k in ("route", "exact", "attn", "head", "chunk")}
    for t in FAMILIES.values():
        ct = c_traits(t)
        for sw, kind, rows in itertools.product(SWITCHES.values(), (0, 1, 2), ROWS_SWEEP):
            for k, v in c_plan(ct, sw, kind, rows, rows + 40, t["act_dtype"]).items():
                seen[k].add(v)
    assert seen == dict(route={0, 1, 2, 3}, exact={0, 1, 2}, attn={0, 1, 2, 3, 4}, head={0, 1, 2, 3}, chunk={0, 512, 2048}) or \
        seen == dict(route={0, 1, 2, 3}, exact={0, 1, 2}, attn={0, 2, 3, 4}, head={0, 1, 2, 3}, chunk={0, 512, 2048}) and "BZ_NO_PF_ATTN_MFMA" in os.environ


# ---- literal anchors: what the existing GPU tests document, so that the restatement cannot drift along with the code ----
def _p(family, kind, rows, total_len=None, kv=None, **sw):
    t = FAMILIES[family]
    return c_plan(c_traits(t), sw, kind, rows, total_len or rows, t["act_dtype"] if kv is None else kv)


def test_anchor_awq_prompts():
    """test_gpu_exact_prefill.py: up to 16 rows the exact rows with the exact scalar attention, beyond them the MFMA path"""
    assert _p("awq", L.PLAN_PROMPT, 16) == dict(route=ROWS, exact=1, attn=L.PF_ATTN_SCALAR_EXACT, head=L.HEAD_GEMV_ROWS, chunk=2048)
    mfma = L.PF_ATTN_SCALAR if "BZ_NO_PF_ATTN_MFMA" in os.environ else L.PF_ATTN_MFMA
    assert _p("awq", L.PLAN_PROMPT, 17) == dict(route=ROWS, exact=0, attn=mfma, head=L.HEAD_GEMM, chunk=2048)
    assert _p("awq", L.PLAN_PROMPT, 7)["route"] == STEPS and _p("awq", L.PLAN_PROMPT, 8)["route"] == ROWS
    assert _p("awq", L.PLAN_PROMPT, 70, exact=2)["exact"] == 2 and _p("awq", L.PLAN_PROMPT, 16, exact=2)["exact"] == 1
    assert _p("awq-cap1", L.PLAN_PROMPT, 70, exact=2)["exact"] == 1
    assert _p("awq", L.PLAN_PROMPT, 70, exact=1)["exact"] == 1 and _p("awq", L.PLAN_PROMPT, 16, exact=0)["exact"] == 0
    assert _p("awq", L.PLAN_PROMPT, 100, exact_i8_max=128)["exact"] == 2 and _p("awq", L.PLAN_PROMPT, 129, exact_i8_max=128)["exact"] == 0


def test_anchor_dense_and_fp8():
    """test_gpu_fullwidth.py / test_gpu_fp8_weights.py: dense 16-bit and fp8 models keep prompts of up to 16 rows on the decode step"""
    for fam in ("bf16", "fp8"):
        assert _p(fam, L.PLAN_PROMPT, 16)["route"] == STEPS
        assert _p(fam, L.PLAN_PROMPT, 17)["route"] == ROWS and _p(fam, L.PLAN_PROMPT, 17)["exact"] == 0
        assert _p(fam, L.PLAN_PROMPT, 16, exact=0)["route"] == ROWS and _p(fam, L.PLAN_PROMPT, 4096, exact=1)["route"] == STEPS
    assert _p("fp8-head", L.PLAN_PROMPT, 40)["route"] == STEPS


def test_anchor_gguf():
    """test_gpu_swa_long.py: f32 block-format models batch from 8 rows with the exact scalar attention; a window of 24 keys admits a 17 000-row prompt that the
    whole context would not (16 360 keys at 4 / 2 heads of 64)"""
    assert _p("q4km", L.PLAN_PROMPT, 8) == dict(route=ROWS, exact=0, attn=L.PF_ATTN_SCALAR_EXACT, head=L.HEAD_STEP, chunk=2048)
    assert _p("q4km", L.PLAN_PROMPT, 17000)["route"] == STEPS
    assert _p("swa-q4km", L.PLAN_PROMPT, 17000)["route"] == ROWS
    assert _p("q4km", L.PLAN_PROMPT, 40, no_gguf_prefill=1)["route"] == STEPS
    assert _p("q4km-dense-head", L.PLAN_PROMPT, 40)["head"] == L.HEAD_GEMV_ROWS


def test_anchor_dsv2_and_mamba():
    """test_gpu_dsv2_prefill.py: 13 and 16 rows on the decode step, 17 batched; q-lora models never"""
    assert _p("dsv2", L.PLAN_PROMPT, 13)["route"] == STEPS and _p("dsv2", L.PLAN_PROMPT, 16)["route"] == STEPS
    assert _p("dsv2", L.PLAN_PROMPT, 17) == dict(route=DSV2, exact=0, attn=L.PF_ATTN_NONE, head=L.HEAD_GEMM, chunk=512)
    assert _p("dsv2", L.PLAN_PROMPT, 17, kv=L.F16)["route"] == STEPS                 # a cache in another dtype
    assert _p("dsv2-q-lora", L.PLAN_PROMPT, 17)["route"] == STEPS and _p("dsv2-f32", L.PLAN_PROMPT, 17)["route"] == STEPS
    assert _p("mamba2", L.PLAN_PROMPT, 16)["route"] == STEPS
    assert _p("mamba2", L.PLAN_PROMPT, 17) == dict(route=MAMBA, exact=0, attn=L.PF_ATTN_NONE, head=L.HEAD_GEMV_ROWS, chunk=512)
    assert _p("mamba2-k", L.PLAN_PROMPT, 17)["route"] == STEPS and _p("mamba2", L.PLAN_PROMPT, 4096, no_mfma_prefill=1)["route"] == STEPS


def test_anchor_verify_and_decode_batch():
    """test_gpu_speculative.py: 16 rows of an f16 int4 model verify in one pass with the multi-row head; a dense model's run on the decode step.
    test_gpu_engine.py / test_gpu_irregular_shapes.py: a decode batch of 2 shares the weights on int4 without act-order, never with act-order"""
    assert _p("awq", L.PLAN_VERIFY, 16, 56) == dict(route=ROWS, exact=1, attn=L.PF_ATTN_SCALAR_EXACT, head=L.HEAD_SPEC, chunk=2048)
    assert _p("awq", L.PLAN_VERIFY, 1, 200)["route"] == ROWS                         # no row floor, any position
    assert _p("bf16", L.PLAN_VERIFY, 16, 56)["route"] == STEPS and _p("awq", L.PLAN_VERIFY, 4, 40, exact=0)["route"] == STEPS
    assert _p("awq", L.PLAN_DECODE_BATCH, 2, 100) == dict(route=ROWS, exact=0, attn=L.PF_ATTN_ROWS, head=L.HEAD_GEMM, chunk=512)
    assert _p("bf16", L.PLAN_DECODE_BATCH, 2, 100)["route"] == ROWS                  # the short-prompt rule is for prompts
    assert _p("gptq-act-order", L.PLAN_DECODE_BATCH, 2, 100)["route"] == STEPS
    assert _p("awq", L.PLAN_DECODE_BATCH, 2, 100, no_mfma_prefill=1)["route"] == ROWS
    assert _p("dsv2", L.PLAN_DECODE_BATCH, 40, 100)["route"] == STEPS and _p("mamba2", L.PLAN_VERIFY, 4, 100)["route"] == STEPS


def test_process_switches_and_bad_arguments(monkeypatch):
    ct = c_traits(FAMILIES["awq"])
    assert runtime.prompt_plan(ct, L.PLAN_PROMPT, 40, 40)["route"] in (STEPS, ROWS)      # sw == NULL: whatever this process's environment says
    for bad in [dict(kind=3), dict(rows=0), dict(total_len=0)]:
        a = dict(dict(kind=0, rows=8, total_len=8), **bad)
        with pytest.raises(L.BlazrHipError):
            runtime.prompt_plan(ct, a["kind"], a["rows"], a["total_len"])
