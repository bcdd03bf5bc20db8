"""Which kernels a decode step launches (bz_layer_plan, bz_step_plan.hip) over hand-built layer traits and explicit switches.  No device is needed.

The expectations are launches recorded on an MI355X: profiles/step_census.json (scripts/step_census.py) and the table tests/test_gpu_irregular_shapes.py held
before it pointed here -- written out below per case, and held to the record file by test_expectations_are_the_record.  tests/test_gpu_step_plan.py checks the
same prediction, through the same name map (tests/step_plan_cases.py), against what a loaded model's step reports."""
import itertools
import json
import os
import sys
from collections import Counter

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step_plan_cases as S  # noqa: E402
from blazr_amd import _lib as L, runtime  # noqa: E402

SWITCH_NAMES = [n for n, _ in L.StepSwitches._fields_]
MLPQ, MLPD = S.MLP_LABEL[L.MLP_Q4G], S.MLP_LABEL[L.MLP_DENSE]
DENSE_HEAD = {"embed": 1, "argmax_final": 1, "gemv_rows<lm_head+argmax>": 1}


def sw(**kw):
    return L.StepSwitches(**kw)


def plan(t, kv, **switches):
    return runtime.layer_plan(t, kv, sw(**switches))


def census(layers, kv, long=False, **switches):
    c = Counter()
    for t in layers:
        c += S.layer_census(t, plan(t, kv, **switches), long)
    c.pop(S.FIX_BIAS, None)      # (the table predates the bias pass; tests/test_gpu_step_plan.py counts these launches too)
    return dict(c)


# name -> layers (two each), cache dtype, record key in profiles/step_census.json, the head's launches, and the layers' launches at position 8 and at 269 under
# BZ_SPLIT_MIN=4 as the record has them
CASES = {
    # H 4096, I 14336, 32 / 8 heads of 128, f16 cache: slim q/k/v, attn+o_proj, split + merge fused with o_proj beyond the threshold, the fused int4 MLP
    "llama3-8b-awq": dict(layers=[S.q4g_layer(4096, 14336, 32, 8, 128)] * 2, kv=L.F16, record="llama3-8b-awq-2l-v4096", head=DENSE_HEAD,
                          short={"gemv_q4g<norm>": 2, "attn+o_proj": 2, MLPQ: 2}, long={"gemv_q4g<norm>": 2, "attn_split": 2, "attn_merge+o_proj": 2, MLPQ: 2}),
    # H 2048, I 8192, 32 / 8 heads of 64: no split pair at head_dim 64 -- the long form is plain attention + the o_proj GEMV (the oddity DESIGN.md records)
    "llama3.2-1b-bf16": dict(layers=[S.dense_layer(2048, 8192, 32, 8, 64, down_slabs=1)] * 2, kv=L.BF16, record="llama3.2-1b-bf16-2l-v4096", head=DENSE_HEAD,
                             short={"gemv_rows2<norm>": 2, "attn+o_proj<dense>": 2, MLPD: 2},
                             long={"gemv_rows2<norm>": 2, "attn_decode": 2, "gemv_rows2": 2, MLPD: 2}),
    # f32 activations and cache; q, k Q4_K and v Q6_K in the layer the rule gives more bits: the mixed slim launch; gate/up and down on the slim kernels
    "mistral-7b-q4km": dict(layers=[S.q4km_layer(4096, 14336, 32, 8, 128, True), S.q4km_layer(4096, 14336, 32, 8, 128, False)], kv=L.F32,
                            record="mistral-7b-q4km-2l-v4096", head={"embed": 1, "argmax_final": 1, "gemv_q6_K<slim>": 1},
                            short={"gemv_q4_K+q6_K<slim>": 1, "gemv_q4_K<slim>": 4, "gemv_q6_K<slim>": 1, "attn+o_proj<q4_K>": 2},
                            long={"gemv_q4_K+q6_K<slim>": 1, "gemv_q4_K<slim>": 4, "gemv_q6_K<slim>": 1, "attn_decode": 2, "gemv_q4_K": 2}),
    "awq-g3": dict(layers=[S.q4g_layer(768, 1408, 6, 2, 128)] * 2, kv=L.F16, record="awq-g3", head=DENSE_HEAD,
                   short={"gemv_q4g<norm>": 4, "attn_decode": 2, "gemv_q4g<plain>": 2, "gemv_q4g<silu>": 2}, long=None),
    "bf16-g3-hd64": dict(layers=[S.dense_layer(384, 704, 6, 2, 64)] * 2, kv=L.BF16, record="bf16-g3-hd64", head=DENSE_HEAD,
                         short={"gemv_rows2<norm>": 4, "attn_decode": 2, "gemv_rows2": 2, "gemv_rows2<silu>": 2}, long=None),
    "bf16-g2-w768": dict(layers=[S.dense_layer(768, 1408, 6, 3, 128)] * 2, kv=L.BF16, record="bf16-g2-w768", head=DENSE_HEAD,
                         short={"gemv_rows2<norm>": 4, "attn_decode": 2, "gemv_rows2": 2, "gemv_rows2<silu>": 2},
                         long={"gemv_rows2<norm>": 4, "attn_split": 2, "attn_merge": 2, "gemv_rows2": 2, "gemv_rows2<silu>": 2}),
    # act-order: q, k, v, gate, up each a norm launch of its own
    "gptq-g6": dict(layers=[S.gptq_actorder_layer(768, 1152, 12, 2, 64)] * 2, kv=L.F16, record="gptq-g6", head=DENSE_HEAD,
                    short={"gemv_q4g<norm>": 10, "attn_decode": 2, "gemv_q4g<plain>": 2, "gemv_q4g<silu>": 2}, long=None),
    # K = 768 is no slim norm width: the generic GGUF kernels, but the slim SILU GEMV on down (K = 1280, five superblocks)
    "q4km-g3": dict(layers=[S.q4km_layer(768, 1280, 6, 2, 128, False), S.q4km_layer(768, 1280, 6, 2, 128, True)], kv=L.F32, record="q4km-g3",
                    head={"embed": 1, "argmax_final": 1, "gemv_q6_K": 1},
                    short={"gemv_q4_K": 6, "gemv_q6_K": 1, "attn_decode": 2, "gemv_q4_K<slim>": 1, "gemv_q6_K<slim>": 1}, long=None),
    "q8_0-g7": dict(layers=[S.one_kind_layer(L.LIN_Q80, 768, 1280, 28, 4, 64)] * 2, kv=L.F32, record="q8_0-g7", head={"embed": 1, "argmax_final": 1, "gemv_q8_0": 1},
                    short={"gemv_q8_0": 8, "attn_decode": 2}, long=None),
}
for _c in CASES.values():
    _c["long"] = _c["long"] or _c["short"]      # nothing fused and no split pair (a GQA group of 3 / 6 / 7, an f32 cache): the same launches at every context


@pytest.mark.parametrize("name", sorted(CASES))
def test_recorded_launches(name):
    c = CASES[name]
    assert census(c["layers"], c["kv"]) == c["short"]
    assert census(c["layers"], c["kv"], long=True) == c["long"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_expectations_are_the_record(name):
    """the literals above, plus the head, are the entries of profiles/step_census.json"""
    c = CASES[name]
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "step_census.json")) as f:
        rec = json.load(f)["cases"]
    for key, want in ((c["record"] + "@8", c["short"]), (c["record"] + "@269/split4", c["long"])):
        got = {n: k for n, k, _ in rec[key] if n != S.FIX_BIAS}
        assert got == dict(Counter(want) + Counter(c["head"])), key


def test_named_forms():
    """the forms behind the labels that two kernels share"""
    p = plan(CASES["llama3-8b-awq"]["layers"][0], L.F16)
    assert p["qkv"][0] == L.GEMV_Q4G_SLIM and p["gateup"][0] == L.GEMV_Q4G and p["attn_short"] == L.ATTN_FUSED_Q4G and p["attn_long"] == L.ATTN_SPLIT_FUSED and p["mlp"] == L.MLP_Q4G
    p = plan(CASES["llama3.2-1b-bf16"]["layers"][0], L.BF16)
    assert (p["attn_short"], p["attn_long"], p["attn_kernel"], p["mlp"]) == (L.ATTN_FUSED_DENSE, L.ATTN_PLAIN, L.ATTN_K_ATTN2, L.MLP_DENSE)
    assert plan(CASES["llama3.2-1b-bf16"]["layers"][0], L.F16)["attn_short"] == L.ATTN_PLAIN        # the fused dense form reads weights in the cache's dtype
    p = plan(CASES["mistral-7b-q4km"]["layers"][0], L.F32)
    assert (p["qkv_mix"], p["attn_short"], p["attn_kernel"], p["mlp"], p["o"][0]) == (1, L.ATTN_FUSED_Q4K, L.ATTN_K_ATTN2F, L.MLP_SPLIT, L.GEMV_GQ)
    assert p["gateup"][0] == L.GEMV_GQ_SLIM and p["down"][0] == L.GEMV_GQ_SLIM
    p = plan(CASES["q4km-g3"]["layers"][1], L.F32)
    assert (p["qkv_mix"], p["qkv"][:2], p["down"][0], p["attn_kernel"]) == (0, [L.GEMV_GQ, L.GEMV_GQ], L.GEMV_GQ_SLIM, L.ATTN_K_ATTN2F)
    p = plan(CASES["bf16-g3-hd64"]["layers"][0], L.BF16)
    assert (p["attn_short"], p["attn_long"], p["attn_kernel"], p["mlp"]) == (L.ATTN_PLAIN, L.ATTN_PLAIN, L.ATTN_K_ATTN2, L.MLP_SPLIT)


# ---- switches: each flips the plan fields INTEGRATION.md names for it, on the families it names, and nothing else -------------------------------------------
def _dsv2_moe():
    r = S.fused(S.lin(L.LIN_ROWS, 1024, 256, wdt=L.BF16, sk=2))
    t = L.LayerTraits(arch=L.ARCH_DEEPSEEK2, act_dtype=L.BF16, hidden=256, inter=512, n_heads=4, qkv=r, o=r, is_moe=1, e_dt=L.BF16, router_dt=L.BF16, moe_inter=128,
                      moe_n_experts=8, moe_slots=3)
    t.mla_x_ok[L.BF16] = 1
    return t


def _mamba():
    return L.LayerTraits(arch=L.ARCH_MAMBA2, act_dtype=L.BF16, hidden=256, qkv=S.fused(S.lin(L.LIN_ROWS, 1304, 256, wdt=L.BF16), fix_out=0),
                         o=S.fused(S.lin(L.LIN_ROWS, 256, 512, wdt=L.BF16, sk=2)), ssm_d_inner=512, ssm_n_groups=1)


FAMILIES = {"awq-8b": (CASES["llama3-8b-awq"]["layers"][0], L.F16), "bf16-1b": (CASES["llama3.2-1b-bf16"]["layers"][0], L.BF16),
            "q4km-7b": (CASES["mistral-7b-q4km"]["layers"][0], L.F32), "awq-g3": (CASES["awq-g3"]["layers"][0], L.F16), "dsv2-moe": (_dsv2_moe(), L.BF16),
            "mamba2": (_mamba(), L.BF16)}
FLIPS = {
    "no_slim_qkv": {"awq-8b": {"qkv"}},                                   # gate/up (N 28672) is beyond the slim kernel's 16384 columns either way
    "no_gq_slim": {"q4km-7b": {"qkv_mix", "qkv", "gateup", "down"}},
    "no_gq_mix": {"q4km-7b": {"qkv_mix"}},
    "no_rows2": {"bf16-1b": {"qkv", "o", "gateup", "down"}, "dsv2-moe": {"qkv", "o", "moe_rows2", "moe_route_fused"}, "mamba2": {"o"}},
    "no_attn_fusion": {"awq-8b": {"attn_short", "attn_long"}, "bf16-1b": {"attn_short"}, "q4km-7b": {"attn_short"}},
    "no_attn_split": {"awq-8b": {"attn_long"}},
    "no_attn_f32": {"q4km-7b": {"attn_short", "attn_kernel"}},
    "no_attn2_hd64": {"bf16-1b": {"attn_short", "attn_kernel"}},
    "no_mlp_fusion": {"awq-8b": {"mlp"}, "bf16-1b": {"mlp"}},
    "gguf_mlp_fusion": {"q4km-7b": {"mlp"}},
    "dsv2_f32_sums": {"dsv2-moe": {"mla_exact"}},
    "no_moe_route_fusion": {"dsv2-moe": {"moe_route_fused"}},
}


@pytest.mark.parametrize("switch", SWITCH_NAMES)
def test_each_switch_flips_its_entries_and_no_others(switch):
    assert set(FLIPS) == set(SWITCH_NAMES)
    for fam, (t, kv) in FAMILIES.items():
        a, b = plan(t, kv), plan(t, kv, **{switch: 1})
        assert {k for k in a if a[k] != b[k]} == FLIPS[switch].get(fam, set()), (switch, fam, a, b)


def test_switch_targets():
    """... and to what: the fallback INTEGRATION.md names"""
    t, kv = FAMILIES["awq-8b"]
    assert plan(t, kv, no_slim_qkv=1)["qkv"][0] == L.GEMV_Q4G and plan(t, kv, no_mlp_fusion=1)["mlp"] == L.MLP_SPLIT
    assert (plan(t, kv, no_attn_fusion=1)["attn_short"], plan(t, kv, no_attn_fusion=1)["attn_long"]) == (L.ATTN_PLAIN, L.ATTN_SPLIT)
    assert plan(t, kv, no_attn_split=1)["attn_long"] == L.ATTN_PLAIN
    t, kv = FAMILIES["bf16-1b"]
    assert plan(t, kv, no_rows2=1)["qkv"][0] == L.GEMV_ROWS and plan(t, kv, no_attn2_hd64=1)["attn_kernel"] == L.ATTN_K_DECODE
    t, kv = FAMILIES["q4km-7b"]
    assert plan(t, kv, no_gq_slim=1)["gateup"][0] == L.GEMV_GQ and plan(t, kv, no_attn_f32=1)["attn_kernel"] == L.ATTN_K_DECODE
    assert plan(t, kv, gguf_mlp_fusion=1)["mlp"] == L.MLP_GQ and plan(t, kv, gguf_mlp_fusion=1, no_mlp_fusion=1)["mlp"] == L.MLP_SPLIT
    t, kv = FAMILIES["dsv2-moe"]
    p = plan(t, kv)
    assert (p["mla_exact"], p["moe_route_fused"], p["moe_rows2"]) == (1, 1, 1) and plan(t, L.F16)["mla_exact"] == 0
    assert plan(t, kv, no_moe_route_fusion=1)["moe_rows2"] == 1 and plan(t, kv, no_rows2=1)["moe_rows2"] == 0
    t, kv = FAMILIES["mamba2"]
    assert (plan(t, kv)["qkv"][0], plan(t, kv)["o"][0]) == (L.GEMV_ROWS, L.GEMV_ROWS2)       # in_proj stores f32 directly; out_proj accumulates


# ---- LoRA masks and windows ------------------------------------------------------------------------------------------------------------------------------------
def test_lora_mask_unfuses():
    for mk, kv in ((lambda **kw: S.q4g_layer(4096, 14336, 32, 8, 128, **kw), L.F16), (lambda **kw: S.dense_layer(2048, 8192, 32, 8, 64, down_slabs=1, **kw), L.BF16)):
        base, o, mlp = plan(mk(), kv), plan(mk(lora_o=1), kv), plan(mk(lora_mlp=1), kv)
        assert base["attn_short"] != L.ATTN_PLAIN and base["mlp"] != L.MLP_SPLIT
        assert o["attn_short"] == L.ATTN_PLAIN and o["attn_long"] in (L.ATTN_PLAIN, L.ATTN_SPLIT) and o["mlp"] == base["mlp"]     # an o_proj adapter reads the attention output
        assert mlp["mlp"] == L.MLP_SPLIT and (mlp["attn_short"], mlp["attn_long"]) == (base["attn_short"], base["attn_long"])
        assert {k for k in base if base[k] != o[k]} <= {"attn_short", "attn_long"} and {k for k in base if base[k] != mlp[k]} == {"mlp"}


def test_window_at_most_split_min_stays_short():
    """the one decision the step takes per call (bz_step_attn_form): a windowed layer reads min(keys, W) keys, and the choice is made on that many"""
    p = L.LayerPlan(attn_short=L.ATTN_FUSED_Q4G, attn_long=L.ATTN_SPLIT_FUSED)
    form = L.lib().bz_step_attn_form
    for keys in (1, 512, 513, 4096, 1 << 20):
        assert form(p, 0, keys, 512) == (L.ATTN_FUSED_Q4G if keys <= 512 else L.ATTN_SPLIT_FUSED)
        assert form(p, 512, keys, 512) == form(p, 24, keys, 512) == L.ATTN_FUSED_Q4G
        assert form(p, 513, keys, 512) == (L.ATTN_FUSED_Q4G if keys <= 512 else L.ATTN_SPLIT_FUSED)
    assert form(p, 0, 270, 4) == L.ATTN_SPLIT_FUSED and form(p, 4, 270, 4) == L.ATTN_FUSED_Q4G and form(p, 5, 270, 4) == L.ATTN_SPLIT_FUSED
    for keys, W, sm in itertools.product((1, 5, 270, 4096), (0, 4, 300), (4, 512)):
        assert (form(p, W, keys, sm) == L.ATTN_SPLIT_FUSED) == S.is_long(L.LayerTraits(window=W), keys - 1, sm)


# ---- property sweep: every form a plan names passes that form's own preconditions -------------------------------------------------------------------------------
def _formats():
    out = {}
    for H, I, nq, nkv, hd in ((4096, 14336, 32, 8, 128), (2048, 5632, 16, 4, 128), (8192, 2048, 16, 2, 128), (2048, 8192, 32, 8, 64), (768, 1408, 6, 2, 128), (768, 1280, 6, 3, 128),
                              (256, 512, 4, 2, 64), (896, 640, 14, 2, 64)):
        g = "%d-%d/%dx%d" % (H, nq, nkv, hd)
        out["awq-" + g] = S.q4g_layer(H, I, nq, nkv, hd)
        out["awq-bf16act-" + g] = S.q4g_layer(H, I, nq, nkv, hd, act=L.BF16)
        out["awq-lora-" + g] = S.q4g_layer(H, I, nq, nkv, hd, lora_o=1, lora_mlp=1)
        out["gptq-actorder-" + g] = S.gptq_actorder_layer(H, I, nq, nkv, hd)
        for dt in (L.F16, L.BF16):
            out["dense%d-%s" % (dt, g)] = S.dense_layer(H, I, nq, nkv, hd, dt=dt, down_slabs=1)
            out["dense%d-noslab-nosplit-%s" % (dt, g)] = S.dense_layer(H, I, nq, nkv, hd, dt=dt, sk=1)
        out["f32w-" + g] = S.dense_layer(H, I, nq, nkv, hd, dt=L.F32)
        for mb in (False, True):
            out["q4km%d-%s" % (mb, g)] = S.q4km_layer(H, I, nq, nkv, hd, mb)
        for kind in (L.LIN_Q80, L.LIN_Q5K, L.LIN_Q40, L.LIN_Q51, L.LIN_F8):
            out["kind%d-%s" % (kind, g)] = S.one_kind_layer(kind, H, I, nq, nkv, hd, act=L.BF16 if kind == L.LIN_F8 else L.F32)
    return out


def test_every_form_passes_its_own_predicate():
    seen = {k: set() for k in ("gemv", "attn", "kernel", "mlp")}
    settings = [{}] + [{n: 1} for n in SWITCH_NAMES] + [dict(no_attn_fusion=1, no_attn_split=1), dict(gguf_mlp_fusion=1, no_gq_slim=1), dict(no_rows2=1, no_mlp_fusion=1)]
    n = 0
    for (name, t), kv, st in itertools.product(_formats().items(), (L.F32, L.F16, L.BF16), settings):
        s, p = sw(**st), plan(t, kv, **st)
        where = (name, kv, st, p)
        for F, forms, mode, H in ((t.qkv, p["qkv"], S.NORM, t.hidden), (t.o, p["o"], S.PLAIN, 0), (t.gateup, p["gateup"], S.NORM, t.hidden), (t.down, p["down"], S.SILU, t.inter)):
            for i in range(3):
                assert (forms[i] == L.GEMV_NONE) == (i >= F.n_parts), where
                if i < F.n_parts:
                    assert S.gemv_form_ok(forms[i], F.parts[i], mode, H, t.act_dtype, s), where
                    seen["gemv"].add(forms[i])
        if p["qkv_mix"]:
            assert not s.no_gq_mix and t.qkv.n_parts == 2 and all(S.gemv_form_ok(L.GEMV_GQ_SLIM, t.qkv.parts[i], S.NORM, t.hidden, t.act_dtype, s) for i in (0, 1)), where
            assert (t.qkv.parts[0].kind, t.qkv.parts[1].kind) == (L.LIN_Q4K, L.LIN_Q6K), where
        assert S.attn_form_ok(p["attn_short"], t, kv, s) and p["attn_short"] not in (L.ATTN_SPLIT, L.ATTN_SPLIT_FUSED), where
        assert S.attn_form_ok(p["attn_long"], t, kv, s) and p["attn_long"] in (L.ATTN_PLAIN, L.ATTN_SPLIT, L.ATTN_SPLIT_FUSED), where
        assert S.attn_kernel_ok(p["attn_kernel"], t, kv, s) and S.mlp_form_ok(p["mlp"], t, s), where
        assert not (p["mla_exact"] or p["moe_route_fused"] or p["moe_rows2"] or p["gateup_mix"]), where
        seen["attn"] |= {p["attn_short"], p["attn_long"]}
        seen["kernel"].add(p["attn_kernel"])
        seen["mlp"].add(p["mlp"])
        n += 1
    assert n == 8 * 16 * 3 * 16      # shapes x formats x cache dtypes x switch settings
    assert seen == dict(gemv=set(range(1, 8)), attn=set(range(6)), kernel={0, 1, 2}, mlp={0, 1, 2, 3}), seen      # the sweep is not vacuous


def test_process_switches_and_bad_arguments():
    t = CASES["llama3-8b-awq"]["layers"][0]
    assert runtime.layer_plan(t, L.F16)["mlp"] in (L.MLP_Q4G, L.MLP_SPLIT)        # sw == NULL: whatever this process's environment says
    with pytest.raises(L.BlazrHipError):
        runtime.layer_plan(t, L.I64)
    with pytest.raises(L.BlazrHipError):
        runtime.layer_plan(L.LayerTraits(arch=7), L.F16)
    with pytest.raises(L.BlazrHipError):
        runtime.layer_plan(L.LayerTraits(arch=L.ARCH_LLAMA, n_kv_heads=2, qkv=L.FusedTraits(n_parts=4)), L.F16)
