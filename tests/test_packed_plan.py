"""What a packed prompt batch does (bz_packed_plan, bz_route.hip) against its restatement (tests/packed_ref.py, on prompt_plan_ref.plan), over the trait families
and switch sets of test_prompt_plan.py and the length sets of packed_cases.py; its refusals; and the two host-side definitions of bz_score_batch (default targets,
per-input totals).  No device is needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import packed_cases as PC  # noqa: E402
import packed_ref as PR  # noqa: E402
import prompt_plan_ref as R  # noqa: E402
from test_prompt_plan import FAMILIES, SWITCHES, c_traits, llama  # noqa: E402
from blazr_amd import _lib as L, runtime  # noqa: E402

LENS = dict(PC.SETS, floor=PC.BELOW_FLOOR)
REP3 = dict(llama(L.F16, nq=6, nkv=2, hd=64, proj_16=1, exact_cap=2, spec_head=1, head_rows=1, head_gemm=1), shapes_ok=0)     # group of 3: shapes_ok is 0 for it


def c_packed(ct, sw, lens, kv_dtype):
    return runtime.packed_plan(ct, lens, kv_dtype, L.PromptSwitches(**dict(R.DEFAULT_SWITCHES, **sw)))


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_sweep_against_the_restatement(family):
    t = FAMILIES[family]
    ct = c_traits(t)
    n = 0
    for swn, sw in SWITCHES.items():
        for name, lens in LENS.items():
            for kv_dtype in ((t["act_dtype"], L.F16) if t["arch"] == L.ARCH_DEEPSEEK2 else (t["act_dtype"],)):
                got, want = c_packed(ct, sw, lens, kv_dtype), PR.plan(t, sw, lens, kv_dtype)
                assert got == want, (family, swn, name, kv_dtype, got, want)
                # packed never comes with a plan that is not ROWS, and is exactly the prompt plan of T rows at the longest input
                single = runtime.prompt_plan(ct, L.PLAN_PROMPT, sum(lens), max(lens), kv_dtype, L.PromptSwitches(**dict(R.DEFAULT_SWITCHES, **sw)))
                assert got["packed"] == int(single["route"] == L.ROUTE_ROWS)
                assert not got["packed"] or (got["plan"] == single and got["plan"]["route"] == L.ROUTE_ROWS)
                assert (got["rows"], got["n_seq"], got["max_len"]) == (sum(lens), len(lens), max(lens))
                n += 1
    assert n >= len(SWITCHES) * len(LENS)


def test_both_answers_occur():
    seen = set()
    for t in FAMILIES.values():
        for sw in SWITCHES.values():
            for lens in LENS.values():
                seen.add(c_packed(c_traits(t), sw, lens, t["act_dtype"])["packed"])
    assert seen == {0, 1}


def test_anchors():
    mfma = L.PF_ATTN_SCALAR if "BZ_NO_PF_ATTN_MFMA" in os.environ else L.PF_ATTN_MFMA
    p = c_packed(c_traits(FAMILIES["awq"]), {}, PC.SETS["B"], L.F16)
    assert p == dict(packed=1, rows=675, n_seq=12, max_len=129, plan=dict(route=L.ROUTE_ROWS, exact=0, attn=mfma, head=L.HEAD_GEMM, chunk=2048))
    # [5, 4, 7]: 16 rows, the exact rows of an f16 int4 model; a dense model keeps 16 rows on the decode step, so its inputs go one by one
    assert c_packed(c_traits(FAMILIES["awq"]), {}, [5, 4, 7], L.F16)["plan"] == dict(route=L.ROUTE_ROWS, exact=1, attn=L.PF_ATTN_SCALAR_EXACT, head=L.HEAD_GEMV_ROWS, chunk=2048)
    assert c_packed(c_traits(FAMILIES["bf16"]), {}, [5, 4, 7], L.BF16)["packed"] == 0
    assert c_packed(c_traits(FAMILIES["bf16"]), {}, PC.SETS["C"], L.BF16)["packed"] == 1
    assert c_packed(c_traits(FAMILIES["q4km"]), {}, PC.SETS["B"], L.F32)["plan"]["attn"] == L.PF_ATTN_SCALAR_EXACT
    # below the row floor, odd groups, head_dim 96, DeepSeek-V2, Mamba2: the single-input path
    for fam, lens in (("awq", PC.BELOW_FLOOR), ("hd96", PC.SETS["B"]), ("dsv2", PC.SETS["B"]), ("mamba2", PC.SETS["B"]), ("gptq-act-order", PC.SETS["B"])):
        t = FAMILIES[fam]
        assert c_packed(c_traits(t), {}, lens, t["act_dtype"])["packed"] == 0, fam
    for sw in SWITCHES.values():
        for lens in LENS.values():
            assert c_packed(c_traits(REP3), sw, lens, L.F16)["packed"] == 0
            assert c_packed(c_traits(FAMILIES["hd96"]), sw, lens, L.F16)["packed"] == 0
    # the context of the plan is the longest input, not the batch: 40 inputs of 16 000 tokens fit the exact scalar kernel's LDS (16 360 keys at 4 / 2 heads of 64)
    assert c_packed(c_traits(FAMILIES["q4km"]), {}, [16000] * 40, L.F32)["packed"] == 1
    assert c_packed(c_traits(FAMILIES["q4km"]), {}, [17000, 8], L.F32)["packed"] == 0


def test_refusals():
    ct = c_traits(FAMILIES["awq"])
    for lens, figure in (([], "n_seq = 0"), ([4, 0, 3], "seq_lens[1] = 0"), ([4, -2], "seq_lens[1] = -2"), ([2 ** 30, 2 ** 30], "2^31")):
        with pytest.raises(PR.Refused):
            PR.plan(FAMILIES["awq"], {}, lens, L.F16)
        with pytest.raises(L.BlazrHipError) as e:
            runtime.packed_plan(ct, lens)
        assert e.value.code == L.E_INVALID and figure in str(e.value), str(e.value)
    assert runtime.packed_plan(ct, [2 ** 30, 2 ** 30 - 1])["rows"] == 2 ** 31 - 1


@pytest.mark.parametrize("name", sorted(LENS))
def test_default_targets_and_totals(name):
    """the host definitions bz_score_batch applies: targets from the packed tokens, totals from the records (built here with bz_score_row_spec on random rows, some
    rows not scored, one logprob made -inf)"""
    lens = LENS[name][:6] if name == "E" else LENS[name]
    lens = [min(n, 50) for n in lens]
    V = 97
    tok = np.concatenate(PC.token_lists(lens, V, seed=3))
    tg = runtime.packed_targets_spec(tok, lens)
    assert np.array_equal(tg, PR.default_targets(tok, lens))
    off = PC.offsets(lens)
    assert all(tg[off[i + 1] - 1] == -1 for i in range(len(lens))) and np.count_nonzero(tg == -1) == len(lens)
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((len(tok), V)) * 3.0).astype(np.float32)
    if len(tok) > 3:
        x[2, :] = -np.inf
        x[2, (tg[2] + 1) % V] = 0.0                                # the target's logprob is -inf: scored, not counted
    rows = np.stack([runtime.score_row_spec(x[r], int(tg[r]), 2) for r in range(len(tok))])
    got, want = runtime.packed_totals_spec(rows, lens), PR.totals(rows["logprob"], rows["n_top"], lens)
    assert got == want
    assert [k for _, k in got] == [int(np.count_nonzero((rows["n_top"][off[i]:off[i + 1]] >= 0) & np.isfinite(rows["logprob"][off[i]:off[i + 1]]))) for i in range(len(lens))]
