"""The launch census a loaded model's layer plans predict (bz_model_layer_traits / bz_model_layer_plan through the name map of tests/step_plan_cases.py) against
what one decode step reports (bz_profile_step, iters=1), name for name and launch for launch: position 8 for every case and, for the Llama family, position 269
under BZ_SPLIT_MIN=4.  The full-width cases are two-layer cuts at vocab 4096, the smallest models that reach the fused kernels.  The plans are made under this
process's switches and the step runs under them, so the module holds under any switch setting; the fresh-process switch runs are tests/test_gpu_fullwidth.py's."""
import os
import sys
from collections import Counter

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import irregular_cases as ic  # noqa: E402
import step_plan_cases as S  # noqa: E402
from blazr_amd import _lib as L, runtime, synth  # noqa: E402

pytestmark = pytest.mark.gpu

CUT = dict(n_layers=2, vocab=4096, max_seq_len=512)
DENSE_HEAD, Q6K_HEAD, Q6K_SLIM_HEAD = "gemv_rows<lm_head+argmax>", "gemv_q6_K", "gemv_q6_K<slim>"       # (a Q4_K_M file stores output.weight as Q6_K; slim at K = 4096)
# name -> (model, the lm_head's launch)
LLAMA = {
    "tiny-awq": (lambda: synth.make_llama("tiny-awq", max_seq_len=512), DENSE_HEAD),
    "tiny-bf16": (lambda: synth.make_llama("tiny-bf16", max_seq_len=512), DENSE_HEAD),
    "tiny-q4km": (lambda: synth.make_llama("tiny-q4km", max_seq_len=512), Q6K_HEAD),
    "tiny-gptq-actorder": (lambda: synth.make_llama("tiny-gptq", act_order=True, bias=True, max_seq_len=512), DENSE_HEAD),
    "q4km-g3": (lambda: ic.make("q4km-g3"), Q6K_HEAD),
    "bf16-g2-w768": (lambda: ic.make("bf16-g2-w768"), DENSE_HEAD),
    "llama3-8b-awq-2l": (lambda: synth.make_llama("llama3-8b-awq", **CUT), DENSE_HEAD),
    "llama3.2-1b-bf16-2l": (lambda: synth.make_llama("llama3.2-1b-bf16", **CUT), DENSE_HEAD),
    "mistral-7b-q4km-2l": (lambda: synth.make_llama("mistral-7b-q4km", **CUT), Q6K_SLIM_HEAD),
}
_LM = {}


def _lm(device, name, make):
    if name not in _LM:
        _LM.clear()                      # one model at a time: the cases of a model run back to back
        _LM[name] = runtime.LoadedModel.from_synth(device, make())
    return _LM[name]


def _predicted(lm, kv_dtype, position, split_min, head):
    c = Counter({"embed": 1, "argmax_final": 1, head: 1})
    for l in range(lm.c.n_layers):
        t = lm.layer_traits(l)
        c += S.layer_census(t, lm.layer_plan(l, kv_dtype), S.is_long(t, position, split_min))
    return dict(c)


def _reported(recs):
    return {r["name"]: r["launches"] for r in recs}


@pytest.mark.parametrize("position,split_min", [(8, None), (269, 4)])
@pytest.mark.parametrize("name", list(LLAMA))
def test_llama_family(device, monkeypatch, name, position, split_min):
    make, head = LLAMA[name]
    lm = _lm(device, name, make)
    if split_min is None:
        monkeypatch.delenv("BZ_SPLIT_MIN", raising=False)
    else:
        monkeypatch.setenv("BZ_SPLIT_MIN", str(split_min))     # read per call
    kv = lm.new_kv_cache(position + 3)
    want = _predicted(lm, lm.c.act_dtype, position, 512 if split_min is None else split_min, head)
    got = _reported(lm.profile_step(kv, 5, position, iters=1))
    print(name, position, got)
    assert got == want


def test_dsv2(device):
    lm = _lm(device, "tiny-dsv2", lambda: synth.make_dsv2("tiny-dsv2"))
    want = _predicted(lm, lm.c.act_dtype, 8, 512, DENSE_HEAD)
    got = _reported(lm.profile_step(lm.new_kv_cache(16), 5, 8, iters=1))
    print("tiny-dsv2", got)
    assert got == want
    assert [lm.layer_traits(l).is_moe for l in range(3)] == [0, 1, 1]


def test_mamba2(device):
    lm = _lm(device, "tiny-mamba2-g2", lambda: synth.make_mamba2("tiny-mamba2-g2"))
    want = _predicted(lm, L.F32, 8, 512, DENSE_HEAD)
    got = _reported(lm.profile_step_ssm(runtime.LayeredSsmState(lm), 5, iters=1))
    print("tiny-mamba2-g2", got)
    assert got == want
    _LM.clear()
