"""The two LoRA kernels on the GPU, through bz_lora_apply, bit for bit against lora_ref.lora_apply (tests/lora_cases.py: OP_CASES).

Exact comparison is licensed by test_lora.py::test_op_references_do_not_depend_on_the_summation_order: on these inputs the exact sums and float64
accumulations in two opposite orders round to the same f32, so the kernels' double accumulators (yet another order) must give those bits too.
Form 0 is the rows form of the batched path (x as rows of the activation dtype, y in place, slot id per row), form 1 the decode form (x through the plain
prologue into LDS, the base row read as a VSrc, one row)."""
import numpy as np
import pytest

from blazr_amd import runtime
import lora_cases

pytestmark = pytest.mark.gpu

_MODELS = {}


def _model(device, mkey):
    """one loaded model per activation dtype / width for the whole module, with a table over every target"""
    if mkey not in _MODELS:
        lm = runtime.LoadedModel.from_synth_streamed(device, lora_cases.op_config(mkey))
        lm.enable_lora(n_slots=4, max_rank=128, targets=lora_cases.TARGETS)
        _MODELS[mkey] = lm
    return _MODELS[mkey]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("case", [c["id"] for c in lora_cases.OP_CASES])
def test_lora_apply_matches_the_reference_bit_for_bit(device, case):
    inp = lora_cases.op_inputs(case)
    lm = _model(device, inp["case"]["model"])
    names = []
    try:
        for i, ad in enumerate(inp["adapters"]):
            a = runtime.LoraAdapter.from_arrays(device, ad["rank"], ad["alpha"], ad["pairs"], ad["use_rslora"])
            assert lm.load_lora(a, "op%d" % i) == i
            names.append("op%d" % i)
        want = lora_cases.op_expected(case)
        got = lm.lora_apply(0, inp["targets"], inp["x"], inp["base"], inp["slots"], form=0)
        bad = np.argwhere(_bits(got) != _bits(want))
        assert bad.size == 0, (case, len(bad), bad[:4].tolist())
        off = [i for i, s in enumerate(inp["slots"]) if s < 0]
        assert np.array_equal(_bits(got[off]), _bits(inp["base"][off]))          # rows without an adapter: untouched
        if inp["case"]["rows"] <= 3:
            for r, s in enumerate(inp["slots"]):                                   # the decode form on each row: the rows form's bits
                one = lm.lora_apply(0, inp["targets"], inp["x"][r:r + 1], inp["base"][r:r + 1], [s], form=1)
                assert np.array_equal(_bits(one[0]), _bits(got[r])), (case, r, s)
    finally:
        for nm in names:
            lm.unload_lora(nm)
