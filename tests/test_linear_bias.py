"""The bias-order construction of bias_cases.py, checked on the CPU: its exact sums are exact, the oracle's linear is R(RN32(sum) + bias) on it, the
staged layer is the oracle's layer, and the construction is SENSITIVE -- folding the bias into the exact sum (what the int4 accumulator kernels used to
do) changes at least 5 % of every observable that tests/test_gpu_linear_bias.py holds the kernels to."""
import math
from fractions import Fraction

import numpy as np
import pytest

import bias_cases as bc
from oracle import orc_py

MIN_SHARE = 0.05
PAIRS = [(w, c) for w in bc.WIDTHS for c in bc.CASES]


@pytest.mark.parametrize("width", list(bc.WIDTHS))
def test_exact_sums_are_fsum_and_the_dequantised_weights_are_the_oracles(width):
    """the integer sums against math.fsum over the doubles x . (q - z) s (every product exact) on 48 columns of each group, weights as orc_linear_dequant has them"""
    case = bc.get(width, "all")
    lay = case.model["layers"][0]
    for name in ("q", "o", "up", "down"):
        qz, sc = bc.gptq_ints(lay[name])
        gs = lay[name]["group_size"]
        w = (qz.astype(np.float32) * np.repeat(sc.astype(np.float32), gs, axis=0)).T
        assert np.array_equal(w, orc_py.OrcLinear(dict(lay[name], bias=None)).dequant()), name
        x = case.stage.input_of(name).astype(np.float64)
        for n in range(0, lay[name]["N"], max(1, lay[name]["N"] // 48)):
            assert float(case.sums[name][n]) == math.fsum((w[n].astype(np.float64) * x).tolist()), (name, n)


@pytest.mark.parametrize("width", list(bc.WIDTHS))
def test_orc_linear_with_a_bias_is_rn32_of_the_sum_plus_the_bias(width):
    """the definition the GPU is held to: OrcLinear.forward == RN32(exact sum) + bias, f32 add, bit for bit -- on the midpoint by construction"""
    case = bc.get(width, "all")
    lay = case.model["layers"][0]
    for name, r in case.rsum.items():
        got = orc_py.OrcLinear(lay[name]).forward(case.stage.input_of(name))[0]
        want = (r + lay[name]["bias"]).astype(np.float32)
        assert np.array_equal(got, want), (name, int((got != want).sum()))
        bare = orc_py.OrcLinear(dict(lay[name], bias=None)).forward(case.stage.input_of(name))[0]
        assert np.array_equal(bare, r), name
        # ... and that value is the chosen midpoint: halfway between two neighbouring f16 values
        b, c = bc.cancelling_bias(r)
        on = b != 0
        assert on.mean() > 0.95 and np.array_equal(got[on], c[on])
        a = np.abs(c[on])
        near = a.astype(np.float16)
        lo = np.where(near.astype(np.float32) > a, np.nextafter(near, np.float16(0)), near)
        hi = np.nextafter(lo, np.float16(np.inf))
        assert np.array_equal(a.astype(np.float64) - lo.astype(np.float64), hi.astype(np.float64) - a.astype(np.float64))


@pytest.mark.parametrize("width,name", PAIRS)
def test_staged_layer_is_the_oracles_layer(width, name):
    """the stage-by-stage pipeline the biases were built against gives orc_llama_forward_kv's K / V rows and orc_llama_layers_range's rows bit for bit"""
    case = bc.get(width, name)
    for k in ("k0", "v0", "hidden", "prev_mlp"):
        assert np.array_equal(getattr(case.stage, k), case.want[k]), k
    assert np.isfinite(case.want["logits"]).all()


@pytest.mark.parametrize("width,name", PAIRS)
def test_the_folded_order_changes_every_sensitised_observable(width, name):
    """bias added to the exact sum, ONE rounding to f32, one to f16 -- at one site at a time -- against the oracle: >= 5 % of the elements of that site's
    observables.  A condition on the inputs: a case that misses it needs another c or T0, not a lower bar."""
    case = bc.get(width, name)
    for site in case.sites:
        for obs in bc.OBSERVABLE[site]:
            share = float((case.folded[site][obs] != case.want[obs]).mean())
            print("%s %-7s site %-7s %-8s folded order differs in %5.1f %% of %d elements" % (width, name, site, obs, 100 * share, case.want[obs].size))
            assert share >= MIN_SHARE, (width, name, site, obs, share)


def test_rn32_decides_a_double_rounding_exactly():
    """1 + 2^-24 + 2^-60 rounds to the double 1 + 2^-24 (an f32 midpoint, which would go to even = 1) but lies above it: RN32 is 1 + 2^-23"""
    v = Fraction(1) + Fraction(1, 1 << 24) + Fraction(1, 1 << 60)
    assert bc.rn32([v, -v, Fraction(1) + Fraction(1, 1 << 24)]).tolist() == [1 + 2.0 ** -23, -(1 + 2.0 ** -23), 1.0]
