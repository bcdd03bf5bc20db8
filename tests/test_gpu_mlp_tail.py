"""The fused int4 MLP (k_mlp_q4g) at the smallest shapes where its request order and its tile-by-tile down phase can go wrong.

The kernel's waves hand work to each other through LDS counters: the down requests wait for the row waves' gate / up requests, one wave turns the
published partials into SiLU * up, and every wave then adds its output tiles to the fixed-point accumulator as they land.  All of its sums are exact
(64-bit fixed-point adds, doubles over exact products), so neither the order of the atomics nor of the waves may change one bit: every logits row of
a 2-layer model must EQUAL the CPU oracle's, a repeated step must repeat its bits, and greedy ids must be the oracle's on the fair prefix.

Shapes: hidden 4096 (16 waves) and 2048 (8 waves); inter 128 = two workgroups that share one quantisation group of down_proj, inter 384 = three
groups, six workgroups; GPTQ without act-order and with biases takes the fused kernel with both bias pointers set.
"""
import numpy as np
import pytest

from blazr_amd import _lib as L
from blazr_amd import runtime, synth
from oracle import orc_py
from test_gpu_llama import _fair_prefix

pytestmark = pytest.mark.gpu

MLP_LAUNCH = "mlp_q4g<norm+gate/up+silu+down>"
SHAPES = {
    "h4096-i128": dict(hidden=4096, n_heads=32, n_kv_heads=8, inter=128),
    "h4096-i384": dict(hidden=4096, n_heads=32, n_kv_heads=8, inter=384),
    "h2048-i128": dict(hidden=2048, n_heads=16, n_kv_heads=4, inter=128),
    # hidden 2048 with inter 384 three ways: AWQ, GPTQ, GPTQ with biases -- the last one differs from the bit-equal shapes above in one thing at a time
    "h2048-i384": dict(hidden=2048, n_heads=16, n_kv_heads=4, inter=384),
    "h2048-i384-gptq": dict(hidden=2048, n_heads=16, n_kv_heads=4, inter=384, quant="gptq"),
    "h2048-i384-gptq-bias": dict(hidden=2048, n_heads=16, n_kv_heads=4, inter=384, quant="gptq", bias=True),
}
P, N = 4, 6   # prompt tokens (fed one by one: the decode kernels) and teacher-forced decode steps


class Pair:
    def __init__(self, device, name):
        self.name = name
        self.model = synth.make_llama("llama3-8b-awq-2l", vocab=512, max_seq_len=64, **SHAPES[name])
        self.cfg = self.model["config"]
        self.lm = runtime.LoadedModel.from_synth(device, self.model)
        self.om = orc_py.OrcLlama(self.model)
        # the oracle's rows, once: prompt token by token, then its own greedy ids fed back
        self.prompt = [int(t) for t in synth.prompt_tokens(P, self.cfg["vocab"], seed=5)]
        okv = self.om.new_kv(P + N + 2)
        self.fed, self.want = [], []
        tok = self.prompt[0]
        for i in range(P + N):
            lo = np.asarray(self.om.forward_kv([tok], okv, i), dtype=np.float32).reshape(-1)
            self.fed.append(tok)
            self.want.append(lo)
            tok = self.prompt[i + 1] if i + 1 < P else int(lo.argmax())
        orc_py.lib().orc_kv_free(okv)
        for a in self.want:
            a.setflags(write=False)

    def new_kv(self, device):
        c = self.cfg
        return runtime.LayeredKvCache(device, c["n_layers"], 1, c["n_kv_heads"], P + N + 2, c["max_seq_len"], c["head_dim"], L.F16)


@pytest.fixture(scope="module", params=list(SHAPES))
def pair(request, device):
    return Pair(device, request.param)


def test_fused_kernel_is_in_the_step(pair, device):
    """none of the other tests may pass on another path: the step's census names the fused launch, once per layer"""
    kv = pair.new_kv(device)
    for i in range(2):
        pair.lm.forward_with_kv_cache([pair.fed[i]], kv, i)
    census = {r["name"]: r["launches"] for r in pair.lm.profile_step(kv, pair.fed[2], 2, iters=1)}
    assert census.get(MLP_LAUNCH) == pair.cfg["n_layers"], census


def test_every_logits_row_equals_the_oracle(pair, device):
    """4 prompt tokens one by one + 6 teacher-forced decode steps: every element of every row equal to the oracle's, on every shape.  (The GPTQ + bias shape
    used to leave the oracle at position 7, by 2^-9 in half of each later row, while its int4 kernels added the bias into the exact sum; with the bias added to
    the sum's f32 rounding, the oracle's order, it is equal in all 10 rows -- tests/test_gpu_linear_bias.py.)"""
    kv = pair.new_kv(device)
    bad = []
    for i, (tok, want) in enumerate(zip(pair.fed, pair.want)):
        got = pair.lm.forward_with_kv_cache([tok], kv, i).to_numpy().reshape(-1)
        ndiff, dmax = int((got != want).sum()), float(np.abs(got - want).max())
        print("step %d: %d of %d elements differ, max |d| = %g" % (i, ndiff, want.size, dmax))
        if ndiff:
            bad.append((i, ndiff, dmax))
    assert not bad, bad


def test_a_repeated_step_repeats_its_bits(pair, device):
    """the same decode step twice from the same cache state (position 5 written again with the same token)"""
    kv = pair.new_kv(device)
    for i in range(5):
        pair.lm.forward_with_kv_cache([pair.fed[i]], kv, i)
    a = pair.lm.forward_with_kv_cache([pair.fed[5]], kv, 5).to_numpy().copy()
    b = pair.lm.forward_with_kv_cache([pair.fed[5]], kv, 5).to_numpy().copy()
    assert np.array_equal(a, b), int((a != b).sum())
    assert np.array_equal(a.reshape(-1), pair.want[5])


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_greedy_ids(pair, device, mode):
    """12 greedy ids against the oracle on the fair prefix (no near-tie of the oracle's top two)"""
    want, trace = pair.om.generate(pair.prompt, 12, trace=True)
    n = _fair_prefix(trace)
    got = runtime.Executor(pair.lm).generate(pair.prompt, 12, use_graph=mode == "graph")
    print("fair prefix %d of 12" % n)
    assert got[:n].tolist() == want[:n].tolist(), (mode, got.tolist(), want.tolist(), n)
