"""One process for a run-time switch (the library reads BZ_* once): tiny-mamba2, a prompt of 512 + r tokens in one call and as a call of 512 followed by a
call of r on the same state; the last row's logits and every layer's state of both go to an .npz.

usage: python tests/mamba2_carry_probe.py <r> <out.npz>
Called by tests/test_gpu_mamba2.py::test_chunk_carry_is_an_identity with BZ_EXACT_PREFILL=0 for r <= 16 (by default a prompt of up to 16 rows stays on the decode
kernels, so the call of r rows would not launch what the last chunk of the long call launches); the parent asserts.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from blazr_amd import runtime, synth  # noqa: E402


def read_state(lm, st):
    """every layer's (SSM state, conv window) of a LayeredSsmState"""
    c = lm.mamba_config()
    conv_dim = c["d_inner"] + 2 * c["n_groups"] * c["d_state"]
    n_ssm, n_win = c["n_heads"] * c["head_dim"] * c["d_state"], conv_dim * (c["conv_kernel"] - 1)
    return [(st.read(l, 0, n_ssm), st.read(l, 1, n_win)) for l in range(lm.c.n_layers)]


def carry(lm, vocab, r):
    """dict of arrays: logits and states of the one-call run (a_*) and of the 512 + r split (b_*)"""
    p = synth.prompt_tokens(530, vocab, seed=77)[:512 + r]
    st_a, st_b = runtime.LayeredSsmState(lm), runtime.LayeredSsmState(lm)
    out = dict(a_logits=lm.forward_with_ssm_state(p, st_a).to_numpy())
    lm.forward_with_ssm_state(p[:512], st_b)
    out["b_logits"] = lm.forward_with_ssm_state(p[512:], st_b).to_numpy()
    for k, st in (("a", st_a), ("b", st_b)):
        for l, (ssm, win) in enumerate(read_state(lm, st)):
            out["%s_ssm%d" % (k, l)], out["%s_win%d" % (k, l)] = ssm, win
    return out


def main():
    r, path = int(sys.argv[1]), sys.argv[2]
    model = synth.make_mamba2("tiny-mamba2")
    dev = runtime.Device(0)
    np.savez(path, **carry(runtime.LoadedModel.from_synth(dev, model), model["config"]["vocab"], r))
    dev.close()


if __name__ == "__main__":
    main()
