"""The GPU side of tests/test_gpu_linear_bias.py: what the library gives for the bias-order models of bias_cases.py, as numpy arrays.

As a module: the functions the test calls in its own process.  As a script: one process per run-time switch (the library reads BZ_* once) --

    python tests/bias_probe.py <mode> <biases.npz> <out.npz>

rebuilds every model of biases.npz (keys "<width>/<case>/<linear>": the f32 biases the parent built; nothing of the oracle runs here), runs `mode` on each with
the switch in the environment and writes "<width>/<case>/<observable>".  The parent asserts.
  step      T0 at position 0 through the decode step: k0, v0, hidden, prev_mlp, logits
  prompt20  a 20-row prompt starting with T0: k0, v0 and logits row 0
  walk10    WALK token by token, positions 0..9: hidden, prev_mlp, logits of every position ([10, ...])
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from blazr_amd import _lib as L  # noqa: E402
from blazr_amd import runtime, synth  # noqa: E402
import bias_cases as bc  # noqa: E402

WALK = [bc.T0] + [int(t) for t in synth.prompt_tokens(9, 512, seed=31)]


def prompt(S):
    """S tokens starting with T0"""
    return [bc.T0] + [int(t) for t in synth.prompt_tokens(S - 1, 512, seed=17)]


def new_kv(device, cfg, cap=32):
    return runtime.LayeredKvCache(device, cfg["n_layers"], 1, cfg["n_kv_heads"], cap, cfg["max_seq_len"], cfg["head_dim"], L.F16)


def kv_row(kv, cfg, pos):
    """(k, v) of layer 0 at `pos`, every kv head: [n_kv * head_dim] each"""
    rows = [[kv.read(0, h, which, pos + 1)[pos] for h in range(cfg["n_kv_heads"])] for which in (0, 1)]
    return np.concatenate(rows[0]), np.concatenate(rows[1])


def pieces(device, lm, cfg, tok, kv, pos):
    """hidden, prev_mlp, logits of `tok` at `pos` through embed -> layers 0..1 -> head (the decode step's launches, cut at the layer's end)"""
    h, pm = lm.forward_layers_range(lm.forward_embed([tok]), None, kv, 0, 1, pos)
    lg = lm.forward_head(h, pm)
    return h.to_numpy().reshape(-1), pm.to_numpy().reshape(-1), lg.to_numpy().reshape(-1)


def run_step(device, lm, cfg):
    kv = new_kv(device, cfg)
    logits = lm.forward_with_kv_cache([bc.T0], kv, 0).to_numpy().reshape(-1)
    k0, v0 = kv_row(kv, cfg, 0)
    hidden, prev_mlp, lg2 = pieces(device, lm, cfg, bc.T0, new_kv(device, cfg), 0)
    assert np.array_equal(lg2, logits), "embed -> layers -> head is not the step"
    return dict(k0=k0, v0=v0, hidden=hidden, prev_mlp=prev_mlp, logits=logits)


def run_prompt(device, lm, cfg, S):
    kv = new_kv(device, cfg)
    rows = lm.forward_with_kv_cache(prompt(S), kv, 0, all_logits=True).to_numpy()
    k0, v0 = kv_row(kv, cfg, 0)
    return dict(k0=k0, v0=v0, logits=rows[0].copy(), rows=rows)


def run_walk(device, lm, cfg):
    kv = new_kv(device, cfg)
    out = [pieces(device, lm, cfg, t, kv, i) for i, t in enumerate(WALK)]
    return dict(hidden=np.stack([o[0] for o in out]), prev_mlp=np.stack([o[1] for o in out]), logits=np.stack([o[2] for o in out]))


def main():
    mode, src, dst = sys.argv[1:4]
    biases = {}
    for key, b in np.load(src).items():
        w, c, name = key.split("/")
        biases.setdefault((w, c), {})[name] = b
    dev = runtime.Device(0)
    out = {}
    for (w, c), bs in sorted(biases.items()):
        model = bc.with_biases(w, {n: b for n, b in bs.items() if n != "none"})
        lm = runtime.LoadedModel.from_synth(dev, model)
        cfg = model["config"]
        got = run_step(dev, lm, cfg) if mode == "step" else run_prompt(dev, lm, cfg, 20) if mode == "prompt20" else run_walk(dev, lm, cfg)
        got.pop("rows", None)
        for k, a in got.items():
            out["%s/%s/%s" % (w, c, k)] = a
    np.savez(dst, **out)
    dev.close()


if __name__ == "__main__":
    main()
