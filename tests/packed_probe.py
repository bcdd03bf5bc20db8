"""A packed batch next to the loop of single calls it replaces, on one fixture: embed_batch("none" and pooled) and score_batch against embed() / score() of every
input alone on a fresh cache.  Used in-process (compare) and, where an environment switch has to be set before the library reads it, as a child process:

usage: python tests/packed_probe.py <fixture> <len,len,...> <out.npz>
Called by tests/test_gpu_embed_batch.py / test_gpu_score_batch.py with the switch in the environment; the parent asserts."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import packed_cases as PC  # noqa: E402
from blazr_amd import runtime  # noqa: E402

TOP = 3
_CHILD = {}


def compare(lm, traits, lens, toks, scratch):
    """every array the parent compares; score records travel as bytes (one SCORE_ROW per row)"""
    plan = runtime.packed_plan(traits, lens, lm.c.act_dtype)
    res = dict(packed=plan["packed"], exact=plan["plan"]["exact"], attn=plan["plan"]["attn"])
    res["batch_rows"] = np.concatenate(lm.embed_batch(toks, scratch, pooling="none"))
    res["single_rows"] = np.concatenate([lm.embed(t, lm.new_kv_cache(len(t)), 0, pooling="none") for t in toks])
    for pooling in ("mean", "cls", "last"):
        res["batch_" + pooling] = lm.embed_batch(toks, scratch, pooling=pooling)
        res["batch_norm_" + pooling] = lm.embed_batch(toks, scratch, pooling=pooling, normalize=True)
    sb = lm.score_batch(toks, scratch, top_logprobs=TOP)
    ss = [lm.score(t, lm.new_kv_cache(len(t)), top_logprobs=TOP) for t in toks]
    res["batch_score"] = np.concatenate([r["rows"] for r in sb]).view(np.uint8)
    res["single_score"] = np.concatenate([r["rows"] for r in ss]).view(np.uint8)
    res["batch_totals"] = np.array([[r["sum_logprob"], r["n_scored"]] for r in sb], dtype=np.float64)
    res["single_totals"] = np.array([[r["sum_logprob"], r["n_scored"]] for r in ss], dtype=np.float64)
    res["scratch_len"] = scratch.seq_len()
    return res


def child(fixture, lens, env, tmp_path):
    """compare() in a process of its own with `env` set; one run per (fixture, lens, env), shared by the tests that need it"""
    key = (fixture, tuple(lens), tuple(sorted(env.items())))
    if key not in _CHILD:
        out = os.path.join(str(tmp_path), "packed_probe.npz")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), fixture, ",".join(str(n) for n in lens), out], env=dict(os.environ, **env), capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        _CHILD[key] = dict(np.load(out))
    return _CHILD[key]


def main():
    import packed_model as PM
    fixture, lens, out = sys.argv[1], [int(x) for x in sys.argv[2].split(",")], sys.argv[3]
    dev = runtime.Device(0)
    _, lm, _ = PM.get(dev, fixture)
    _, toks = PM.inputs(fixture, "probe", lens)
    np.savez(out, **compare(lm, runtime.prompt_traits(lm), lens, toks, PM.scratch(lm, lens)))
    dev.close()


if __name__ == "__main__":
    main()
