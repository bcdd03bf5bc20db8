"""bz-run --score / --embed: the C ABI's score and embed calls driven from compiled C++ against a checkpoint on disk, compared with the Python runtime's results."""
import os
import subprocess

import numpy as np
import pytest

import ckpt_writer as W
from blazr_amd import runtime, synth

pytestmark = pytest.mark.gpu
EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "blazr_amd", "bz-run")


def test_bz_run_score_and_embed(device, tmp_path):
    assert os.path.exists(EXE), "bz-run was not built (python -c 'import __graft_entry__ as g; g.build()')"
    model = synth.make_llama("tiny-awq")
    W.write_hf_checkpoint(str(tmp_path), model, shards=2)
    S = 14
    p = synth.prompt_tokens(S, 1024, seed=33)
    ids = ",".join(str(int(x)) for x in p)
    lm = runtime.LoadedModel.from_synth(device, model)
    want = lm.score(p, lm.new_kv_cache(S), top_logprobs=2)
    r = subprocess.run([EXE, str(tmp_path), "--prompt", ids, "--score", "--top-logprobs", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == S
    for i, line in enumerate(lines[:-1]):
        f = line.split()
        row = want["rows"][i]
        assert int(f[0]) == i + 1 and int(f[1]) == int(p[i + 1]) == int(row["target"]) and int(f[3]) == int(row["rank"])
        assert f[2] == "%.6f" % float(row["logprob"])
        assert [int(t.split(":")[0]) for t in f[4:]] == [int(t) for t in row["top_ids"][:2]]
    tot = lines[-1].split()
    assert tot[0] == "total" and int(tot[3]) == S - 1 and tot[1] == "%.6f" % want["sum_logprob"] and tot[5] == "%.6f" % want["perplexity"]
    for pooling, extra in (("mean", []), ("last", ["--normalize"]), ("none", [])):
        r = subprocess.run([EXE, str(tmp_path), "--prompt", ids, "--embed", pooling] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        got = np.array([[float(x) for x in line.split(",")] for line in r.stdout.strip().split("\n")], dtype=np.float32)
        ref = lm.embed(p, lm.new_kv_cache(S), pooling=pooling, normalize=bool(extra))
        assert np.array_equal(got.reshape(ref.shape), ref), pooling                  # %.9g round-trips an f32
    r = subprocess.run([EXE, str(tmp_path), "--prompt", ids, "--embed", "max"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--embed takes" in r.stderr
