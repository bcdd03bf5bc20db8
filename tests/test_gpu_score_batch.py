"""score_batch (bz_score_batch): the log-likelihoods of many inputs from one prompt pass against the single calls they replace and against the oracle's rows of
every input alone.  Exact rows (tiny-awq): every field of every record is the single call's.  MFMA route: each input's logprobs at the bars single MFMA prompts
are held to.  f32 activations (tiny-q4km, exact scalar attention, GGUF GEMMs): 1e-4 per row.  Fallbacks: the loop's bits.  The CLI."""
import os
import subprocess

import numpy as np
import pytest

import ckpt_writer as W
import kquant_ref
import packed_cases as PC
import packed_model as PM
import packed_probe
from blazr_amd import _lib as L
from blazr_amd import runtime

pytestmark = pytest.mark.gpu
EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "blazr_amd", "bz-run")
MFMA_CASES = [(n, s) for n in ("tiny-bf16", "bf16-g2-w768", "awq-g4-w768") for s in ("B", "C", "E")]


def _check_exact(res, lens):
    assert res["packed"] == 1 and res["exact"] == 1
    b, s = res["batch_score"].view(runtime.SCORE_ROW), res["single_score"].view(runtime.SCORE_ROW)
    assert len(b) == len(s) == sum(lens)
    for n in b.dtype.names:
        assert np.array_equal(b[n], s[n]), n
    assert np.array_equal(res["batch_totals"], res["single_totals"])
    assert [int(k) for k in res["batch_totals"][:, 1]] == [n - 1 for n in lens]


def test_exact_records_are_the_single_calls_records(device):
    lens = [5, 4, 7]
    _, lm, _ = PM.get(device, "tiny-awq")
    _, toks = PM.inputs("tiny-awq", "probe", lens)
    _check_exact(packed_probe.compare(lm, runtime.prompt_traits(lm), lens, toks, PM.scratch(lm, lens)), lens)


def test_exact_records_set_b(tmp_path):
    """set B with BZ_EXACT_PREFILL=1, in a process of its own (the run test_gpu_embed_batch.py shares)"""
    _check_exact(packed_probe.child("tiny-awq", PC.SETS["B"], dict(BZ_EXACT_PREFILL="1"), tmp_path), PC.SETS["B"])


@pytest.mark.parametrize("name,set_name", MFMA_CASES, ids=["%s-%s" % c for c in MFMA_CASES])
def test_mfma_logprobs_at_the_bar(device, name, set_name):
    """per input: the logprobs of its scored rows against log_softmax of the oracle's rows for that input alone, relative L2; the records' own consistency
    (targets, totals) against the host definitions"""
    model, lm, _ = PM.get(device, name)
    lens, toks = PM.inputs(name, set_name)
    res = lm.score_batch(toks, PM.scratch(lm, lens), top_logprobs=2)
    want = PM.oracle_rows(device, name, set_name)
    bar = PM.bar(model["config"], int4=name.startswith("awq"))
    flat = np.concatenate([r["rows"] for r in res])
    assert np.array_equal(flat["target"], runtime.packed_targets_spec(np.concatenate(toks), lens))
    assert [(r["sum_logprob"], r["n_scored"]) for r in res] == runtime.packed_totals_spec(flat, lens)
    errs = []
    for i, n in enumerate(lens):
        rows = res[i]["rows"]
        assert len(rows) == n and res[i]["n_scored"] == n - 1 and int(rows["n_top"][-1]) == -1
        if n > 1:
            ref = PM.log_softmax64(want[i])[np.arange(n - 1), toks[i][1:]]
            errs.append(PM.rel_l2(rows["logprob"][:-1], ref))
    print("PACKED_SCORE_BAR %s %s worst %.3e of %.3e" % (name, set_name, max(errs), bar))
    assert max(errs) <= bar, errs


def test_isolation_whole_model(device):
    _, lm, _ = PM.get(device, "bf16-g2-w768")
    lens, toks = PM.inputs("bf16-g2-w768", "C")
    base = lm.score_batch(toks, PM.scratch(lm, lens), top_logprobs=3)
    for i in range(len(lens)):
        other = list(toks)
        other[i] = (toks[i] + 11) % PM.VOCAB["bf16-g2-w768"]
        got = lm.score_batch(other, PM.scratch(lm, lens), top_logprobs=3)
        for j in range(len(lens)):
            if j != i:
                assert PM.rows_equal(got[j]["rows"], base[j]["rows"]) and got[j]["sum_logprob"] == base[j]["sum_logprob"], (i, j)


def test_gguf_rows_set_b(device):
    """tiny-q4km: f32 activations, the exact scalar attention, split-operand GEMMs, the decode step's quantised head.  Every row of every input, the inputs' last
    rows and the one-token inputs among them: the row of embed_batch("none") through the dequantised head in float64 against the oracle's row of that input
    alone, 1e-4 relative L2 per row.  Then the head score_batch runs: per scored row the target's logit and the 20 likeliest logits (logprob + lse) against the
    oracle's row at the same ids, to the same bar"""
    model, lm, _ = PM.get(device, "tiny-q4km")
    lens, toks = PM.inputs("tiny-q4km", "B")
    plan = runtime.packed_plan(runtime.prompt_traits(lm), lens, lm.c.act_dtype)
    assert plan["packed"] == 1 and plan["plan"]["attn"] == L.PF_ATTN_SCALAR_EXACT
    want = PM.oracle_rows(device, "tiny-q4km", "B")
    W64 = kquant_ref.dequant(model["lm_head"]).astype(np.float64)
    hid = lm.embed_batch(toks, PM.scratch(lm, lens), pooling="none")
    worst_row, n_rows = 0.0, 0
    for i, n in enumerate(lens):
        got = hid[i].astype(np.float64) @ W64.T
        assert got.shape == want[i].shape == (n, W64.shape[0])
        err = np.linalg.norm(got - want[i], axis=1) / np.linalg.norm(want[i], axis=1)
        worst_row, n_rows = max(worst_row, float(err.max())), n_rows + n
    print("PACKED_GGUF_BAR worst of %d full rows %.3e of 1e-4" % (n_rows, worst_row))
    assert n_rows == sum(lens) and worst_row <= 1e-4
    res = lm.score_batch(toks, PM.scratch(lm, lens), top_logprobs=20)
    worst = 0.0
    for i, n in enumerate(lens):
        rows = res[i]["rows"]
        for r in range(n - 1):
            ids = np.concatenate([[int(rows["target"][r])], rows["top_ids"][r].astype(np.int64)])
            got = np.concatenate([[rows["logit"][r]], rows["top_logprobs"][r].astype(np.float64) + np.float64(rows["lse"][r])])
            worst = max(worst, PM.rel_l2(got, want[i][r, ids]))
    print("PACKED_GGUF_BAR worst scored row (target + top 20) %.3e of 1e-4" % worst)
    assert worst <= 1e-4


@pytest.mark.parametrize("name,lens", [("bf16-g3-hd64", [20, 3, 33]), ("tiny-dsv2", [24, 5, 19]), ("tiny-bf16", PC.BELOW_FLOOR)], ids=["g3", "dsv2", "below-floor"])
def test_fallbacks_are_the_loop(device, name, lens):
    _, lm, _ = PM.get(device, name)
    _, toks = PM.inputs(name, "fallback", lens)
    assert runtime.packed_plan(runtime.prompt_traits(lm), lens, lm.c.act_dtype)["packed"] == 0
    kv = PM.scratch(lm, lens)
    tg = [np.concatenate([t[1:], [-1]]) for t in toks]
    tg[0][1] = -1
    for targets in (None, tg):
        got = lm.score_batch(toks, kv, targets=targets, top_logprobs=2)
        assert kv.seq_len() == 0
        for i, t in enumerate(toks):
            one = lm.score(t, lm.new_kv_cache(len(t)), targets=None if targets is None else targets[i], top_logprobs=2)
            assert PM.rows_equal(got[i]["rows"], one["rows"]) and (got[i]["sum_logprob"], got[i]["n_scored"]) == (one["sum_logprob"], one["n_scored"]), i


def test_bz_run_prompts_file(device, tmp_path):
    """one packed call from compiled C++ against a checkpoint on disk: per input what the single-prompt form prints, after `# input i`"""
    assert os.path.exists(EXE), "bz-run was not built (python -c 'import __graft_entry__ as g; g.build()')"
    model, lm, _ = PM.get(device, "tiny-awq")
    W.write_hf_checkpoint(str(tmp_path), model, shards=2)
    lens = [14, 3, 9]
    _, toks = PM.inputs("tiny-awq", "cli", lens)
    path = os.path.join(str(tmp_path), "prompts.txt")
    with open(path, "w") as f:
        f.write("\n".join(",".join(str(int(x)) for x in t) for t in toks) + "\n")
    want = lm.score_batch(toks, PM.scratch(lm, lens), top_logprobs=2)
    r = subprocess.run([EXE, str(tmp_path), "--prompts-file", path, "--score", "--top-logprobs", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    blocks = r.stdout.strip().split("# input ")[1:]
    assert len(blocks) == len(lens)
    for i, blk in enumerate(blocks):
        lines = blk.strip().split("\n")
        assert lines[0] == str(i) and len(lines) == lens[i] + 1
        for k, line in enumerate(lines[1:-1]):
            f, row = line.split(), want[i]["rows"][k]
            assert int(f[0]) == k + 1 and int(f[1]) == int(toks[i][k + 1]) == int(row["target"]) and int(f[3]) == int(row["rank"]) and f[2] == "%.6f" % float(row["logprob"])
            assert [int(t.split(":")[0]) for t in f[4:]] == [int(t) for t in row["top_ids"][:2]]
        tot = lines[-1].split()
        assert tot[0] == "total" and int(tot[3]) == lens[i] - 1 and tot[1] == "%.6f" % want[i]["sum_logprob"]
    for pooling, extra in (("mean", []), ("none", ["--normalize"])):
        r = subprocess.run([EXE, str(tmp_path), "--prompts-file", path, "--embed", pooling] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        ref = lm.embed_batch(toks, PM.scratch(lm, lens), pooling=pooling, normalize=bool(extra))
        for i, blk in enumerate(r.stdout.strip().split("# input ")[1:]):
            lines = blk.strip().split("\n")
            got = np.array([[float(x) for x in line.split(",")] for line in lines[1:]], dtype=np.float32)
            assert lines[0] == str(i) and np.array_equal(got.reshape(ref[i].shape), ref[i]), (pooling, i)


def test_refusals(device):
    _, lm, _ = PM.get(device, "tiny-bf16")
    V = PM.VOCAB["tiny-bf16"]
    toks = PC.token_lists([10, 10], V, seed=4)
    kv = lm.new_kv_cache(16, max_seq_len=64)
    for kw, figure in ((dict(targets=[[V] + [-1] * 9, [-1] * 10]), "targets[0] = %d" % V), (dict(targets=[[-1] * 10, [-2] + [-1] * 9]), "targets[10] = -2"), (dict(top_logprobs=21), "21")):
        with pytest.raises(L.BlazrHipError) as e:
            lm.score_batch(toks, kv, **kw)
        assert e.value.code == L.E_INVALID and figure in str(e.value), str(e.value)
        assert kv.seq_len() == 0
    with pytest.raises(L.BlazrHipError) as e:
        lm.score_batch(PC.token_lists([40, 30], V, seed=4), kv)
    assert "70 packed rows, the scratch cache holds 64" in str(e.value)
    with pytest.raises(ValueError):
        lm.score_batch(toks, kv, targets=[[-1] * 10])
