#!/usr/bin/env python3
"""What per-row logit bias and logprobs (bz_batch_sampler_enable, bz_logprobs.hip) add to a step of the sampled batch graph, in one process.

llama3-8b-awq at 64 sequences, the sampled graph of scripts/bench_batch_sampler.py (temperature 0.7, top-k 40, top-p 0.9, a 64-token penalty window) in four
variants: without the flags, with BZ_BS_BIAS only (every row carries 8 entries), with both flags and top_n = 0 on every row, with both flags and top_n = 20 on every row.
Times are a host clock around `--steps` replays that end in a device synchronise; every figure is the median of `--rounds` rounds, the variants alternating
inside a round, after a warm-up round; every round reseeds so that the positions are the same.  `--plain-only` measures the first variant alone with nothing but
the entry points an earlier commit has (run from that commit's tree for the figure beside it); `--parent-json` merges such results.  Writes profiles/logprobs.json."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from blazr_amd import _lib as L   # noqa: E402
from blazr_amd import runtime, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--steps", type=int, default=24)
ap.add_argument("--preset", default="llama3-8b-awq")
ap.add_argument("--n", type=int, default=64)
ap.add_argument("--plain-only", action="store_true")
ap.add_argument("--parent-json", action="append", default=[], help="a --plain-only result of the parent commit's tree; may be given more than once")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logprobs.json"))
args = ap.parse_args()

dev = runtime.Device(0)
KW = dict(temperature=0.7, top_k=40, top_p=0.9, min_p=0.0, repeat_penalty=1.1, frequency_penalty=0.1, presence_penalty=0.05, repeat_last_n=64)
cfg = synth.make_config(args.preset)
lm = runtime.LoadedModel.from_synth_streamed(dev, cfg)
N, bs, per = args.n, 16, 4
tables = [[i + N * j for j in range(per)] for i in range(N)]
lens = [8 + i % 5 for i in range(N)]


def timed(fn, reps):
    dev.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    dev.synchronize()
    return (time.perf_counter() - t0) / reps


def make(bias, top_n):
    pool = runtime.LayeredPagedKvCache(dev, cfg["n_layers"], N * per, bs, cfg["n_kv_heads"], cfg["head_dim"], L.F16)
    for i in range(N):
        p = synth.prompt_tokens(lens[i], cfg["vocab"], seed=i)
        lm.forward_with_paged_kv_cache(p, pool, [tables[i][k // bs] * bs + k % bs for k in range(lens[i])], tables[i], lens[i], 0)
    smp = runtime.BatchSampler(dev, N, cfg["vocab"])
    if bias or top_n is not None:
        smp.enable(bias=bias, logprobs=top_n is not None)
    for r in range(N):
        smp.set_row(r, history=synth.prompt_tokens(lens[r], cfg["vocab"], seed=r).tolist(), seed=r, **KW)
        if bias:
            smp.set_row_bias(r, {100 + 7 * r + k: 0.5 - 0.25 * k for k in range(8)})
        if top_n is not None:
            smp.set_row_logprobs(r, top_n)
    return runtime.BatchDecodeGraph(lm, pool, N, per, sampler=smp), pool


variants = {"plain": (False, None)}
if not args.plain_only:
    variants.update({"bias": (True, None), "both_top0": (True, 0), "both_top20": (True, 20)})
graphs = {k: make(*v) for k, v in variants.items()}
times = {k: [] for k in graphs}
for rnd in range(args.rounds + 1):      # round 0 warms up
    for name, (g, _) in graphs.items():
        g.seed([1 + i for i in range(N)], [n + 1 for n in lens], tables)
        dt = timed(g.replay, args.steps)
        if rnd:
            times[name].append(dt)
result = {"device": dev.name(), "preset": args.preset, "N": N, "steps": args.steps, "rounds": args.rounds, "params": KW,
          "ms_per_step": {k: round(statistics.median(v) * 1e3, 4) for k, v in times.items()},
          "ms_per_step_min": {k: round(min(v) * 1e3, 4) for k, v in times.items()}}
if not args.plain_only:
    m = result["ms_per_step"]
    result["excess_ms_over_plain"] = {k: round(m[k] - m["plain"], 4) for k in m if k != "plain"}
if args.parent_json:      # the parent's figure comes from other processes: each reading is listed, the difference is taken to their mean
    reads = []
    for path in args.parent_json:
        with open(path) as f:
            reads.append(json.load(f)["ms_per_step"]["plain"])
    result["parent_plain_ms_per_step"] = reads
    result["plain_minus_parent_ms"] = round(result["ms_per_step"]["plain"] - sum(reads) / len(reads), 4)
for g, _ in graphs.values():
    del g
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print(json.dumps(result))
