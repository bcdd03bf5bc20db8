#!/usr/bin/env python3
"""Batched device sampler (bz_batch_sampler_*, bz_sample_batch.hip) against the path a caller had before it, in one process.

Sampler rows: at V = 128256 and N in {1, 8, 64}, one bz_batch_sampler_sample (temperature 0.7, top-k 40, top-p 0.9, a 64-token penalty window) beside the
same work done as N consecutive bz_logits_to_token calls, each with its window upload.  Graph row: on llama3-8b-awq at N = 64, the sampled batch graph's
time per step beside the greedy graph's.  Times are a host clock around work that ends in a device synchronise; every figure is the median of `--rounds`
rounds, the variants alternating inside a round, after a warm-up of every shape.  Writes profiles/batch_sampler.json."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from blazr_amd import _lib as L   # noqa: E402
from blazr_amd import runtime, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--vocab", type=int, default=128256)
ap.add_argument("--batches", default="1,8,64")
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--calls", type=int, default=20, help="batched calls per timed window")
ap.add_argument("--preset", default="llama3-8b-awq")
ap.add_argument("--graph-n", type=int, default=64)
ap.add_argument("--graph-steps", type=int, default=24)
ap.add_argument("--no-graph", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_sampler.json"))
args = ap.parse_args()

dev = runtime.Device(0)
V = args.vocab
KW = dict(temperature=0.7, top_k=40, top_p=0.9, min_p=0.0, repeat_penalty=1.1, frequency_penalty=0.1, presence_penalty=0.05, repeat_last_n=64)
rng = np.random.default_rng(0)
result = {"device": dev.name(), "vocab": V, "params": KW, "rounds": args.rounds, "sampler": [], "graph": None}


def timed(fn, reps):
    dev.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    dev.synchronize()
    return (time.perf_counter() - t0) / reps


for N in [int(x) for x in args.batches.split(",")]:
    logits = (rng.standard_normal((N, V)) * 2.5).astype(np.float32)
    hists = [rng.integers(0, V, size=200).tolist() for _ in range(N)]
    t_all = dev.tensor(logits)
    t_rows = [dev.tensor(logits[r:r + 1]) for r in range(N)]
    out = dev.zeros((N,), L.I64)
    s = runtime.BatchSampler(dev, N, V)
    for r in range(N):
        s.set_row(r, history=hists[r], seed=r, **KW)
    windows = [runtime.penalty_window(h, 64) for h in hists]
    kw1 = {k: v for k, v in KW.items() if k != "repeat_last_n"}

    def batched():
        s.sample(t_all, out)

    def single():           # what a caller did before: per row, upload the window, one bz_logits_to_token
        for r in range(N):
            runtime.logits_to_token(dev, t_rows[r], windows[r][0], windows[r][1], seed=r, **kw1)

    timed(batched, 3); timed(single, 1)
    tb, ts = [], []
    for _ in range(args.rounds):
        tb.append(timed(batched, args.calls))
        ts.append(timed(single, max(1, args.calls // 8)))
    mb, ms = statistics.median(tb), statistics.median(ts)
    result["sampler"].append({"N": N, "batched_us": round(mb * 1e6, 1), "batched_us_min": round(min(tb) * 1e6, 1), "single_row_calls_us": round(ms * 1e6, 1),
                              "single_row_calls_us_min": round(min(ts) * 1e6, 1), "ratio_single_over_batched": round(ms / mb, 2)})
    del s

if not args.no_graph:
    cfg = synth.make_config(args.preset)
    lm = runtime.LoadedModel.from_synth_streamed(dev, cfg)
    N, bs, per = args.graph_n, 16, 4
    tables = [[i + N * j for j in range(per)] for i in range(N)]
    lens = [8 + i % 5 for i in range(N)]

    def make(sampled):
        pool = runtime.LayeredPagedKvCache(dev, cfg["n_layers"], N * per, bs, cfg["n_kv_heads"], cfg["head_dim"], L.F16)
        for i in range(N):
            p = synth.prompt_tokens(lens[i], cfg["vocab"], seed=i)
            lm.forward_with_paged_kv_cache(p, pool, [tables[i][k // bs] * bs + k % bs for k in range(lens[i])], tables[i], lens[i], 0)
        smp = None
        if sampled:
            smp = runtime.BatchSampler(dev, N, cfg["vocab"])
            for r in range(N):
                smp.set_row(r, history=synth.prompt_tokens(lens[r], cfg["vocab"], seed=r).tolist(), seed=r, **KW)
        return runtime.BatchDecodeGraph(lm, pool, N, per, sampler=smp), pool

    graphs = {"greedy": make(False), "sampled": make(True)}
    times = {k: [] for k in graphs}
    for rnd in range(args.rounds + 1):      # round 0 warms up; every round reseeds so that the positions are the same
        for name, (g, _) in graphs.items():
            g.seed([1 + i for i in range(N)], [n + 1 for n in lens], tables)
            dt = timed(g.replay, args.graph_steps)
            if rnd:
                times[name].append(dt)
    gm, sm = statistics.median(times["greedy"]), statistics.median(times["sampled"])
    result["graph"] = {"preset": args.preset, "N": N, "steps": args.graph_steps, "greedy_ms_per_step": round(gm * 1e3, 4), "sampled_ms_per_step": round(sm * 1e3, 4),
                       "excess_ms": round((sm - gm) * 1e3, 4), "excess_over_greedy": round((sm - gm) / gm, 4), "design_step_ms": 5.05}
    for g, _ in graphs.values():
        del g

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print(json.dumps(result))
