#!/usr/bin/env python3
"""Packed prompt batches (bz_embed_batch / bz_score_batch) against the loop of single calls they replace, in one process.

Inputs: 64 x 32 tokens and 256 x 16 tokens, on the llama3-8b-awq and llama3.2-1b-bf16 presets (--layers to cut the depth).  embed_batch(mean) beside a loop of
reset + embed(mean), score_batch beside a loop of reset + score.  Times are a host clock around work that ends with its result on the host; every figure is the
median of `--rounds` rounds, the two variants alternating inside a round, after a warm-up of every shape.  No profiler, no captured graph.  Merges its figures into
profiles/packed_prompts.json under "bench" (the file also holds the kernel-resource comparison and the op-level error figures)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from blazr_amd import runtime, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--presets", default="llama3-8b-awq,llama3.2-1b-bf16")
ap.add_argument("--layers", type=int, default=0)                 # 0: the preset's own depth
ap.add_argument("--shapes", default="64x32,256x16")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_prompts.json"))
args = ap.parse_args()
if args.rounds < 5:
    sys.exit("bench_packed: at least 5 rounds")

dev = runtime.Device(0)


def timed(fn):
    dev.synchronize()
    t0 = time.perf_counter()
    fn()
    dev.synchronize()
    return time.perf_counter() - t0


def medians(variants, rounds):
    for fn in variants.values():
        fn()
    ts = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ts[k].append(timed(fn))
    return {k: statistics.median(v) for k, v in ts.items()}, {k: min(v) for k, v in ts.items()}


bench = {"device": dev.name(), "rounds": args.rounds, "cases": []}
for preset in args.presets.split(","):
    cfg = synth.make_config(preset, **({"n_layers": args.layers} if args.layers else {}))
    lm = runtime.LoadedModel.from_synth_streamed(dev, cfg)
    V = cfg["vocab"]
    traits = runtime.prompt_traits(lm)
    for shape in args.shapes.split(","):
        n_seq, n_tok = (int(x) for x in shape.split("x"))
        rng = np.random.default_rng(n_seq)
        inputs = [rng.integers(1, V, size=n_tok).astype(np.int64) for _ in range(n_seq)]
        T = n_seq * n_tok
        kv = lm.new_kv_cache(T, max_seq_len=max(T, cfg["max_seq_len"]))
        plan = runtime.packed_plan(traits, [n_tok] * n_seq, lm.c.act_dtype)
        keep = {}

        def embed_packed():
            keep["ep"] = lm.embed_batch(inputs, kv, pooling="mean")

        def embed_loop():
            out = []
            for x in inputs:
                kv.reset()
                out.append(lm.embed(x, kv, 0, pooling="mean"))
            keep["el"] = np.stack(out)

        def score_packed():
            keep["sp"] = lm.score_batch(inputs, kv)

        def score_loop():
            out = []
            for x in inputs:
                kv.reset()
                out.append(lm.score(x, kv, 0))
            keep["sl"] = out

        med, mn = medians({"embed_packed": embed_packed, "embed_loop": embed_loop, "score_packed": score_packed, "score_loop": score_loop}, args.rounds)
        kv.reset()
        rel = float(np.linalg.norm(keep["ep"].astype(np.float64) - keep["el"]) / np.linalg.norm(keep["el"].astype(np.float64)))
        dsum = max(abs(a["sum_logprob"] - b["sum_logprob"]) for a, b in zip(keep["sp"], keep["sl"]))
        bench["cases"].append({
            "preset": preset, "layers": cfg["n_layers"], "n_seq": n_seq, "tokens_per_input": n_tok, "rows": T, "packed": plan["packed"], "plan": plan["plan"],
            "embed_packed_ms": round(med["embed_packed"] * 1e3, 3), "embed_loop_ms": round(med["embed_loop"] * 1e3, 3),
            "embed_packed_ms_min": round(mn["embed_packed"] * 1e3, 3), "embed_loop_ms_min": round(mn["embed_loop"] * 1e3, 3),
            "embed_loop_over_packed": round(med["embed_loop"] / med["embed_packed"], 2),
            "score_packed_ms": round(med["score_packed"] * 1e3, 3), "score_loop_ms": round(med["score_loop"] * 1e3, 3),
            "score_packed_ms_min": round(mn["score_packed"] * 1e3, 3), "score_loop_ms_min": round(mn["score_loop"] * 1e3, 3),
            "score_loop_over_packed": round(med["score_loop"] / med["score_packed"], 2),
            "embed_rel_l2_packed_vs_loop": rel, "max_abs_sum_logprob_difference": float(dsum)})
        print(json.dumps(bench["cases"][-1]), flush=True)
        del kv
    del lm

doc = {}
if os.path.exists(args.out):
    with open(args.out) as f:
        doc = json.load(f)
doc["bench"] = bench
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
