#!/usr/bin/env python3
"""Decode cost of a sliding window on the Mistral-7B Q4_K_M shape: one decode step at contexts 4096 / 16384 / 32768 with W = 0 and W = 4096 (same
weights, only the config field differs).  Per context: wall ms/step of eager steps (host-synchronised) and of the captured decode graph, and the
per-kernel times of bz_profile_step with the attention launches singled out.  The cache is grown to the context without being filled: the kernels'
time depends on how many rows they read, not on what the rows hold.  Writes one JSON document to stdout (or --out)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from blazr_amd import runtime, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--preset", default="mistral-7b-q4km")
ap.add_argument("--contexts", default="4096,16384,32768")
ap.add_argument("--window", type=int, default=4096)
ap.add_argument("--steps", type=int, default=32)
ap.add_argument("--layers", type=int, default=0)       # 0: the preset's
ap.add_argument("--out")
args = ap.parse_args()
ctxs = [int(x) for x in args.contexts.split(",")]
over = dict(max_seq_len=max(ctxs) + 2 * args.steps + 64)
if args.layers:
    over["n_layers"] = args.layers
dev = runtime.Device(0)
res = dict(command=" ".join(["python"] + sys.argv), preset=args.preset, steps=args.steps, device=dev.name() if hasattr(dev, "name") else "", rows=[])
for W in (0, args.window):
    cfg = synth.make_config(args.preset, **over)
    if W:
        cfg["sliding_window"] = W
    lm = runtime.LoadedModel.from_synth_streamed(dev, cfg)
    for ctx in ctxs:
        kv = lm.new_kv_cache(ctx + 2 * args.steps + 8)
        lm.forward_with_kv_cache([1], kv, ctx + 2 * args.steps)              # grow the cache once
        for i in range(4):
            lm.forward_with_kv_cache([1], kv, ctx + i).to_numpy()
        t0 = time.perf_counter()
        for i in range(args.steps):
            lm.forward_with_kv_cache([1], kv, ctx + i).to_numpy()
        eager_ms = (time.perf_counter() - t0) * 1e3 / args.steps
        prof = lm.profile_step(kv, 1, ctx, iters=8)
        att = {r["name"]: round(r["total_ms"] / 8 * 1e3, 1) for r in prof if "attn" in r["name"]}       # us per step, all layers
        total_us = sum(r["total_ms"] for r in prof) / 8 * 1e3
        g = runtime.DecodeGraph(lm, kv)
        g.seed_next_token(1, ctx)
        for _ in range(4):
            g.replay()
        g.read_token(3)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            g.replay()
        g.read_token(3 + args.steps)
        graph_ms = (time.perf_counter() - t0) * 1e3 / args.steps
        row = dict(window=W, context=ctx, eager_ms_per_step=round(eager_ms, 4), graph_ms_per_step=round(graph_ms, 4), kernels_us_per_step=round(total_us, 1),
                   attention_us_per_step=att)
        print(json.dumps(row), file=sys.stderr, flush=True)
        res["rows"].append(row)
        del g, kv
    del lm
text = json.dumps(res, indent=1)
if args.out:
    open(args.out, "w").write(text + "\n")
print(text)
dev.close()
