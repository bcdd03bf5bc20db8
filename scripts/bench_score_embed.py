#!/usr/bin/env python3
"""Prompt scoring and pooled embeddings (bz_score_kv / bz_embed_kv, bz_score.hip) against what a caller had before them, in one process.

Shape: the llama3.2-1b-bf16 preset's widths and vocabulary at 2 layers.  score at S = 512 and 2 048 beside forward_with_kv_cache(all_logits=True) + to_numpy()
+ a numpy log-softmax with the targets gathered; embed(mean) at S = 512 beside forward_embed + forward_layers_range + a final norm and a mean on the host.  Times are a
host clock around work that ends with its result on the host (or a device synchronise); every figure is the median of `--rounds` rounds, the variants alternating
inside a round, after a warm-up of every shape.  No profiler, no captured graph.  The library's workspace is read off the device's free memory around the first call
of each kind.  Writes profiles/score_embed.json."""
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
ap.add_argument("--preset", default="llama3.2-1b-bf16")
ap.add_argument("--layers", type=int, default=2)
ap.add_argument("--score-lens", default="512,2048")
ap.add_argument("--embed-len", type=int, default=512)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_embed.json"))
args = ap.parse_args()

dev = runtime.Device(0)
cfg = synth.make_config(args.preset, n_layers=args.layers)
lm = runtime.LoadedModel.from_synth_streamed(dev, cfg)
V, H = cfg["vocab"], cfg["hidden"]
final_norm = synth.llama_head(dict(cfg, vocab=8))[1].astype(np.float64)       # the norm weights only (same generator name and seed)
result = {"device": dev.name(), "preset": args.preset, "layers": args.layers, "vocab": V, "hidden": H, "rounds": args.rounds, "score": [], "embed": None}


def timed(fn):
    dev.synchronize()
    t0 = time.perf_counter()
    fn()
    dev.synchronize()
    return time.perf_counter() - t0


def free_bytes():
    dev.synchronize()
    return dev.memory_info()[0]


def medians(variants, rounds):
    for fn in variants.values():
        fn()
    ts = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ts[k].append(timed(fn))
    return {k: statistics.median(v) for k, v in ts.items()}, {k: min(v) for k, v in ts.items()}


for S in [int(x) for x in args.score_lens.split(",")]:
    p = synth.prompt_tokens(S, V, seed=S)
    tg = np.concatenate([p[1:], [-1]])
    kv = lm.new_kv_cache(S)
    keep = {}

    def score():
        keep["score"] = lm.score(p, kv, 0, targets=tg)

    def host():            # what a caller did before: every logits row to the host, a log-softmax there
        x = lm.forward_with_kv_cache(p, kv, 0, all_logits=True).to_numpy().reshape(S, V)
        m = x.max(axis=1, keepdims=True)
        lse = m[:, 0] + np.log(np.exp(x - m).sum(axis=1))
        keep["host"] = x[np.arange(S - 1), tg[:-1]] - lse[:-1]

    host()                 # the prompt path's own workspace is grown by now: what the next call adds is the sink's
    f0 = free_bytes()
    score()
    ws = f0 - free_bytes()
    med, mn = medians({"score": score, "host": host}, args.rounds)
    worst = float(np.max(np.abs(keep["score"]["rows"]["logprob"][:-1].astype(np.float64) - keep["host"])))
    result["score"].append({"S": S, "score_ms": round(med["score"] * 1e3, 3), "score_ms_min": round(mn["score"] * 1e3, 3),
                            "all_logits_host_softmax_ms": round(med["host"] * 1e3, 3), "all_logits_host_softmax_ms_min": round(mn["host"] * 1e3, 3),
                            "ratio_host_over_score": round(med["host"] / med["score"], 2), "workspace_bytes_grown": int(ws),
                            "logits_workspace_bytes": int(min(S, 2048) * V * 4), "caller_logits_bytes_before": int(S * V * 4),
                            "max_abs_logprob_difference": worst})
    del kv

S = args.embed_len
p = synth.prompt_tokens(S, V, seed=3)
kv = lm.new_kv_cache(S)
keep = {}


def embed():
    keep["embed"] = lm.embed(p, kv, 0, pooling="mean")


def staged():              # what a caller did before: the pieces API (token by token on the decode step) and the final norm on the host
    h, prev = lm.forward_layers_range(lm.forward_embed(p), None, kv, 0, cfg["n_layers"], 0)
    v = h.to_numpy().reshape(S, H).astype(np.float64) + prev.to_numpy().reshape(S, H)
    x = v / np.sqrt((v * v).mean(axis=1, keepdims=True) + cfg["rms_eps"]) * final_norm
    keep["staged"] = x.mean(axis=0)


f0 = free_bytes()
embed()
ws = f0 - free_bytes()
med, mn = medians({"embed": embed, "staged": staged}, args.rounds)
result["embed"] = {"S": S, "pooling": "mean", "embed_ms": round(med["embed"] * 1e3, 3), "embed_ms_min": round(mn["embed"] * 1e3, 3),
                   "staged_host_norm_ms": round(med["staged"] * 1e3, 3), "staged_host_norm_ms_min": round(mn["staged"] * 1e3, 3),
                   "ratio_staged_over_embed": round(med["staged"] / med["embed"], 2), "workspace_bytes_grown": int(ws),
                   "rows_workspace_bytes": int((min(S, 2048) + 2) * H * 4),
                   "max_abs_difference": float(np.max(np.abs(keep["embed"].astype(np.float64) - keep["staged"])))}

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print(json.dumps(result))
