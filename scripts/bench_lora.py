#!/usr/bin/env python3
"""What LoRA costs, and that a model without a table costs nothing.  Writes profiles/lora.json (or --out); every part can be run on its own and merged.

(a) --part a --parent-tree DIR: bench.py's headline (defaults: llama3-8b-awq, 128 steps, 3 reps inside) with NO table, this tree against a built checkout of
    the parent commit in DIR, one fresh process per reading, the two alternating (the way profiles/mlp_tail.json was taken).  The medians must differ by no more
    than the parent's own min-max spread in this session; asserted.  The launch labels of a decode step (bz_profile_step on llama3-8b-awq-2l) are identical by
    construction: asserted, not timed.
(b) --part b: llama3-8b-awq greedy decode tok/s (bz_generate with use_graph, 16-token prompt, --steps new tokens, median of --reps) without a table, then with a
    table under mask {q,v} and one r = 16 adapter active, the same with slot -1, and (a second model instance) mask all seven with one adapter active.
(c) --part c: the 64-row batched decode graph, ms per replay (host clock around --steps replays and a synchronise, after 8 untimed ones), with no table and with
    a {q,v} table and every row on one of four r = 16 adapters.
(b) and (c) are reported, not gated."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--part", default="a,b,c")
ap.add_argument("--parent-tree", default=None)
ap.add_argument("--procs", type=int, default=5)
ap.add_argument("--preset", default="llama3-8b-awq")
ap.add_argument("--steps", type=int, default=128)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--rows", type=int, default=64)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora.json"))
args = ap.parse_args()
parts = set(args.part.split(","))
med = statistics.median
result = json.load(open(args.out)) if os.path.exists(args.out) else {}

LABELS = ("import json, sys; sys.path.insert(0, '.'); from blazr_amd import runtime, synth; d = runtime.Device(0); "
          "lm = runtime.LoadedModel.from_synth_streamed(d, synth.make_config('llama3-8b-awq-2l', vocab=2048)); kv = lm.new_kv_cache(16); "
          "print(json.dumps(sorted((r['name'], r['launches']) for r in lm.profile_step(kv, 1, 0, iters=1))))")


def child(tree, argv):
    out = subprocess.run([sys.executable] + argv, cwd=tree, check=True, capture_output=True, text=True).stdout
    return json.loads(out.strip().splitlines()[-1])


if "a" in parts:
    if not args.parent_tree:
        sys.exit("--part a needs --parent-tree DIR (a built checkout of the parent commit)")
    trees = {"parent": os.path.abspath(args.parent_tree), "change": ROOT}
    labels = {k: child(t, ["-c", LABELS]) for k, t in trees.items()}
    assert labels["parent"] == labels["change"], labels
    runs = {k: [] for k in trees}
    for _ in range(args.procs):
        for k, t in trees.items():
            r = child(t, ["bench.py", "--gpus", "1"])
            runs[k].append(dict(value=r["value"], runs=r.get("runs")))
            print(k, r["value"], flush=True)
    summary = {}
    for k in trees:
        v = [x["value"] for x in runs[k]]
        summary[k] = dict(processes=v, reps_inside=[x["runs"] for x in runs[k]], median=med(v), min=min(v), max=max(v), spread=round(max(v) - min(v), 3))
    diff = abs(summary["change"]["median"] - summary["parent"]["median"])
    result["headline_tok_s_no_table"] = dict(command="python bench.py --gpus 1 (defaults), one process per reading, trees alternating", step_labels_2l=labels["change"],
                                             labels_identical=True, **summary, median_difference=round(diff, 3), within_parent_spread=bool(diff <= summary["parent"]["spread"]))
    json.dump(result, open(args.out, "w"), indent=1)
    assert diff <= summary["parent"]["spread"], (diff, summary["parent"]["spread"])

if parts & {"b", "c"}:
    from blazr_amd import runtime, synth
    import lora_cases
    dev = runtime.Device(0)
    cfg = synth.make_config(args.preset)
    prompt = [int(t) for t in synth.prompt_tokens(16, cfg["vocab"], seed=26)]

    def adapter(mask, seed):
        ad = lora_cases.make_adapter(cfg, mask, rank=16, alpha=32.0, seed=seed)
        return runtime.LoraAdapter.from_arrays(dev, ad["rank"], ad["alpha"], ad["pairs"])

    def tok_s(lm, name):
        ex, v = runtime.Executor(lm), []
        for _ in range(args.reps):
            ex.generate(prompt, args.steps, use_graph=True, lora_adapter=name)
            v.append(round(ex.last_stats["decode_tok_per_s"], 2))
        return dict(readings=v, median=med(v))

    def batch_ms(lm, names):
        per = (args.steps + 8 + 2 + 15) // 16
        pool = runtime.LayeredPagedKvCache(dev, cfg["n_layers"], args.rows * per, 16, cfg["n_kv_heads"], cfg["head_dim"], runtime.L.F16)
        tables = [[i + args.rows * j for j in range(per)] for i in range(args.rows)]
        g = runtime.BatchDecodeGraph(lm, pool, args.rows, per)
        if names is not None:
            g.set_adapters(names)
        v = []
        for _ in range(args.reps):
            g.seed([prompt[i % 16] for i in range(args.rows)], [1] * args.rows, tables)
            for _ in range(8):
                g.replay()
            dev.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                g.replay()
            dev.synchronize()
            v.append(round((time.perf_counter() - t0) * 1e3 / args.steps, 4))
        return dict(readings=v, median=med(v))

    lm = runtime.LoadedModel.from_synth_streamed(dev, cfg)
    dec, bat = {}, {}
    if "b" in parts:
        dec["no_table"] = tok_s(lm, None)
    if "c" in parts:
        bat["no_table"] = batch_ms(lm, None)
    lm.enable_lora(n_slots=4, max_rank=16, targets=("q", "v"))
    for i in range(4):
        lm.load_lora(adapter(("q", "v"), 10 + i), "a%d" % i)
    if "b" in parts:
        dec["mask_qv_r16_active"] = tok_s(lm, "a0")
        dec["mask_qv_r16_slot_none"] = tok_s(lm, None)
    if "c" in parts:
        bat["mask_qv_every_row_on_one_of_four_r16"] = batch_ms(lm, ["a%d" % (i % 4) for i in range(args.rows)])
        bat["mask_qv_no_row_adapted"] = batch_ms(lm, [None] * args.rows)
        result["batched_graph_ms_per_step"] = dict(rows=args.rows, steps=args.steps, preset=args.preset, **bat)
    if "b" in parts:
        del lm
        lm = runtime.LoadedModel.from_synth_streamed(dev, cfg)
        lm.enable_lora(n_slots=2, max_rank=16, targets=lora_cases.TARGETS)
        lm.load_lora(adapter(lora_cases.TARGETS, 20), "a0")
        dec["mask_all_r16_active"] = tok_s(lm, "a0")
        result["decode_tok_s"] = dict(preset=args.preset, steps=args.steps, command="bz_generate, use_graph, 16-token prompt", **dec)
    result["device"] = dev.name()
    json.dump(result, open(args.out, "w"), indent=1)
print(json.dumps(result))
