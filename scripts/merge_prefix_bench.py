#!/usr/bin/env python3
"""Puts the shared-stem runs of scripts/bench_engine.py (part d, one process each) into profiles/prefix_cache.json.

  merge_prefix_bench.py --parent P1.json P2.json .. --off O1.json .. --on N1.json .. [--kernel-stats kernel_stats.csv] [--out profiles/prefix_cache.json]

--parent: the scenario with the cache off on the parent commit's library; --off / --on: this commit, cache off / on.  The between-process spread of a group is
max - min of its wall times.  --kernel-stats: the kernel statistics of a traced cache-on run of its own (rocprofv3 --kernel-trace --stats), from which
k_kv_copy_slots' calls and time are taken; per copied block = total time / blocks copied in that run (--traced-blocks)."""
import argparse
import csv
import json
import os
import statistics

ap = argparse.ArgumentParser()
ap.add_argument("--parent", nargs="*", default=[])
ap.add_argument("--off", nargs="*", default=[])
ap.add_argument("--on", nargs="*", default=[])
ap.add_argument("--kernel-stats", default=None)
ap.add_argument("--traced-blocks", type=int, default=0)
ap.add_argument("--copy-note", default="not measured", help="what to record for the copy kernel when there is no kernel trace")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "prefix_cache.json"))
args = ap.parse_args()


def group(paths):
    runs = [json.load(open(p))["shared_stem"] for p in paths]
    if not runs:
        return None
    walls = [r["wall_s"] for r in runs]
    return {"processes": len(runs), "wall_s_median": round(statistics.median(walls), 4), "wall_s_min": min(walls), "wall_s_max": max(walls),
            "between_process_spread_s": round(max(walls) - min(walls), 4),
            "admit_host_ms_per_admission_median": round(statistics.median(r["admit_host_ms_per_admission"] for r in runs), 4),
            "median_steps_to_first_token": statistics.median(r["median_steps_to_first_token"] for r in runs),
            "prompt_tokens_prefilled_per_round": runs[0]["prompt_tokens_prefilled_per_round"], "prompt_tokens_predicted": runs[0]["prompt_tokens_predicted"], "runs": runs}


out = {"scenario": "scripts/bench_engine.py --skip a,b,c [--prefix-cache 1]: 64 requests behind one stem, one process per run",
       "parent_cache_off": group(args.parent), "cache_off": group(args.off), "cache_on": group(args.on), "copy_kernel": args.copy_note}
if out["parent_cache_off"] and out["cache_off"]:
    p, o = out["parent_cache_off"], out["cache_off"]
    out["cache_off_within_parent_spread"] = bool(p["wall_s_min"] - p["between_process_spread_s"] <= o["wall_s_median"] <= p["wall_s_max"] + p["between_process_spread_s"])
if out["cache_off"] and out["cache_on"]:
    out["wall_ratio_off_over_on"] = round(out["cache_off"]["wall_s_median"] / out["cache_on"]["wall_s_median"], 3)
if args.kernel_stats:
    for row in csv.DictReader(open(args.kernel_stats)):
        if "k_kv_copy_slots" in row.get("Name", ""):
            calls, total_ns = int(row["Calls"]), float(row["TotalDurationNs"])
            out["copy_kernel"] = {"source": "rocprofv3 --kernel-trace --stats, a run of its own", "launches": calls, "total_us": round(total_ns / 1e3, 2),
                                  "us_per_launch": round(total_ns / 1e3 / calls, 2), "blocks_copied": args.traced_blocks,
                                  "us_per_copied_block": round(total_ns / 1e3 / args.traced_blocks, 3) if args.traced_blocks else None}
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps({k: v for k, v in out.items() if k not in ("parent_cache_off", "cache_off", "cache_on")}))
