#!/usr/bin/env python3
"""Batched decode attention at long contexts: the scalar kernel (k_pf_attn, scores in LDS) beside the split-KV pair (k_rows_attn_split + k_rows_attn_merge,
bz_rows_attn.hip), inside the captured batched decode step.

  probe    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_rows_attn.py probe > DIR/probe.json
           Llama-3-8B heads (32 q / 8 kv, head_dim 128, f16 AWQ) on a 2-layer model of small widths, block size 16.  For every (N, context, kernel) one
           BatchDecodeGraph is captured at a capacity of `context` positions (rounded down to whole blocks), every row seeded just below the capacity, and
           replayed --warm + --iters times.  The scalar kernel runs with BZ_ROWS_SPLIT_MIN out of reach, the pair with the switch at 1 (a graph keeps what was
           decided at its capture).  Contexts beyond the scalar kernel's 8 180 positions run the pair only: nothing ran there before.  The kernels' names do
           not say N or the context, so the probe prints the order of its groups and `collect` cuts the trace's dispatches by it.
  collect  python scripts/bench_rows_attn.py collect --trace DIR --out profiles/rows_attn.json
           attention time per layer = the average duration of the group's attention dispatches (the warm-up replays dropped); beside it the K / V bytes a layer's
           attention has to read (N x context x n_kv_heads x head_dim x 2 bytes x 2) per second of that time, against the 6.15 TB/s streaming ceiling of DESIGN
           section 8.
The pool is zero-filled: the kernels' work does not depend on the values."""
import argparse
import csv
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BS, CEILING = 16, 6.15e12
KERNELS = {"scalar": ["k_pf_attn"], "split": ["k_rows_attn_split", "k_rows_attn_merge"]}


def cmd_probe(args):
    from blazr_amd import _lib as L
    from blazr_amd import runtime, synth
    rows = [int(x) for x in args.rows.split(",")]
    both = [int(x) for x in args.contexts.split(",")]
    new = [int(x) for x in args.new_contexts.split(",")] if args.new_contexts else []
    dev = runtime.Device(0)
    model = synth.make_llama("llama3-8b-awq-2l", hidden=2048, inter=1024, vocab=1024, max_seq_len=max(both + new))
    cfg = model["config"]
    lm = runtime.LoadedModel.from_synth(dev, model)
    nq, nkv, hd, nl = cfg["n_heads"], cfg["n_kv_heads"], cfg["head_dim"], cfg["n_layers"]
    pool = runtime.LayeredPagedKvCache(dev, nl, max(rows) * (max(both + new) // BS) + 1, BS, nkv, hd, L.F16)
    order = []
    total = args.warm + args.iters
    for ctx in both + new:
        per = ctx // BS
        for N in rows:
            for kernel in (["scalar", "split"] if ctx in both else ["split"]):
                if kernel == "split":
                    os.environ["BZ_ROWS_SPLIT_MIN"] = "1"
                else:
                    os.environ.pop("BZ_ROWS_SPLIT_MIN", None)
                plan = runtime.rows_attn_plan(nq, nkv, hd, L.F16, 0, N, per * BS)
                assert plan["kernel"] == (1 if kernel == "split" else 0), (ctx, N, kernel, plan)
                g = runtime.BatchDecodeGraph(lm, pool, N, per)
                tables = [[1 + i * per + j for j in range(per)] for i in range(N)]
                first = per * BS - total - 1                  # the context of the first replay; the last one ends below the capacity
                g.seed([5 + i for i in range(N)], [first] * N, tables)
                for _ in range(total):
                    g.replay()
                g.read_tokens(total - 1)                      # waits for the device
                order.append(dict(kernel=kernel, rows=N, capacity=per * BS, context_first=first, context_last=first + total - 1, replays=total, warm=args.warm, layers=nl,
                                  grid_slices=plan["grid_slices"], rows_per_pass=plan["rows_per_pass"], ws_bytes=plan["ws_bytes"]))
                del g
    print(json.dumps(dict(device=dev.name(), heads=[nq, nkv, hd], kv_dtype="f16", block_size=BS, layers=nl, order=order)))
    dev.close()


def cmd_collect(args):
    files = glob.glob(os.path.join(args.trace, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel_trace.csv under " + args.trace
    run = json.loads(open(os.path.join(args.trace, "probe.json")).read().strip().split("\n")[-1])
    pat = re.compile(r"\b(k_pf_attn|k_rows_attn_split|k_rows_attn_merge)\b")
    disp = {}
    for r in csv.DictReader(open(files[0])):
        m = pat.search(r["Kernel_Name"])
        if m:
            disp.setdefault(m.group(1), []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    for v in disp.values():
        v.sort()
    nq, nkv, hd = run["heads"]
    pos, out = {}, []
    for o in run["order"]:
        per_replay = o["layers"] * -(-o["rows"] // o["rows_per_pass"]) if o["kernel"] == "split" else o["layers"]
        n, skip = o["replays"] * per_replay, o["warm"] * per_replay
        us = 0.0
        parts = {}
        for name in KERNELS[o["kernel"]]:
            k = pos.get(name, 0)
            ds = [x[1] / 1e3 for x in disp.get(name, [])[k:k + n]]
            assert len(ds) == n, (name, o, len(ds))
            pos[name] = k + n
            ds = ds[skip:]
            parts[name] = dict(calls=len(ds), avg_us=round(sum(ds) / len(ds), 2), min_us=round(min(ds), 2), max_us=round(max(ds), 2))
            us += sum(ds) / len(ds) * (per_replay // o["layers"])
        ctx = (o["context_first"] + o["warm"] + o["context_last"]) / 2.0        # mean context of the timed replays
        kv_bytes = o["rows"] * ctx * nkv * hd * 2 * 2
        out.append(dict(o, attention_us_per_layer=round(us, 2), kernels=parts, kv_bytes_per_layer=int(kv_bytes), kv_tb_per_s=round(kv_bytes / (us * 1e-6) / 1e12, 3),
                        share_of_streaming_ceiling=round(kv_bytes / (us * 1e-6) / CEILING, 3)))
    for name, v in disp.items():
        assert pos.get(name, 0) == len(v), (name, pos.get(name), len(v))
    res = dict(what="attention time per layer of the captured batched decode step, scalar k_pf_attn (BZ_ROWS_SPLIT_MIN out of reach) beside k_rows_attn_split + "
                    "k_rows_attn_merge (BZ_ROWS_SPLIT_MIN=1); per-dispatch durations of one rocprofv3 --kernel-trace --stats run, warm-up replays dropped; "
                    "K / V bytes per second against the 6.15 TB/s streaming ceiling (DESIGN section 8)",
               device=run["device"], heads=run["heads"], kv_dtype=run["kv_dtype"], block_size=run["block_size"], layers=run["layers"], streaming_ceiling_tb_per_s=CEILING / 1e12,
               results=out)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for r in out:
        print("%-6s N %3d capacity %6d: %9.2f us per layer, %.3f TB/s of K / V (%.0f %% of the ceiling)" % (r["kernel"], r["rows"], r["capacity"], r["attention_us_per_layer"],
                                                                                                         r["kv_tb_per_s"], 100 * r["share_of_streaming_ceiling"]))


ap = argparse.ArgumentParser()
sub = ap.add_subparsers(dest="cmd", required=True)
p = sub.add_parser("probe")
p.add_argument("--rows", default="4,16,64")
p.add_argument("--contexts", default="1024,4096,8180", help="both kernels")
p.add_argument("--new-contexts", default="16384,32768", help="the split pair only (the scalar kernel cannot hold them)")
p.add_argument("--warm", type=int, default=3)
p.add_argument("--iters", type=int, default=12)
c = sub.add_parser("collect")
c.add_argument("--trace", required=True)
c.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_attn.json"))
args = ap.parse_args()
{"probe": cmd_probe, "collect": cmd_collect}[args.cmd](args)
