#!/usr/bin/env python3
"""INT8 W8A8 beside FP8 weights at the same commit, shape and context: decode ms/step and tokens/s, 512- and 2048-token prompt times, and the per-launch times of
one decode step (k_gemv_i8 against k_gemv_f8 on the q/k/v, o, gate/up and down shapes).

    python scripts/int8_weights_bench.py [--layers N] [--rounds R] [--out profiles/int8.json]

Protocol: each model runs in a process of its own, the two alternating for R rounds (int8, fp8, int8, fp8, ...), so that drift of the machine falls on both; per
process one warm-up and three runs of (prompt 32, 128 decode tokens, captured graphs), the median; prompts: one warm-up and three runs of 2 tokens after the
prompt, the median time to the first token.  The spread of the FP8 medians over the rounds is the noise floor the comparison is read against.  Timed with
events and the wall clock only (bz_generate's statistics, bz_profile_step's event pairs).  For kernel times from the profiler, run one child under it in a run of
its own, both models in one process:  rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/int8_weights_bench.py --child trace --layers N"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(kind, layers, trace=False):
    from blazr_amd import _lib as L
    from blazr_amd import runtime, synth
    over = dict(max_seq_len=2304)
    if layers:
        over["n_layers"] = layers
    cfg = synth.make_config("llama3.1-8b-%s" % kind, **over)
    dev = runtime.Device(0)
    lm = runtime.LoadedModel(dev, cfg)
    for i in range(cfg["n_layers"]):
        lm.add_llama_layer(i, synth.llama_layer(cfg, i))
    lm.add_llama_head(*synth.llama_head(cfg))
    lm.finalize()
    ex = runtime.Executor(lm)
    res = dict(kind=kind, n_layers=cfg["n_layers"], bytes_per_token=lm.weight_bytes()[1])
    prompt = synth.prompt_tokens(32, cfg["vocab"], seed=26)
    runs = []
    for i in range(2 if trace else 4):
        ex.generate(prompt, 128, use_graph=not trace)      # (under the profiler: eager steps, so that every launch is a dispatch of its own in the trace)
        if i:
            runs.append(ex.last_stats["decode_tok_per_s"])
    if trace:
        return dev.close()
    res["decode_tok_per_s"] = dict(median=statistics.median(runs), runs=runs)
    res["decode_ms_per_step"] = 1e3 / res["decode_tok_per_s"]["median"]
    for n in (512, 2048):
        p, runs = synth.prompt_tokens(n, cfg["vocab"], seed=27), []
        for i in range(4):
            ex.generate(p, 2)
            if i:
                runs.append(ex.last_stats["ttft_ms"])
        res["prompt_%d_ms" % n] = dict(median=statistics.median(runs), runs=runs)
    kv = runtime.LayeredKvCache(dev, cfg["n_layers"], 1, cfg["n_kv_heads"], 64, cfg["max_seq_len"], cfg["head_dim"], L.BF16)
    lm.forward_with_kv_cache(prompt, kv, 0)
    prof = lm.profile_step(kv, 1, 32, iters=4)
    res["step_launches"] = [dict(name=k["name"], launches_per_step=k["launches"] / 4.0, us_per_launch=1e3 * k["total_ms"] / max(k["launches"], 1),
                                 gbs=k["algo_bytes"] / (1e6 * k["total_ms"]) if k["total_ms"] > 0 else 0.0) for k in prof]
    print("RESULT " + json.dumps(res))
    dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=0, help="layers of the 8B shape to build (0: all 32)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "int8.json"))
    ap.add_argument("--child", choices=["int8", "fp8", "trace"], help="trace: both models in this process, decode steps only (for a profiler run)")
    args = ap.parse_args()
    if args.child == "trace":
        return [child(k, args.layers, trace=True) for k in ("int8", "fp8")]
    if args.child:
        return child(args.child, args.layers)
    rounds = []
    for r in range(args.rounds):
        for kind in ("int8", "fp8"):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--layers", str(args.layers)], capture_output=True, text=True, check=True, timeout=600).stdout
            rounds.append(json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:]))
            print("round %d %s: %.1f tok/s" % (r, kind, rounds[-1]["decode_tok_per_s"]["median"]), flush=True)
    med = {k: statistics.median(x["decode_tok_per_s"]["median"] for x in rounds if x["kind"] == k) for k in ("int8", "fp8")}
    f8 = [x["decode_tok_per_s"]["median"] for x in rounds if x["kind"] == "fp8"]
    summary = dict(decode_tok_per_s=med, int8_over_fp8=med["int8"] / med["fp8"], fp8_spread=(max(f8) - min(f8)) / med["fp8"],
                   **{"prompt_%d_ms" % n: {k: statistics.median(x["prompt_%d_ms" % n]["median"] for x in rounds if x["kind"] == k) for k in ("int8", "fp8")} for n in (512, 2048)})
    with open(args.out, "w") as f:
        json.dump(dict(protocol=__doc__.split("Protocol: ")[1].split("  For kernel times")[0], layers=args.layers or 32, summary=summary, rounds=rounds), f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
