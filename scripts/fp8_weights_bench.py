#!/usr/bin/env python3
"""FP8 (E4M3) weights against the same model as dense bf16: decode tokens/s (eager and --graphs), the FP8 step's achieved GB/s against the measured read
ceiling, per-launch times of one step, and the time to the first token of a 2048-token prompt.

    python scripts/fp8_weights_bench.py [--layers N] [--out profiles/fp8_weights.json]

Protocol (bench.py's): prompt 32, 128 decode tokens, one warm-up and three runs, the median.  Timed with events and the wall clock only (bz_generate's
statistics, bz_profile_step's event pairs).  The dense model is the FP8 model's own matrices read as bf16 (every E4M3 value is a bf16 value), so both
models have the same dims and the dense one is built by a table lookup instead of 7 G normal draws.  Results are merged into --out (keys this script
does not write, such as the GEMM error figures of tests/test_gpu_fp8_weights.py, are kept)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from blazr_amd import _lib as L          # noqa: E402
from blazr_amd import runtime, synth    # noqa: E402


def bf16_twin(spec, lut):
    """dense bf16 linear holding e4m3(q) 2^-9 (the scale's magnitude; the numbers do not matter to a timing)"""
    return dict(kind="dense", N=spec["N"], K=spec["K"], weight=lut[spec["weight"]])


def load(dev, cfg, dense):
    lut = synth.f32_to_bf16_bits(np.nan_to_num(synth.e4m3_table()) * np.float32(2.0 ** -9))
    lm = runtime.LoadedModel(dev, cfg)
    for i in range(cfg["n_layers"]):
        lay = synth.llama_layer(cfg, i)
        if dense:
            lay = {k: (bf16_twin(v, lut) if isinstance(v, dict) and v["kind"] == "fp8" else v) for k, v in lay.items()}
        lm.add_llama_layer(i, lay)
    lm.add_llama_head(*synth.llama_head(cfg))
    lm.finalize()
    return lm


def decode_runs(ex, prompt, graphs):
    """one warm-up and three runs of 128 tokens -> (median tok/s, all runs)"""
    runs = []
    for i in range(4):
        ex.generate(prompt, 128, use_graph=graphs)
        if i:
            runs.append(ex.last_stats["decode_tok_per_s"])
    return statistics.median(runs), runs


def ttft_runs(ex, prompt):
    runs = []
    for i in range(4):
        ex.generate(prompt, 2)
        if i:
            runs.append(ex.last_stats["ttft_ms"])
    return statistics.median(runs), runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=0, help="layers of the 8B shape to build (0: all 32)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp8_weights.json"))
    ap.add_argument("--no-ttft", action="store_true")
    args = ap.parse_args()
    over = dict(max_seq_len=2304)
    if args.layers:
        over["n_layers"] = args.layers
    cfg = synth.make_config("llama3.1-8b-fp8", **over)
    dev = runtime.Device(0)
    peak = C.c_double()
    L.check(L.lib().bz_probe_hbm_read(dev.h, 1 << 30, 6, C.byref(peak)))
    prompt, long_prompt = synth.prompt_tokens(32, cfg["vocab"], seed=26), synth.prompt_tokens(2048, cfg["vocab"], seed=27)
    res = dict(preset="llama3.1-8b-fp8", n_layers=cfg["n_layers"], protocol="prompt 32, 128 decode tokens, 1 warm-up + 3 runs, median", hbm_read_ceiling_gbs=peak.value, models={})
    for key, dense in (("fp8", False), ("bf16", True)):
        lm = load(dev, cfg, dense)
        ex = runtime.Executor(lm)
        resident, per_token = lm.weight_bytes()
        m = dict(resident_bytes=resident, bytes_per_token=per_token)
        for mode, graphs in (("eager", False), ("graphs", True)):
            med, runs = decode_runs(ex, prompt, graphs)
            m[mode] = dict(decode_tok_per_s=med, runs=runs, achieved_gbs=med * per_token / 1e9, of_read_ceiling=med * per_token / 1e9 / peak.value)
        kv = runtime.LayeredKvCache(dev, cfg["n_layers"], 1, cfg["n_kv_heads"], 64, cfg["max_seq_len"], cfg["head_dim"], L.BF16)
        lm.forward_with_kv_cache(prompt, kv, 0)
        prof = lm.profile_step(kv, 1, 32, iters=4)
        m["step_launches"] = [dict(name=k["name"], launches_per_step=k["launches"] / 4.0, us_per_launch=1e3 * k["total_ms"] / max(k["launches"], 1),
                                   gbs=k["algo_bytes"] / (1e6 * k["total_ms"]) if k["total_ms"] > 0 else 0.0) for k in prof]
        m["step_us_in_kernels"] = sum(1e3 * k["total_ms"] for k in prof) / 4.0
        if not args.no_ttft:
            med, runs = ttft_runs(ex, long_prompt)
            m["ttft_2048_ms"] = dict(median=med, runs=runs)
        res["models"][key] = m
        del ex, kv, lm
    f8, b16 = res["models"]["fp8"], res["models"]["bf16"]
    res["fp8_over_bf16"] = dict(eager=f8["eager"]["decode_tok_per_s"] / b16["eager"]["decode_tok_per_s"], graphs=f8["graphs"]["decode_tok_per_s"] / b16["graphs"]["decode_tok_per_s"])
    if not args.no_ttft:
        res["fp8_over_bf16"]["ttft_2048"] = f8["ttft_2048_ms"]["median"] / b16["ttft_2048_ms"]["median"]
    out = {}
    if os.path.exists(args.out):
        out = json.load(open(args.out))
    out["decode_and_prompt"] = res
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(dict(fp8_over_bf16=res["fp8_over_bf16"], fp8_graphs=f8["graphs"], bf16_graphs=b16["graphs"])))
    dev.close()


if __name__ == "__main__":
    main()
