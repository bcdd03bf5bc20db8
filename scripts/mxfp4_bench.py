#!/usr/bin/env python3
"""MXFP4 weights beside the FP8 and AWQ forms of the 8B shape: decode ms per step and tokens/s (--graphs), the per-launch times of one MXFP4 step as a
fraction of the measured read ceiling, the time to the first token of a 512-token prompt (MXFP4, FP8, dense bf16), and the registers of the new kernels.

    python scripts/mxfp4_bench.py [--layers N] [--out profiles/mxfp4.json]            # needs an MI355X
    python scripts/mxfp4_bench.py --resources-only [--out profiles/mxfp4.json]        # needs blazr_amd/csrc/bz_mxfp4.o (a local build), no device

Protocol (bench.py's): prompt 32, 128 decode tokens, one warm-up and three runs, the median; all models in one session.  Timed with events and the wall clock
only (bz_generate's statistics, bz_profile_step's event pairs).  The dense bf16 model is the FP8 model's own matrices read as bf16, as in
scripts/fp8_weights_bench.py.  Results are merged into --out."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from blazr_amd import _lib as L          # noqa: E402
from blazr_amd import runtime, synth    # noqa: E402

KV = dict(f16=L.F16, bf16=L.BF16)


def load(dev, cfg, bf16_twin=False):
    lut = synth.f32_to_bf16_bits(np.nan_to_num(synth.e4m3_table()) * np.float32(2.0 ** -9))
    lm = runtime.LoadedModel(dev, cfg)
    for i in range(cfg["n_layers"]):
        lay = synth.llama_layer(cfg, i)
        if bf16_twin:
            lay = {k: (dict(kind="dense", N=v["N"], K=v["K"], weight=lut[v["weight"]]) if isinstance(v, dict) and v["kind"] == "fp8" else v) for k, v in lay.items()}
        lm.add_llama_layer(i, lay)
    lm.add_llama_head(*synth.llama_head(cfg))
    lm.finalize()
    return lm


def median_of(fn, key):
    runs = []
    for i in range(4):
        fn()
        if i:
            runs.append(fn.ex.last_stats[key])
    return statistics.median(runs), runs


def resources(out_path):
    obj = os.path.join(ROOT, "blazr_amd", "csrc", "bz_mxfp4.o")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_resources.py"), obj], capture_output=True, text=True, check=True)
    merge(out_path, "kernel_resources", json.loads(r.stdout))
    print(r.stdout)


def merge(path, key, value):
    out = json.load(open(path)) if os.path.exists(path) else {}
    out[key] = value
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=0, help="layers of the 8B shape to build (0: all 32)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mxfp4.json"))
    ap.add_argument("--resources-only", action="store_true")
    args = ap.parse_args()
    if args.resources_only:
        return resources(args.out)
    over = dict(max_seq_len=768)
    if args.layers:
        over["n_layers"] = args.layers
    dev = runtime.Device(0)
    peak = C.c_double()
    L.check(L.lib().bz_probe_hbm_read(dev.h, 1 << 30, 6, C.byref(peak)))
    res = dict(protocol="prompt 32, 128 decode tokens, 1 warm-up + 3 runs, median; 512-token prompt: time to the first token, same repetitions",
               hbm_read_ceiling_gbs=peak.value, models={})
    for key, preset, twin in (("mxfp4", "llama3.1-8b-mxfp4", False), ("fp8", "llama3.1-8b-fp8", False), ("awq", "llama3-8b-awq", False), ("bf16", "llama3.1-8b-fp8", True)):
        cfg = synth.make_config(preset, **over)
        prompt, long_prompt = synth.prompt_tokens(32, cfg["vocab"], seed=26), synth.prompt_tokens(512, cfg["vocab"], seed=27)
        lm = load(dev, cfg, twin)
        ex = runtime.Executor(lm)
        resident, per_token = lm.weight_bytes()
        m = dict(preset=preset, n_layers=cfg["n_layers"], resident_bytes=resident, bytes_per_token=per_token)
        if key != "bf16":
            dec = lambda: ex.generate(prompt, 128, use_graph=True)
            dec.ex = ex
            med, runs = median_of(dec, "decode_tok_per_s")
            m["decode"] = dict(tok_per_s=med, ms_per_step=1e3 / med, runs=runs, achieved_gbs=med * per_token / 1e9, of_read_ceiling=med * per_token / 1e9 / peak.value)
        if key != "awq":
            pf = lambda: ex.generate(long_prompt, 2)
            pf.ex = ex
            med, runs = median_of(pf, "ttft_ms")
            m["ttft_512_ms"] = dict(median=med, runs=runs)
        if key == "mxfp4":
            kv = runtime.LayeredKvCache(dev, cfg["n_layers"], 1, cfg["n_kv_heads"], 64, cfg["max_seq_len"], cfg["head_dim"], KV[cfg["act_dtype"]])
            lm.forward_with_kv_cache(prompt, kv, 0)
            prof = lm.profile_step(kv, 1, 32, iters=4)
            m["step_launches"] = [dict(name=k["name"], launches_per_step=k["launches"] / 4.0, us_per_launch=1e3 * k["total_ms"] / max(k["launches"], 1),
                                       gbs=k["algo_bytes"] / (1e6 * k["total_ms"]) if k["total_ms"] > 0 else 0.0,
                                       of_read_ceiling=(k["algo_bytes"] / (1e6 * k["total_ms"]) if k["total_ms"] > 0 else 0.0) / peak.value) for k in prof]
            del kv
        res["models"][key] = m
        print(json.dumps({key: {k: v for k, v in m.items() if k != "step_launches"}}), flush=True)
        del ex, lm
    merge(args.out, "decode_and_prompt", res)
    dev.close()


if __name__ == "__main__":
    main()
