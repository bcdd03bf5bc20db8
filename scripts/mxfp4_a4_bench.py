#!/usr/bin/env python3
"""MXFP4 with FP4 activations (W4A4) beside the W4A16 GEMM, at the linear shapes of llama3.1-8b-mxfp4, and one 2048-token prompt with the mode off and on.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/mxfp4_a4_bench.py gemm --trace DIR           # needs an MI355X
    python scripts/mxfp4_a4_bench.py reduce --trace DIR [--out profiles/mxfp4_a4.json]                               # no device
    python scripts/mxfp4_a4_bench.py prompt [--layers N] [--out profiles/mxfp4_a4.json]                              # needs an MI355X, no profiler
    python scripts/mxfp4_a4_bench.py decode [--layers N] [--out profiles/mxfp4_a4.json]                              # needs an MI355X, no profiler
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/mxfp4_a4_bench.py decode --trace DIR       # needs an MI355X
    python scripts/mxfp4_a4_bench.py decode-reduce --trace DIR [--out profiles/mxfp4_a4.json]                        # no device

gemm: per shape and row count two warm-up calls of bz_prefill_matmul per mode, then nine alternating pairs (mode off, mode on); the calls are written in
order to DIR/calls.json.  reduce: the per-dispatch durations of the trace, cut into calls at k_pf_cvt16 (every call's first launch); a call's time is the sum of its quantiser,
GEMM and split-K reduction dispatches; medians per (shape, rows, mode), achieved FLOP/s = 2 S N K over that time.  prompt: the time to the first token of a
2048-token prompt (the wall clock of bz_generate's prefill, which ends in a synchronise), one warm-up and three runs per mode, the median.  decode: single-token
steps in modes 0, 1 and 3 (3: the FP4 decode GEMV k_gemv_mx4a4) in one process, captured step graphs, 16 prompt tokens + 257 generated, one warm-up and three runs
per mode, alternating; ms/step = (arrival of the last token - arrival of the first) / 256, the median run.  With --trace it runs 4 + 32 eager steps in modes 0 and
3 instead (a number known to decode-reduce, which divides the gemv_mx4* dispatches of the trace by it); decode-reduce: time per step in k_gemv_mx4 / k_gemv_mx4a4
and the bytes of all MXFP4 linears (4.25 bits per weight) over that time."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("qkv", 6144, 4096), ("o", 4096, 4096), ("gate_up", 28672, 4096), ("down", 4096, 14336)]
ROWS = [64, 512, 2048]
DOWN = "model.layers.0.mlp.down_proj.weight"
REPS = 9


def merge(path, key, value):
    out = json.load(open(path)) if os.path.exists(path) else {}
    out[key] = value
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


def gemm(trace):
    from blazr_amd import _lib as L
    from blazr_amd import runtime, synth
    dev = runtime.Device(0)
    calls = []
    for name, N, K in SHAPES:
        cfg = dict(arch="llama", hidden=N, n_layers=1, n_heads=1, n_kv_heads=1, head_dim=64, inter=K, vocab=64, rms_eps=1e-5, rope_theta=10000.0, act_dtype="bf16",
                   quant="none", max_seq_len=64, tie_embeddings=True)
        model = synth.make_llama(cfg)
        model["layers"][0]["down"] = synth.mxfp4_linear("bench." + name, N, K)
        lm = runtime.LoadedModel.from_synth(dev, model)
        for S in ROWS:
            tx = dev.tensor(np.random.default_rng(S).standard_normal((S, K)).astype(np.float32))
            ty = dev.zeros((S, N))
            for rep in range(-2, REPS):
                for mode in (0, 1):
                    lm.set_mxfp4_activations(mode)
                    L.check(L.lib().bz_prefill_matmul(lm.h, DOWN.encode(), tx.h, S, ty.h))
                    calls.append(dict(shape=name, N=N, K=K, S=S, mode=mode, warm=rep < 0))
        del lm
    with open(os.path.join(trace, "calls.json"), "w") as f:
        json.dump(calls, f)
    dev.close()


def reduce(trace, out):
    calls = json.load(open(os.path.join(trace, "calls.json")))
    files = glob.glob(os.path.join(trace, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel_trace.csv under " + trace
    disp = []
    for f in files:
        for r in csv.DictReader(open(f)):
            disp.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"]))
    disp.sort()
    per_call = []
    for _, dur, name in disp:
        if "k_pf_cvt16" in name:
            per_call.append(dict(quant=0, gemm=0, reduce=0))
        elif per_call and "k_mx4_quant_rows" in name:
            per_call[-1]["quant"] += dur
        elif per_call and ("k_gemm_mx4a4" in name or "k_gemm_mx4w<" in name or "k_gemm_mx4wI" in name):
            per_call[-1]["gemm"] += dur
        elif per_call and "k_gemm_mx4w_reduce" in name:
            per_call[-1]["reduce"] += dur
    assert len(per_call) == len(calls), (len(per_call), len(calls))
    groups = {}
    for c, t in zip(calls, per_call):
        if not c["warm"]:
            groups.setdefault((c["shape"], c["N"], c["K"], c["S"], c["mode"]), []).append(t)
    rows = []
    for (shape, N, K, S, mode), ts in groups.items():
        us = statistics.median(sum(t.values()) for t in ts) / 1e3
        rows.append(dict(shape=shape, N=N, K=K, S=S, mode="w4a4" if mode else "w4a16", us=us, quant_us=statistics.median(t["quant"] for t in ts) / 1e3,
                         reduce_us=statistics.median(t["reduce"] for t in ts) / 1e3, tflops=2.0 * S * N * K / us / 1e6, n=len(ts)))
    merge(out, "gemm", dict(protocol="rocprofv3 --kernel-trace, one process, modes alternating, 2 warm-up + %d timed calls each, medians; us = quantiser + GEMM + split-K reduction" % REPS,
                            rows=sorted(rows, key=lambda r: (r["shape"], r["S"], r["mode"]))))


def prompt(layers, out):
    from blazr_amd import runtime, synth
    dev = runtime.Device(0)
    cfg = synth.make_config("llama3.1-8b-mxfp4", max_seq_len=2304, **(dict(n_layers=layers) if layers else {}))
    lm = runtime.LoadedModel(dev, cfg)
    for i in range(cfg["n_layers"]):
        lm.add_llama_layer(i, synth.llama_layer(cfg, i))
    lm.add_llama_head(*synth.llama_head(cfg))
    lm.finalize()
    ex = runtime.Executor(lm)
    p = synth.prompt_tokens(2048, cfg["vocab"], seed=27)
    res = dict(preset="llama3.1-8b-mxfp4", n_layers=cfg["n_layers"], prompt=2048, protocol="time to the first token, 1 warm-up + 3 runs per mode, alternating, median")
    runs = {0: [], 1: []}
    for rep in range(4):
        for mode in (0, 1):
            lm.set_mxfp4_activations(mode)
            ex.generate(p, 2)
            if rep:
                runs[mode].append(ex.last_stats["ttft_ms"])
    res["ttft_ms_w4a16"], res["ttft_ms_w4a4"] = statistics.median(runs[0]), statistics.median(runs[1])
    res["runs_w4a16"], res["runs_w4a4"] = runs[0], runs[1]
    print(json.dumps(res))
    merge(out, "prompt_2048", res)
    dev.close()


def build_8b(runtime, synth, dev, layers, max_seq_len):
    cfg = synth.make_config("llama3.1-8b-mxfp4", max_seq_len=max_seq_len, **(dict(n_layers=layers) if layers else {}))
    lm = runtime.LoadedModel(dev, cfg)
    for i in range(cfg["n_layers"]):
        lm.add_llama_layer(i, synth.llama_layer(cfg, i))
    lm.add_llama_head(*synth.llama_head(cfg))
    lm.finalize()
    return cfg, lm


TRACE_WARM, TRACE_STEPS = 4, 32
MODE_NAME = {0: "w4a16", 1: "w4a4_gemm", 3: "w4a4_gemm_gemv"}


def decode(layers, out, trace):
    from blazr_amd import _lib as L
    from blazr_amd import runtime, synth
    dev = runtime.Device(0)
    cfg, lm = build_8b(runtime, synth, dev, layers, 512)
    p = synth.prompt_tokens(16, cfg["vocab"], seed=27)
    if trace:
        kvdt = L.BF16 if cfg["act_dtype"] == "bf16" else L.F16
        for mode in (0, 3):
            lm.set_mxfp4_activations(mode)
            kv = runtime.LayeredKvCache(dev, cfg["n_layers"], 1, cfg["n_kv_heads"], 64, cfg["max_seq_len"], cfg["head_dim"], kvdt)
            for i in range(TRACE_WARM + TRACE_STEPS):
                lm.forward_with_kv_cache([int(p[i % 16])], kv, i)
        with open(os.path.join(trace, "decode_calls.json"), "w") as f:
            json.dump(dict(n_layers=cfg["n_layers"], steps=TRACE_WARM + TRACE_STEPS), f)
        dev.close()
        return
    ex = runtime.Executor(lm)
    res = dict(preset="llama3.1-8b-mxfp4", n_layers=cfg["n_layers"], generated=257,
               protocol="captured step graphs, 1 warm-up + 3 runs per mode in one process, alternating; ms/step = (last token - first token) / 256, median run")
    runs = {0: [], 1: [], 3: []}
    for rep in range(4):
        for mode in (0, 1, 3):
            lm.set_mxfp4_activations(mode)
            ex.generate(p, 257, use_graph=True)
            st = ex.last_stats
            if rep:
                runs[mode].append((st["total_ms"] - st["ttft_ms"]) / (st["n_generated"] - 1))
    lm.set_mxfp4_activations(0)
    for mode, name in MODE_NAME.items():
        ms = statistics.median(runs[mode])
        res[name] = dict(ms_per_step=ms, tok_s=1e3 / ms, runs_ms_per_step=runs[mode])
    print(json.dumps(res))
    merge(out, "decode", res)
    dev.close()


def decode_reduce(trace, out):
    meta = json.load(open(os.path.join(trace, "decode_calls.json")))
    files = glob.glob(os.path.join(trace, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel_trace.csv under " + trace
    t = {"k_gemv_mx4a4": [], "k_gemv_mx4": []}
    for f in files:
        for r in csv.DictReader(open(f)):
            for key in t:                                      # (the longer name first)
                if key + "(" in r["Kernel_Name"] or r["Kernel_Name"].startswith(key + " ") or r["Kernel_Name"] == key:
                    t[key].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
                    break
    step_bytes = meta["n_layers"] * sum(N * (K // 2 + K // 32) for _, N, K in SHAPES)
    res = dict(protocol="rocprofv3 --kernel-trace, eager steps, %d warm-up + %d timed per mode; per step: all gemv_mx4* dispatches of the timed steps / %d; bytes = 4.25 bits per weight "
                        "of every MXFP4 linear" % (TRACE_WARM, TRACE_STEPS, TRACE_STEPS), n_layers=meta["n_layers"], bytes_per_step=step_bytes, read_ceiling_tb_s=6.15)
    for key, d in t.items():
        d.sort()
        assert d and len(d) % meta["steps"] == 0, (key, len(d), meta["steps"])
        per = len(d) // meta["steps"]
        timed = d[per * TRACE_WARM:]
        us = sum(x[1] for x in timed) / 1e3 / TRACE_STEPS
        res[key] = dict(dispatches_per_step=per, us_per_step=us, tb_s=step_bytes / us / 1e6, us_per_dispatch_median=statistics.median(x[1] for x in timed) / 1e3)
    print(json.dumps(res))
    merge(out, "decode_kernels", res)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["gemm", "reduce", "prompt", "decode", "decode-reduce"])
    ap.add_argument("--trace")
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mxfp4_a4.json"))
    a = ap.parse_args()
    if a.what == "decode":
        decode(a.layers, a.out, a.trace)
    elif a.what == "decode-reduce":
        decode_reduce(a.trace, a.out)
    else:
        gemm(a.trace) if a.what == "gemm" else reduce(a.trace, a.out) if a.what == "reduce" else prompt(a.layers, a.out)
