#!/usr/bin/env python3
"""bench.py -- decode tokens/sec + HBM-roofline fraction, Llama-3-8B AWQ-INT4 (gs=128), seq=1 greedy decode.

Contract (driver):  python bench.py --gpus N --steps K --warmup W   prints ONE JSON line on rank 0.
  * a "step" is one pass of the hot path = one decoded token (one hipGraph replay of the whole decode step).
  * N > 1 (launched by torch.distributed.run, one rank per GPU): the decode loop does not shard (SURVEY.md 8e,
    "replicas only"): every rank runs an independent replica on its own GPU, no data-path collective;
    value = tokens decoded by all ranks / max-over-ranks time ("scaling": "weak").
  * weights are seeded synthetic at the reference shapes (no network, no checkpoints): SURVEY.md 8d.
  * timed region: inputs resident in HBM (model loaded, prompt prefilled, graph captured) before the first event.
  * protocol of the reference's own bench (/root/reference/src/cli/bench.rs:30-33,142-146): warm-up, then `--reps` timed runs of exactly
    K steps each (every run bracketed by a barrier + device synchronise, MAX over ranks), the MEDIAN run is reported; all runs are listed.
  * --dump-outputs DIR: the last timed step's logits row and greedy id, DIR/logits.npy (float32) and DIR/next_token.npy (float64).
  * a plain run does only that: load, prefill, probe the read ceiling (so that the timed steps start from the same device state whatever
    the options), capture, warm up, time, dump, print.  Its "roofline" holds the whole step's fractions of the 8 TB/s spec peak and of the
    measured read ceiling alone (tokens/s x algorithmic bytes per token: no run of their own).
--full adds what takes runs of its own, after the timed region: "roofline" in full (dominant kernel,
pure dispatch time from HIP events on the launch stream vs the 8 TB/s spec peak AND vs the read ceiling measured on this device in the same
process) and "kernels", "cpu_baseline" (the CPU oracle -- a port, the reference's own --cpu path cannot be built here: BASELINE.md 4),
"parity" (GPU vs CPU oracle on the full model: free-running greedy ids, and the CPU ids teacher-forced through bz_forward_kv with per-step
logit errors), "prefill" (the prompt phase on its own) and "latency" (the reference bench's TTFT / ITL matrix).
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 GB/s is the measured copy ceiling
TOKEN_LOG = 4096        # bz_decode_graph::LOGCAP: a decode graph keeps the ids of its last 4096 replays since the seed


def hip_events(stream):
    """Minimal HIP event timer on a given stream (torch.cuda.Event only sees torch's current stream)."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]

    class T:
        def __init__(self):
            self.a, self.b = C.c_void_p(), C.c_void_p()
            assert hip.hipEventCreate(C.byref(self.a)) == 0 and hip.hipEventCreate(C.byref(self.b)) == 0

        def start(self):
            assert hip.hipEventRecord(self.a, stream) == 0

        def stop(self):
            assert hip.hipEventRecord(self.b, stream) == 0

        def ms(self):
            assert hip.hipEventSynchronize(self.b) == 0
            out = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(out), self.a, self.b) == 0
            return float(out.value)
    return T()


def kernels_sha16():
    """identity of the kernel sources this library was built from (the PMC pass is stamped with it)"""
    h = hashlib.sha256()
    for f in ("bz_kernels.hip", "bz_internal.h", "bz_dev.h"):
        h.update(open(os.path.join(ROOT, "blazr_amd", "csrc", f), "rb").read())
    return h.hexdigest()[:16]


def pmc_traffic(label):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 --pmc passes (profiles/r03_pmc_traffic.json, made by
    scripts/pmc_traffic.py: separate FETCH_SIZE / WRITE_SIZE passes, gfx950 correction (2*FETCH + WRITE) * 1024).  A process cannot collect
    PMC counters on itself, so the value is read back from the file -- and only when the file was made from THESE kernel sources
    (`kernels_sha16` stamp); a stale pass gives None and says so.  Returns (bytes or None, note)."""
    try:
        d = json.load(open(os.path.join(ROOT, "profiles", "r03_pmc_traffic.json")))
    except (OSError, ValueError):
        return None, "no PMC pass committed for this round"
    if d.get("kernels_sha16") != kernels_sha16():
        return None, "stale: the committed PMC pass was taken on other kernel sources (%s)" % d.get("kernels_sha16")
    for lbl, sym in d.get("labels", {}).items():
        if label.startswith(lbl):
            for name, v in d.get("kernels", {}).items():
                if name.startswith(sym):
                    return v["hbm_bytes_per_launch"], "rocprofv3 --pmc pass of these kernel sources (%s)" % d.get("kernels_sha16")
    return None, "kernel not in the PMC pass"


def run_ids(graph, first, n_run, n_head):
    """[first] + the ids of the first n_head steps of a graph run of n_run replays, as far as the token log still holds them
    (a run longer than TOKEN_LOG has overwritten its first ids)"""
    return [first] + [graph.read_token(i) for i in range(min(n_head, n_run) if n_run <= TOKEN_LOG else 0)]


def dump_outputs(d, graph, last):
    """--dump-outputs: what the caller of the timed path received from its last step -- the logits row (float32) and the greedy id it
    picked (float64) -- as DIR/<name>.npy, so that two builds can be compared output for output on the same seeded inputs"""
    os.makedirs(d, exist_ok=True)
    np.save(os.path.join(d, "logits.npy"), graph.read_logits().astype(np.float32))
    np.save(os.path.join(d, "next_token.npy"), np.array([last], dtype=np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=128)      # /root/reference/src/cli/bench.rs:27 decode tokens per run
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--preset", default="llama3-8b-awq")
    ap.add_argument("--prompt-len", type=int, default=16)   # 16 fixed prompt ids, context <= 144 + warmup
    # seed of the 16 prompt ids: the first seed >= 7 whose CPU-oracle greedy run on this model has no near-tie (top-2 gap >= 1e-2 of max|logit|,
    # SURVEY.md 7) in its first 28 decode steps, found offline by scripts/find_bench_seed.py -- so that the free-running id comparison is fair
    ap.add_argument("--prompt-seed", type=int, default=26)
    ap.add_argument("--reps", type=int, default=3)           # timed runs of exactly --steps steps each; the median is reported
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-latency", action="store_true")     # skip the TTFT / ITL matrix of the reference's bench (prompt 32 / 128 / 512)
    ap.add_argument("--cpu-tokens", type=int, default=32)    # ~10 s of CPU work on the GPU box's host cores (bounded sample)
    # OpenMP threads of the CPU baseline (SURVEY 8d planned OMP_NUM_THREADS = nproc; the count actually used is what `cpu_baseline.cores` reports).  Default 16:
    # measured on the GPU box (256 logical CPUs, its share for one GPU is 16), 64 threads gave 2.6 tok/s against 3.4 with 16 -- the GEMVs are bound by
    # the host's memory system, and oversubscribing the share only adds contention
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--dump-outputs", metavar="DIR")         # write the last timed step's outputs as DIR/<name>.npy (dump_outputs)
    # also measure what the headline does not need (docstring): roofline and per-kernel figures, CPU baseline + parity, prompt phase, latency matrix;
    # --no-cpu-baseline / --no-latency / --cpu-tokens / --cpu-threads apply to such a run
    ap.add_argument("--full", action="store_true")
    args = ap.parse_args()

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    dist = None
    if world > 1:
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    n_gpus = max(world, 1)

    from blazr_amd import runtime, synth

    if args.preset in synth.MAMBA_PRESETS or args.preset in synth.DSV2_PRESETS:
        if args.preset in synth.DSV2_PRESETS and "--prompt-len" not in sys.argv:
            args.prompt_len = 512          # BASELINE.json configs[4]: prefill 512 + decode 128
        return bench_aux(args, rank, local_rank, world, dist)
    cfg = synth.make_config(args.preset)
    need = args.prompt_len + args.warmup + args.steps + 8
    if need > cfg["max_seq_len"]:
        cfg["max_seq_len"] = need
    dev = runtime.Device(local_rank)
    t0 = time.time()
    want_cpu = (args.full and rank == 0 and world == 1 and not args.no_cpu_baseline)
    lm = runtime.LoadedModel(dev, cfg)
    host_layers = []
    for i in range(cfg["n_layers"]):
        lay = synth.llama_layer(cfg, i)
        lm.add_llama_layer(i, lay)
        if want_cpu:
            host_layers.append(lay)
    emb, fnorm, lmh = synth.llama_head(cfg)
    lm.add_llama_head(emb, fnorm, lmh)
    lm.finalize()
    load_s = time.time() - t0
    resident, per_token = lm.weight_bytes()
    algo_bytes = synth.algorithmic_bytes_per_token(cfg)
    assert per_token == algo_bytes, (per_token, algo_bytes)

    from blazr_amd import _lib as L
    prompt = synth.prompt_tokens(args.prompt_len, cfg["vocab"], seed=args.prompt_seed)
    kv_dt = {"f16": L.F16, "bf16": L.BF16, "f32": L.F32}[cfg["act_dtype"]]
    kv = runtime.LayeredKvCache(dev, cfg["n_layers"], 1, cfg["n_kv_heads"], need, cfg["max_seq_len"], cfg["head_dim"], kv_dt)
    logits = lm.forward_with_kv_cache(prompt, kv, 0)                       # prefill (untimed)
    prefill_row = logits.to_numpy().reshape(-1).copy()
    first = int(runtime.logits_to_token(dev, logits, [], []).to_numpy()[0])  # argmax_on_gpu (cuda_graphs.rs:149-163)
    # the read ceiling of this device, measured in this process before the timed region (rotating 1 GiB buffers, no arithmetic); a plain run
    # keeps it too, so that the timed steps start from the same device state as in a --full run
    peak_meas = C.c_double()
    L.check(L.lib().bz_probe_hbm_read(dev.h, 1 << 30, 6, C.byref(peak_meas)))
    graph = runtime.DecodeGraph(lm, kv)
    timer = hip_events(C.c_void_p(dev.stream()))
    from blazr_amd import replicas
    runs = []
    for _ in range(max(1, args.reps)):
        # every run starts from the same state: first generated token at the first free position (later cache rows are simply rewritten)
        graph.seed_next_token(first, args.prompt_len)
        for _ in range(args.warmup):
            graph.replay()
        dev.synchronize()
        if dist is not None:
            dist.barrier()
        dev.synchronize()
        t_host0 = time.perf_counter()
        timer.start()
        for _ in range(args.steps):
            graph.replay()
        timer.stop()
        gpu_ms = timer.ms()
        dev.synchronize()
        host_ms = (time.perf_counter() - t_host0) * 1e3
        if dist is not None:
            dist.barrier()
        runs.append(replicas.aggregate_tokens_per_s(max(gpu_ms, host_ms), args.steps, dist, "cuda" if dist is not None else None) + (gpu_ms, host_ms))
    runs_sorted = sorted(runs, key=lambda r: r[1])
    tok_s, wall_ms, gpu_ms, host_ms = runs_sorted[len(runs_sorted) // 2]      # the median run
    n_run = args.warmup + args.steps
    last = graph.read_token(n_run - 1)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, graph, last)      # before profile_step below overwrites the model's logits row
    tokens = run_ids(graph, first, n_run, max(2, args.cpu_tokens) if want_cpu else 0)

    pos = args.prompt_len + args.warmup + args.steps
    pm = float(peak_meas.value)
    whole_step_frac = round(algo_bytes * (tok_s / n_gpus) / (HBM_PEAK_GBS * 1e9), 4)
    whole_step_frac_of_measured = round(algo_bytes * (tok_s / n_gpus) / (pm * 1e9), 4) if pm > 0 else None
    roof = {"bound": "hbm", "peak": HBM_PEAK_GBS, "unit": "GB/s", "peak_measured": round(pm, 1),
            "whole_step_frac": whole_step_frac, "whole_step_frac_of_measured": whole_step_frac_of_measured}
    if args.full:
        # per-kernel dispatch times of real decode steps (pure kernel time, hipExtLaunchKernelGGL start/stop events)
        prof = lm.profile_step(kv, last, min(pos, cfg["max_seq_len"] - 5), iters=4)
        for p in prof:
            p["avg_us"] = 1e3 * p["total_ms"] / max(p["launches"], 1)
            p["gbs"] = (p["algo_bytes"] / 1e9) / (p["total_ms"] / 1e3) if p["total_ms"] > 0 and p["algo_bytes"] > 0 else None
        dom = max(prof, key=lambda p: p["total_ms"])
        traffic, traffic_note = pmc_traffic(dom["name"])
        roof = {"bound": "hbm", "kernel": dom["name"], "achieved": round(dom["gbs"], 1) if dom["gbs"] else None, "peak": HBM_PEAK_GBS,
                "unit": "GB/s", "frac": round(dom["gbs"] / HBM_PEAK_GBS, 4) if dom["gbs"] else None, "traffic": traffic, "traffic_note": traffic_note,
                "peak_measured": round(pm, 1), "frac_of_measured": round(dom["gbs"] / pm, 4) if dom["gbs"] and pm > 0 else None,
                "bytes_per_launch": dom["algo_bytes"] / max(dom["launches"], 1), "avg_launch_us": round(dom["avg_us"], 2),
                "whole_step_frac": whole_step_frac, "whole_step_frac_of_measured": whole_step_frac_of_measured}

    out = {"metric": "decode tokens/sec, Llama-3-8B AWQ-INT4 seq=1 on MI355X (and HBM-roofline fraction)", "value": round(tok_s, 2),
           "unit": "tokens/s", "n_gpus": n_gpus, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(wall_ms / args.steps, 5),
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "i4", "data": "synthetic",
           "config": {"workload": "%s greedy decode, batch 1, seq=1, prompt %d (seed %d), whole step as one hipGraph; N>1 = independent replicas"
                                  % (args.preset, args.prompt_len, args.prompt_seed), "algorithmic_bytes_per_token": algo_bytes,
                      "resident_weight_bytes": resident, "context_at_end": pos},
           "runs": {"protocol": "%d warm-up steps + %d timed steps per run, %d runs, median reported (cli/bench.rs:30-33,142-146)" % (args.warmup, args.steps, len(runs)),
                    "tokens_per_s": [round(r[0], 2) for r in runs], "ms": [round(r[1], 3) for r in runs]},
           "roofline": roof}
    if args.full:
        out["kernels"] = [{k: (round(v, 3) if isinstance(v, float) else v) for k, v in p.items()} for p in prof]
    out.update({"gpu_ms_events": round(gpu_ms, 3), "host_ms": round(host_ms, 3), "load_s": round(load_s, 1)})

    if want_cpu:
        # CPU baseline: the oracle (a port -- BASELINE.md 4), same weights, same prompt, bounded sample; and the parity gate
        from oracle import orc_py
        orc_py.set_threads(max(1, min(args.cpu_threads, os.cpu_count() or 1)))
        model = dict(config=cfg, embed=emb, final_norm=fnorm, lm_head=lmh, layers=host_layers)
        om = orc_py.OrcLlama(model)
        n_cpu = max(2, args.cpu_tokens)
        okv = om.new_kv(args.prompt_len + n_cpu + 1)
        tp0 = time.perf_counter()
        lo = om.forward_kv(prompt, okv, 0)
        t_prefill = time.perf_counter() - tp0
        cpu_rows = [np.asarray(lo).reshape(-1).copy()]
        cpu_tokens = [int(cpu_rows[0].argmax())]
        td0 = time.perf_counter()
        for i in range(n_cpu - 1):
            lo = om.forward_kv([cpu_tokens[-1]], okv, args.prompt_len + i)
            cpu_rows.append(np.asarray(lo).reshape(-1).copy())
            cpu_tokens.append(int(cpu_rows[-1].argmax()))
        t_decode = time.perf_counter() - td0
        orc_py.lib().orc_kv_free(okv)
        cpu_tok_s = (n_cpu - 1) / t_decode          # bench.rs:299-306: (tokens - 1) / (total - TTFT)
        out["cpu_baseline"] = {"value": round(cpu_tok_s, 3), "unit": "tokens/s", "cores": orc_py.lib().orc_num_threads(), "kind": "port",
                               "sample": "oracle/liborc.so (C + OpenMP, exactly rounded dot products), same synthetic weights and prompt: %d-token prefill (%.1f s) + %d "
                                         "greedy decode tokens (%.1f s); host has %d logical CPUs" % (args.prompt_len, t_prefill, n_cpu - 1, t_decode, os.cpu_count())}

        # (1) free-running ids: the graph's greedy ids against the CPU's, up to the first step whose oracle top-2 gap is a near-tie
        def gap_of(row):
            top2 = np.partition(row, -2)[-2:]
            return float(top2[1] - top2[0]) / max(float(np.abs(row).max()), 1e-30)
        gaps = [gap_of(r) for r in cpu_rows]
        # near-tie guard = 8 rounding units of the activation dtype: 4e-3 for f16 (2^-11; also used for f32 models), 3.1e-2 for bf16 (2^-8) -- two correct
        # pipelines in that dtype differ by about that much after a few layers (tests/test_gpu_parity_truth.py, scripts/parity_depth.py)
        guard = 8.0 * 2.0 ** -8 if cfg["act_dtype"] == "bf16" else 4e-3
        fair_prefix = next((i for i, g in enumerate(gaps) if g < guard), len(gaps))
        n_both = min(len(cpu_tokens), len(tokens))          # the graph ran warmup + steps tokens, the CPU --cpu-tokens: compare what both have
        n_same = next((i for i, (a, g) in enumerate(zip(cpu_tokens, tokens)) if a != g), n_both)
        # (2) teacher forcing: the CPU's ids are fed through bz_forward_kv one by one on a fresh cache (the prompt row comes from the prefill
        #     above), so EVERY step is comparable whatever happened before it: per-step logit errors, and the argmax wherever the step is fair
        kv2 = runtime.LayeredKvCache(dev, cfg["n_layers"], 1, cfg["n_kv_heads"], args.prompt_len + n_cpu + 1, cfg["max_seq_len"], cfg["head_dim"], kv_dt)
        # (the prompt goes through the single-token decode path too, as the oracle's does: the kernels under test from the first position on; the batched
        #  prompt path -- MFMA GEMMs whose f32 sums differ from the exact sums in the last bit -- is compared with the oracle in tests/ and in "prefill" below)
        for i, t in enumerate(prompt):
            row = lm.forward_with_kv_cache([int(t)], kv2, i)
        gpu_rows = [row.to_numpy().reshape(-1).copy()]
        for i in range(n_cpu - 1):
            gpu_rows.append(lm.forward_with_kv_cache([cpu_tokens[i]], kv2, args.prompt_len + i).to_numpy().reshape(-1).copy())
        l2 = [float(np.linalg.norm(g.astype(np.float64) - c) / np.linalg.norm(c)) for g, c in zip(gpu_rows, cpu_rows)]
        mx = [float(np.abs(g.astype(np.float64) - c).max() / np.abs(c).max()) for g, c in zip(gpu_rows, cpu_rows)]
        fair = [g >= guard for g in gaps]
        same = [int(g.argmax()) == t for g, t in zip(gpu_rows, cpu_tokens)]
        n_cmp = sum(fair)
        n_eq = sum(1 for f, e in zip(fair, same) if f and e)
        out["parity"] = {"greedy_ids_match": bool(n_eq == n_cmp and n_same >= min(fair_prefix, n_both)), "n_compared": n_cmp, "n_equal": n_eq, "n_tokens": n_cpu,
                         "free_running": {"n_identical_prefix": n_same, "fair_prefix": fair_prefix, "n_available": n_both, "cpu": cpu_tokens[:n_cpu], "gpu": tokens[:n_cpu]},
                         "prefill_row_rel_l2": round(float(np.linalg.norm(prefill_row.astype(np.float64) - cpu_rows[0]) / np.linalg.norm(cpu_rows[0])), 9),
                         "teacher_forced": {"rel_l2_max": round(max(l2), 9), "rel_l2_mean": round(float(np.mean(l2)), 9), "max_norm_max": round(max(mx), 9),
                                            "rel_l2_per_step": [round(v, 9) for v in l2], "max_norm_per_step": [round(v, 9) for v in mx],
                                            "top2_gap_per_step": [round(g, 5) for g in gaps], "argmax_equal_per_step": same},
                         "gap_guard": guard,
                         "note": "ids compared on every step whose oracle top-2 gap is >= gap_guard of max|logit| (8 rounding units of the activation dtype: a rounding-level "
                                 "tie below that); logit errors relative to the CPU row (L2) and to its largest magnitude (max-norm); bar: 1e-3 relative L2 (f16 / f32 activations)"}

    # the prompt phase on its own (outside the timed decode region): a 512-token prompt through the batched prefill (matrix-core GEMMs + flash attention),
    # 1 warm-up + 2 timed passes, best of the two; 2 FLOP per linear weight per token against the dense 16-bit MFMA peak
    if args.full and cfg["act_dtype"] in ("f16", "bf16") and cfg["max_seq_len"] >= 520:
        pf_len = 512
        kv2 = runtime.LayeredKvCache(dev, cfg["n_layers"], 1, cfg["n_kv_heads"], pf_len + 8, cfg["max_seq_len"], cfg["head_dim"], kv_dt)
        p2 = synth.prompt_tokens(pf_len, cfg["vocab"], seed=11)
        ptimer = hip_events(C.c_void_p(dev.stream()))
        pf_ms = []
        for _ in range(3):
            dev.synchronize()
            ptimer.start()
            lm.forward_with_kv_cache(p2, kv2, 0)
            ptimer.stop()
            pf_ms.append(ptimer.ms())
        H, I, nq, nkv, hd = cfg["hidden"], cfg["inter"], cfg["n_heads"], cfg["n_kv_heads"], cfg["head_dim"]
        lin = cfg["n_layers"] * (H * nq * hd + 2 * H * nkv * hd + nq * hd * H + 3 * H * I)
        best = min(pf_ms[1:])
        out["prefill"] = {"tokens": pf_len, "ms": round(best, 3), "tokens_per_s": round(pf_len / (best / 1e3), 1), "gemm_tflops": round(2.0 * lin * pf_len / (best / 1e3) / 1e12, 2),
                          "mfma_peak_tflops": 2500.0, "frac_of_mfma_peak": round(2.0 * lin * pf_len / (best / 1e3) / 2.5e15, 4), "runs_ms": [round(v, 3) for v in pf_ms],
                          "note": "whole prompt phase of a 512-token prompt (norms, GEMMs on the matrix cores, RoPE / cache append, flash attention), not part of `value`"}
    # the reference bench's own report (cli/bench.rs:24-33,142-160): prompt lengths 32 / 128 / 512, 1 warm-up + 3 measured generations of `--steps` tokens
    # each through the whole generate loop (prefill, first token, graph capture, one replay per token, event-synchronised token reads); TTFT / total: median
    # over the runs, inter-token latency: percentiles over all gaps of all runs, decode tok/s = (tokens - 1) / (total - TTFT), median.  Not part of `value`.
    if args.full and rank == 0 and not args.no_latency:
        out["latency"] = latency_matrix(runtime, synth, lm, cfg, max(args.steps, 16))
    if rank == 0:
        print(json.dumps(out))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def latency_matrix(runtime, synth, lm, cfg, n_decode, lengths=(32, 128, 512), warm=1, runs=3):
    ex = runtime.Executor(lm)
    rows = []
    for pl in lengths:
        if pl + n_decode + 8 > cfg["max_seq_len"]:
            continue
        prompt = synth.prompt_tokens(pl, cfg["vocab"], seed=100 + pl)
        stats = []
        for r in range(warm + runs):
            ex.generate(prompt, n_decode, use_graph=True)
            if r >= warm:
                stats.append(dict(ex.last_stats))
        med = lambda k: float(np.median([s[k] for s in stats]))   # noqa: E731
        rows.append({"prompt_tokens": pl, "decode_tokens": n_decode, "runs": runs,
                     "ttft_ms": {"median": round(med("ttft_ms"), 3), "samples": [round(s["ttft_ms"], 3) for s in stats]},
                     "decode_tok_per_sec": {"median": round(med("decode_tok_per_s"), 2), "samples": [round(s["decode_tok_per_s"], 2) for s in stats]},
                     "total_ms": {"median": round(med("total_ms"), 3)},
                     "itl_ms": {"p50": round(med("itl_p50_ms"), 4), "p99": round(max(s["itl_p99_ms"] for s in stats), 4), "max": round(max(s["itl_max_ms"] for s in stats), 4)}})
    return rows


def bench_aux(args, rank, local_rank, world, dist):
    """Secondary workloads (BASELINE.json configs[3], [4]): Mamba2-2.7B (state + weights streamed once per token) and
    DeepSeek-V2-Lite (MLA latent cache + MoE: only the routed + shared experts' weights are streamed)."""
    from blazr_amd import replicas, runtime, synth
    mamba = args.preset in synth.MAMBA_PRESETS
    cfg = synth.make_mamba_config(args.preset) if mamba else synth.make_dsv2_config(args.preset)
    need = args.prompt_len + args.warmup + args.steps + 8
    if not mamba and need > cfg["max_seq_len"]:
        cfg["max_seq_len"] = need
    dev = runtime.Device(local_rank)
    t0 = time.time()
    lm = runtime.LoadedModel.from_synth_streamed(dev, cfg)
    load_s = time.time() - t0
    w_bytes, s_bytes = synth.mamba2_bytes_per_token(cfg) if mamba else (synth.dsv2_bytes_per_token(cfg), 0)
    resident, per_token = lm.weight_bytes()
    assert per_token == w_bytes, (per_token, w_bytes)
    prompt = synth.prompt_tokens(args.prompt_len, cfg["vocab"])
    ptimer = hip_events(C.c_void_p(dev.stream()))
    pf_ms = []
    # prompt prefill; --full times it on its own (BASELINE.json configs[4]: "prefill 512 (MFMA) + decode 128"): 3 passes, first pass = warm-up.
    # The decode starts from the state of the last pass either way
    for rep_i in range(3 if args.full else 1):
        if mamba:
            st = runtime.LayeredSsmState(lm)
        else:
            st = lm.new_kv_cache(need)
        dev.synchronize()
        ptimer.start()
        logits = lm.forward_with_ssm_state(prompt, st) if mamba else lm.forward_with_kv_cache(prompt, st, 0)
        ptimer.stop()
        pf_ms.append(ptimer.ms())
    first = int(runtime.logits_to_token(dev, logits, [], []).to_numpy()[0])
    graph = runtime.DecodeGraph(lm, st)
    graph.seed_next_token(first, args.prompt_len)
    for _ in range(args.warmup):
        graph.replay()
    dev.synchronize()
    timer = hip_events(C.c_void_p(dev.stream()))
    if dist is not None:
        dist.barrier()
    dev.synchronize()
    t_host0 = time.perf_counter()
    timer.start()
    for _ in range(args.steps):
        graph.replay()
    timer.stop()
    gpu_ms = timer.ms()
    dev.synchronize()
    host_ms = (time.perf_counter() - t_host0) * 1e3
    if dist is not None:
        dist.barrier()
    n_gpus = max(world, 1)
    tok_s, wall_ms = replicas.aggregate_tokens_per_s(max(gpu_ms, host_ms), args.steps, dist, "cuda" if dist is not None else None)
    n_run = args.warmup + args.steps
    last = graph.read_token(n_run - 1)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, graph, last)
    tokens = run_ids(graph, first, n_run, 7)
    algo = w_bytes + s_bytes
    whole_step_frac = round(algo * (tok_s / n_gpus) / (HBM_PEAK_GBS * 1e9), 4)
    roof = {"bound": "hbm", "peak": HBM_PEAK_GBS, "unit": "GB/s", "whole_step_frac": whole_step_frac}
    if args.full:
        prof = lm.profile_step_ssm(st, last, iters=4) if mamba else lm.profile_step(st, last, args.prompt_len + args.warmup + args.steps, iters=4)
        for p in prof:
            p["avg_us"] = 1e3 * p["total_ms"] / max(p["launches"], 1)
            p["gbs"] = (p["algo_bytes"] / 1e9) / (p["total_ms"] / 1e3) if p["total_ms"] > 0 and p["algo_bytes"] > 0 else None
        dom = max(prof, key=lambda p: p["total_ms"])
        roof = {"bound": "hbm", "kernel": dom["name"], "achieved": round(dom["gbs"], 1) if dom["gbs"] else None, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(dom["gbs"] / HBM_PEAK_GBS, 4) if dom["gbs"] else None, "traffic": None, "whole_step_frac": whole_step_frac}
    out = {"metric": "decode tokens/sec, %s seq=1 on MI355X (and HBM-roofline fraction)" % args.preset, "value": round(tok_s, 2), "unit": "tokens/s",
           "n_gpus": n_gpus, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(wall_ms / args.steps, 5), "higher_is_better": True,
           "scaling": "weak", "vs_baseline": None, "dtype": cfg["act_dtype"], "data": "synthetic",
           "config": {"workload": "%s greedy decode, batch 1, prompt %d, whole step as one hipGraph" % (args.preset, args.prompt_len),
                      "algorithmic_bytes_per_token": algo, "weight_bytes": w_bytes, "state_bytes_rw": s_bytes, "resident_weight_bytes": resident},
           "roofline": roof}
    if args.full:
        out["kernels"] = [{k: (round(v, 3) if isinstance(v, float) else v) for k, v in p.items()} for p in prof]
    out.update({"gpu_ms_events": round(gpu_ms, 3), "host_ms": round(host_ms, 3), "load_s": round(load_s, 1), "tokens_head": tokens[:8]})
    if args.full:
        # the prompt phase: 2 FLOP per active weight per token (embedding row and norms excluded), against the dense 16-bit MFMA peak
        prefill_ms = sorted(pf_ms[1:])[0]
        active_params = w_bytes / {"f16": 2, "bf16": 2, "f32": 4}[cfg["act_dtype"]]
        pf_flops = 2.0 * active_params * args.prompt_len
        out["prefill"] = {"tokens": args.prompt_len, "ms": round(prefill_ms, 3), "tokens_per_s": round(args.prompt_len / (prefill_ms / 1e3), 1),
                          "tflops": round(pf_flops / (prefill_ms / 1e3) / 1e12, 2), "mfma_peak_tflops": 2500.0,
                          "frac_of_mfma_peak": round(pf_flops / (prefill_ms / 1e3) / 2.5e15, 4), "runs_ms": [round(v, 3) for v in pf_ms],
                          "note": "whole prompt phase (GEMMs on the matrix cores + attention / scan + routing), 2 x active weights x tokens FLOP"}
    if args.full and mamba and rank == 0 and world == 1 and not args.no_cpu_baseline:
        # CPU baseline + parity gate for the Mamba2 workload: the oracle on the same synthetic weights (a second, host-resident copy of the model: 2 bytes per
        # weight), the prompt token by token (the step kernels under test from the first position on) and `--cpu-tokens` teacher-forced steps
        from oracle import orc_py
        orc_py.set_threads(max(1, min(args.cpu_threads, os.cpu_count() or 1)))
        model = synth.make_mamba2(cfg)
        om = orc_py.OrcMamba2(model)
        lm2 = runtime.LoadedModel.from_synth(dev, model)
        n_cpu = max(2, min(args.cpu_tokens, 16))
        ost, st2 = om.new_state(), runtime.LayeredSsmState(lm2)
        tp0 = time.perf_counter()
        cpu_rows = [np.asarray(om.forward(prompt, ost)).reshape(-1).copy()]
        t_prefill = time.perf_counter() - tp0
        cpu_tokens = [int(cpu_rows[0].argmax())]
        td0 = time.perf_counter()
        for i in range(n_cpu - 1):
            cpu_rows.append(np.asarray(om.forward([cpu_tokens[-1]], ost)).reshape(-1).copy())
            cpu_tokens.append(int(cpu_rows[-1].argmax()))
        t_decode = time.perf_counter() - td0
        orc_py.lib().orc_ssm_state_free(ost)
        for t in prompt:
            row = lm2.forward_with_ssm_state([int(t)], st2)
        gpu_rows = [row.to_numpy().reshape(-1).copy()]
        for i in range(n_cpu - 1):
            gpu_rows.append(lm2.forward_with_ssm_state([cpu_tokens[i]], st2).to_numpy().reshape(-1).copy())
        l2 = [float(np.linalg.norm(g.astype(np.float64) - c) / np.linalg.norm(c)) for g, c in zip(gpu_rows, cpu_rows)]
        out["cpu_baseline"] = {"value": round((n_cpu - 1) / t_decode, 3), "unit": "tokens/s", "cores": orc_py.lib().orc_num_threads(), "kind": "port",
                               "sample": "oracle/liborc.so (C + OpenMP), same synthetic weights and prompt: %d-token prompt (%.1f s) + %d greedy decode tokens (%.1f s); host has %d "
                                         "logical CPUs" % (args.prompt_len, t_prefill, n_cpu - 1, t_decode, os.cpu_count())}
        out["parity"] = {"greedy_ids_match": bool(all(int(g.argmax()) == t for g, t in zip(gpu_rows, cpu_tokens))), "n_tokens": n_cpu,
                         "teacher_forced": {"rel_l2_max": round(max(l2), 9), "rel_l2_mean": round(float(np.mean(l2)), 9), "rel_l2_per_step": [round(v, 9) for v in l2],
                                            "logits_differing": int(sum(int((g != c.astype(np.float32)).sum()) for g, c in zip(gpu_rows, cpu_rows))), "logits_compared": int(sum(g.size for g in gpu_rows))},
                         "note": "prompt row + teacher-forced decode rows of the step kernels against the CPU oracle (exact sums on both sides: DESIGN 4)"}
        del lm2
    if args.full and rank == 0 and not args.no_latency:
        out["latency"] = latency_matrix(runtime, synth, lm, cfg, max(args.steps, 16))
    if rank == 0:
        print(json.dumps(out))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
