#!/usr/bin/env python3
"""The request engine (bz_engine_*, bz_engine.hip) against what a caller had before it, in one process, on llama3-8b-awq.

(a) steady state: ms per replay of the engine's captured step at N rows, all rows live and no stop firing, for depth 1 / 2 / 4, beside the plain sampled batch
    graph's replay loop at the same positions.  Per round every variant starts from fresh sequences of the same lengths, runs one untimed step, then `--steps`
    timed ones; the engine's loop reads its records `depth` replays late, the plain loop reads nothing.
(b) an admission: one 128-token prompt into a running batch of 63.  Host time of the step that admits it (and the share spent enqueueing the prompt and the
    row writes), and the wall time a 12-step window gains over the same window without an admission, beside the prompt's own device time.
(c) churn: 256 requests, 16-token prompts, 16 .. 256 new tokens, over 64 rows, against the same requests as four static batches of 64, each run to its longest member.
(d) a shared stem (the prefix cache, bz_engine_config.prefix_cache): 64 requests behind one stem of `--stem` tokens with private tails of 8 .. 24 tokens, 32 new tokens
    each, over 64 rows.  The first request is submitted one step ahead of the others (prompts in flight are not deduplicated).  Run it once with --prefix-cache 0
    and once with --prefix-cache 1, each in a process of its own (--skip a,b,c --out ...): prompt tokens prefilled, host ms per admission, steps to the first
    token, wall time; the run asserts that the prompt tokens prefilled are what the scheduler predicts.  The default stem of 520 tokens is 32 whole blocks and 8
    slots, so every sharer copies 8 slots and the 63 copies of the step are one launch; the launch's time comes from a kernel trace of a run of its own.
    scripts/merge_prefix_bench.py puts the runs' outputs into profiles/prefix_cache.json.
Times are a host clock around work that ends in a device synchronise; medians of `--rounds` rounds, the variants alternating inside a round.  Writes profiles/engine.json (or --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from blazr_amd import _lib as L   # noqa: E402
from blazr_amd import runtime, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--preset", default="llama3-8b-awq")
ap.add_argument("--rows", default="16,64")
ap.add_argument("--depths", default="1,2,4")
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--steps", type=int, default=24)
ap.add_argument("--churn-rounds", type=int, default=3)
ap.add_argument("--churn-requests", type=int, default=256)
ap.add_argument("--skip", default="", help="comma-separated parts to leave out: a,b,c,d")
ap.add_argument("--stem", type=int, default=520)
ap.add_argument("--prefix-cache", type=int, default=0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "engine.json"))
args = ap.parse_args()
skip = set(args.skip.split(","))

dev = runtime.Device(0)
cfg = synth.make_config(args.preset)
V, BS = cfg["vocab"], 16
lm = runtime.LoadedModel.from_synth_streamed(dev, cfg)
KW = dict(temperature=0.7, top_k=40, top_p=0.9, min_p=0.0, repeat_penalty=1.1, frequency_penalty=0.1, presence_penalty=0.05, repeat_last_n=64)
med = statistics.median
result = {"device": dev.name(), "preset": args.preset, "params": KW, "rounds": args.rounds, "steps": args.steps, "steady": [], "admission": None, "churn": None, "shared_stem": None}


def drain(eng):
    while eng.step():
        eng.poll()
    eng.poll()


# ---- (a) -----------------------------------------------------------------------------------------------------------------------------------------------
if "a" not in skip:
    depths = [int(x) for x in args.depths.split(",")]
    for N in [int(x) for x in args.rows.split(",")]:
        lens = [9 + i % 5 for i in range(N)]                          # the sequence length at the first replay (bench_batch_sampler.py's, plus the token fed)
        prompts = [synth.prompt_tokens(n, V, seed=i) for i, n in enumerate(lens)]
        mt = args.steps + 1 + max(depths) + 2                         # no row ends inside the timed window
        per = -(-(max(lens) + mt) // BS)
        pool = runtime.LayeredPagedKvCache(dev, cfg["n_layers"], N * per, BS, cfg["n_kv_heads"], cfg["head_dim"], L.F16)
        tables = [[i + N * j for j in range(per)] for i in range(N)]
        smp = runtime.BatchSampler(dev, N, V)
        plain = runtime.BatchDecodeGraph(lm, pool, N, per, sampler=smp)
        engines = {d: runtime.BatchEngine(lm, N, N * per + N, BS, per * BS, 0, d, True) for d in depths}
        times = {"plain": [], **{"depth%d" % d: [] for d in depths}}

        def round_plain():
            for i, p in enumerate(prompts):
                lm.forward_with_paged_kv_cache(p[:-1], pool, [tables[i][k // BS] * BS + k % BS for k in range(len(p) - 1)], tables[i], len(p) - 1, 0)
                smp.set_row(i, history=p.tolist(), seed=i, **KW)
            plain.seed([int(p[-1]) for p in prompts], lens, tables)
            plain.replay()
            dev.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                plain.replay()
            dev.synchronize()
            return (time.perf_counter() - t0) / args.steps

        def round_engine(eng):
            for i, p in enumerate(prompts):
                eng.submit(p, mt, seed=i, **KW)
            eng.step()                                                # admissions, prompts, replay 0
            dev.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                eng.step()
            dev.synchronize()
            dt = (time.perf_counter() - t0) / args.steps
            drain(eng)
            return dt

        for rnd in range(args.rounds + 1):                            # round 0 warms up
            t = {"plain": round_plain()}
            for d in depths:
                t["depth%d" % d] = round_engine(engines[d])
            if rnd:
                for k, v in t.items():
                    times[k].append(v)
        row = {"N": N, "plain_sampled_graph_ms": round(med(times["plain"]) * 1e3, 4), "plain_min_ms": round(min(times["plain"]) * 1e3, 4)}
        for d in depths:
            k = "depth%d" % d
            row["engine_%s_ms" % k] = round(med(times[k]) * 1e3, 4)
            row["engine_%s_min_ms" % k] = round(min(times[k]) * 1e3, 4)
            row["engine_%s_excess_ms" % k] = round((med(times[k]) - med(times["plain"])) * 1e3, 4)
        result["steady"].append(row)
        print(json.dumps(row), flush=True)
        del plain, engines, smp, pool

# ---- (b) -----------------------------------------------------------------------------------------------------------------------------------------------
if "b" not in skip:
    N, W, rounds = 64, 12, args.rounds
    per = 512 // BS
    eng = runtime.BatchEngine(lm, N, N * per + N, BS, 512, 0, 2, True)
    for i in range(N - 1):
        eng.submit(synth.prompt_tokens(9 + i % 5, V, seed=i), 512 - 16, seed=i, **KW)
    for _ in range(4):
        eng.step()
    eng.poll()
    newcomer = synth.prompt_tokens(128, V, seed=999)
    # the prompt alone: its device time through the existing call
    ppool = runtime.LayeredPagedKvCache(dev, cfg["n_layers"], 8, BS, cfg["n_kv_heads"], cfg["head_dim"], L.F16)
    ptab = list(range(8))
    alone = []
    for _ in range(rounds + 1):
        dev.synchronize()
        t0 = time.perf_counter()
        lm.forward_with_paged_kv_cache(newcomer[:-1], ppool, list(range(127)), ptab, 127, 0)
        dev.synchronize()
        alone.append(time.perf_counter() - t0)

    def window(admit):
        dev.synchronize()
        host = enq = None
        t0 = time.perf_counter()
        for k in range(W):
            if admit and k == 2:
                eng.submit(newcomer, 4, seed=7, **KW)
                e0 = eng.stats()["admit_host_ms"]
                h0 = time.perf_counter()
                eng.step()
                host = time.perf_counter() - h0
                enq = eng.stats()["admit_host_ms"] - e0
            else:
                eng.step()
        dev.synchronize()
        dt = time.perf_counter() - t0
        eng.poll()
        return dt, host, enq

    w0, w1, hs, es, plain_step = [], [], [], [], []
    for rnd in range(rounds + 1):
        a, _, _ = window(False)
        b, h, e = window(True)
        if rnd:
            w0.append(a); w1.append(b); hs.append(h); es.append(e * 1e-3); plain_step.append(a / W)
    result["admission"] = {"rows": N, "running": N - 1, "prompt_tokens": 128, "window_steps": W, "depth": 2,
                           "step_ms": round(med(plain_step) * 1e3, 4),
                           "admitting_step_host_ms": round(med(hs) * 1e3, 4), "of_which_enqueue_ms": round(med(es) * 1e3, 4),
                           "window_without_ms": round(med(w0) * 1e3, 4), "window_with_ms": round(med(w1) * 1e3, 4),
                           "window_excess_ms": round((med(w1) - med(w0)) * 1e3, 4), "prompt_alone_ms": round(med(alone[1:]) * 1e3, 4),
                           "device_idle_ms": round((med(w1) - med(w0) - med(alone[1:])) * 1e3, 4)}
    print(json.dumps(result["admission"]), flush=True)
    del eng, ppool

# ---- (c) -----------------------------------------------------------------------------------------------------------------------------------------------
if "c" not in skip:
    N, R = 64, args.churn_requests
    rng = np.random.default_rng(3)
    news = [int(x) for x in rng.integers(16, 257, size=R)]
    prompts = [synth.prompt_tokens(16, V, seed=2000 + i) for i in range(R)]
    per = -(-(16 + 256) // BS)
    te, ts = [], []
    eng = runtime.BatchEngine(lm, N, N * per + N, BS, per * BS, 0, 4, True)
    pool = runtime.LayeredPagedKvCache(dev, cfg["n_layers"], N * per, BS, cfg["n_kv_heads"], cfg["head_dim"], L.F16)
    tables = [[i + N * j for j in range(per)] for i in range(N)]
    smp = runtime.BatchSampler(dev, N, V)
    static = runtime.BatchDecodeGraph(lm, pool, N, per, sampler=smp)
    replays = 0
    for rnd in range(args.churn_rounds + 1):
        dev.synchronize()
        t0 = time.perf_counter()
        r0 = eng.stats()["replays"]
        for i in range(R):
            eng.submit(prompts[i], news[i], seed=i, **KW)
        drain(eng)
        dev.synchronize()
        dt_e = time.perf_counter() - t0
        replays = eng.stats()["replays"] - r0
        t0 = time.perf_counter()
        static_replays = 0
        for b0 in range(0, R, N):
            idx = list(range(b0, min(R, b0 + N)))
            for r, i in enumerate(idx):
                p = prompts[i]
                lm.forward_with_paged_kv_cache(p[:-1], pool, [tables[r][k // BS] * BS + k % BS for k in range(len(p) - 1)], tables[r], len(p) - 1, 0)
                smp.set_row(r, history=p.tolist(), seed=i, **KW)
            pad = [prompts[idx[r % len(idx)]] for r in range(N)]
            static.seed([int(p[-1]) for p in pad], [len(p) for p in pad], tables)
            longest = max(news[i] for i in idx)
            for s in range(longest):
                static.replay()
            static.read_tokens(longest - 1)                           # the batch's last tokens reach the host
            static_replays += longest
        dev.synchronize()
        dt_s = time.perf_counter() - t0
        if rnd:
            te.append(dt_e); ts.append(dt_s)
    total = sum(news)
    result["churn"] = {"requests": R, "rows": N, "depth": 4, "generated_tokens": total, "engine_s": round(med(te), 4), "engine_replays": replays,
                       "engine_tokens_per_s": round(total / med(te), 1), "static_s": round(med(ts), 4), "static_replays": static_replays,
                       "static_tokens_per_s": round(total / med(ts), 1), "ratio_engine_over_static": round(med(ts) / med(te), 3)}
    print(json.dumps(result["churn"]), flush=True)

# ---- (d) -----------------------------------------------------------------------------------------------------------------------------------------------
if "d" not in skip:
    N, R, NEW = 64, 64, 32
    on = bool(args.prefix_cache)
    stem = synth.prompt_tokens(args.stem, V, seed=3000)
    tails = [synth.prompt_tokens(9 + i % 17, V, seed=3001 + i) for i in range(R)]
    for i in range(1, R):
        if tails[i][0] == tails[0][0]:                                # the common part ends with the stem
            tails[i][0] = (tails[i][0] + 1) % V
    prompts = [np.concatenate([stem, t]) for t in tails]
    per = -(-(args.stem + 25 + NEW) // BS)
    eng = runtime.BatchEngine(lm, N, N * per + N, BS, per * BS, 0, 4, True, **(dict(prefix_cache=True) if on else {}))
    walls, first_steps, admit, prefilled, last = [], [], [], [], None
    for rnd in range(args.rounds + 1):
        if on:
            eng.prefix_flush()
        s0 = eng.stats()
        dev.synchronize()
        t0 = time.perf_counter()
        ids = [eng.submit(prompts[0], NEW, seed=0, **KW)]
        seen, step, busy = {}, 0, True
        while busy:
            if step == 1:
                ids += [eng.submit(prompts[i], NEW, seed=i, **KW) for i in range(1, R)]
            busy = eng.step() or step == 0
            for rid, tok, idx, fin, rep_ in eng.poll():
                seen.setdefault(rid, step)
            step += 1
        dev.synchronize()
        dt = time.perf_counter() - t0
        s1 = eng.stats()
        prefilled.append(s1["prompt_tokens"] - s0["prompt_tokens"])
        if rnd:
            walls.append(dt)
            first_steps.append(med([seen[i] - (0 if k == 0 else 1) for k, i in enumerate(ids)]))
            admit.append((s1["admit_host_ms"] - s0["admit_host_ms"]) / R)
        if on:
            p1 = eng.prefix_stats()
            last = {k: p1[k] for k in ("hits", "misses", "cached_tokens", "copied_blocks", "copy_launches", "evictions")}
    # what the scheduler predicts: with the cache off everything; with it on the donor prefills everything and every other request what follows the stem
    total = int(sum(len(p) - 1 for p in prompts))
    predicted = int(len(prompts[0]) - 1 + sum(len(p) - 1 - args.stem for p in prompts[1:])) if on else total
    assert all(x == predicted for x in prefilled), (prefilled, predicted)
    row = {"rows": N, "requests": R, "stem": args.stem, "new_tokens": NEW, "prefix_cache": int(on), "prompt_tokens_total": total, "prompt_tokens_predicted": predicted,
           "prompt_tokens_prefilled_per_round": int(prefilled[-1]), "admit_host_ms_per_admission": round(med(admit), 4), "median_steps_to_first_token": med(first_steps),
           "wall_s": round(med(walls), 4), "wall_s_rounds": [round(w, 4) for w in walls]}
    if on:
        row["prefix_stats_cumulative"] = last
    result["shared_stem"] = row
    print(json.dumps(row), flush=True)
    del eng

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print(json.dumps(result))
