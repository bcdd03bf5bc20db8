"""Host time of an eager bz_forward_paged_batch step on a tiny model (profiles/prompt_route_bench.json): N = 4 sequences of tiny-awq, 200 steps per run, the wall
clock of each call (the device idle before it), the median per run, `--runs` runs.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.environ.get("BZ_BENCH_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from blazr_amd import runtime, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    dev = runtime.Device(0)
    model = synth.make_llama("tiny-awq")
    cfg = model["config"]
    lm = runtime.LoadedModel.from_synth(dev, model)
    bs, per = 16, 14
    tables = [[i + a.n * j for j in range(per)] for i in range(a.n)]
    medians = []
    for run in range(a.runs + 1):                      # the first run warms up
        pool = runtime.LayeredPagedKvCache(dev, cfg["n_layers"], a.n * per, bs, cfg["n_kv_heads"], cfg["head_dim"], lm.c.act_dtype)
        lens = [3 + i for i in range(a.n)]
        for tb, n in zip(tables, lens):
            lm.forward_with_paged_kv_cache(synth.prompt_tokens(n, cfg["vocab"], seed=n), pool, [tb[i // bs] * bs + i % bs for i in range(n)], tb, n, 0)
        toks = [int(t) for t in synth.prompt_tokens(a.n, cfg["vocab"], seed=5)]
        us = []
        for _ in range(a.steps):
            lens = [n + 1 for n in lens]
            slots = [tb[(n - 1) // bs] * bs + (n - 1) % bs for n, tb in zip(lens, tables)]
            dev.synchronize()
            t0 = time.perf_counter()
            out = lm.forward_paged_batch(toks, pool, slots, tables, lens)
            us.append((time.perf_counter() - t0) * 1e6)
            toks = [int(r.argmax()) for r in out.to_numpy()]
        if run:
            medians.append(round(float(np.median(us)), 2))
    print(json.dumps({"what": "eager forward_paged_batch call, host wall clock", "preset": "tiny-awq", "n": a.n, "steps": a.steps, "median_us_per_run": medians,
                      "median_us": round(float(np.median(medians)), 2)}))


if __name__ == "__main__":
    main()
