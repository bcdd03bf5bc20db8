#!/usr/bin/env python3
"""Graph-replayed decode of 2-layer Mistral-7B-width GGUF files in the Q4_K_M layout and the legacy Q4_0 / Q4_1 / Q5_0 / Q5_1 layouts (block-
quantised token_embd, Q6_K output, vocab 8192), all in one process: ms per decode step of each.  Kernel times come from a separate
`rocprofv3 --kernel-trace --stats` run of this script (gemv_q4_0<slim> ... against gemv_q4_K<slim> / gemv_q5_K<slim> on the same (N, K) shapes)."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import kquant_ref as kq   # noqa: E402
import legacy_quant_ref as lq   # noqa: E402
from blazr_amd import runtime, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--formats", default="q4_k_m,q5_k_m,q4_0,q4_1,q5_0,q5_1")
args = ap.parse_args()
dev = runtime.Device(0)
out = {}
with tempfile.TemporaryDirectory() as td:
    for ftype in args.formats.split(","):
        mk = lq.make_model if ftype in lq.TYPE_OF else kq.make_model
        model = mk(ftype, preset="mistral-7b-q4km", n_layers=2, vocab=8192, max_seq_len=512)
        path = os.path.join(td, ftype + ".gguf")
        kq.write_gguf(path, model)
        del model
        lm = runtime.load_model(dev, path)
        ex = runtime.Executor(lm)
        prompt = [int(t) for t in synth.prompt_tokens(16, 8192, seed=26)]
        ex.generate(prompt, 16, use_graph=True)                     # warm-up (capture, first-touch)
        ms = []
        for _ in range(args.reps):
            ids = ex.generate(prompt, args.steps, use_graph=True)
            st = ex.last_stats
            ms.append(st["decode_ms"] / max(st["n_generated"] - 1, 1))
        res, per_tok = lm.weight_bytes()
        out[ftype] = dict(ms_per_step=sorted(ms)[len(ms) // 2], all_ms=ms, steps=args.steps, n_generated=int(len(ids)), bytes_per_token=int(per_tok))
        del ex, lm
        os.remove(path)
print(json.dumps(dict(bench="gguf_legacy_2l_mistral_width", **out)))
dev.close()
