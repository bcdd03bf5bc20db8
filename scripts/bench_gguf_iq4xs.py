#!/usr/bin/env python3
"""IQ4_XS against Q4_K on the same shapes, in one process: graph-replayed decode of two 2-layer Mistral-7B-width GGUF files whose seven linears per layer
are all Q4_K, or all IQ4_XS (token_embd in the same type, Q6_K output, vocab 8192).  Prints ms per decode step of each and the weight bytes each slim /
fused-MLP launch streams, so that kernel times from a separate `rocprofv3 --kernel-trace --stats` run of this script turn into bytes/s:
  k_gemv_gq_slim<FMT, 1, 0, 2>  norm prologue: q/k/v [6144, 4096] and gate/up [28672, 4096], one launch each per layer     (FMT: 1 = Q4_K, 9 = IQ4_XS)
  k_gemv_gq_slim<FMT, 2, 0, 1>  SiLU prologue: down [4096, 14336]
  k_mlp_gq<FMT, FMT, 0, 16, 4>  with BZ_GGUF_MLP_FUSION=1: gate/up + down in one launch"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import iq4xs_ref as iq   # noqa: E402
import kquant_ref as kq   # noqa: E402
from blazr_amd import runtime, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--formats", default="q4_k,iq4_xs,q4_k,iq4_xs")      # alternating: the spread between the two runs of a format is the noise
args = ap.parse_args()
dev = runtime.Device(0)
out, files = {}, {}
with tempfile.TemporaryDirectory() as td:
    for ftype in sorted(set(args.formats.split(","))):
        model = kq.make_model("q4_k_m", preset="mistral-7b-q4km", n_layers=2, vocab=8192, max_seq_len=512)
        mk = (lambda n, N, K: iq.blocks(n, N, K)) if ftype == "iq4_xs" else (lambda n, N, K: synth.gguf_blocks(n, kq.GGML_Q4_K, N, K))
        model["embed"] = mk("embed", model["embed"]["N"], model["embed"]["K"])
        for i, lay in enumerate(model["layers"]):
            for s in ("q", "k", "v", "o", "gate", "up", "down"):
                lay[s] = mk("l%d.%s" % (i, s), lay[s]["N"], lay[s]["K"])
        path = os.path.join(td, ftype + ".gguf")
        kq.write_gguf(path, model)
        lay = model["layers"][0]
        bpw = (136 if ftype == "iq4_xs" else 144) / 256.0
        launches = dict(qkv=sum(lay[s]["N"] for s in "qkv") * lay["q"]["K"] * bpw, gate_up=2 * lay["gate"]["N"] * lay["gate"]["K"] * bpw,
                        down=lay["down"]["N"] * lay["down"]["K"] * bpw)
        files[ftype] = (path, launches)
        del model
    for run, ftype in enumerate(args.formats.split(",")):
        path, launches = files[ftype]
        lm = runtime.load_model(dev, path)
        ex = runtime.Executor(lm)
        prompt = [int(t) for t in synth.prompt_tokens(16, 8192, seed=26)]
        ex.generate(prompt, 16, use_graph=True)                     # warm-up (capture, first-touch)
        ms = []
        for _ in range(args.reps):
            ids = ex.generate(prompt, args.steps, use_graph=True)
            st = ex.last_stats
            ms.append(st["decode_ms"] / max(st["n_generated"] - 1, 1))
        out["%s#%d" % (ftype, run)] = dict(ms_per_step=sorted(ms)[len(ms) // 2], all_ms=ms, steps=args.steps, n_generated=int(len(ids)),
                                         bytes_per_token=int(lm.weight_bytes()[1]), launch_bytes={k: int(v) for k, v in launches.items()})
        del ex, lm
print(json.dumps(dict(bench="gguf_iq4xs_2l_mistral_width", fused_mlp=bool(os.environ.get("BZ_GGUF_MLP_FUSION")), **out)))
dev.close()
