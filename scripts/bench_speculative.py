#!/usr/bin/env python3
"""What speculative decoding costs on the headline shape: target llama3-8b-awq, draft llama3.2-1b-bf16 (synthetic weights, vocabularies equal).
For R in {2, 4, 6, 8, 9, 16}: device time of one verify pass of R rows (k = R - 1 proposals) at a context of ~144 tokens, and of one draft step, both from the
HIP events bz_generate_speculative records around the two phases.  Synthetic weights accept almost nothing, so every iteration verifies k + 1 rows and no
end-to-end tok/s is claimed.  From these and the target's plain decode ms/step (--decode-ms: as bench.py reports it) the break-even acceptance per k:
an iteration costs k * draft + verify(k + 1) and must emit more than that many plain steps' worth of tokens.
The multi-row lm_head's own kernel time is read from a kernel trace of this script (the launch is named k_spec_head):
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_speculative.py --rows 8
Writes one JSON document to stdout (or --out).  No test asserts any of these times."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from blazr_amd import runtime, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--target", default="llama3-8b-awq")
ap.add_argument("--draft", default="llama3.2-1b-bf16")
ap.add_argument("--rows", default="2,4,6,8,9,16")
ap.add_argument("--context", type=int, default=144)
ap.add_argument("--iterations", type=int, default=24)
ap.add_argument("--decode-ms", type=float, default=None, help="the target's plain decode ms/step as bench.py reports it (1000 / tok_per_s)")
ap.add_argument("--layers", type=int, default=0)
ap.add_argument("--out")
args = ap.parse_args()
rows = [int(x) for x in args.rows.split(",")]
dev = runtime.Device(0)
tcfg = synth.make_config(args.target, **(dict(n_layers=args.layers) if args.layers else {}))
dcfg = synth.make_config(args.draft, vocab=tcfg["vocab"], **(dict(n_layers=args.layers) if args.layers else {}))
tm = runtime.LoadedModel.from_synth_streamed(dev, tcfg)
dm = runtime.LoadedModel.from_synth_streamed(dev, dcfg)
prompt = [int(t) for t in synth.prompt_tokens(args.context, tcfg["vocab"], seed=7)]
res = dict(command=" ".join(["python"] + sys.argv), target=args.target, draft=args.draft, context=args.context, device=dev.name(), rows=[])
plain = runtime.Executor(tm)
plain.generate(prompt, 8, temperature=0.0, repeat_penalty=1.0)
want = [int(t) for t in plain.generate(prompt, args.iterations, temperature=0.0, repeat_penalty=1.0)]
res["plain_eager_decode_ms_per_step"] = round(1e3 / plain.last_stats["decode_tok_per_s"], 4) if plain.last_stats["decode_tok_per_s"] else None
decode_ms = args.decode_ms or res["plain_eager_decode_ms_per_step"]
res["decode_ms_per_step_used"] = decode_ms
res["decode_ms_source"] = "--decode-ms (bench.py)" if args.decode_ms else "eager bz_generate in this process (bench.py's graph-mode figure is lower: pass it with --decode-ms)"
for R in rows:
    k = R - 1
    sx = runtime.SpeculativeExecutor(tm, dm, num_speculative_tokens=k)
    sx.generate(prompt, 2 * R, temperature=0.0, repeat_penalty=1.0)          # warm-up (workspaces)
    got = [int(t) for t in sx.generate(prompt, args.iterations, temperature=0.0, repeat_penalty=1.0)]
    ss = sx.last_spec_stats

    verify_ms = ss["verify_ms"] / max(1, ss["iterations"])
    draft_ms = ss["draft_ms"] / max(1, ss["drafted_tokens"])
    cost = k * draft_ms + verify_ms
    need = cost / decode_ms                                                   # tokens an iteration must emit to match plain decoding
    row = dict(R=R, k=k, same_tokens_as_plain=got == want[:len(got)], iterations=ss["iterations"], accepted=ss["accepted_tokens"], verify_path=ss["verify_path"],
               verify_ms=round(verify_ms, 4), draft_step_ms=round(draft_ms, 4), iteration_ms=round(cost, 4), tokens_per_iteration_to_break_even=round(need, 3),
               break_even_accepted_per_iteration=round(max(0.0, need - 1.0), 3), break_even_acceptance_rate=round(max(0.0, need - 1.0) / k, 3), reachable=need <= k + 1)
    print(json.dumps(row), file=sys.stderr, flush=True)
    res["rows"].append(row)
    del sx
txt = json.dumps(res, indent=1)
if args.out:
    open(args.out, "w").write(txt + "\n")
print(txt)
