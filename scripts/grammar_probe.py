#!/usr/bin/env python3
"""Cost of grammar-constrained decoding on the MI355X (profiles/grammar_mask.json).

  kernels   python scripts/grammar_probe.py kernels --dfa six|hundred|global
            runs the mask kernel `--iters` times at V = 128 256 on the synthetic vocabulary of tests/grammar_ref.py for one DFA (6 states, 100 states, or a 300-state
            table that takes the global-memory path), from the start state and from a state reached after a few tokens, and the greedy logits_to_token kernels
            (argmax partials + final) the same number of times as the yardstick.  Meant to run under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR --`,
            one run per DFA (the kernel's name does not say which DFA it served).
  generate  python scripts/grammar_probe.py generate [--lib PATH]
            eager bz_generate tokens/s on the headline synthetic model (bench.py's shape: llama3-8b-awq, prompt 16, 128 tokens, median of 3), unconstrained and, when the
            library has the grammar entry points, constrained by a 100-state DFA.  --lib: another build of the library (the parent commit's, for the unconstrained figure).
  collect   python scripts/grammar_probe.py collect --six DIR --hundred DIR --global DIR [--generate FILE --generate-parent FILE] --out profiles/grammar_mask.json
            reduces the rocprofv3 kernel_stats.csv files and the generate legs' JSON lines to one file.
"""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

V = 128256
SIX = 'root ::= "yes" | "no"'
HUNDRED = 'root ::= "the quick brown fox jumps over the lazy dog" | "pack my box with five dozen liquor jugs" | "{\\"name\\": \\"Ada\\"}"'      # 1 + 43 + 39 + 15 + ... states


def make_dfa(runtime, kind):
    import numpy as np
    if kind == "six":
        g = runtime.GrammarDfa(SIX)
        assert g.num_states() == 6
    elif kind == "hundred":
        g = runtime.GrammarDfa(HUNDRED)
        assert 95 <= g.num_states() <= 105, g.num_states()
    else:
        rng = np.random.RandomState(11)
        n = 300
        t = np.full((n, 256), -1, dtype=np.int32)
        for b in list(range(32, 127)) + [9, 10]:
            keep = rng.rand(n) < 0.7
            t[keep, b] = rng.randint(0, n, size=int(keep.sum()))
        g = runtime.GrammarDfa(table=t, accepting=(rng.rand(n) < 0.5).astype(np.uint8))
    return g


def cmd_kernels(args):
    import numpy as np
    import grammar_ref as G
    from blazr_amd import runtime
    dev = runtime.Device(0)
    vocab, _ = G.synth_vocab(V, seed=V + 1)
    packed = runtime.pack_vocab(vocab)
    g = make_dfa(runtime, args.dfa)
    dg = g.to_device(dev, packed)
    info = dg.info()
    x = (np.random.RandomState(0).randn(1, V) * 4).astype(np.float32)
    t, _ = g.table()
    # a state a few tokens in (first allowed non-empty single-byte token each time), besides the start state
    mid = 0
    for _ in range(3):
        nxt = [int(t[mid, b]) for b in range(256) if t[mid, b] >= 0]
        if not nxt:
            break
        mid = nxt[0]
    out = dict(dfa=args.dfa, num_states=info["num_states"], lds_table=info["lds_table"], vocab=V, iters=args.iters, states=[0, mid], allowed={})
    for s in (0, mid):
        dg.set_state(s)
        logits = dev.tensor(x)
        for _ in range(args.iters):
            dg.mask_logits(logits)
        got = logits.to_numpy()[0]
        out["allowed"][str(s)] = int(np.isfinite(got).sum())
    logits = dev.tensor(x)
    for _ in range(2 * args.iters):
        runtime.logits_to_token(dev, logits, [], [])          # greedy: argmax partials + final
    dev.synchronize()
    print(json.dumps(out))
    dev.close()


def cmd_generate(args):
    import numpy as np
    from blazr_amd import _lib as L
    if args.lib:
        L.LIB_PATH = args.lib
    import ctypes as C
    probe = C.CDLL(L.LIB_PATH)
    has_grammar = hasattr(probe, "bz_generate_grammar")
    if not has_grammar:            # a build from before this feature: resolve only what it exports
        for k in [k for k in L.SYMBOLS if "grammar" in k]:
            del L.SYMBOLS[k]
    from blazr_amd import runtime, synth
    cfg = synth.make_config("llama3-8b-awq")
    dev = runtime.Device(0)
    lm = runtime.LoadedModel(dev, cfg)
    for i in range(cfg["n_layers"]):
        lm.add_llama_layer(i, synth.llama_layer(cfg, i))
    lm.add_llama_head(*synth.llama_head(cfg))
    lm.finalize()
    ex = runtime.Executor(lm)
    prompt = synth.prompt_tokens(16, cfg["vocab"], seed=26)
    out = dict(lib=os.path.basename(L.LIB_PATH), has_grammar=has_grammar, preset="llama3-8b-awq", tokens=args.tokens, reps=args.reps)

    def run(**kw):
        ex.generate(prompt, 16, **kw)          # warm-up
        rates = []
        for _ in range(args.reps):
            if "grammar" in kw:
                kw["grammar"].reset()
            ids = ex.generate(prompt, args.tokens, **kw)
            assert len(ids) == args.tokens
            rates.append(ex.last_stats["decode_tok_per_s"])
        return dict(median_tok_per_s=sorted(rates)[len(rates) // 2], all=rates)

    out["unconstrained"] = run()
    if has_grammar:
        import grammar_ref as G
        assert cfg["vocab"] == V
        vocab, _ = G.synth_vocab(V, seed=V + 1)
        g = make_dfa(runtime, "hundred")
        out["constrained_100_states"] = run(grammar=g, vocab_bytes=runtime.pack_vocab(vocab))
    print(json.dumps(out))
    dev.close()


def kernel_rows(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    assert files, "no kernel_stats.csv under " + d
    rows = {}
    for r in csv.DictReader(open(files[0])):
        name = r["Name"]
        if "k_grammar_mask" in name or "argmax" in name:
            rows[name.split("(")[0].replace("void ", "")] = dict(calls=int(r["Calls"]), avg_us=float(r["AverageNs"]) / 1e3, min_us=float(r["MinNs"]) / 1e3, max_us=float(r["MaxNs"]) / 1e3)
    return rows


def cmd_collect(args):
    out = dict(what="k_grammar_mask at V = 128256 on the synthetic vocabulary beside the greedy logits_to_token kernels, rocprofv3 --kernel-trace --stats, one run per DFA; "
                    "eager bz_generate tokens/s on llama3-8b-awq (prompt 16, 128 tokens, median of 3)", kernels={})
    for kind, d in (("six", args.six), ("hundred", args.hundred), ("global", getattr(args, "global"))):
        if d:
            out["kernels"][kind] = kernel_rows(d)
            js = os.path.join(d, "probe.json")
            if os.path.exists(js):
                out["kernels"][kind]["run"] = json.loads(open(js).read().strip().split("\n")[-1])
    for key, f in (("generate", args.generate), ("generate_parent", args.generate_parent)):
        if f and os.path.exists(f):
            out[key] = json.loads(open(f).read().strip().split("\n")[-1])
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


ap = argparse.ArgumentParser()
sub = ap.add_subparsers(dest="cmd", required=True)
k = sub.add_parser("kernels"); k.add_argument("--dfa", choices=["six", "hundred", "global"], required=True); k.add_argument("--iters", type=int, default=50)
g = sub.add_parser("generate"); g.add_argument("--lib"); g.add_argument("--tokens", type=int, default=128); g.add_argument("--reps", type=int, default=3)
c = sub.add_parser("collect")
for name in ("--six", "--hundred", "--global", "--generate", "--generate-parent"):
    c.add_argument(name)
c.add_argument("--out", default=os.path.join(ROOT, "profiles", "grammar_mask.json"))
a = ap.parse_args()
{"kernels": cmd_kernels, "generate": cmd_generate, "collect": cmd_collect}[a.cmd](a)
