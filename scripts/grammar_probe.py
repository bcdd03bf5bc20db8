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

Per-row grammars (profiles/grammar_rows.json):
  rows      python scripts/grammar_probe.py rows --dfa hundred|global
            k_grammar_mask_rows and k_grammar_advance_rows at V = 128 256 for N = 1, 8, 64, 512 rows (every row constrained, rows alternating between the start state and
            a state a few tokens in), `--iters` launches each, N after N, and k_grammar_mask on one row as the yardstick.  Meant to run under
            `rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/grammar_probe.py rows --dfa KIND > DIR/probe.json`: the kernels' names do not say N, so
            `collect-rows` reads the JSON line this command prints from DIR/probe.json and splits the trace's dispatches, in start order, into the groups it lists.
  batch     python scripts/grammar_probe.py batch [--lib PATH]
            ms per replay of the sampled batched decode graph on llama3-8b-awq at N = 8 and 64 without a grammar and, when the library has the cursor, with every row
            constrained by the 98-state DFA; then bz_generate_grammar tokens/s with that DFA, eager and (use_graph = 1) captured.  --lib: the parent commit's library.
  collect-rows  python scripts/grammar_probe.py collect-rows --hundred DIR --global DIR --batch FILE --batch-parent FILE FILE --out profiles/grammar_rows.json
            (FILE: the stdout of a `batch` run).  Also evaluates the two required comparisons -- this library's grammarless replay within the parent's between-process
            spread, the captured constrained run not slower than the parent's eager one by more than the spread -- writes them under "checks" and exits 1 if one fails.
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


ROWS_N = (1, 8, 64, 512)


def cmd_rows(args):
    import numpy as np
    import grammar_ref as G
    from blazr_amd import runtime
    dev = runtime.Device(0)
    vocab, _ = G.synth_vocab(V, seed=V + 1)
    packed = runtime.pack_vocab(vocab)
    g = make_dfa(runtime, args.dfa)
    dg = g.to_device(dev, packed)
    info = dg.info()
    t, _ = g.table()
    mid = 0
    for _ in range(3):
        nxt = [int(t[mid, b]) for b in range(256) if t[mid, b] >= 0]
        if not nxt:
            break
        mid = nxt[0]
    rng = np.random.RandomState(0)
    out = dict(dfa=args.dfa, num_states=info["num_states"], lds_table=info["lds_table"], vocab=V, iters=args.iters, rows=list(ROWS_N), states=[0, mid], order=[])
    one = dev.tensor((rng.randn(1, V) * 4).astype(np.float32))
    for _ in range(args.iters):
        dg.mask_logits(one)                                    # the yardstick: k_grammar_mask on one row
    out["order"].append(["k_grammar_mask", 1, args.iters])
    for n in ROWS_N:
        cur = runtime.GrammarCursor(dg, n)
        for r in range(1, n, 2):
            cur.set_row(r, mid)
        logits = dev.tensor((rng.randn(n, V) * 4).astype(np.float32))
        toks = dev.tensor(rng.randint(0, V, size=n).astype(np.int64))
        for _ in range(args.iters):
            cur.mask(logits)
        for _ in range(args.iters):
            cur.advance(toks)
        dev.synchronize()
        out["order"] += [["k_grammar_mask_rows", n, args.iters], ["k_grammar_advance_rows", n, args.iters]]
        del cur
    print(json.dumps(out))
    dev.close()


def cmd_batch(args):
    import time
    import numpy as np
    from blazr_amd import _lib as L
    if args.lib:
        L.LIB_PATH = args.lib
    import ctypes as C
    has_cursor = hasattr(C.CDLL(L.LIB_PATH), "bz_grammar_cursor_create")
    if not has_cursor:             # the parent's build: resolve only what it exports
        for k in ("bz_grammar_concat", "bz_grammar_advance_tokens", "bz_decode_batch_graph_capture_grammar", "bz_decode_graph_capture_grammar",
                  "bz_decode_graph_capture_paged_grammar") + tuple(k for k in L.SYMBOLS if "grammar_cursor" in k):
            del L.SYMBOLS[k]
    import grammar_ref as G
    from blazr_amd import runtime, synth
    cfg = synth.make_config("llama3-8b-awq")
    assert cfg["vocab"] == V
    dev = runtime.Device(0)
    lm = runtime.LoadedModel(dev, cfg)
    for i in range(cfg["n_layers"]):
        lm.add_llama_layer(i, synth.llama_layer(cfg, i))
    lm.add_llama_head(*synth.llama_head(cfg))
    lm.finalize()
    vocab, _ = G.synth_vocab(V, seed=V + 1)
    packed = runtime.pack_vocab(vocab)
    g = make_dfa(runtime, "hundred")
    out = dict(lib=os.path.basename(L.LIB_PATH), has_cursor=has_cursor, preset="llama3-8b-awq", replays=args.replays, reps=args.reps, batch={})
    dt = {"f16": L.F16, "bf16": L.BF16, "f32": L.F32}[cfg["act_dtype"]]
    bs, per = 16, 8
    for n in (8, 64):
        res = {}
        for mode in (("plain", "grammar") if has_cursor else ("plain",)):
            pool = runtime.LayeredPagedKvCache(dev, cfg["n_layers"], n * per, bs, cfg["n_kv_heads"], cfg["head_dim"], dt)
            tables = [[i + n * j for j in range(per)] for i in range(n)]
            sampler = runtime.BatchSampler(dev, n, V)
            for r in range(n):
                sampler.set_row(r, history=[1, 2, 3], temperature=0.8, top_k=40, top_p=0.95, seed=1000 + r)
            cur = None
            if mode == "grammar":
                g.reset()
                dg = g.to_device(dev, packed)
                cur = runtime.GrammarCursor(dg, n)
                graph = runtime.BatchDecodeGraph(lm, pool, n, per, sampler=sampler, grammar=cur)
            else:
                graph = runtime.BatchDecodeGraph(lm, pool, n, per, sampler=sampler)
            times = []
            for rep in range(args.reps + 1):                  # the first repetition warms up
                graph.seed([5 + r for r in range(n)], [1] * n, tables)
                if cur is not None:
                    for r in range(n):
                        cur.set_row(r, 0)
                dev.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.replays):
                    graph.replay()
                dev.synchronize()
                times.append((time.perf_counter() - t0) * 1e3 / args.replays)
            res[mode] = dict(ms_per_replay_median=sorted(times[1:])[len(times[1:]) // 2], all=times[1:])
            if cur is not None:
                st, rej = cur.read()
                res[mode]["rejected_bytes"] = int(rej.sum())
            del graph, cur, sampler, pool
        out["batch"][str(n)] = res
    # single stream: bz_generate_grammar with the 98-state DFA, eager and captured
    ex = runtime.Executor(lm)
    prompt = synth.prompt_tokens(16, V, seed=26)

    def run(**kw):
        g.reset()
        ex.generate(prompt, 16, grammar=g, vocab_bytes=packed, **kw)
        rates = []
        for _ in range(args.reps):
            g.reset()
            ids = ex.generate(prompt, args.tokens, grammar=g, vocab_bytes=packed, **kw)
            assert len(ids) == args.tokens
            rates.append(ex.last_stats["decode_tok_per_s"])
        return dict(median_tok_per_s=sorted(rates)[len(rates) // 2], all=rates)
    out["generate_grammar_eager"] = run()
    out["generate_grammar_use_graph"] = run(use_graph=True)       # the parent's library takes the eager loop here
    print(json.dumps(out))
    dev.close()


def trace_groups(d):
    """per-dispatch durations of the grammar kernels in start order, split into the groups cmd_rows launched"""
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel_trace.csv under " + d
    run = json.loads(open(os.path.join(d, "probe.json")).read().strip().split("\n")[-1])
    disp = {}
    for r in csv.DictReader(open(files[0])):
        name = r["Kernel_Name"].split("(")[0].replace("void ", "").split("<")[0]
        if name.startswith("k_grammar_"):
            disp.setdefault(name, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    for v in disp.values():
        v.sort()
    pos, out = {}, dict(run=run, kernels=[])
    for name, n, iters in run["order"]:
        k = pos.get(name, 0)
        ds = [x[1] / 1e3 for x in disp[name][k:k + iters]]
        assert len(ds) == iters, (name, n, len(ds))
        pos[name] = k + iters
        ds = ds[len(ds) // 5:]                                # the first fifth warms the caches
        out["kernels"].append(dict(kernel=name, rows=n, calls=len(ds), avg_us=sum(ds) / len(ds), min_us=min(ds), max_us=max(ds)))
    for name, v in disp.items():
        assert pos.get(name, 0) == len(v), (name, pos.get(name), len(v))
    return out


def cmd_collect_rows(args):
    out = dict(what="k_grammar_mask_rows / k_grammar_advance_rows at V = 128256 on the synthetic vocabulary for N = 1, 8, 64, 512 beside k_grammar_mask on one row "
                    "(rocprofv3 --kernel-trace, no counters in the run, one run per DFA, the first fifth of each group dropped); ms per replay of the sampled batched "
                    "decode graph on llama3-8b-awq with and without per-row grammars, this library and the parent commit's (two processes of the parent for the "
                    "between-process spread); bz_generate_grammar tokens/s, eager and captured (prompt 16, 128 tokens, median of 3)",
               rows_per_workgroup=64, kernels={})
    for kind, d in (("hundred", args.hundred), ("global", getattr(args, "global"))):
        if d:
            out["kernels"][kind] = trace_groups(d)
    if args.batch and os.path.exists(args.batch):
        out["this_library"] = json.loads(open(args.batch).read().strip().split("\n")[-1])
    out["parent_library"] = [json.loads(open(f).read().strip().split("\n")[-1]) for f in (args.batch_parent or []) if os.path.exists(f)]
    checks = {}
    par = out["parent_library"]
    if "this_library" in out and len(par) >= 2:
        for n in ("8", "64"):
            p = [x["batch"][n]["plain"]["ms_per_replay_median"] for x in par]
            spread = max(p) - min(p)
            mine = out["this_library"]["batch"][n]["plain"]["ms_per_replay_median"]
            checks["grammarless_replay_N%s" % n] = dict(this_ms=mine, parent_ms=p, spread_ms=spread, within_spread=bool(mine <= max(p) + spread))
        p = [x["generate_grammar_eager"]["median_tok_per_s"] for x in par]
        spread = max(p) - min(p)
        mine = out["this_library"]["generate_grammar_use_graph"]["median_tok_per_s"]
        checks["single_stream_use_graph"] = dict(this_tok_per_s=mine, parent_eager_tok_per_s=p, spread_tok_per_s=spread, not_slower=bool(mine >= min(p) - spread))
    out["checks"] = checks
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))
    if not all(v.get("within_spread", v.get("not_slower")) for v in checks.values()):
        sys.exit(1)


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
r = sub.add_parser("rows"); r.add_argument("--dfa", choices=["hundred", "global"], required=True); r.add_argument("--iters", type=int, default=50)
b = sub.add_parser("batch"); b.add_argument("--lib"); b.add_argument("--replays", type=int, default=64); b.add_argument("--reps", type=int, default=3)
b.add_argument("--tokens", type=int, default=128)
cr = sub.add_parser("collect-rows")
for name in ("--hundred", "--global", "--batch"):
    cr.add_argument(name)
cr.add_argument("--batch-parent", nargs="*")
cr.add_argument("--out", default=os.path.join(ROOT, "profiles", "grammar_rows.json"))
a = ap.parse_args()
{"kernels": cmd_kernels, "generate": cmd_generate, "collect": cmd_collect, "rows": cmd_rows, "batch": cmd_batch, "collect-rows": cmd_collect_rows}[a.cmd](a)
