"""Kernel census of the prompt routes (profiles/prompt_census.json): the calls below, made once per (preset, switch setting, library), each process under
`rocprofv3 --kernel-trace --stats`.  Two libraries launch the same work iff every process's kernel name -> call count is equal.

  run:    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o census -- python scripts/prompt_census.py run PRESET
  merge:  python scripts/prompt_census.py merge ROOT_A ROOT_B OUT.json      (ROOT_x/<preset>/<setting>/ holds one process's rocprofv3 output)
"""
import csv
import glob
import json
import os
import sys

PRESETS = ["tiny-awq", "tiny-gptq", "tiny-bf16", "tiny-fp8", "tiny-q4km", "tiny-dsv2", "tiny-dsv2-f32", "tiny-mamba2"]
SETTINGS = {"default": {}, "exact0": {"BZ_EXACT_PREFILL": "0"}, "exact1": {"BZ_EXACT_PREFILL": "1"}, "exact2": {"BZ_EXACT_PREFILL": "2"},
            "no-mfma-prefill": {"BZ_NO_MFMA_PREFILL": "1"}, "no-gguf-prefill": {"BZ_NO_GGUF_PREFILL": "1"}, "no-pf-attn-mfma": {"BZ_NO_PF_ATTN_MFMA": "1"},
            "prefill-min4": {"BZ_PREFILL_MIN": "4"}}


def run(preset):
    from blazr_amd import runtime
    dev = runtime.Device(0)
    _calls(dev, preset)
    dev.synchronize()


def _calls(dev, preset):
    import numpy as np
    from blazr_amd import _lib as L, runtime, synth
    if preset.startswith("tiny-mamba2"):
        lm = runtime.LoadedModel.from_synth(dev, synth.make_mamba2(preset))
        V = lm.c.vocab
        for n in (7, 16, 17, 40):
            st = runtime.LayeredSsmState(lm)
            lm.forward_with_ssm_state(synth.prompt_tokens(n, V, seed=n), st, all_logits=True)
        lm.forward_with_ssm_state(synth.prompt_tokens(9, V, seed=9), st)          # a 9-token chunk behind the 40
        return
    dsv2 = preset.startswith("tiny-dsv2")
    model = synth.make_dsv2(preset) if dsv2 else synth.make_llama(preset, **({"act_order": True} if preset == "tiny-gptq" else {}))
    lm = runtime.LoadedModel.from_synth(dev, model)
    V, bs, per = lm.c.vocab, 16, 4
    for n in (7, 16, 17, 40):                                                   # prompts at position 0, contiguous
        kv = lm.new_kv_cache(64)
        lm.forward_with_kv_cache(synth.prompt_tokens(n, V, seed=n), kv, 0, all_logits=(n == 40))
    lm.forward_with_kv_cache(synth.prompt_tokens(9, V, seed=9), kv, 40)          # a 9-token chunk at position 40
    if not dsv2:
        lm.forward_kv_verify(synth.prompt_tokens(4, V, seed=4), kv, 49)          # one verify of R = 4

    def pool(nseq):
        return runtime.LayeredPagedKvCache(dev, lm.c.n_layers, nseq * per, bs, lm.num_kv_heads(), lm.head_dim(), lm.c.act_dtype)
    for n in (7, 16, 17, 40):                                                   # the same prompts, paged
        pk = pool(1)
        tb = list(range(per))
        lm.forward_with_paged_kv_cache(synth.prompt_tokens(n, V, seed=n), pk, [tb[i // bs] * bs + i % bs for i in range(n)], tb, n, 0, all_logits=(n == 17))
    lm.forward_with_paged_kv_cache(synth.prompt_tokens(9, V, seed=9), pk, [tb[i // bs] * bs + i % bs for i in range(40, 49)], tb, 49, 40)
    if dsv2:
        return
    for nseq in (2, 9):                                                         # eager decode batches; rows 3 + i long
        pk = pool(nseq)
        tables = [[i + nseq * j for j in range(per)] for i in range(nseq)]
        lens = [3 + i for i in range(nseq)]
        for tb, n in zip(tables, lens):
            lm.forward_with_paged_kv_cache(synth.prompt_tokens(n, V, seed=n), pk, [tb[i // bs] * bs + i % bs for i in range(n)], tb, n, 0)
        lens = [n + 1 for n in lens]
        toks = [int(t) for t in synth.prompt_tokens(nseq, V, seed=50 + nseq)]
        lm.forward_paged_batch(toks, pk, [tb[(n - 1) // bs] * bs + (n - 1) % bs for n, tb in zip(lens, tables)], tables, lens)
    try:                                                                        # one batch-graph capture + 2 replays where the model takes it
        g = runtime.BatchDecodeGraph(lm, pk, nseq, per)
    except L.BlazrHipError as e:
        assert e.code == L.E_UNSUPPORTED, e
        print("census: no batch graph for", preset)
        return
    g.seed(toks, [n + 1 for n in lens], tables)
    g.replay(); g.replay()
    g.read_tokens(1)
    np.asarray(g.read_logits())


def _counts(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    assert len(files) == 1, (d, files)
    with open(files[0]) as f:
        return {r["Name"]: int(r["Calls"]) for r in csv.DictReader(f)}


def merge(root_a, root_b, out):
    rec = {"what": "kernel name -> calls of one process per (preset, switch setting): `processes` names its census in `censuses` (many settings launch the same "
                   "work); every one was equal for the parent's library and this commit's", "processes": {}, "censuses": [], "equal": True}

    def census_id(c):
        if c not in rec["censuses"]:
            rec["censuses"].append(c)
        return rec["censuses"].index(c)
    for p in PRESETS:
        for s in SETTINGS:
            da, db = os.path.join(root_a, p, s), os.path.join(root_b, p, s)
            if not (os.path.isdir(da) and os.path.isdir(db)):
                continue
            a, b = _counts(da), _counts(db)
            if a == b:
                rec["processes"]["%s/%s" % (p, s)] = census_id(a)
            else:
                rec["equal"] = False
                rec["processes"]["%s/%s" % (p, s)] = {"parent": census_id(a), "new": census_id(b)}
                print("DIFFERS", p, s, {k: (a.get(k), b.get(k)) for k in set(a) | set(b) if a.get(k) != b.get(k)})
    rec["n_processes"] = len(rec["processes"])
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print("census: %d processes, equal = %s" % (rec["n_processes"], rec["equal"]))
    return 0 if rec["equal"] and rec["n_processes"] else 1


if __name__ == "__main__":
    sys.exit(run(sys.argv[2]) if sys.argv[1] == "run" else merge(*sys.argv[2:5]))
