"""Launch census of one decode step (profiles/step_census.json): `[name, launches, algo_bytes]` per kernel label of bz_profile_step / bz_profile_step_ssm, for
every case below at position 8 and -- Llama family -- at position 269 under BZ_SPLIT_MIN=4, taken under the default switches and once per switch of the step's
table (DESIGN.md "Which kernels a decode step launches").  One fresh child process per library and switch setting: the switches are read once per process.
Two libraries launch the same work iff their records are equal entry for entry.

  record:   python scripts/step_census.py record OUT.json [--root CHECKOUT] [--lib LIBRARY.so]
            --root: a built checkout whose package and library the children import (a library that predates this one's symbols needs its own package);
            --lib: BZ_LIB_PATH for the children, with this checkout's package
  compare:  python scripts/step_census.py compare A.json B.json
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SWITCHES = ["BZ_NO_SLIM_QKV", "BZ_NO_GQ_SLIM", "BZ_NO_GQ_MIX", "BZ_NO_ROWS2", "BZ_NO_ATTN_FUSION", "BZ_NO_ATTN_SPLIT", "BZ_NO_ATTN_F32", "BZ_NO_ATTN2_HD64",
            "BZ_NO_MLP_FUSION", "BZ_GGUF_MLP_FUSION", "BZ_DSV2_F32_SUMS", "BZ_NO_MOE_ROUTE_FUSION"]
CUT = dict(n_layers=2, vocab=4096, max_seq_len=512)          # two layers at full width: the smallest models that reach the fused kernels
LLAMA = {"tiny-awq": ("tiny-awq", {}), "tiny-q4km": ("tiny-q4km", {}), "tiny-bf16": ("tiny-bf16", {}), "tiny-gptq-actorder": ("tiny-gptq", dict(act_order=True, bias=True)),
         "llama3-8b-awq-2l-v4096": ("llama3-8b-awq", CUT), "llama3.2-1b-bf16-2l-v4096": ("llama3.2-1b-bf16", CUT), "mistral-7b-q4km-2l-v4096": ("mistral-7b-q4km", CUT)}
OTHER = ["tiny-dsv2", "tiny-dsv2-f32", "tiny-mamba2", "tiny-mamba2-g2"]


def _rows(recs):
    return sorted([r["name"], r["launches"], int(r["algo_bytes"])] for r in recs)


def child(out):
    """every case in this process, under whatever switches its environment holds"""
    sys.path.insert(0, os.path.join(os.environ.get("STEP_CENSUS_ROOT") or os.path.dirname(HERE), "tests"))
    import irregular_cases as ic
    from blazr_amd import runtime, synth
    dev = runtime.Device(0)
    cases = {}
    models = [(n, lambda n=n: ic.make(n)) for n in ic.CASES] + [(n, lambda p=p, o=o: synth.make_llama(p, **dict(dict(max_seq_len=512), **o))) for n, (p, o) in LLAMA.items()]
    for name, make in models:
        lm = runtime.LoadedModel.from_synth(dev, make())
        os.environ.pop("BZ_SPLIT_MIN", None)
        cases[name + "@8"] = _rows(lm.profile_step(lm.new_kv_cache(16), 5, 8, iters=1))
        os.environ["BZ_SPLIT_MIN"] = "4"                     # read per call
        cases[name + "@269/split4"] = _rows(lm.profile_step(lm.new_kv_cache(272), 5, 269, iters=1))
        del lm
    os.environ.pop("BZ_SPLIT_MIN", None)
    for name in OTHER:
        if name.startswith("tiny-mamba2"):
            lm = runtime.LoadedModel.from_synth(dev, synth.make_mamba2(name))
            cases[name + "@8"] = _rows(lm.profile_step_ssm(runtime.LayeredSsmState(lm), 5, iters=1))
        else:
            lm = runtime.LoadedModel.from_synth(dev, synth.make_dsv2(name))
            cases[name + "@8"] = _rows(lm.profile_step(lm.new_kv_cache(16), 5, 8, iters=1))
        del lm
    dev.synchronize()
    with open(out, "w") as f:
        json.dump(cases, f)


def record(out, root=None, lib=None):
    rec = {"what": "[name, launches, algo_bytes] per kernel label of one decode step (bz_profile_step, iters=1): `cases` under the default switches; `switches`: per "
                   "switch (set to 1) the cases whose census differs from the default one -- every other case launched the same", "cases": None, "switches": {}}
    tmp = out + ".child"
    for sw in [None] + SWITCHES:
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES and k != "BZ_SPLIT_MIN"}
        if sw:
            env[sw] = "1"
        if root:
            env["PYTHONPATH"], env["STEP_CENSUS_ROOT"] = os.path.abspath(root), os.path.abspath(root)
        else:
            env["PYTHONPATH"] = os.path.dirname(HERE)
        if lib:
            env["BZ_LIB_PATH"] = os.path.abspath(lib)
        subprocess.run([sys.executable, os.path.abspath(__file__), "child", tmp], env=env, check=True, timeout=600)     # a child that fails ends the record
        with open(tmp) as f:
            cases = json.load(f)
        if sw is None:
            rec["cases"] = cases
        else:
            rec["switches"][sw] = {k: v for k, v in cases.items() if v != rec["cases"][k]}
        print("census:", sw or "default", len(cases), "cases", flush=True)
    os.remove(tmp)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    return 0


def compare(a, b):
    with open(a) as f:
        ra = json.load(f)
    with open(b) as f:
        rb = json.load(f)
    bad = 0
    for sw in ["cases"] + sorted(set(ra.get("switches", {})) | set(rb.get("switches", {}))):
        ca, cb = (ra["cases"], rb["cases"]) if sw == "cases" else (ra["switches"].get(sw), rb["switches"].get(sw))
        if ca != cb:
            bad += 1
            keys = sorted(set(ca or {}) | set(cb or {}))
            print("DIFFERS", sw, {k: ((ca or {}).get(k), (cb or {}).get(k)) for k in keys if (ca or {}).get(k) != (cb or {}).get(k)})
    print("census: %d cases, %d switch records, equal = %s" % (len(ra["cases"]), len(ra.get("switches", {})), not bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "child":
        sys.exit(child(sys.argv[2]))
    if sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    opts = dict(zip(sys.argv[3::2], sys.argv[4::2]))
    sys.exit(record(sys.argv[2], opts.get("--root"), opts.get("--lib")))
