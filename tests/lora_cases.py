"""Seeded LoRA adapters, a PEFT directory writer and the shared cases of the LoRA tests (test infrastructure; nothing here is used by the product).

An adapter is a dict(rank, alpha, use_rslora, pairs = {"model.layers.L.self_attn.q_proj": (A [r, K], B [N, r])}) with A and B as STORED arrays
(float16 / float32, uint16 = bf16 bits).  Magnitudes are the ones the gap condition was checked for (test_lora.py): A ~ 0.05 N(0,1), B ~ 0.02 N(0,1)."""
import functools
import json
import os

import numpy as np

from blazr_amd import synth
import ckpt_writer
import lora_ref
import npref

TARGETS = ("q", "k", "v", "o", "gate", "up", "down")
MASKS = {"qv": ("q", "v"), "all": TARGETS}
GROUPS = {"qkv": ("q", "k", "v"), "o": ("o",), "gateup": ("gate", "up"), "down": ("down",)}


def dims(cfg):
    """target -> (in_features K, out_features N)"""
    H, I, qn, kn = cfg["hidden"], cfg["inter"], cfg["n_heads"] * cfg["head_dim"], cfg["n_kv_heads"] * cfg["head_dim"]
    return {"q": (H, qn), "k": (H, kn), "v": (H, kn), "o": (qn, H), "gate": (H, I), "up": (H, I), "down": (I, H)}


def store(x, dtype):
    x = np.asarray(x, np.float32)
    if dtype == "f16":
        return x.astype(np.float16)
    if dtype == "bf16":
        return (npref.round_act(x, "bf16").view(np.uint32) >> 16).astype(np.uint16)
    return x


def make_adapter(cfg, targets, rank=8, alpha=16.0, dtype="f16", seed=1, ranks=None, layers=None, use_rslora=False):
    """ranks: optional {target: rank of that target's pair} (the adapter's own `rank` still sets the scaling)"""
    rng = np.random.Generator(np.random.PCG64([0x10A, seed]))
    d = dims(cfg)
    pairs = {}
    for l in (range(cfg["n_layers"]) if layers is None else layers):
        for t in TARGETS:
            if t not in targets:
                continue
            K, N = d[t]
            r = (ranks or {}).get(t, rank)
            A = store(0.05 * rng.standard_normal((r, K)), dtype)
            B = store(0.02 * rng.standard_normal((N, r)), dtype)
            pairs[lora_ref.layer_key(l, t)] = (A, B)
    return dict(rank=rank, alpha=float(alpha), use_rslora=use_rslora, pairs=pairs)


def write_peft_dir(path, adapter, prefix="base_model.", config=True, config_extra=None, drop_b=(), extra=None, config_text=None):
    """adapter_model.safetensors (+ adapter_config.json) as PEFT saves them, tensor names `<prefix><key>.lora_{A,B}.weight`.  config: True = r / lora_alpha /
    use_rslora from the adapter, a dict = exactly that, False = no file; config_text: the file's raw text (an unparseable config); drop_b: keys saved
    without their lora_B; extra: further tensors."""
    os.makedirs(path, exist_ok=True)
    tensors = {}
    for key, (A, B) in adapter["pairs"].items():
        tensors[prefix + key + ".lora_A.weight"] = A
        if key not in drop_b:
            tensors[prefix + key + ".lora_B.weight"] = B
    tensors.update(extra or {})
    ckpt_writer.write_safetensors(os.path.join(path, "adapter_model.safetensors"), tensors)
    if config_text is not None:
        open(os.path.join(path, "adapter_config.json"), "w").write(config_text)
    elif config is not False:
        c = dict(config) if isinstance(config, dict) else dict(peft_type="LORA", r=adapter["rank"], lora_alpha=adapter["alpha"], use_rslora=adapter["use_rslora"],
                                                                 bias="none", target_modules=sorted({k.rsplit(".", 1)[-1] for k in adapter["pairs"]}))
        c.update(config_extra or {})
        json.dump(c, open(os.path.join(path, "adapter_config.json"), "w"))
    return path


# ---- model cases (test_gpu_lora.py; the gap condition of test_lora.py) ----------------------------------------------------------------
MODELS = {
    "tiny-awq": ("tiny-awq", {}),
    "tiny-awq-hd128": ("tiny-awq", dict(head_dim=128)),
    "tiny-bf16": ("tiny-bf16", {}),
    "tiny-q4km": ("tiny-q4km", dict(n_layers=2)),
}
N_TOKENS = 12


@functools.lru_cache(maxsize=None)
def model(key):
    preset, over = MODELS[key]
    return synth.make_llama(preset, **over)


@functools.lru_cache(maxsize=None)
def adapter(key, mask, seed=1):
    return make_adapter(model(key)["config"], MASKS[mask], rank=8, alpha=16.0, dtype="f16", seed=seed)


def tokens(key):
    return [int(t) for t in synth.prompt_tokens(N_TOKENS, model(key)["config"]["vocab"], seed=23)]       # seed 23: every model x mask meets test_lora.py's gap condition (22 leaves tiny-bf16 / q,v at a median of 33 bars)


@functools.lru_cache(maxsize=None)
def reference(key, mask, seed=1):
    """logits [N_TOKENS, vocab] of the rounded reference under the adapter, of the float64 truth under it, and of the base model without it.  Computed once per
    case and shared by every test that needs them; callers must not modify the arrays."""
    m, ad, toks = model(key), adapter(key, mask, seed), tokens(key)
    out = dict(ref=lora_ref.run(lora_ref.LoraLlama(m, ad), toks), truth=lora_ref.run(lora_ref.LoraTruth(m, ad), toks), base=lora_ref.run(npref.NpLlama(m), toks))
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- op cases (test_gpu_lora_ops.py; the stability condition of test_lora.py) --------------------------------------------------------
OP_MODELS = {
    "f16": ("tiny-awq", {}),
    "bf16": ("tiny-bf16", {}),
    "f32": ("tiny-q4km", dict(n_layers=2)),
    "8b": ("llama3-8b-awq-2l", dict(n_layers=1, vocab=2048)),
}


def op_config(mkey):
    preset, over = OP_MODELS[mkey]
    return synth.make_config(preset, **over)


def _slots(rows):
    return [0] if rows == 1 else [(0, -1, 1)[i % 3] for i in range(rows)]


def _op_cases():
    cases = []
    for r in (1, 5, 8, 64, 128):                       # K = N = 256 (o_proj of the tiny models): every rank class, one / a few / more rows than a wave has
        for rows in (1, 3, 17):
            cases.append(dict(id="o-r%d-rows%d" % (r, rows), model="f16", group="o", ranks=[{"o": r}, {"o": r % 7 + 2}], rows=rows, dtype="f16"))
    for act in ("f16", "bf16", "f32"):                 # activation dtype x adapter dtype
        for dt in ("f16", "bf16", "f32"):
            cases.append(dict(id="o-act_%s-w_%s" % (act, dt), model=act, group="o", ranks=[{"o": 8}, {"o": 3}], rows=3, dtype=dt))
    cases.append(dict(id="qkv-ranks-4-9-16", model="f16", group="qkv", ranks=[{"q": 4, "k": 9, "v": 16}, {"q": 2, "k": 1, "v": 7}], rows=3, dtype="f16"))
    cases.append(dict(id="gateup-bf16", model="bf16", group="gateup", ranks=[{"gate": 6, "up": 11}, {"gate": 3, "up": 2}], rows=3, dtype="bf16"))
    cases.append(dict(id="8b-qkv-r16", model="8b", group="qkv", ranks=[{"q": 16, "k": 16, "v": 16}], rows=1, dtype="f16"))      # K 4096 -> N 6144
    cases.append(dict(id="8b-down-r16", model="8b", group="down", ranks=[{"down": 16}], rows=1, dtype="f16"))                      # K 14336 -> N 4096
    for i, c in enumerate(cases):
        c["seed"] = 100 + i
    return cases


OP_CASES = _op_cases()


@functools.lru_cache(maxsize=None)
def op_inputs(case_id):
    """dict(cfg, act, adapters [one per slot, layer 0 only], slots, x [rows, K], base [rows, N], K, N, offs {target: (n_off, N)}) of one op case"""
    c = next(c for c in OP_CASES if c["id"] == case_id)
    cfg = op_config(c["model"])
    act = cfg["act_dtype"]
    d = dims(cfg)
    tg = GROUPS[c["group"]]
    K = d[tg[0]][0]
    offs, off = {}, 0
    for t in tg:
        offs[t] = (off, d[t][1])
        off += d[t][1]
    rng = np.random.Generator(np.random.PCG64([0x10B, c["seed"]]))
    x = npref.round_act(rng.standard_normal((c["rows"], K)).astype(np.float32), act)
    base = npref.round_act(rng.standard_normal((c["rows"], off)).astype(np.float32), act)
    ads = [make_adapter(cfg, tuple(rk), rank=max(rk.values()), alpha=16.0, dtype=c["dtype"], seed=c["seed"] * 8 + i, ranks=rk, layers=[0])
           for i, rk in enumerate(c["ranks"])]
    slots = [s if s < len(ads) else -1 for s in _slots(c["rows"])]
    return dict(case=c, cfg=cfg, act=act, adapters=ads, slots=slots, x=x, base=base, K=K, N=off, offs=offs, targets=tg)


def op_expected(case_id, order="fsum"):
    """y [rows, N] of lora_ref.lora_apply, group member by group member; a row without an adapter keeps R(b) = b"""
    inp = op_inputs(case_id)
    y = inp["base"].copy()
    for row, slot in enumerate(inp["slots"]):
        if slot < 0:
            continue
        ad = inp["adapters"][slot]
        s = lora_ref.scaling(ad["rank"], ad["alpha"], ad["use_rslora"])
        for t in inp["targets"]:
            pair = ad["pairs"].get(lora_ref.layer_key(0, t))
            if pair is None:
                continue
            o, n = inp["offs"][t]
            y[row, o:o + n] = lora_ref.lora_apply(inp["base"][row, o:o + n], inp["x"][row], pair[0], pair[1], s, inp["act"], order)
    return y
