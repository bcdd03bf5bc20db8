"""FP8 (E4M3) weight checkpoints: the cases tests/test_fp8_weights.py and tests/test_gpu_fp8_weights.py share, the exact oracle restatement of an FP8 model
and a minimal SafeTensors writer that can emit F8_E4M3 (tests/ckpt_writer.py knows the 16- and 32-bit dtypes only).  The numpy side of the encoding is
tests/kv_fp8_ref.py (TABLE / quant).  Data only; nothing here touches the GPU."""
import json
import os
import struct

import numpy as np

import ckpt_writer
import kv_fp8_ref
from blazr_amd import synth

TABLE = np.asarray(kv_fp8_ref.TABLE, dtype=np.float32)     # f32 value of every code (NaN at 0x7F / 0xFF)
FINITE_CODES = np.array([c for c in range(256) if (c & 0x7F) != 0x7F], dtype=np.uint8)

# (N, K) of the op-level tests and what each reaches
GEMV_SHAPES = [
    (64, 64),        # one tile, one chunk
    (192, 704),      # K = 11 x 64: a ragged last chunk at any per-wave chunk of 128 / 256 / 512
    (1408, 768),     # the irregular fixtures' widths
    (256, 4096),     # the row-major (256, 4096) case, 1 MiB; the split-K form (bzk_f8_choose_sk gives 4)
    (64, 14336),     # the 8B down-projection's K; split-K over 14 slices
]
GEMM_SHAPES = [(192, 704), (1408, 768), (256, 4096)]
GEMM_ROWS = [9, 17, 64, 130]

# whole-model cases: name -> (preset, overrides)
MODELS = {
    "tiny-fp8-channel-bf16": ("tiny-fp8", dict()),
    "tiny-fp8-tensor-bf16": ("tiny-fp8", dict(fp8_strategy="tensor")),
    "tiny-fp8-channel-f16": ("tiny-fp8", dict(act_dtype="f16")),
    "tiny-fp8-tensor-f16": ("tiny-fp8", dict(act_dtype="f16", fp8_strategy="tensor")),
    # the bf16-g2-w768 dims of tests/irregular_cases.py with FP8 projections
    "fp8-g2-w768": ("tiny-fp8", dict(hidden=768, n_heads=6, n_kv_heads=3, head_dim=128, inter=1408, vocab=1003, max_seq_len=512)),
}


def make(name):
    preset, over = MODELS[name]
    return synth.make_llama(preset, **over)


def choose_sk(N, K):
    """the library's split rule for an FP8 [N, K] GEMV (bzk_f8_choose_sk), restated"""
    rbs, KC = (N + 15) // 16, (K + 255) // 256
    if rbs >= 256 or KC < 8:
        return 1
    sk = min((512 + rbs - 1) // rbs, KC // 4)
    if sk < 2:
        return 1
    kcs = (KC + sk - 1) // sk
    return (KC + kcs - 1) // kcs


def pow2_scales(n, seed, lo=-12, hi=-6):
    return np.exp2(np.random.default_rng(seed).integers(lo, hi + 1, size=n)).astype(np.float32)


def bf16_scales(n, seed):
    """general scales with 8 significant bits (bf16-representable), around 2^-9"""
    r = np.random.default_rng(seed)
    return synth._repr((r.uniform(0.5, 2.0, size=n) * 2.0 ** -9).astype(np.float32), "bf16")


def random_codes(N, K, seed):
    """finite codes whose values look like quantised weights: normal values over the whole E4M3 range, encoded"""
    r = np.random.default_rng(seed)
    return synth.e4m3_encode((r.standard_normal((N, K)) * 120.0).astype(np.float32))


def weight_f64(spec):
    """float64 W = s . e4m3(q) of an FP8 spec (exact: 8 + 4 significant bits)"""
    s = np.asarray(spec["scale"], dtype=np.float64).reshape(-1)
    w = TABLE[np.asarray(spec["weight"], dtype=np.uint8)].astype(np.float64)
    return w * (s[:, None] if s.size > 1 else s[0])


def restate_linear(spec):
    if spec["kind"] != "fp8":
        return spec
    w64 = weight_f64(spec)
    w32 = w64.astype(np.float32)
    assert np.array_equal(w32.astype(np.float64), w64), "scale . e4m3 must be exact in f32 (scales with at most 8 significant bits)"
    bias = None if spec.get("bias") is None else np.asarray(spec["bias"], dtype=np.float32)
    return dict(kind="dense", N=spec["N"], K=spec["K"], weight=w32, bias=bias)


def restate_f32(model):
    """the same model with every FP8 linear as a dense f32 linear holding s . e4m3(q): what the CPU oracle runs (ORC_LIN_DENSE, ORC_F32)"""
    out = dict(model)
    out["layers"] = [{k: (restate_linear(v) if isinstance(v, dict) else v) for k, v in lay.items()} for lay in model["layers"]]
    out["lm_head"] = restate_linear(model["lm_head"])
    return out


# ---- SafeTensors with F8_E4M3 --------------------------------------------------------------------------------------------------------
ST_DT = dict(ckpt_writer.ST_DT)


class F8(object):
    """marks a uint8 array as F8_E4M3 for write_safetensors"""
    def __init__(self, a):
        self.a = np.ascontiguousarray(a, dtype=np.uint8)


def write_safetensors(path, tensors):
    header, off, blobs = {}, 0, []
    for name, a in tensors.items():
        if isinstance(a, F8):
            dt, a = "F8_E4M3", a.a
        else:
            a = np.asarray(a)
            dt = ST_DT[a.dtype]
        b = np.ascontiguousarray(a).tobytes()
        header[name] = {"dtype": dt, "shape": list(a.shape), "data_offsets": [off, off + len(b)]}
        off += len(b)
        blobs.append(b)
    header["__metadata__"] = {"format": "pt"}
    h = json.dumps(header).encode()
    h += b" " * ((8 - len(h) % 8) % 8)
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(h)))
        f.write(h)
        for b in blobs:
            f.write(b)


def quantization_config(form):
    if form == "compressed-tensors":
        return dict(quant_method="compressed-tensors", format="float-quantized", ignore=["lm_head"], quantization_status="compressed",
                    config_groups=dict(group_0=dict(targets=["Linear"],
                                                    weights=dict(num_bits=8, type="float", strategy="channel", symmetric=True, dynamic=False),
                                                    input_activations=dict(num_bits=8, type="float", strategy="token", symmetric=True, dynamic=True))))
    if form == "fp8":
        return dict(quant_method="fp8", activation_scheme="static", ignored_layers=["lm_head"])
    raise ValueError(form)


def write_fp8_checkpoint(dirpath, model, form, with_quant_config=True):
    """form "compressed-tensors": channel scales as BF16 [N,1]; form "fp8": per-tensor scales as F32 [].  Both carry an input_scale per linear (ignored by a
    weight-only run); every other tensor is written as tests/ckpt_writer.py writes it."""
    os.makedirs(dirpath, exist_ok=True)
    t = {}
    plain = dict(model)
    fp8 = {}
    layers = []
    for i, lay in enumerate(model["layers"]):
        keep = {}
        for k, v in lay.items():
            if isinstance(v, dict) and v["kind"] == "fp8":
                fp8["model.layers.%d.%s" % (i, dict(q="self_attn.q_proj", k="self_attn.k_proj", v="self_attn.v_proj", o="self_attn.o_proj", gate="mlp.gate_proj",
                                                     up="mlp.up_proj", down="mlp.down_proj")[k])] = v
                keep[k] = dict(kind="dense", N=v["N"], K=v["K"], weight=np.zeros((1, 1), dtype=np.float32))   # placeholder, dropped below
            else:
                keep[k] = v
        layers.append(keep)
    plain["layers"] = layers
    for name, a in ckpt_writer.hf_tensors(plain).items():
        if name[:-len(".weight")] in fp8:
            continue
        t[name] = a
    for base, spec in fp8.items():
        t[base + ".weight"] = F8(spec["weight"])
        s = np.asarray(spec["scale"], dtype=np.float32).reshape(-1)
        if form == "compressed-tensors":
            assert s.size == spec["N"]
            t[base + ".weight_scale"] = synth.f32_to_bf16_bits(s).reshape(spec["N"], 1)
        else:
            assert s.size == 1
            t[base + ".weight_scale"] = s.reshape(())
        t[base + ".input_scale"] = np.float32(0.0123).reshape(())
        if spec.get("bias") is not None:
            t[base + ".bias"] = np.asarray(spec["bias"], dtype=np.float32)
    j = ckpt_writer.hf_config(model["config"])
    if with_quant_config:
        j["quantization_config"] = quantization_config(form)
    json.dump(j, open(os.path.join(dirpath, "config.json"), "w"))
    write_safetensors(os.path.join(dirpath, "model.safetensors"), t)
