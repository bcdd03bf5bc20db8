"""MXFP4 weight checkpoints (E2M1 codes in blocks of 32, one E8M0 scale per block): the cases tests/test_mxfp4_weights.py and tests/test_gpu_mxfp4_weights.py
share -- the code tables, an independent restatement of the quantiser, the exact oracle restatement of an MXFP4 model and a Quark-style SafeTensors writer on
tests/ckpt_writer.py.  ASSUMPTION (also in include/blazr_hip.h and DESIGN 4): the nibble order (low nibble = the even element) and the Quark field names are
what this writer and the loader define; neither could be checked against a published file.  Data only; nothing here touches the GPU."""
import json
import os
import struct

import numpy as np

import ckpt_writer
from blazr_amd import synth

E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0], dtype=np.float32)   # code -> value; bit 3 is the sign
E8M0 = np.array([2.0 ** (c - 127) for c in range(255)] + [np.nan], dtype=np.float64)                                           # code -> 2^(c - 127); 255 is NaN
MAX_SCALE_CODE = 252       # 6 . 2^(c - 127) is a finite f32 up to here

# (N, K) of the op-level tests and what each reaches in k_gemv_mx4 (tiles of four rows x 512 k)
GEMV_SHAPES = [
    (64, 64),        # the smallest linear: one tile per row group, 7/8 of it padding
    (192, 704),      # K = 11 x 64: a second tile of 192 valid k
    (1408, 768),     # the irregular fixtures' widths
    (256, 4096),     # eight full tiles per row
    (64, 14336),     # the 8B down-projection's K: 28 tiles, 70 KiB of activations in LDS
]
GEMM_SHAPES = [(192, 704), (1408, 768), (256, 4096)]
GEMM_ROWS = [9, 17, 64, 130]

# whole-model cases: name -> (preset, overrides)
MODELS = {
    "tiny-mxfp4-bf16": ("tiny-mxfp4", dict()),
    "tiny-mxfp4-f16": ("tiny-mxfp4", dict(act_dtype="f16")),
    # the dims of fp8-g2-w768 (tests/fp8_cases.py) with MXFP4 projections
    "mxfp4-g2-w768": ("tiny-mxfp4", dict(hidden=768, n_heads=6, n_kv_heads=3, head_dim=128, inter=1408, vocab=1003, max_seq_len=512)),
}


def make(name):
    preset, over = MODELS[name]
    return synth.make_llama(preset, **over)


def unpack(packed):
    """bytes [N, K/2] -> codes [N, K]: the low nibble of byte j is element 2 j"""
    p = np.asarray(packed, dtype=np.uint8)
    return np.stack([p & 15, p >> 4], axis=-1).reshape(p.shape[0], -1)


def pack(codes):
    c = np.asarray(codes, dtype=np.uint8).reshape(codes.shape[0], -1, 2)
    return (c[:, :, 0] | (c[:, :, 1] << 4)).astype(np.uint8)


def spec_of(codes, scale, bias=None):
    N, K = codes.shape
    return dict(kind="mxfp4", N=N, K=K, weight=pack(codes), scale=np.asarray(scale, dtype=np.uint8).reshape(N, K // 32), bias=bias)


def weight_f64(spec):
    """float64 W = 2^(s - 127) . e2m1(q) of an MXFP4 spec (exact: a power of two times a two-bit significand)"""
    w = E2M1[unpack(spec["weight"])].astype(np.float64)
    s = E8M0[np.asarray(spec["scale"], dtype=np.uint8)]
    return w * np.repeat(s, 32, axis=1)


def encode_ref(w):
    """the OCP MX quantiser restated without synth's tables: per block of 32 the shared exponent floor(log2(max|w|)) - 2 (clamped to the codes 0..252, code
    127 for an all-zero block), then the nearest E2M1 value by exhaustive distance, ties to the code with the even significand, saturated at 6"""
    w = np.asarray(w, dtype=np.float64)
    N, K = w.shape
    codes, scales = np.zeros((N, K), np.uint8), np.zeros((N, K // 32), np.uint8)
    mags = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    for n in range(N):
        for b in range(K // 32):
            blk = w[n, 32 * b:32 * b + 32]
            amax = float(np.abs(blk).max())
            c = 127 if amax == 0.0 else int(min(max(int(np.floor(np.log2(amax))) - 2 + 127, 0), MAX_SCALE_CODE))
            scales[n, b] = c
            for i, v in enumerate(blk):
                a = min(abs(float(v)) / 2.0 ** (c - 127), 6.0)
                best = min(range(8), key=lambda m: (abs(a - mags[m]), m & 1))
                codes[n, 32 * b + i] = best | (8 if np.signbit(v) else 0)
    return codes, scales


def quantised(N, K, seed, std=0.02):
    """e2m1_encode of N(0, std) weights, as a spec"""
    w = (np.random.default_rng(seed).standard_normal((N, K)) * std).astype(np.float32)
    codes, scale = synth.e2m1_encode(w)
    return spec_of(codes, scale)


def restate_linear(spec):
    if spec["kind"] != "mxfp4":
        return spec
    w64 = weight_f64(spec)
    with np.errstate(over="ignore"):          # (a code above 252 overflows here and fails the assertion below)
        w32 = w64.astype(np.float32)
    assert np.array_equal(w32.astype(np.float64), w64), "2^(s - 127) . e2m1 must be exact in f32 (scale codes 0 .. 252)"
    bias = None if spec.get("bias") is None else np.asarray(spec["bias"], dtype=np.float32)
    return dict(kind="dense", N=spec["N"], K=spec["K"], weight=w32, bias=bias)


def restate_f32(model):
    """the same model with every MXFP4 linear as a dense f32 linear holding W: what the CPU oracle runs (ORC_LIN_DENSE, ORC_F32)"""
    out = dict(model)
    out["layers"] = [{k: (restate_linear(v) if isinstance(v, dict) else v) for k, v in lay.items()} for lay in model["layers"]]
    out["lm_head"] = restate_linear(model["lm_head"])
    return out


# ---- SafeTensors with U8 tensors and a Quark quantization_config ----------------------------------------------------------------------
ST_DT = dict(ckpt_writer.ST_DT)
ST_DT[np.dtype(np.uint8)] = "U8"


def write_safetensors(path, tensors):
    header, off, blobs = {}, 0, []
    for name, a in tensors.items():
        a = np.ascontiguousarray(a)
        b = a.tobytes()
        header[name] = {"dtype": ST_DT[a.dtype], "shape": list(a.shape), "data_offsets": [off, off + len(b)]}
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


def quantization_config(**weight_over):
    """what a Quark MXFP4 export is taken to write: one weight scheme for the model, FP4 activations in input_tensors (ignored by a weight-only run), the
    16-bit tensors on the exclude list"""
    weight = dict(dtype="fp4", qscheme="per_group", group_size=32, ch_axis=-1, scale_format="e8m0", scale_calculation_mode="even", is_dynamic=False,
                  symmetric=None, round_method="half_even", observer_cls="PerBlockMXObserver")
    weight.update(weight_over)
    acts = dict(weight, is_dynamic=True)
    return dict(quant_method="quark", global_quant_config=dict(weight=weight, input_tensors=acts, output_tensors=None, bias=None), layer_quant_config={},
                layer_type_quant_config={}, exclude=["lm_head"], export=dict(kv_cache_group=[], pack_method="reorder", weight_format="real_quantized"))


LINEARS = dict(q="self_attn.q_proj", k="self_attn.k_proj", v="self_attn.v_proj", o="self_attn.o_proj", gate="mlp.gate_proj", up="mlp.up_proj", down="mlp.down_proj")


def write_mxfp4_checkpoint(dirpath, model, quant_config=None):
    """<linear>.weight U8 [N, K/2] and <linear>.weight_scale U8 [N, K/32] for every MXFP4 linear, an optional F32 bias; every other tensor as
    tests/ckpt_writer.py writes it"""
    os.makedirs(dirpath, exist_ok=True)
    t, mx, layers = {}, {}, []
    plain = dict(model)
    for i, lay in enumerate(model["layers"]):
        keep = {}
        for k, v in lay.items():
            if isinstance(v, dict) and v["kind"] == "mxfp4":
                mx["model.layers.%d.%s" % (i, LINEARS[k])] = v
                keep[k] = dict(kind="dense", N=v["N"], K=v["K"], weight=np.zeros((1, 1), dtype=np.float32))   # placeholder, dropped below
            else:
                keep[k] = v
        layers.append(keep)
    plain["layers"] = layers
    for name, a in ckpt_writer.hf_tensors(plain).items():
        if name[:-len(".weight")] in mx:
            continue
        t[name] = a
    for base, spec in mx.items():
        t[base + ".weight"] = np.asarray(spec["weight"], dtype=np.uint8)
        t[base + ".weight_scale"] = np.asarray(spec["scale"], dtype=np.uint8)
        if spec.get("bias") is not None:
            t[base + ".bias"] = np.asarray(spec["bias"], dtype=np.float32)
    j = ckpt_writer.hf_config(model["config"])
    j["quantization_config"] = quantization_config() if quant_config is None else quant_config
    json.dump(j, open(os.path.join(dirpath, "config.json"), "w"))
    write_safetensors(os.path.join(dirpath, "model.safetensors"), t)


# every refusal of the loader's config branch: (name, quantization_config, the field its message names)
def loader_refusals():
    out = [("dtype", quantization_config(dtype="fp6_e2m3"), "global_quant_config.weight.dtype"),
           ("group_size", quantization_config(group_size=16), "global_quant_config.weight.group_size"),
           ("scale_format", quantization_config(scale_format="float32"), "global_quant_config.weight.scale_format")]
    q = quantization_config(); q["layer_quant_config"] = {"*down_proj": dict(weight=dict(dtype="fp8_e4m3"))}
    out.append(("layer_quant_config", q, "layer_quant_config"))
    q = quantization_config(); q["layer_type_quant_config"] = {"Linear": dict(weight=dict(dtype="int8"))}
    out.append(("layer_type_quant_config", q, "layer_type_quant_config"))
    q = quantization_config(); del q["global_quant_config"]
    out.append(("no-global", q, "global_quant_config.weight"))
    return out
