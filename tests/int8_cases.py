"""INT8 W8A8 (compressed-tensors int-quantized): the numpy restatement of the linear, op shapes and planted rows, models, a checkpoint writer."""
import json
import os
import struct

import numpy as np

import ckpt_writer
from blazr_amd import synth

GEMV_SHAPES = [(64, 64), (192, 704), (256, 4096), (64, 14336)]     # one tile; a ragged last 256-chunk; the split-K form (4 slices); the long K (14 slices)
GEMM_SHAPES = [(192, 704), (1408, 768), (256, 4096)]
GEMM_ROWS = [1, 9, 17, 64, 130]
MODELS = {"tiny-int8-channel-bf16": dict(), "tiny-int8-tensor-f16": dict(act_dtype="f16", int8_strategy="tensor", bias=True)}
LINEARS = dict(q="self_attn.q_proj", k="self_attn.k_proj", v="self_attn.v_proj", o="self_attn.o_proj", gate="mlp.gate_proj", up="mlp.up_proj", down="mlp.down_proj")


def ref_linear(x, q, sw, bias=None):
    """y = f32(acc . (sx . sw)) + b with sx = amax / 127 (1 for a zero row), a = clip(rint(x / sx)), acc = a . q^T exact; x [S, K] f32, q [N, K] int8, sw [1 | N]"""
    amax = np.abs(x).max(axis=-1, keepdims=True)
    sx = np.where(amax == 0, np.float32(1), amax / np.float32(127)).astype(np.float32)
    acc = np.clip(np.rint(x / sx), -127, 127).astype(np.int64) @ q.astype(np.int64).T
    v = (acc.astype(np.float64) * (sx.astype(np.float64) * np.broadcast_to(np.asarray(sw, np.float32).reshape(-1), q.shape[:1]).astype(np.float64))).astype(np.float32)
    return v if bias is None else v + np.asarray(bias, np.float32)


def planted_rows(K, act, seed):
    """x [8, K] of act-representable f32: N(0,1) rows but 2 all zero, 3 quotient ties k + 0.5 of both parities (amax = 127 . 2^-3, so sx = 2^-3), 4 the dtype's
    subnormals only, 5 one element at the dtype's largest finite value, 6 every other element -0.0"""
    x = synth._repr(np.random.default_rng(seed).standard_normal((8, K)).astype(np.float32), act)
    k, alt = np.arange(K), np.where(np.arange(K) % 2, -1.0, 1.0)
    x[2] = 0.0
    x[3] = (k % 127 + 0.5) * 0.125 * np.where(k % 3 == 0, -1.0, 1.0)
    x[3, K // 2] = 127.0 * 0.125
    if act == "bf16":
        x[4] = ((1 + k % 127).astype(np.uint32) << 16).view(np.float32) * alt      # bf16 subnormals are f32 subnormals
        x[5, K // 3] = (np.uint32(0x7F7F) << 16).view(np.float32)
    else:
        x[4] = (1 + k % 1023) * 2.0 ** -24 * alt
        x[5, K // 3] = 65504.0
    x[6, ::2] = -0.0
    assert np.array_equal(synth._repr(x, act), x)
    return x


def make(name, **over):
    return synth.make_llama("tiny-int8", **dict(MODELS[name], **over))


def restate_f32(model):
    """the same model with every int8 linear as the dense f32 tensor sw . q (16 significant bits: exact) -- what a 16-bit-activation run multiplies by"""
    dense = lambda v: dict(kind="dense", N=v["N"], K=v["K"], bias=v.get("bias"), weight=v["weight"].astype(np.float32) * np.broadcast_to(v["scale"], (v["N"],))[:, None])
    return dict(model, layers=[{k: dense(v) if isinstance(v, dict) and v.get("kind") == "int8" else v for k, v in lay.items()} for lay in model["layers"]])


def quantization_config(weight_strategy="channel", **act_over):
    act = dict(dict(num_bits=8, type="int", strategy="token", symmetric=True, dynamic=True), **act_over)
    return dict(quant_method="compressed-tensors", format="int-quantized", ignore=["lm_head"], quantization_status="compressed", config_groups=dict(group_0=dict(
        targets=["Linear"], weights=dict(num_bits=8, type="int", strategy=weight_strategy, symmetric=True, dynamic=False), input_activations=act)))


def write_int8_checkpoint(dirpath, model, with_quant_config=True, zero_point=None):
    """channel scales as BF16 [N,1], a tensor scale as F32 [1]; zero_point: an I8 weight_zero_point [N,1] of that value beside every weight (None: no such tensor)"""
    os.makedirs(dirpath, exist_ok=True)
    i8 = {"model.layers.%d.%s" % (i, LINEARS[k]): v for i, lay in enumerate(model["layers"]) for k, v in lay.items() if isinstance(v, dict) and v.get("kind") == "int8"}
    t = {n: a for n, a in ckpt_writer.hf_tensors(restate_f32(model)).items() if n[:-len(".weight")] not in i8}
    for base, spec in i8.items():
        t[base + ".weight"] = spec["weight"]
        t[base + ".weight_scale"] = synth.f32_to_bf16_bits(spec["scale"]).reshape(-1, 1) if spec["scale"].size > 1 else spec["scale"].astype(np.float32)
        if zero_point is not None:
            t[base + ".weight_zero_point"] = np.full((spec["N"], 1), zero_point, np.int8)
        if spec.get("bias") is not None:
            t[base + ".bias"] = np.asarray(spec["bias"], dtype=np.float32)
    j = ckpt_writer.hf_config(model["config"])
    if with_quant_config:
        j["quantization_config"] = quantization_config(model["config"].get("int8_strategy", "channel"))
    json.dump(j, open(os.path.join(dirpath, "config.json"), "w"))
    header, blobs, off = {"__metadata__": {"format": "pt"}}, [np.ascontiguousarray(a).tobytes() for a in t.values()], 0
    for (name, a), b in zip(t.items(), blobs):
        header[name] = {"dtype": {**ckpt_writer.ST_DT, np.dtype(np.int8): "I8"}[np.asarray(a).dtype], "shape": list(np.shape(a)), "data_offsets": [off, off + len(b)]}
        off += len(b)
    h = json.dumps(header).encode()
    h += b" " * (-len(h) % 8)
    open(os.path.join(dirpath, "model.safetensors"), "wb").write(struct.pack("<Q", len(h)) + h + b"".join(blobs))
