"""NVFP4 weight checkpoints (E2M1 codes in groups of 16, one E4M3 scale per group, one global scale per tensor): the shapes, the float64 weight, the exact
oracle restatement and a compressed-tensors writer that tests/test_nvfp4_weights.py and tests/test_gpu_nvfp4_weights.py share.  ASSUMPTION (also in
include/blazr_hip.h and DESIGN 4): the nibble order (low nibble = the even element), the tensor and field names and the global scale being a divisor are what
this writer and the loader define; none could be checked against a published file.  Data only; nothing here touches the GPU."""
import json
import os

import numpy as np

import ckpt_writer
import fp8_cases
from blazr_amd import synth
from mxfp4_cases import E2M1, LINEARS, pack, unpack

E4M3 = fp8_cases.TABLE.astype(np.float64)          # code -> value; 0x7F / 0xFF are NaN
fp8_cases.ST_DT.setdefault(np.dtype(np.uint8), "U8")      # fp8_cases.write_safetensors writes plain uint8 arrays (the packed codes) as U8

# (N, K) of the op-level tests and what each reaches (tiles of four rows x 512 k; the four waves of a workgroup split a row group's tiles)
GEMV_SHAPES = [
    (64, 64),        # the smallest linear: one tile per row group, three waves without a share of K
    (192, 704),      # K = 11 x 64: a ragged second tile, two waves with a share
    (256, 4096),     # eight full tiles per row: two per wave
]
GEMM_SHAPES = [(192, 704), (256, 4096)]     # N % 128 == 64 with a ragged K; full tiles, K split across workgroups at small S
GEMM_ROWS = [9, 64, 130]

MODELS = {
    "tiny-nvfp4-bf16": ("tiny-nvfp4", dict()),
    "tiny-nvfp4-f16": ("tiny-nvfp4", dict(act_dtype="f16")),
    "nvfp4-g2-w768": ("tiny-nvfp4", dict(hidden=768, n_heads=6, n_kv_heads=3, head_dim=128, inter=1408, vocab=1003, max_seq_len=512)),
}


def make(name):
    preset, over = MODELS[name]
    return synth.make_llama(preset, **over)


def spec_of(codes, scale, global_scale, bias=None):
    N, K = codes.shape
    return dict(kind="nvfp4", N=N, K=K, weight=pack(codes), scale=np.asarray(scale, dtype=np.uint8).reshape(N, K // 16), global_scale=float(global_scale), bias=bias)


def weight_f64(lin):
    """float64 W = e2m1(q) . e4m3(s) . r with r = f32(1 / global_scale): the first product is exact (six bits), the second rounds for a general r only"""
    r = float(np.float32(1.0 / float(lin["global_scale"])))
    w = E2M1[unpack(lin["weight"])].astype(np.float64) * np.repeat(E4M3[np.asarray(lin["scale"], dtype=np.uint8)], 16, axis=1)
    return w * r


def restate_linear(spec):
    if spec["kind"] != "nvfp4":
        return spec
    w64 = weight_f64(spec)
    w32 = w64.astype(np.float32)
    assert np.array_equal(w32.astype(np.float64), w64), "e2m1 . e4m3 / global_scale must be exact in f32 (a power-of-two global scale)"
    bias = None if spec.get("bias") is None else np.asarray(spec["bias"], dtype=np.float32)
    return dict(kind="dense", N=spec["N"], K=spec["K"], weight=w32, bias=bias)


def restate_f32(model):
    """the same model with every NVFP4 linear as a dense f32 linear holding W: what the CPU oracle runs"""
    out = dict(model)
    out["layers"] = [{k: (restate_linear(v) if isinstance(v, dict) else v) for k, v in lay.items()} for lay in model["layers"]]
    out["lm_head"] = restate_linear(model["lm_head"])
    return out


def quantization_config(fmt="nvfp4-pack-quantized", **weight_over):
    """what llm-compressor is taken to write for NVFP4: one group for every Linear, FP4 activations in input_activations (ignored by a weight-only run)"""
    weights = dict(num_bits=4, type="float", strategy="tensor_group", group_size=16, symmetric=True, dynamic=False)
    weights.update(weight_over)
    acts = dict(num_bits=4, type="float", strategy="tensor_group", group_size=16, symmetric=True, dynamic="local")
    return dict(quant_method="compressed-tensors", format=fmt, ignore=["lm_head"], quantization_status="compressed",
                config_groups=dict(group_0=dict(targets=["Linear"], weights=weights, input_activations=acts)))


def write_nvfp4_checkpoint(dirpath, model, quant_config=None):
    """<base>.weight_packed U8 [N, K/2], <base>.weight_scale F8_E4M3 [N, K/16], <base>.weight_global_scale and .input_global_scale F32 [1], an optional F32
    bias for every NVFP4 linear; every other tensor as tests/ckpt_writer.py writes it"""
    os.makedirs(dirpath, exist_ok=True)
    t, nv, layers = {}, {}, []
    plain = dict(model)
    for i, lay in enumerate(model["layers"]):
        keep = {}
        for k, v in lay.items():
            if isinstance(v, dict) and v["kind"] == "nvfp4":
                nv["model.layers.%d.%s" % (i, LINEARS[k])] = v
                keep[k] = dict(kind="dense", N=v["N"], K=v["K"], weight=np.zeros((1, 1), dtype=np.float32))   # placeholder, dropped below
            else:
                keep[k] = v
        layers.append(keep)
    plain["layers"] = layers
    for name, a in ckpt_writer.hf_tensors(plain).items():
        if name[:-len(".weight")] not in nv:
            t[name] = a
    for base, spec in nv.items():
        t[base + ".weight_packed"] = np.asarray(spec["weight"], dtype=np.uint8)
        t[base + ".weight_scale"] = fp8_cases.F8(spec["scale"])
        t[base + ".weight_global_scale"] = np.array([spec["global_scale"]], dtype=np.float32)
        t[base + ".input_global_scale"] = np.array([345.0], dtype=np.float32)
        if spec.get("bias") is not None:
            t[base + ".bias"] = np.asarray(spec["bias"], dtype=np.float32)
    j = ckpt_writer.hf_config(model["config"])
    j["quantization_config"] = quantization_config() if quant_config is None else quant_config
    json.dump(j, open(os.path.join(dirpath, "config.json"), "w"))
    fp8_cases.write_safetensors(os.path.join(dirpath, "model.safetensors"), t)
