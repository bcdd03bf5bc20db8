"""Numpy reference of the LoRA arithmetic (include/blazr_hip.h "LoRA adapters", DESIGN.md section 4 "LoRA"), for an adapted linear with base output b and
input row x, R = rounding to the activation dtype, s = alpha / r (alpha / sqrt(r) with use_rslora) in f32:

    t_j = R(sum_k A[j,k] x_k)     u_n = R(sum_j B[n,j] t_j)     v_n = R(s u_n)     y_n = R(R(b_n) + v_n)

Every sum is the exact sum of exact products (math.fsum over float64 products: two f32 factors give at most 48 significant bits), rounded once to f32
before R.  A and B are taken at their stored values (float16 / float32 arrays, uint16 arrays = bf16 bits)."""
import math

import numpy as np

import npref


def to_f64(a):
    """a stored adapter matrix (float16 / float32 / uint16 = bf16 bits) -> its exact values in float64"""
    a = np.asarray(a)
    if a.dtype == np.uint16:
        return (a.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return a.astype(np.float64)


def scaling(rank, alpha, use_rslora=False):
    r = np.float32(rank)
    return np.float32(alpha) / (np.sqrt(r) if use_rslora else r)


def _dots(M, x, order):
    """[rows of M] . x as float32: order "fsum" = the exact sum; "fwd" / "rev" = a plain float64 accumulation in index order / reversed (what a
    double accumulator gives in some order -- test_lora.py checks that the three agree on every op-test input)"""
    P = M * x[None, :]                                    # exact in float64
    if order == "fsum":
        return np.array([math.fsum(row) for row in P], dtype=np.float64).astype(np.float32)
    if order == "rev":
        P = P[:, ::-1]
    return np.cumsum(P, axis=1)[:, -1].astype(np.float32) if P.shape[1] else np.zeros(P.shape[0], np.float32)


def lora_delta(x, A, B, s, act, order="fsum"):
    """v = R(s R(B R(A x))) for one row x (float32 values of the activation dtype)"""
    R = lambda a: npref.round_act(a, act)
    t = R(_dots(to_f64(A), np.asarray(x, np.float64), order))
    u = R(_dots(to_f64(B), t.astype(np.float64), order))
    return R(np.float32(s) * u)


def lora_apply(b, x, A, B, s, act, order="fsum"):
    """y = R(R(b) + v); b [N] / x [K] for one row, or [rows, N] / [rows, K]"""
    R = lambda a: npref.round_act(a, act)
    b, x = np.asarray(b, np.float32), np.asarray(x, np.float32)
    if b.ndim == 2:
        return np.stack([lora_apply(b[i], x[i], A, B, s, act, order) for i in range(b.shape[0])])
    return R(R(b) + lora_delta(x, A, B, s, act, order))


TARGET_KEY = {"q": "self_attn.q_proj", "k": "self_attn.k_proj", "v": "self_attn.v_proj", "o": "self_attn.o_proj", "gate": "mlp.gate_proj",
              "up": "mlp.up_proj", "down": "mlp.down_proj"}


def layer_key(layer, target):
    return "model.layers.%d.%s" % (layer, TARGET_KEY[target])


class LoraLlama(npref.NpLlama):
    """npref.NpLlama under one adapter (lora_cases.make_adapter's dict): _lin returns R(base) + v, the caller's R completes y = R(R(b) + v)"""

    def __init__(self, model, adapter):
        super().__init__(model)
        self.adapter = adapter
        self.s = scaling(adapter["rank"], adapter["alpha"], adapter.get("use_rslora", False))

    def _lin(self, l, name, x):
        base = super()._lin(l, name, x)
        pair = self.adapter["pairs"].get(layer_key(l, name))
        if pair is None:
            return base
        act = self.cfg["act_dtype"]
        return npref.round_act(base, act) + lora_delta(x, pair[0], pair[1], self.s, act)


class LoraTruth(npref.NpLlamaTruth):
    """the same model and adapter with no rounding anywhere (float64)"""

    def __init__(self, model, adapter):
        super().__init__(model)
        self.adapter = adapter
        self.s = float(adapter["alpha"]) / (math.sqrt(adapter["rank"]) if adapter.get("use_rslora", False) else float(adapter["rank"]))

    def _lin(self, l, name, x):
        base = super()._lin(l, name, x)
        pair = self.adapter["pairs"].get(layer_key(l, name))
        if pair is None:
            return base
        return base + self.s * (to_f64(pair[1]) @ (to_f64(pair[0]) @ x))


def run(ref, toks):
    return np.stack([np.asarray(ref.step(int(t), i), np.float64).reshape(-1) for i, t in enumerate(toks)])
