"""Reference pieces for the GGUF legacy-quant tests (ggml's original 32-weight blocks: Q4_0, Q4_1, Q5_0, Q5_1): numpy block generators and
dequantisers in ggml's order (every product and sum one float32 rounding, no FMA), and synthetic models in llama.cpp's legacy file layouts.

Block layouts (public ggml spec), weight j (0..15) in the low nibble of qs[j], weight j + 16 in its high nibble:
  Q4_0 {f16 d; u8 qs[16]}            18 B   y = (q - 8) * d
  Q4_1 {f16 d, m; u8 qs[16]}         20 B   y = q * d + m
  Q5_0 {f16 d; u8 qh[4]; u8 qs[16]}  22 B   5th bit of weight j = bit j of qh (little-endian u32); y = (q - 16) * d
  Q5_1 {f16 d, m; u8 qh[4]; u8 qs[16]} 24 B y = q * d + m

File layouts (llama.cpp's quantiser for these file types): every linear and token_embd in the base type, output.weight in Q6_K; a tied file has no
output.weight.  The "mixed" layout is a Q4_K_M file whose attn_v is Q5_0 and ffn_down Q5_1 (one layer's q / k and v of different types).
"""
import numpy as np

import kquant_ref as kq
from blazr_amd import synth

GGML_Q4_0, GGML_Q4_1, GGML_Q5_0, GGML_Q5_1 = 2, 3, 6, 7
LEGACY = (GGML_Q4_0, GGML_Q4_1, GGML_Q5_0, GGML_Q5_1)
BLOCK_BYTES = {GGML_Q4_0: 18, GGML_Q4_1: 20, GGML_Q5_0: 22, GGML_Q5_1: 24}
NAME = {GGML_Q4_0: "q4_0", GGML_Q4_1: "q4_1", GGML_Q5_0: "q5_0", GGML_Q5_1: "q5_1"}
TYPE_OF = {v: k for k, v in NAME.items()}


def _affine(t):
    return t in (GGML_Q4_1, GGML_Q5_1)


def _five(t):
    return t in (GGML_Q5_0, GGML_Q5_1)


def row_bytes(ggml_type, K):
    if ggml_type in LEGACY:
        return K // 32 * BLOCK_BYTES[ggml_type]
    return kq.row_bytes(ggml_type, K)


def pack_block(ggml_type, d, q, m=0.0):
    """one raw block from d (and m) and the 32 stored values q (0..15, or 0..31 for Q5_0 / Q5_1) -> uint8 [bytes]"""
    q = np.asarray(q, dtype=np.uint32)
    assert q.shape == (32,) and q.max() < (32 if _five(ggml_type) else 16)
    b = np.zeros(BLOCK_BYTES[ggml_type], np.uint8)
    b[0:2] = np.array([d], np.float16).view(np.uint8)
    at = 2
    if _affine(ggml_type):
        b[2:4] = np.array([m], np.float16).view(np.uint8)
        at = 4
    if _five(ggml_type):
        qh = int(sum(int((q[j] >> 4) & 1) << j for j in range(32)))
        b[at:at + 4] = np.array([qh], "<u4").view(np.uint8)
        at += 4
    b[at:at + 16] = ((q[:16] & 15) | ((q[16:] & 15) << 4)).astype(np.uint8)
    return b


def legacy_blocks(name, ggml_type, N, K, seed=synth.BASE_SEED):
    """Random but well-conditioned blocks (|w| < ~0.07, m about -q_mid d so that rows are centred) -> gguf linear spec, uint8 [N, K/32 * bytes]."""
    r = synth._rng(name + "#" + NAME[ggml_type], seed)
    nb, bs = K // 32, BLOCK_BYTES[ggml_type]
    blk = np.zeros((N, nb, bs), dtype=np.uint8)
    lo, hi = (0.004, 0.008) if not _five(ggml_type) else (0.002, 0.004)
    d = r.uniform(lo, hi, size=(N, nb))
    blk[:, :, 0:2] = d.astype(np.float16).view(np.uint8).reshape(N, nb, 2)
    at = 2
    if _affine(ggml_type):
        mid = 8.0 if ggml_type == GGML_Q4_1 else 16.0
        m = -d * r.uniform(mid - 2.0, mid + 2.0, size=(N, nb))
        blk[:, :, 2:4] = m.astype(np.float16).view(np.uint8).reshape(N, nb, 2)
        at = 4
    blk[:, :, at:] = r.integers(0, 256, size=(N, nb, bs - at), dtype=np.uint8)
    return dict(kind="gguf", N=N, K=K, ggml_type=ggml_type, blocks=blk.reshape(N, -1))


def dequant_blocks(ggml_type, blocks, N, K):
    """float32 [N, K] in ggml's order (dequantize_row_q4_0 / q4_1 / q5_0 / q5_1): x = q (- 8 | - 16) as int -> float, y = x * d (+ m)"""
    bs = BLOCK_BYTES[ggml_type]
    b = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(N, K // 32, bs)
    d = b[..., 0:2].copy().view(np.float16)[..., 0].astype(np.float32)
    at = 2
    m = None
    if _affine(ggml_type):
        m = b[..., 2:4].copy().view(np.float16)[..., 0].astype(np.float32)
        at = 4
    q = np.zeros((N, K // 32, 32), dtype=np.int32)
    if _five(ggml_type):
        qh = b[..., at:at + 4].copy().view("<u4")[..., 0].astype(np.uint64)
        at += 4
        for j in range(32):
            q[..., j] = ((qh >> np.uint64(j)) & np.uint64(1)).astype(np.int32) << 4
    qs = b[..., at:at + 16].astype(np.int32)
    q[..., :16] |= qs & 15
    q[..., 16:] |= qs >> 4
    if ggml_type == GGML_Q4_0:
        y = (q - 8).astype(np.float32) * d[..., None]
    elif ggml_type == GGML_Q5_0:
        y = (q - 16).astype(np.float32) * d[..., None]
    else:
        y = q.astype(np.float32) * d[..., None] + m[..., None]
    return y.astype(np.float32).reshape(N, K)


def dequant(spec):
    """f32 [N, K] of a gguf spec: the legacy formats here, the others through kquant_ref"""
    if spec["kind"] == "gguf" and spec["ggml_type"] in LEGACY:
        return dequant_blocks(spec["ggml_type"], spec["blocks"], spec["N"], spec["K"])
    return kq.dequant(spec)


def blocks(name, ggml_type, N, K, seed=synth.BASE_SEED):
    return legacy_blocks(name, ggml_type, N, K, seed) if ggml_type in LEGACY else kq.blocks(name, ggml_type, N, K, seed)


# ---- synthetic files in llama.cpp's legacy type layouts --------------------------------------------------------------------------------------
SHAPES_HF = {"q": "self_attn.q_proj", "k": "self_attn.k_proj", "v": "self_attn.v_proj", "o": "self_attn.o_proj", "gate": "mlp.gate_proj",
             "up": "mlp.up_proj", "down": "mlp.down_proj"}


def _layer_type(ftype, role, i, n_layers):
    if ftype in TYPE_OF:
        return TYPE_OF[ftype]
    if ftype == "mixed":     # Q4_K_M with attn_v in Q5_0 and ffn_down in Q5_1
        return GGML_Q5_0 if role == "v" else GGML_Q5_1 if role == "down" else kq.GGML_Q4_K
    raise ValueError(ftype)


def make_model(ftype, preset="tiny-q4km", embed_type=None, tied=False, seed=synth.BASE_SEED, **over):
    """ftype: "q4_0" / "q4_1" / "q5_0" / "q5_1" / "mixed" -> dict(config, embed=gguf spec [V, H], final_norm, lm_head=gguf spec or None (tied),
    layers=[{short: gguf spec}])"""
    cfg = synth.make_config(preset, **over)
    cfg["tie_embeddings"] = bool(tied)
    H, I, V, nl = cfg["hidden"], cfg["inter"], cfg["vocab"], cfg["n_layers"]
    nq, nkv, hd = cfg["n_heads"], cfg["n_kv_heads"], cfg["head_dim"]
    et = embed_type if embed_type is not None else (TYPE_OF[ftype] if ftype in TYPE_OF else kq.GGML_Q4_K)
    emb = blocks("model.embed_tokens.weight", et, V, H, seed)
    fn = synth._repr(1.0 + synth._normal(synth._rng("model.norm.weight", seed), (H,), 0.02), "f32")
    if tied:
        lm = None
    elif V % 64 == 0:
        lm = synth.gguf_blocks("lm_head", kq.GGML_Q6_K, V, H, seed)
    else:      # the block GEMV layouts tile columns by 64: an F32 output for a vocabulary that is not a multiple of 64
        lm = synth.dense_linear("lm_head", V, H, "f32", seed=seed)
    shapes = {"q": (nq * hd, H), "k": (nkv * hd, H), "v": (nkv * hd, H), "o": (H, nq * hd), "gate": (I, H), "up": (I, H), "down": (H, I)}
    layers = []
    for i in range(nl):
        p = "model.layers.%d." % i
        lay = {"attn_norm": synth._repr(1.0 + synth._normal(synth._rng(p + "input_layernorm.weight", seed), (H,), 0.02), "f32"),
               "ffn_norm": synth._repr(1.0 + synth._normal(synth._rng(p + "post_attention_layernorm.weight", seed), (H,), 0.02), "f32")}
        for short, (N, K) in shapes.items():
            lay[short] = blocks(p + SHAPES_HF[short], _layer_type(ftype, short, i, nl), N, K, seed)
        layers.append(lay)
    return dict(config=cfg, embed=emb, final_norm=fn, lm_head=lm, layers=layers)


def oracle_model(model):
    """the synth-style dict OrcLlama takes: f32 dequantised embedding, legacy (and Q5_K) linears as their f32 dequant (the oracle has neither),
    other block types as their ggml blocks; a tied head is the embedding's dequantised table"""
    def lin(spec):
        if spec["kind"] == "gguf" and (spec["ggml_type"] in LEGACY or spec["ggml_type"] == kq.GGML_Q5_K):
            return dict(kind="dense", N=spec["N"], K=spec["K"], weight=dequant(spec))
        return spec
    lm = model["lm_head"] if model["lm_head"] is not None else model["embed"]
    layers = [dict({k: v for k, v in lay.items() if k in ("attn_norm", "ffn_norm")}, **{k: lin(v) for k, v in lay.items() if isinstance(v, dict)})
              for lay in model["layers"]]
    return dict(config=model["config"], embed=dequant(model["embed"]), final_norm=model["final_norm"], lm_head=lin(lm), layers=layers)


write_gguf = kq.write_gguf
patch_tensor_info = kq.patch_tensor_info
