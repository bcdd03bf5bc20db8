"""Reference pieces for the GGUF k-quant tests: a numpy Q5_K block generator and dequant (ggml's formula and rounding order), a GGUF v3
writer that takes a ggml type per tensor (block-quantised token_embd, optional output.weight), and the llama.cpp type layouts of
Q4_K_M / Q5_K_M / Q4_K_S files as synthetic models.

Tensor-type rules (llama.cpp's quantiser): token_embd is stored in the file's base block type; output.weight is Q6_K; Q4_K_M / Q5_K_M put
attn_v and ffn_down in Q6_K on the `use_more_bits` layers (synth.q4km_uses_q6k); Q4_K_S puts attn_v / ffn_down of the first layers in Q5_K.
"""
import struct

import numpy as np

from blazr_amd import synth
from ckpt_writer import GG_F32, GG_STR, GG_U32, _gs
from oracle import orc_py

GGML_Q8_0, GGML_Q4_K, GGML_Q5_K, GGML_Q6_K = 8, 12, 13, 14
ROW_BYTES = {GGML_Q8_0: (32, 34), GGML_Q4_K: (256, 144), GGML_Q5_K: (256, 176), GGML_Q6_K: (256, 210)}


def row_bytes(ggml_type, K):
    blk, b = ROW_BYTES[ggml_type]
    return K // blk * b


def q5k_blocks(name, N, K, seed=synth.BASE_SEED):
    """Random but well-conditioned Q5_K blocks (q <= 31, sc <= 63: d in 0.5e-4..1e-4, dmin 1e-4..2e-4) -> gguf linear spec, uint8 [N, K/256*176]."""
    r = synth._rng(name + "#q5_k", seed)
    nb = K // 256
    blk = np.zeros((N, nb, 176), dtype=np.uint8)
    blk[:, :, 0:2] = r.uniform(0.5e-4, 1.0e-4, size=(N, nb)).astype(np.float16).view(np.uint8).reshape(N, nb, 2)
    blk[:, :, 2:4] = r.uniform(1e-4, 2e-4, size=(N, nb)).astype(np.float16).view(np.uint8).reshape(N, nb, 2)
    blk[:, :, 4:] = r.integers(0, 256, size=(N, nb, 172), dtype=np.uint8)
    return dict(kind="gguf", N=N, K=K, ggml_type=GGML_Q5_K, blocks=blk.reshape(N, -1))


def _scale_min(s, j):
    """ggml get_scale_min_k4 over the 12 packed bytes s[..., 12] (uint8 arrays) -> (sc, m) as uint8 arrays"""
    if j < 4:
        return s[..., j] & 63, s[..., j + 4] & 63
    return (s[..., j + 4] & 0xF) | ((s[..., j - 4] >> 6) << 4), (s[..., j + 4] >> 4) | ((s[..., j] >> 6) << 4)


def q5k_dequant(blocks, N, K):
    """float32 [N, K] in ggml's order: d1 = d*sc, m1 = dmin*m, y = d1*q - m1 (every step an f32 rounding, no FMA)"""
    b = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(N, K // 256, 176)
    d = b[..., 0:2].copy().view(np.float16)[..., 0].astype(np.float32)
    dmin = b[..., 2:4].copy().view(np.float16)[..., 0].astype(np.float32)
    sc12, qh, qs = b[..., 4:16], b[..., 16:48], b[..., 48:176]
    out = np.empty((N, K // 256, 256), dtype=np.float32)
    for j in range(8):
        sc, m = _scale_min(sc12, j)
        d1 = d * sc.astype(np.float32)
        m1 = dmin * m.astype(np.float32)
        byte = qs[..., 32 * (j // 2):32 * (j // 2) + 32]
        nib = (byte & 0xF) if j % 2 == 0 else (byte >> 4)
        q = (nib | (((qh >> j) & 1) << 4)).astype(np.float32)
        out[..., 32 * j:32 * j + 32] = d1[..., None] * q - m1[..., None]
    return out.reshape(N, K)


def dequant(spec):
    """f32 [N, K] of a gguf spec: Q5_K here, Q8_0 / Q4_K / Q6_K through the oracle's ggml dequant"""
    N, K, t = spec["N"], spec["K"], spec["ggml_type"]
    if t == GGML_Q5_K:
        return q5k_dequant(spec["blocks"], N, K)
    return orc_py.ggml_dequant(t, spec["blocks"], N * K).reshape(N, K)


def blocks(name, ggml_type, N, K, seed=synth.BASE_SEED):
    return q5k_blocks(name, N, K, seed) if ggml_type == GGML_Q5_K else synth.gguf_blocks(name, ggml_type, N, K, seed)


# ---- synthetic files in llama.cpp's type layouts ---------------------------------------------------------------------------------------------
def _layer_type(ftype, role, i, n_layers):
    if ftype == "q4_k_m":
        return GGML_Q6_K if role in ("v", "down") and synth.q4km_uses_q6k(i, n_layers) else GGML_Q4_K
    if ftype == "q5_k_m":
        return GGML_Q6_K if role in ("v", "down") and synth.q4km_uses_q6k(i, n_layers) else GGML_Q5_K
    if ftype == "q4_k_s":
        return GGML_Q5_K if role in ("v", "down") and i < max(1, n_layers // 8) else GGML_Q4_K
    raise ValueError(ftype)


EMBED_TYPE = {"q4_k_m": GGML_Q4_K, "q5_k_m": GGML_Q5_K, "q4_k_s": GGML_Q4_K}


def make_model(ftype, preset="tiny-q4km", embed_type=None, tied=False, seed=synth.BASE_SEED, **over):
    """dict(config, embed=gguf spec [V, H], final_norm, lm_head=gguf spec or None (tied), layers=[{short: gguf spec}])"""
    cfg = synth.make_config(preset, **over)
    cfg["tie_embeddings"] = bool(tied)
    H, I, V, nl = cfg["hidden"], cfg["inter"], cfg["vocab"], cfg["n_layers"]
    nq, nkv, hd = cfg["n_heads"], cfg["n_kv_heads"], cfg["head_dim"]
    et = embed_type if embed_type is not None else EMBED_TYPE[ftype]
    emb = blocks("model.embed_tokens.weight", et, V, H, seed)
    fn = synth._repr(1.0 + synth._normal(synth._rng("model.norm.weight", seed), (H,), 0.02), "f32")
    if tied:
        lm = None
    elif V % 64 == 0:
        lm = synth.gguf_blocks("lm_head", GGML_Q6_K, V, H, seed)
    else:      # the block GEMV layouts tile columns by 64: an F32 output for a vocabulary that is not a multiple of 64
        lm = synth.dense_linear("lm_head", V, H, "f32", seed=seed)
    shapes = {"q": (nq * hd, H), "k": (nkv * hd, H), "v": (nkv * hd, H), "o": (H, nq * hd), "gate": (I, H), "up": (I, H), "down": (H, I)}
    hf = {"q": "self_attn.q_proj", "k": "self_attn.k_proj", "v": "self_attn.v_proj", "o": "self_attn.o_proj", "gate": "mlp.gate_proj",
          "up": "mlp.up_proj", "down": "mlp.down_proj"}
    layers = []
    for i in range(nl):
        p = "model.layers.%d." % i
        lay = {"attn_norm": synth._repr(1.0 + synth._normal(synth._rng(p + "input_layernorm.weight", seed), (H,), 0.02), "f32"),
               "ffn_norm": synth._repr(1.0 + synth._normal(synth._rng(p + "post_attention_layernorm.weight", seed), (H,), 0.02), "f32")}
        for short, (N, K) in shapes.items():
            lay[short] = blocks(p + hf[short], _layer_type(ftype, short, i, nl), N, K, seed)
        layers.append(lay)
    return dict(config=cfg, embed=emb, final_norm=fn, lm_head=lm, layers=layers)


def oracle_model(model):
    """the synth-style dict OrcLlama takes: f32 dequantised embedding, Q5_K linears as their f32 dequant (the oracle has no Q5_K), other
    block types as their ggml blocks; a tied head is the embedding's block tensor"""
    def lin(spec):
        if spec["kind"] == "gguf" and spec["ggml_type"] == GGML_Q5_K:
            return dict(kind="dense", N=spec["N"], K=spec["K"], weight=q5k_dequant(spec["blocks"], spec["N"], spec["K"]))
        return spec
    lm = model["lm_head"] if model["lm_head"] is not None else lin(model["embed"])
    layers = [dict({k: v for k, v in lay.items() if k in ("attn_norm", "ffn_norm")}, **{k: lin(v) for k, v in lay.items() if isinstance(v, dict)})
              for lay in model["layers"]]
    return dict(config=model["config"], embed=dequant(model["embed"]), final_norm=model["final_norm"], lm_head=lin(lm), layers=layers)


def patch_tensor_info(path, name, ggml_type=None, offset=None):
    """rewrite the type and / or data offset of one tensor-info record of a written file"""
    with open(path, "r+b") as f:
        data = f.read()
        key = _gs(name)
        at = data.index(key) + len(key)
        nd = struct.unpack_from("<I", data, at)[0]
        at += 4 + 8 * nd
        if ggml_type is not None:
            f.seek(at)
            f.write(struct.pack("<I", ggml_type))
        if offset is not None:
            f.seek(at + 4)
            f.write(struct.pack("<Q", offset))


def write_gguf(path, model, extra_tensors=()):
    """GGUF v3 with a ggml type per tensor (the writer of ckpt_writer.write_gguf, generalised to block-quantised token_embd and a missing output)"""
    cfg = model["config"]
    a = "llama"
    kv = [("general.architecture", GG_STR, a), ("general.alignment", GG_U32, 32), (a + ".embedding_length", GG_U32, cfg["hidden"]),
          (a + ".block_count", GG_U32, cfg["n_layers"]), (a + ".context_length", GG_U32, cfg["max_seq_len"]),
          (a + ".feed_forward_length", GG_U32, cfg["inter"]), (a + ".attention.head_count", GG_U32, cfg["n_heads"]),
          (a + ".attention.head_count_kv", GG_U32, cfg["n_kv_heads"]), (a + ".attention.key_length", GG_U32, cfg["head_dim"]),
          (a + ".attention.layer_norm_rms_epsilon", GG_F32, cfg["rms_eps"]), (a + ".rope.freq_base", GG_F32, cfg["rope_theta"]),
          ("general.vocab_size", GG_U32, cfg["vocab"])]
    tensors = []   # (name, ne innermost first, ggml type, bytes)

    def add(name, spec):
        if spec["kind"] == "dense":
            tensors.append((name, [spec["K"], spec["N"]], 0, np.ascontiguousarray(spec["weight"], dtype=np.float32).tobytes()))
            return
        tensors.append((name, [spec["K"], spec["N"]], spec["ggml_type"], np.ascontiguousarray(spec["blocks"], dtype=np.uint8).tobytes()))

    add("token_embd.weight", model["embed"])
    tensors.append(("output_norm.weight", [cfg["hidden"]], 0, np.asarray(model["final_norm"], np.float32).tobytes()))
    if model["lm_head"] is not None:
        add("output.weight", model["lm_head"])
    for i, lay in enumerate(model["layers"]):
        p = "blk.%d." % i
        tensors.append((p + "attn_norm.weight", [cfg["hidden"]], 0, np.asarray(lay["attn_norm"], np.float32).tobytes()))
        tensors.append((p + "ffn_norm.weight", [cfg["hidden"]], 0, np.asarray(lay["ffn_norm"], np.float32).tobytes()))
        for short, gg in (("q", "attn_q"), ("k", "attn_k"), ("v", "attn_v"), ("o", "attn_output"), ("gate", "ffn_gate"), ("up", "ffn_up"), ("down", "ffn_down")):
            add(p + gg + ".weight", lay[short])
    tensors += list(extra_tensors)
    with open(path, "wb") as f:
        f.write(b"GGUF" + struct.pack("<IQQ", 3, len(tensors), len(kv)))
        for k, ty, v in kv:
            f.write(_gs(k) + struct.pack("<I", ty))
            f.write(struct.pack("<I", v) if ty == GG_U32 else (struct.pack("<f", v) if ty == GG_F32 else _gs(v)))
        off, offs = 0, []
        for name, ne, ty, b in tensors:
            offs.append(off)
            off = (off + len(b) + 31) // 32 * 32
        for (name, ne, ty, b), o in zip(tensors, offs):
            f.write(_gs(name) + struct.pack("<I", len(ne)) + b"".join(struct.pack("<Q", d) for d in ne) + struct.pack("<IQ", ty, o))
        f.write(b"\0" * ((32 - f.tell() % 32) % 32))
        base = f.tell()
        for (name, ne, ty, b), o in zip(tensors, offs):
            f.seek(base + o)
            f.write(b)
        f.write(b"\0" * ((32 - f.tell() % 32) % 32))
