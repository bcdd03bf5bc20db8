"""IQ4_XS reference: the numpy dequantiser of the public block spec and a random-block builder.  Block of 256 weights, 136 bytes {f16 d; u16 scales_h;
u8 scales_l[4]; u8 qs[128]}; sub-block ib: ls = 4 bits of scales_l | 2 bits of scales_h, dl = f32(d) * (ls - 32), y[32 ib + j] = dl * KV[qs[16 ib + j] & 15],
y[32 ib + j + 16] = dl * KV[qs[16 ib + j] >> 4]; each product one float32 rounding."""
import numpy as np

from blazr_amd import synth

GGML_IQ4_XS, BLOCK_BYTES = 23, 136
KV = np.array([-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113], np.float32)


def pack_block(d, ls, codes):
    """one raw block from d, the 8 scales ls (0..63) and the 256 codes (0..15) -> uint8 [136]"""
    ls, c = np.asarray(ls, np.uint32), np.asarray(codes, np.uint8).reshape(8, 32)
    b = np.zeros(BLOCK_BYTES, np.uint8)
    b[0:2] = np.array([d], np.float16).view(np.uint8)
    b[2:4] = np.array([sum(int(ls[i] >> 4) << (2 * i) for i in range(8))], "<u2").view(np.uint8)
    b[4:8] = [int(ls[2 * i] & 15) | (int(ls[2 * i + 1] & 15) << 4) for i in range(4)]
    b[8:] = (c[:, :16] | (c[:, 16:] << 4)).reshape(-1)
    return b


def dequant_blocks(blocks, N, K):
    b = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(N, K // 256, BLOCK_BYTES)
    d = b[..., 0:2].copy().view(np.float16)[..., 0].astype(np.float32)
    sh, sl, qs = b[..., 2:4].copy().view("<u2")[..., 0].astype(np.int32), b[..., 4:8].astype(np.int32), b[..., 8:].reshape(N, K // 256, 8, 16)
    out = np.empty((N, K // 256, 8, 32), np.float32)
    for ib in range(8):
        ls = ((sl[..., ib // 2] >> (4 * (ib % 2))) & 15) | (((sh >> (2 * ib)) & 3) << 4)
        dl = (d * (ls - 32).astype(np.float32))[..., None]
        out[..., ib, :16], out[..., ib, 16:] = dl * KV[qs[..., ib, :] & 15], dl * KV[qs[..., ib, :] >> 4]
    return out.reshape(N, K)


def blocks(name, N, K, seed=synth.BASE_SEED):
    """random blocks (|w| < 0.07: d drawn uniformly, as legacy_quant_ref does); blocks 0..7 carry all 64 ls values, block 0 all 16 codes -> gguf linear spec"""
    r = synth._rng(name + "#iq4_xs", seed)
    blk = r.integers(0, 256, size=(N * (K // 256), BLOCK_BYTES), dtype=np.uint8)
    blk[:, 0:2] = r.uniform(0.8e-5, 1.6e-5, size=(len(blk), 1)).astype(np.float16).view(np.uint8)
    for t in range(8):
        codes = np.concatenate([blk[t, 8:].reshape(8, 16) & 15, blk[t, 8:].reshape(8, 16) >> 4], axis=1)
        blk[t] = pack_block(blk[t, 0:2].copy().view(np.float16)[0], np.arange(8) + 8 * t, np.arange(256) % 16 if t == 0 else codes)
    return dict(kind="gguf", N=N, K=K, ggml_type=GGML_IQ4_XS, blocks=blk.reshape(N, -1))
