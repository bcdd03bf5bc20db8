"""Length sets of packed prompt batches, chosen for the edges of the segment-masked attention kernels (bz_prefill.hip, the SEG forms): a wave of the MFMA kernel
owns 32 queries, a key tile is 64 keys, a workgroup owns 32 QT queries (QT = 4 / min(group, 4): 128, 64 or 32), a prompt chunk is 2048 rows."""
import numpy as np

SETS = {
    "A": [1] * 40,                                              # 32 segments inside one wave's query tile: every row sees its own key and nothing else
    "B": [31, 1, 32, 33, 63, 64, 65, 1, 1, 127, 128, 129],      # boundaries around the 32-query wave tile, the 64-key tile and the workgroup tile for every QT
    "C": [200, 3, 5],                                           # long then short: early key tiles wholly masked for a wave's later queries
    "D": [3, 300],
    "E": [2040, 20, 9],                                         # a segment across the 2048-row chunk edge (whole-model tests on the tiny fixtures)
}
BELOW_FLOOR = [4, 3]                                            # 7 rows: below the row floor of the batched prompt path (BZ_PREFILL_MIN = 8)
OP_SETS = ("A", "B", "C", "D")


def offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def token_lists(lens, vocab, seed):
    """one list of token ids per input; fixed by the seed"""
    rng = np.random.default_rng(seed)
    return [rng.integers(1, vocab, size=int(n)).astype(np.int64) for n in lens]


def qkv_rows(lens, nq, nkv, hd, dt, seed):
    """N(0, 1) rows of [q | k | v], rounded to the 16-bit dtype `dt` ("f16" / "bf16"; "f32": as they are), as float32"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((int(np.sum(lens)), (nq + 2 * nkv) * hd)).astype(np.float32)
    return round_to(x, dt)


def round_to(x, dt):
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dt == "f16":
        return x.astype(np.float16).astype(np.float32)
    if dt == "bf16":                                            # round to nearest even on the upper 16 bits
        u = x.view(np.uint32).astype(np.uint64)
        u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
        return u.astype(np.uint32).view(np.float32)
    return x
