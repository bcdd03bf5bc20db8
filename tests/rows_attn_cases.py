"""Helpers of tests/test_gpu_rows_attn.py: paged pools with INJECTED rows (LayeredPagedKvCache.write_block), planted rows, and the float64 truth.

The constructions are those of tests/test_gpu_long_context.py (see its docstring: random caches cannot catch a dropped or doubled row, so each planted key is
chosen from the query with a set score margin and carries a V pattern of its own), restated for decode BATCHES over block tables: every sequence of a batch is a
row with its own length, its own blocks (permuted, interleaved with the other rows') and its own planted case.  Block 0 belongs to no row and holds large finite
values: it is what a padded block-table entry (0) points at."""
import numpy as np

from blazr_amd import _lib as L
from blazr_amd import runtime
from oracle import orc_py

BS = 16
DT = {"f16": L.F16, "bf16": L.BF16}
UNIT = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}         # unit roundoff of the activation dtype: what a correctly rounded row can reach (the f32 sums add orders less)
TRUTH_FACTOR = 1.25                                   # test_gpu_long_context.py
POISON = 3.0e4                                        # block 0: large, finite in f16


def rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def bits16(x, act):
    """float32 values representable in `act` -> the 16-bit patterns the pool stores"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if act == "f16":
        return x.astype(np.float16).view(np.uint16)
    return (x.view(np.uint32) >> 16).astype(np.uint16)


def slice_len(n):
    return runtime.rows_attn_slice_len(n)


def truth(q, K, V, window=0, drop=()):
    """float64 softmax attention of q [nq, hd] over rows [lo, T) of K / V [T, nkv, hd] (lo from the window), without the rows in `drop`"""
    q, K, V = np.asarray(q, np.float64), np.asarray(K, np.float64), np.asarray(V, np.float64)
    T = K.shape[0]
    lo = T - window if 0 < window < T else 0
    keep = np.setdiff1d(np.arange(lo, T), np.asarray(list(drop), dtype=np.int64))
    rep = q.shape[0] // K.shape[1]
    out = np.zeros_like(q)
    if len(keep) == 0:                          # (the only row removed: nothing is left of the output)
        return out
    for h in range(q.shape[0]):
        s = K[keep, h // rep] @ q[h] / np.sqrt(q.shape[1])
        p = np.exp(s - s.max())
        out[h] = (p / p.sum()) @ V[keep, h // rep]
    return out


class Pool:
    """one paged pool; sequences get their blocks from a seeded permutation of 1 .. num_blocks - 1, so consecutive sequences interleave"""

    def __init__(self, device, layers, num_blocks, nkv, hd, act, seed=0):
        self.act, self.nkv, self.hd, self.layers = act, nkv, hd, layers
        self.kv = runtime.LayeredPagedKvCache(device, layers, num_blocks, BS, nkv, hd, DT[act])
        self.free = list(1 + np.random.default_rng(seed).permutation(num_blocks - 1))
        poison = bits16(np.full((nkv, BS, hd), POISON, np.float32), act)
        for l in range(layers):
            self.kv.write_block(l, 0, 0, poison)
            self.kv.write_block(l, 0, 1, poison)

    def take(self, n_rows):
        """blocks for a sequence of n_rows rows (its table), handed out interleaved with the other sequences'"""
        nb = -(-n_rows // BS)
        assert nb <= len(self.free), "pool too small"
        blocks, self.free = [int(b) for b in self.free[:nb]], self.free[nb:]
        return blocks

    def write(self, layer, blocks, K, V, first=0):
        """rows first .. first + T - 1 of a sequence into its blocks; K / V [T, nkv, hd].  `first` must sit on a block boundary; a partial last block is
        filled up with the poison value (slots beyond the sequence's length must never be read into a result)"""
        assert first % BS == 0
        T = K.shape[0]
        for which, X in ((0, K), (1, V)):
            pad = (-T) % BS
            Xp = np.concatenate([X, np.full((pad,) + X.shape[1:], POISON, np.float32)]) if pad else X
            blk = bits16(Xp, self.act).reshape(-1, BS, self.nkv, self.hd).transpose(0, 2, 1, 3)      # [block][kv head][slot][hd]
            for j in range(blk.shape[0]):
                self.kv.write_block(layer, blocks[first // BS + j], which, blk[j])


def make_q(rng, nq, nkv, hd, act):
    """query heads that share a direction inside each GQA group, so that one key can score high for all of them"""
    g = rng.standard_normal((nkv, 1, hd))
    q = g + 0.3 * rng.standard_normal((nkv, nq // nkv, hd))
    return orc_py.round_act(q.reshape(nq, hd).astype(np.float32), act)


def key_with_score(q, nkv, score, act):
    """one key per kv head whose score against EVERY query head of its group is `score` (before the key is rounded): the least-norm solution of
    Q k = score sqrt(hd) 1, which exists whenever the group's heads are linearly independent"""
    hd = q.shape[1]
    qg = q.reshape(nkv, -1, hd).astype(np.float64)
    k = np.stack([np.linalg.pinv(Q) @ np.full(Q.shape[0], 1.001 * score * np.sqrt(hd)) for Q in qg])
    k = orc_py.round_act(k.astype(np.float32), act)
    assert (np.einsum("ghd,gd->gh", qg, k.astype(np.float64)) / np.sqrt(hd) >= 0.97 * score).all()
    return k


def pattern(j, nkv, hd, act):
    """a V row of its own for planted row j: large, and orthogonal-ish to every other pattern"""
    d = np.arange(hd)
    v = 4.0 * np.sign(np.cos((j + 1) * 0.7 * d + j)) * (1.0 + (d % (j + 3) == 0))
    return orc_py.round_act(np.broadcast_to(v, (nkv, hd)).astype(np.float32), act)


def background(rng, T, nkv, hd, act):
    K = orc_py.round_act(rng.standard_normal((T, nkv, hd)).astype(np.float32) * 0.05, act)
    V = orc_py.round_act(rng.standard_normal((T, nkv, hd)).astype(np.float32), act)
    return K, V


def planted_cases(T, window=0):
    """names of the planted constructions that exist at a context of T rows: (name, planted rows, rows whose removal must move the truth)"""
    lo = T - window if 0 < window < T else 0
    wl = T - lo
    spl = slice_len(wl)
    ns = -(-wl // spl)
    edges = {lo + spl - 1, lo + spl, lo + (ns - 1) * spl}
    spots = sorted(({lo, T - 2} | edges) & set(range(lo, T)))
    out = [("dominant row %d" % r, [r]) for r in spots]
    if ns >= 2:
        out.append(("two equal rows", [lo, lo + (ns - 1) * spl]))
        out.append(("all keys equal", []))
    if wl >= 3:
        out.append(("margin 120 at row %d" % (lo + wl // 2), [lo + wl // 2]))
    return out


def build_case(rng, q, T, name, rows, nkv, act, window=0):
    """-> (K, V, sensitivity): a background cache of T rows with the named construction planted, and how far (relative L2) the float64 truth moves when the
    planted row (a whole first or last slice for 'all keys equal') is removed"""
    hd = q.shape[1]
    K, V = background(rng, T, nkv, hd, act)
    lo = T - window if 0 < window < T else 0
    if name.startswith("dominant"):
        K[rows[0]], V[rows[0]] = key_with_score(q, nkv, 16.0, act), pattern(rows[0] % 5, nkv, hd, act)
        drops = [rows]
    elif name.startswith("two equal"):
        k = key_with_score(q, nkv, 16.0, act)
        K[rows[0]], K[rows[1]] = k, k
        V[rows[0]], V[rows[1]] = pattern(1, nkv, hd, act), pattern(2, nkv, hd, act)
        drops = [[rows[0]], [rows[1]]]
    elif name.startswith("margin"):
        K[rows[0]], V[rows[0]] = key_with_score(q, nkv, 120.0, act), pattern(3, nkv, hd, act)
        drops = [rows]
    else:                                       # all keys equal: uniform weights; the first and the last slice carry V patterns of their own with equal totals
        wl = T - lo
        spl = slice_len(wl)
        sl = (np.arange(lo, T) - lo) // spl
        first, last = sl == 0, sl == sl[-1]
        K[:] = 0.0
        w = np.where(first, 16.0, np.where(last, min(16.0 * spl / last.sum(), 2048.0), 0.0)).astype(np.float32)
        pat = np.where(first[:, None, None], pattern(5, nkv, hd, act)[None], pattern(6, nkv, hd, act)[None])
        V[lo:] = orc_py.round_act(V[lo:] * 0.25 + w[:, None, None] * pat, act)
        drops = [list(lo + np.nonzero(first)[0]), list(lo + np.nonzero(last)[0])]
    base = truth(q, K, V, window)
    sens = min(rel(truth(q, K, V, window, d), base) for d in drops)
    return K, V, sens
