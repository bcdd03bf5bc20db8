"""numpy restatement of prompt scoring and pooling (include/blazr_hip.h: bz_score_* / bz_embed_*; blazr_amd/csrc/bz_score.hip), plus the rows and shapes the GPU
tests use (shared, so the CPU test checks them against the host routines first).

A row's record: the lse and the top list are logprobs_ref.py's (lse_parts / order); new here is the target's raw logit and its rank = #{x_j > x_t} + #{x_j == x_t, j < t}
(0-based; -0 ties with +0; a NaN logit is never counted; -1 when the target's logit is NaN).  A row with target -1 is not scored: rank = n_top = -1, the rest 0.
Pooling: mean = the SEQUENTIAL float64 sum of the rows (np.cumsum(...)[-1]; np.sum adds pairwise) / S, rounded to f32 once; normalize = v / sqrt(sum v^2) in float64,
rounded once, if the norm exceeds 1e-12."""
import numpy as np

import logprobs_ref as LR

F = np.float32
VS = (1, 255, 1003, 33025)           # 33025: the smallest row that takes a block's stride loop twice (128 x 256 = 32768)
TOP_NS = (0, 1, 20)
POOL_S, POOL_H = (1, 2, 257), (8, 256, 4104)
POOLINGS = ("none", "mean", "cls", "last")


def rank_of(x, t):
    x = np.asarray(x, dtype=F)
    xt = x[t]
    if np.isnan(xt):
        return -1
    with np.errstate(all="ignore"):
        return int(np.count_nonzero(x > xt) + np.count_nonzero(x[:t] == xt))      # NaN compares false both times; -0 == +0


def make_rows(V, seed=0):
    """[5, V] float32: random normal, all equal, -inf entries with +-0 ties, a dominant entry, wide random.  No NaN: every row's lse is compared."""
    rng = np.random.default_rng(7000 + V + seed)
    x = np.empty((5, V), dtype=F)
    x[0] = (rng.standard_normal(V) * 2.5).astype(F)
    x[1] = F(-0.375)
    x[2] = (rng.standard_normal(V) * 2.0).astype(F)
    x[2, rng.random(V) < 0.5] = -np.inf
    z = np.nonzero(rng.random(V) < 0.3)[0]
    x[2, z] = np.where(np.arange(len(z)) % 2 == 0, F(0.0), F(-0.0))     # +0 and -0 alternate: they tie, the id decides
    x[2, V // 2] = F(0.5)                                                # at least one finite entry
    x[3] = (rng.standard_normal(V) * 1.0).astype(F)
    x[3, V // 3] = F(140.0)                                              # every other q_i is 0
    x[4] = (rng.standard_normal(V) * 9.0).astype(F)
    return x


def nan_row(V, seed=0):
    """a row with NaN entries, for the rank and the top list only (lse_parts takes np.max)"""
    rng = np.random.default_rng(7100 + V + seed)
    x = (rng.standard_normal(V) * 2.0).astype(F)
    x[rng.random(V) < 0.25] = np.nan
    x[0] = np.nan
    x[V - 1] = F(0.25)
    return x


def targets_for(V):
    return sorted({0, V - 1, -1, V // 2})


def check_record(rec, x, t, top_n, where=""):
    """one SCORE_ROW record against numpy: lse within one f32 ulp of numpy's (the double log), everything else exact, the values from the lse as returned"""
    x = np.asarray(x, dtype=F)
    assert int(rec["target"]) == t, where
    if t < 0:
        assert int(rec["rank"]) == -1 and int(rec["n_top"]) == -1 and rec["logprob"] == 0 and rec["lse"] == 0 and rec["logit"] == 0, (where, rec)
        return
    lse = F(rec["lse"])
    if not np.isnan(x).any():
        ref = LR.lse_parts(x)[3]
        assert lse == ref or abs(float(lse) - float(ref)) <= LR.ulp(ref), (where, lse, ref)
    assert np.array_equal(F(rec["logit"]), x[t], equal_nan=True), (where, rec["logit"], x[t])
    with np.errstate(all="ignore"):
        assert np.array_equal(F(rec["logprob"]), F(x[t] - lse), equal_nan=True), (where, rec["logprob"], F(x[t] - lse))
    assert int(rec["rank"]) == rank_of(x, t), (where, int(rec["rank"]), rank_of(x, t))
    ids = LR.order(x, min(top_n, len(x), LR.TOP_MAX))
    n = int(rec["n_top"])
    assert n == len(ids), (where, n, len(ids))
    assert np.array_equal(rec["top_ids"][:n].astype(np.int64), ids), (where, rec["top_ids"][:n], ids)
    with np.errstate(all="ignore"):
        assert np.array_equal(rec["top_logprobs"][:n], (x[ids] - lse).astype(F), equal_nan=True), where
    assert not rec["top_ids"][n:].any() and not rec["top_logprobs"][n:].any(), where


def records_equal(a, b, where=""):
    """two SCORE_ROW records of the same row: bit for bit except the lse, which may differ by one f32 ulp between two evaluations of the double log -- and then the values
    that subtract it follow their own lse"""
    assert int(a["target"]) == int(b["target"]) and int(a["rank"]) == int(b["rank"]) and int(a["n_top"]) == int(b["n_top"]), (where, a, b)
    assert np.array_equal(a["logit"], b["logit"], equal_nan=True) and np.array_equal(a["top_ids"], b["top_ids"]), (where, a, b)
    la, lb = F(a["lse"]), F(b["lse"])
    if la.tobytes() == lb.tobytes() or (np.isnan(la) and np.isnan(lb)):
        assert np.array_equal(a["logprob"], b["logprob"], equal_nan=True) and np.array_equal(a["top_logprobs"], b["top_logprobs"], equal_nan=True), (where, a, b)
    else:
        assert abs(float(la) - float(lb)) <= LR.ulp(lb), (where, la, lb)


def pool(hidden, pooling, normalize=False):
    h = np.asarray(hidden, dtype=F)
    S = h.shape[0]
    if pooling == "none":
        v = h.copy()
    elif pooling == "cls":
        v = h[0].copy()
    elif pooling == "last":
        v = h[S - 1].copy()
    else:
        v = (np.cumsum(h.astype(np.float64), axis=0)[-1] / np.float64(S)).astype(F)
    if normalize:
        v2 = np.atleast_2d(v).astype(np.float64)
        norm = np.sqrt(np.cumsum(v2 * v2, axis=1)[:, -1])
        keep = norm > 1e-12
        with np.errstate(all="ignore"):
            out = np.where(keep[:, None], v2 / np.where(keep, norm, 1.0)[:, None], v2).astype(F)
        v = out.reshape(v.shape)
    return v


def pool_rows_case(S, H, seed=0):
    rng = np.random.default_rng(7200 + 31 * S + H + seed)
    h = (rng.standard_normal((S, H)) * 3.0).astype(F)
    h[:, 0] *= F(1e4)                    # a column whose sum loses bits in f32
    if S > 1:
        h[1] = 0                         # a zero row: normalize leaves it as it is
    return h


def within_ulp(a, b, n=1):
    a, b = np.asarray(a, dtype=F), np.asarray(b, dtype=F)
    return bool(np.all(np.abs(a.astype(np.float64) - b.astype(np.float64)) <= n * np.spacing(np.abs(b)).astype(np.float64)))


def cosine64(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(a @ b / (np.sqrt(a @ a) * np.sqrt(b @ b)))
