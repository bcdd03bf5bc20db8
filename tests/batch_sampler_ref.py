"""numpy restatement of the per-row semantics of the batched sampler (include/blazr_hip.h: bz_batch_sampler_*), i.e. of
oracle/orc_ops.c::orc_logits_to_token applied to one row with ids / cnts = penalty_window(history, repeat_last_n) and seed = seed + draw_index --
plus the DECISION MARGIN of a case, and the cases the GPU tests use (shared, so the CPU test can check them against the oracle first).

The margin is the smallest of |cum - top_p| at the top-p cut index and at its predecessor, and |u - cum| at the drawn index and at its predecessor,
in float64 over the sorted p.  Two implementations that hold the same p_i bits can only disagree on a case whose margin is below the difference of
their cumulative sums (<= V * 2^-53 ~ 1.4e-11 at V = 128 k)."""
import numpy as np

MARGIN = 1e-6
PENALTIES = dict(repeat_penalty=1.1, frequency_penalty=0.1, presence_penalty=0.05, repeat_last_n=64)
# the five sets of test_gpu_ops.py::test_logits_to_token_sampling_matches_oracle, the three degenerate filters, a greedy row
PSETS = [dict(temperature=1.0, top_k=0, top_p=1.0, min_p=0.0), dict(temperature=0.7, top_k=40, top_p=0.9, min_p=0.05),
         dict(temperature=1.3, top_k=0, top_p=0.8, min_p=0.0), dict(temperature=0.5, top_k=5, top_p=1.0, min_p=0.0),
         dict(temperature=1.0, top_k=0, top_p=1.0, min_p=0.2), dict(temperature=0.9, top_k=1, top_p=1.0, min_p=0.0),
         dict(temperature=0.9, top_k=0, top_p=1e-6, min_p=0.0), dict(temperature=0.9, top_k=0, top_p=1.0, min_p=1.0),
         dict(temperature=0.0, top_k=0, top_p=1.0, min_p=0.0)]
F = np.float32


def expf_spec(x):
    """bz_expf / orc_expf: Cephes expf as one fixed sequence of f32 operations."""
    x = np.asarray(x, dtype=F)
    with np.errstate(all="ignore"):
        n = np.rint(x * F(1.44269504088896341)).astype(F)
        n = np.where(np.isfinite(n), n, F(0))
        r = (n.astype(np.float64) * np.float64(F(-0.693145751953125)) + x.astype(np.float64)).astype(F)
        r = (n.astype(np.float64) * np.float64(F(-1.42860682030941723212e-6)) + r.astype(np.float64)).astype(F)
        p = np.full_like(r, F(1.9875691500e-4))
        for c in (1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1):
            p = (p.astype(np.float64) * r.astype(np.float64) + np.float64(F(c))).astype(F)
        r2 = (r * r).astype(F)
        y = (p.astype(np.float64) * r2.astype(np.float64) + r.astype(np.float64)).astype(F)
        y = (y + F(1.0)).astype(F)
        sc = ((np.clip(n, -125, 127).astype(np.int32) + 127).astype(np.uint32) << np.uint32(23)).view(F)
        out = (y * sc).astype(F)
    out = np.where(x < F(-86.0), F(0), out)
    out = np.where(x > F(88.0), F(np.inf), out)
    return np.where(np.isnan(x), x, out).astype(F)


def penalty_window(history, repeat_last_n):
    """sampling.rs:169-191: unique ids + counts over the last repeat_last_n tokens (runtime.penalty_window restated)."""
    h = list(history)
    w = h[-repeat_last_n:] if 0 < repeat_last_n < len(h) else h
    ids, cnts = [], []
    for t in w:
        if t in ids:
            cnts[ids.index(t)] += 1
        else:
            ids.append(int(t)); cnts.append(1)
    return np.asarray(ids, dtype=np.int64), np.asarray(cnts, dtype=np.int32)


def penalties_active(p):
    return p.get("repeat_penalty", 1.0) != 1.0 or p.get("frequency_penalty", 0.0) != 0.0 or p.get("presence_penalty", 0.0) != 0.0


def splitmix_unit(seed):
    m = (1 << 64) - 1
    z = (seed + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    z = z ^ (z >> 31)
    return float(z >> 11) * (1.0 / 9007199254740992.0)


def sample_row(logits, history=(), draw_index=0, temperature=0.0, top_k=0, top_p=1.0, min_p=0.0, repeat_penalty=1.0, frequency_penalty=0.0,
               presence_penalty=0.0, repeat_last_n=64, seed=0):
    """-> (token, margin) of one row."""
    l = np.array(logits, dtype=F)
    V = len(l)
    p_ = dict(repeat_penalty=repeat_penalty, frequency_penalty=frequency_penalty, presence_penalty=presence_penalty)
    ids, cnts = penalty_window(history, repeat_last_n) if penalties_active(p_) else ((), ())
    rp, fp, pp = F(repeat_penalty), F(frequency_penalty), F(presence_penalty)
    for i, c in zip(ids, cnts):
        if i < 0 or i >= V:
            continue
        x = l[i]
        if rp != F(1.0):
            x = F(x / rp) if x > 0 else F(x * rp)
        l[i] = F(x - F(F(fp * F(c)) + pp))
    if temperature == 0.0:
        return int(np.argmax(l)), float("inf")        # first maximum
    with np.errstate(all="ignore"):
        l = (l / F(temperature)).astype(F)
        m = l.max() if not np.all(np.isnan(l)) else F(-np.inf)
        e = expf_spec(l - m)
        total = np.cumsum(e.astype(np.float64))[-1]   # sequential, as the oracle's loop
        p = (e.astype(np.float64) / total).astype(F)
    if not np.all(np.isfinite(p)):
        return -1, 0.0                                # a row without mass: any id in range is acceptable
    order = np.lexsort((np.arange(V), -p.astype(np.float64)))
    ps = p[order].astype(np.float64)
    cum = np.cumsum(ps)
    keep = top_k if 0 < top_k < V else V
    margin = float("inf")
    if 0.0 < top_p < 1.0:
        tp = float(F(top_p))
        hit = np.nonzero(cum[:keep] >= tp)[0]
        i = int(hit[0]) if len(hit) else None
        if i is not None:
            margin = min(margin, abs(cum[i] - tp))
            if i > 0:
                margin = min(margin, abs(cum[i - 1] - tp))
            if i + 1 < keep:
                keep = i + 1
    if min_p > 0.0:
        thr = F(ps[0].astype(F) * F(min_p))
        below = np.nonzero(p[order][1:keep] < thr)[0]
        keep = 1 + int(below[0]) if len(below) else keep
    tot = cum[keep - 1]
    u = splitmix_unit((seed + draw_index) & ((1 << 64) - 1)) * tot
    hit = np.nonzero(u < cum[:keep])[0]
    i = int(hit[0]) if len(hit) else keep - 1
    margin = min(margin, abs(u - cum[i]))
    if i > 0:
        margin = min(margin, abs(u - cum[i - 1]))
    return int(order[i]), float(margin)


# ---- the cases of tests/test_gpu_batch_sampler.py ---------------------------------------------------------------------------------------------------
def make_case(N, V, case_seed):
    """One batch: logits [N, V], per-row keyword arguments of sample_row / BatchSampler.set_row.  The nine parameter sets are mixed over the rows."""
    rng = np.random.default_rng(1000 + case_seed)
    logits = (rng.standard_normal((N, V)) * 2.5).astype(F)
    rows = []
    for r in range(N):
        kw = dict(PSETS[(r + case_seed) % len(PSETS)])
        kw.update(PENALTIES)
        kw["seed"] = 7919 * case_seed + 31 * r + SEED_SHIFT.get((N, V, r), 0)
        kw["history"] = [5 % V, 5 % V, 9 % V, V - 1, int(rng.integers(0, V))]
        kw["draw_index"] = r % 3
        rows.append(kw)
    return logits, rows


# (N, V, row) -> seed offset: a seed whose case falls below MARGIN is replaced (tests/test_batch_sampler.py checks that none is left)
SEED_SHIFT = {(64, 32000, 7): 1}

GRID = [(N, V) for V in (1, 255, 257, 1003, 32000) for N in (1, 2, 7, 64)] + [(8, 128256), (512, 1003)]
GRID += [(207, 257)]        # 23 more rows per parameter set: with it every set has 121 (row, seed) pairs, the unit of the oracle bar


def case_id(N, V):
    return 100 * GRID.index((N, V)) + 1


def oracle_row(row_logits, kw):
    """orc_logits_to_token for one row of a case."""
    import ctypes as C
    from oracle import orc_py
    ids, cnts = penalty_window(kw["history"], kw["repeat_last_n"]) if penalties_active(kw) else (np.zeros(0, np.int64), np.zeros(0, np.int32))
    row = np.ascontiguousarray(row_logits, dtype=F)
    return int(orc_py.lib().orc_logits_to_token(row.ctypes.data_as(C.c_void_p), len(row), ids.ctypes.data_as(C.c_void_p), cnts.ctypes.data_as(C.c_void_p), len(ids),
                                                kw["repeat_penalty"], kw["frequency_penalty"], kw["presence_penalty"], kw["temperature"], kw["top_k"], kw["top_p"],
                                                kw["min_p"], (kw["seed"] + kw["draw_index"]) & ((1 << 64) - 1)))


def degenerate_cases():
    """name -> (logits [N, V], rows): ties and rows without mass.  Every row is drawn with several seeds (one row per seed)."""
    rng = np.random.default_rng(77)
    out = {}
    nseed = 12
    def rows_of(base, **kw):
        rows = []
        for s in range(nseed):
            r = dict(temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, repeat_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0, repeat_last_n=64,
                     history=[], draw_index=0, seed=1234 + 17 * s)
            r.update(kw)
            rows.append(r)
        return np.repeat(np.asarray(base, dtype=F)[None, :], nseed, axis=0), rows
    V = 3001                                               # more equal values than any one bin of a short list could hold
    out["all_equal"] = rows_of(np.full(V, 0.25))
    out["all_equal_top_p"] = rows_of(np.full(V, -3.0), top_p=0.37)
    out["all_equal_top_k"] = rows_of(np.full(V, 1.5), top_k=700, temperature=0.8)
    tie = (rng.standard_normal(V) * 0.5).astype(F)
    tie[[40, 7, 2900, 1500, 333, 12]] = 4.0                # six equal values behind two leaders
    tie[[100, 2000]] = 5.0
    out["ties_straddle_top_k"] = rows_of(tie, top_k=6)     # the two 5.0s and four of the six 4.0s, by ascending id
    masked = (rng.standard_normal(V) * 2.0).astype(F)
    masked[rng.permutation(V)[: (9 * V) // 10]] = -np.inf  # a grammar mask
    out["masked_90"] = rows_of(masked, temperature=1.2, top_p=0.95)
    out["all_neg_inf"] = rows_of(np.full(V, -np.inf))
    out["top_k_above_v"] = rows_of((rng.standard_normal(V) * 2.0).astype(F), top_k=V + 50, top_p=0.9)
    return out
