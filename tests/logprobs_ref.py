"""numpy restatement of the device logprobs and logit bias of the batched sampler (include/blazr_hip.h: bz_batch_sampler_enable and what follows it;
blazr_amd/csrc/bz_logprobs.hip), plus the rows the GPU tests use (shared, so the CPU test checks them against the host routines first).

Per row x (the raw logits):  M = max x;  e_i = bz_expf(x_i - M) (the library's specified exp, through bz_expf_spec);  q_i = floor(e_i * 2^40) as an integer;
S = sum q_i (exact);  lse = f32(f32(log(S * 2^-40)) + M);  logprob_i = f32(x_i - lse);  top = the first min(top_n, V, 20) ids by (x descending, id ascending).
The only step that depends on the platform is the double log, rounded to f32 on either side: lse may differ by one f32 ulp between two machines."""
import ctypes as C

import numpy as np

from blazr_amd import _lib as L

F = np.float32
TOP_MAX, BIAS_MAX = 20, 512
TOP_NS = (-1, 0, 1, 5, 20)


def expf(x):
    x = np.ascontiguousarray(x, dtype=F)
    y = np.empty_like(x)
    L.check(L.lib().bz_expf_spec(x.ctypes.data_as(C.c_void_p), x.size, y.ctypes.data_as(C.c_void_p)))
    return y


def lse_parts(x):
    """(M, S, L, lse) of one row"""
    x = np.asarray(x, dtype=F)
    M = F(np.max(x))
    with np.errstate(all="ignore"):
        e = expf((x - M).astype(F))
        q = np.where(e > 0, np.floor(e.astype(np.float64) * 2.0 ** 40), 0.0)
    S = int(q.astype(np.uint64).sum(dtype=np.uint64))
    with np.errstate(all="ignore"):
        Lg = F(np.log(np.float64(S) * 2.0 ** -40))
    return M, S, Lg, F(Lg + M)


def order(x, n):
    """the first n ids by (logit descending, id ascending); NaN logits are never listed"""
    x = np.asarray(x, dtype=F)
    ids = np.nonzero(~np.isnan(x))[0]
    with np.errstate(all="ignore"):
        key = -(x[ids] + F(0))                       # -0 orders as +0
    return ids[np.argsort(key, kind="stable")][:max(n, 0)].astype(np.int64)


def logprobs_row(x, top_n, lse=None):
    """dict(lse, n_top, top_ids, top_logprobs) of one row with top_n >= 0; lse: use this one (the device's) for the values instead of the reference's"""
    x = np.asarray(x, dtype=F)
    ref_lse = lse_parts(x)[3]
    use = ref_lse if lse is None else F(lse)
    ids = order(x, min(top_n, len(x), TOP_MAX))
    with np.errstate(all="ignore"):
        lps = (x[ids] - use).astype(F)
    return dict(lse=ref_lse, n_top=len(ids), top_ids=ids, top_logprobs=lps)


def order_is_decided(x, lse, n):
    """True when, among the first n + 1 entries, distinct logits give distinct f32 logprobs under `lse`: then sorting by logprob (the reference's
    compute_logprobs) and sorting by logit agree"""
    x = np.asarray(x, dtype=F)
    ids = order(x, min(n + 1, len(x)))
    xs = x[ids]
    with np.errstate(all="ignore"):
        lp = (xs - F(lse)).astype(F)
    return all(lp[i] != lp[i + 1] for i in range(len(ids) - 1) if xs[i] != xs[i + 1])


def log_softmax64(x):
    x = np.asarray(x, dtype=np.float64)
    m = np.max(x)
    with np.errstate(all="ignore"):
        return x - (m + np.log(np.sum(np.exp(x - m))))


def ulp(v):
    v = abs(F(v))
    return float(np.spacing(v)) if np.isfinite(v) else 0.0


def value_bound(x, lp):
    """Largest |logprob - float64 log-softmax| the arithmetic above allows for a finite logprob `lp` of row x.  bz_expf is within 1 ulp (2^-23 relative) of exp, so
    S * 2^-40 is within 2^-23 relative plus V * 2^-40 absolute of the true sum (>= 1); the log carries that as an absolute error; then three f32 roundings:
    of L, of L + M, of x - lse (half an ulp of each result), and the double log's own last bit (below 2^-50)."""
    M, S, Lg, lse = lse_parts(x)
    return 2.0 ** -23 + len(x) * 2.0 ** -40 + 2.0 ** -50 + 0.5 * ulp(Lg) + 0.5 * ulp(lse) + 0.5 * ulp(lp)


# ---- logit bias -----------------------------------------------------------------------------------------------------------------------------
def dedupe(V, ids, vals):
    """sampling.rs:470-476 as a sparse list: later entries of an id overwrite earlier ones, ids >= V find no place -> (ids, vals), first-occurrence order"""
    at, oi, ov = {}, [], []
    for i, v in zip(ids, vals):
        if int(i) >= V:
            continue
        if int(i) in at:
            ov[at[int(i)]] = F(v)
        else:
            at[int(i)] = len(oi); oi.append(int(i)); ov.append(F(v))
    return np.asarray(oi, dtype=np.uint32), np.asarray(ov, dtype=F)


def apply_bias(x, ids, vals):
    """the row after the device's bias launch: every entry of the deduplicated list added once"""
    y = np.array(x, dtype=F, copy=True)
    di, dv = dedupe(len(y), ids, vals)
    with np.errstate(all="ignore"):
        for i, v in zip(di, dv):
            y[i] = F(y[i] + v)
    return y


def host_apply_bias(x, ids, vals):
    """bz_apply_logit_bias on a copy of the row"""
    y = np.array(x, dtype=F, copy=True)
    i = np.ascontiguousarray(ids, dtype=np.uint32); v = np.ascontiguousarray(vals, dtype=F)
    L.check(L.lib().bz_apply_logit_bias(y.ctypes.data_as(C.c_void_p), len(y), i.ctypes.data_as(C.c_void_p) if len(i) else None,
                                        v.ctypes.data_as(C.c_void_p) if len(v) else None, len(i)))
    return y


def host_logprobs(x, chosen, top_n):
    """bz_compute_logprobs -> (chosen logprob, ids, logprobs)"""
    x = np.ascontiguousarray(x, dtype=F)
    clp, n = C.c_float(), C.c_int()
    tid, tlp = np.zeros(TOP_MAX, np.uint32), np.zeros(TOP_MAX, F)
    L.check(L.lib().bz_compute_logprobs(x.ctypes.data_as(C.c_void_p), len(x), int(chosen), int(top_n), C.byref(clp), tid.ctypes.data_as(C.c_void_p),
                                        tlp.ctypes.data_as(C.c_void_p), C.byref(n)))
    return F(clp.value), tid[:n.value].astype(np.int64), tlp[:n.value]


# ---- the rows of the GPU tests ------------------------------------------------------------------------------------------------------------------
ROW_KINDS = ("random", "all_equal", "block_ties", "neg_inf", "dominant", "wide")


def tie_ids(V):
    """ids on both sides of the boundaries between the workgroups' slices (256 ids each, 128 slices per pass) and the last id"""
    return sorted({i for i in (3, 255, 256, 511, 512, 32767, 32768, 32769, V - 1) if i < V})


def make_rows(V, seed=0):
    """[6, V] float32, one row per ROW_KINDS"""
    rng = np.random.default_rng(1000 + V + seed)
    x = np.empty((len(ROW_KINDS), V), dtype=F)
    x[0] = (rng.standard_normal(V) * 2.5).astype(F)
    x[1] = F(1.25)
    x[2] = (rng.standard_normal(V) * 1.5).astype(F)
    x[2, tie_ids(V)] = F(np.max(x[2]) + F(0.5))                    # exact ties at the top, spread over the slices
    if V > 40:
        x[2, rng.choice(V, size=30, replace=False)] = F(-0.75)     # and a plateau further down
    x[3] = (rng.standard_normal(V) * 2.0).astype(F)
    x[3, rng.random(V) < 0.6] = -np.inf
    x[3, V // 2] = F(0.5)                                           # at least one finite entry
    x[4] = (rng.standard_normal(V) * 1.0).astype(F)
    x[4, V // 3] = F(140.0)                                         # every other q_i is 0
    x[5] = (rng.standard_normal(V) * 9.0).astype(F)
    return x
