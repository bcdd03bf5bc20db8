"""An independent restatement of the packed prompt batch: which path it takes (on prompt_plan_ref.plan), the default targets and per-input totals of a scoring
call, and float64 segment-masked attention.  Plain numpy -- no library, no device."""
import numpy as np

import prompt_plan_ref as R


class Refused(Exception):
    pass


def check_lens(lens):
    if len(lens) <= 0:
        raise Refused("n_seq = %d" % len(lens))
    for i, n in enumerate(lens):
        if n <= 0:
            raise Refused("seq_lens[%d] = %d" % (i, n))
    if int(np.sum(np.asarray(lens, dtype=np.int64))) >= 2 ** 31:
        raise Refused("2^31")


def plan(t, sw, lens, kv_dtype):
    """packed = 1 exactly when the prompt plan of T rows at a context of the longest input is ROWS; else the plan of the longest input alone"""
    check_lens(lens)
    T, max_len = int(np.sum(lens)), int(max(lens))
    p = R.plan(t, sw, R.PROMPT, T, max_len, kv_dtype)
    packed = 1 if p["route"] == R.ROWS else 0
    if not packed:
        p = R.plan(t, sw, R.PROMPT, max_len, max_len, kv_dtype)
    return dict(packed=packed, rows=T, n_seq=len(lens), max_len=max_len, plan=p)


def default_targets(tokens, lens):
    """row r reads the next token of its own input; an input's last row is not scored"""
    tokens = np.asarray(tokens, dtype=np.int64)
    out = np.empty_like(tokens)
    o = 0
    for n in lens:
        out[o:o + n - 1] = tokens[o + 1:o + n]
        out[o + n - 1] = -1
        o += n
    return out


def totals(logprob, n_top, lens):
    """per input: (sum of the finite logprobs of its scored rows as a double running sum in row order, their count)"""
    res, o = [], 0
    for n in lens:
        s, k = 0.0, 0
        for r in range(o, o + n):
            if n_top[r] >= 0 and np.isfinite(logprob[r]):
                s += float(np.float64(logprob[r]))
                k += 1
        res.append((s, k))
        o += n
    return res


def seg_lo(lens):
    return np.repeat(np.concatenate([[0], np.cumsum(lens)[:-1]]), lens).astype(np.int64)


def attention(qkv, lens, nq, nkv, hd, window=0):
    """float64 attention of packed rows [T, (nq + 2 nkv) hd]: query i sees the keys of its own input at packed rows max(seg_lo[i], i - window + 1) .. i"""
    x = np.asarray(qkv, dtype=np.float64)
    T, rep = x.shape[0], nq // nkv
    q = x[:, :nq * hd].reshape(T, nq, hd)
    k = x[:, nq * hd:(nq + nkv) * hd].reshape(T, nkv, hd)
    v = x[:, (nq + nkv) * hd:].reshape(T, nkv, hd)
    lo = seg_lo(lens)
    if window > 0:
        lo = np.maximum(lo, np.arange(T) - window + 1)
    out = np.zeros((T, nq, hd))
    scale = 1.0 / np.sqrt(np.float64(hd))
    o = 0
    for n in lens:                                              # one input at a time: its rows only
        rows = np.arange(o, o + n)
        mask = (rows[None, :] <= rows[:, None]) & (rows[None, :] >= lo[rows][:, None])
        for h in range(nq):
            s = (q[rows, h] @ k[rows, h // rep].T) * scale
            s = np.where(mask, s, -np.inf)
            p = np.exp(s - s.max(axis=1, keepdims=True))
            out[rows, h] = (p / p.sum(axis=1, keepdims=True)) @ v[rows, h // rep]
        o += n
    return out.reshape(T, nq * hd)
