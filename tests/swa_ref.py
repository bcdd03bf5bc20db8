"""Sliding-window attention references: npref's two numpy forwards with the window mask added.

A window of W keys means the query at position p attends to positions max(0, p - W + 1) .. p (HF Mistral: W keys including itself).
`pattern` n > 1 makes every n-th layer (l % n == n - 1) global and the others windowed (Gemma2: 2); 0 / 1 windows every layer.  The CPU
oracle has no window, so these stand where it stands elsewhere: SwaLlama restates npref.NpLlama.step (its arithmetic and rounding points: the oracle's),
SwaTruth restates npref.NpLlamaTruth.step -- float64, no rounding anywhere -- each with the cached rows sliced to the window.  Both take the window
from the model's config unless one is given; tests/test_swa.py holds them to their base classes bit for bit when W >= context.
"""
import numpy as np

import npref


def layer_window(window, pattern, layer):
    if not window or window <= 0:
        return 0
    return 0 if (pattern and pattern > 1 and layer % pattern == pattern - 1) else int(window)


def first_key(pos, window):
    """first position the query at `pos` attends to"""
    return max(0, pos + 1 - window) if window > 0 else 0


def _windows(model, window, pattern):
    cfg = model["config"]
    w = cfg.get("sliding_window", 0) if window is None else window
    p = cfg.get("sliding_window_pattern", 0) if pattern is None else pattern
    return [layer_window(w, p, l) for l in range(len(model["layers"]))]


class SwaLlama(npref.NpLlama):
    """npref.NpLlama.step restated with the rows of each layer's window sliced out explicitly (same operations, same rounding points, same order)"""

    def __init__(self, model, window=None, pattern=None):
        super().__init__(model)
        self.win = _windows(model, window, pattern)

    def step(self, token, pos):
        c = self.cfg
        act = c["act_dtype"]
        R = lambda a: npref.round_act(a, act)
        nq, nkv, hd = c["n_heads"], c["n_kv_heads"], c["head_dim"]
        h = R(self.emb[token])
        prev = None
        for l, lay in enumerate(self.m["layers"]):
            if prev is not None:
                h = R(h + prev)
            xn = npref.rms_norm(h, lay["attn_norm"], c["rms_eps"], act)
            q = R(self._lin(l, "q", xn)).reshape(nq, hd)
            k = R(self._lin(l, "k", xn)).reshape(nkv, hd)
            v = R(self._lin(l, "v", xn)).reshape(nkv, hd)
            q = R(npref.rope(q, self.cos[pos], self.sin[pos], c["rope_interleaved"]))
            k = R(npref.rope(k, self.cos[pos], self.sin[pos], c["rope_interleaved"]))
            self.K[l].append(k)
            self.V[l].append(v)
            assert len(self.K[l]) == pos + 1, "steps must run in order from position 0"
            lo = first_key(pos, self.win[l])
            Kc = np.stack(self.K[l][lo:], axis=1)  # [nkv, T - lo, hd]
            Vc = np.stack(self.V[l][lo:], axis=1)
            rep = nq // nkv
            o = np.empty((nq, hd), dtype=np.float32)
            for hh in range(nq):
                s = (Kc[hh // rep] @ q[hh]) * np.float32(1.0 / np.sqrt(hd))
                p = np.exp(s - s.max())
                o[hh] = (p / p.sum()) @ Vc[hh // rep]
            o = R(o.reshape(-1))
            h = R(h + R(self._lin(l, "o", o)))
            xn = npref.rms_norm(h, lay["ffn_norm"], c["rms_eps"], act)
            g = R(self._lin(l, "gate", xn))
            u = R(self._lin(l, "up", xn))
            a = R(R(g / (1.0 + np.exp(-g))) * u)
            prev = R(self._lin(l, "down", a))
        h = R(h + prev)
        xn = npref.rms_norm(h, self.m["final_norm"], c["rms_eps"], act)
        return R(xn @ self.lm.T)


class SwaTruth(npref.NpLlamaTruth):
    """npref.NpLlamaTruth.step (float64, no rounding) with the window sliced out explicitly"""

    def __init__(self, model, window=None, pattern=None):
        super().__init__(model)
        self.win = _windows(model, window, pattern)

    def step(self, token, pos):
        c = self.cfg
        nq, nkv, hd = c["n_heads"], c["n_kv_heads"], c["head_dim"]
        h = self.emb[token].astype(np.float64)
        for l, lay in enumerate(self.m["layers"]):
            xn = self._norm(h, lay["attn_norm"], c["rms_eps"])
            q = npref.rope(self._lin(l, "q", xn).reshape(nq, hd), self.cos[pos], self.sin[pos], c["rope_interleaved"])
            k = npref.rope(self._lin(l, "k", xn).reshape(nkv, hd), self.cos[pos], self.sin[pos], c["rope_interleaved"])
            v = self._lin(l, "v", xn).reshape(nkv, hd)
            self.K[l].append(k)
            self.V[l].append(v)
            assert len(self.K[l]) == pos + 1, "steps must run in order from position 0"
            lo = first_key(pos, self.win[l])
            Kc, Vc = np.stack(self.K[l][lo:], axis=1), np.stack(self.V[l][lo:], axis=1)
            rep = nq // nkv
            o = np.empty((nq, hd), dtype=np.float64)
            for hh in range(nq):
                s = (Kc[hh // rep] @ q[hh]) / np.sqrt(hd)
                p = np.exp(s - s.max())
                o[hh] = (p / p.sum()) @ Vc[hh // rep]
            h = h + self._lin(l, "o", o.reshape(-1))
            xn = self._norm(h, lay["ffn_norm"], c["rms_eps"])
            g, u = self._lin(l, "gate", xn), self._lin(l, "up", xn)
            h = h + self._lin(l, "down", (g / (1.0 + np.exp(-g))) * u)
        return self.lm @ self._norm(h, self.m["final_norm"], c["rms_eps"])


def run(ref, tokens):
    """logits [len(tokens), vocab] of a token-by-token run from position 0"""
    return np.stack([np.asarray(ref.step(int(t), i)).reshape(-1) for i, t in enumerate(tokens)])


def attn_decode(q, K, V, window):
    """float64 softmax attention of one query per head over the last `window` rows (all rows for window 0): q [nq, hd], K / V [T, nkv, hd]"""
    q, K, V = np.asarray(q, np.float64), np.asarray(K, np.float64), np.asarray(V, np.float64)
    T, nkv, hd = K.shape
    lo = first_key(T - 1, window)
    rep = q.shape[0] // nkv
    out = np.empty_like(q)
    for h in range(q.shape[0]):
        s = K[lo:, h // rep] @ q[h] / np.sqrt(hd)
        p = np.exp(s - s.max())
        out[h] = (p / p.sum()) @ V[lo:, h // rep]
    return out
