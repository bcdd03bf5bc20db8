"""One-layer GPTQ models whose biases make the ORDER in which a linear adds its bias visible on the first token (data and numpy only, no GPU).

The oracle's linear is y = R(RN32(s) + b): the exact sum s rounded to f32 once, the bias added in f32, the result rounded to the activation dtype
(oracle/orc_quant.c).  A kernel that folds the bias into the exact sum computes R(RN32(s + b)) instead.  With ordinary biases the two agree except where
RN32(s)'s own error, at most half an f32 ulp of s, carries the result across a 16-bit rounding boundary: about one output in 10^5.  Here the biases are
built so that it happens in more than a third of the outputs of one chosen token T0 at position 0:

    b[n] = c[n] - RN32(s[n]),     c[n] = sign(s[n]) . (the midpoint above the f16 value nearest to |RN32(s[n])| / 4)

s[n] is computed exactly (integer arithmetic over (q - z), the f16 scale's and the f16 activation's integer significands; test_linear_bias.py checks it
against math.fsum).  c has the sign of RN32(s), at most its magnitude and no bits below its last one, so b is exact in f32 and RN32(s) + b == c exactly: the
oracle lands ON the midpoint and rounds to the even neighbour.  The folded order gives RN32(c + (s - RN32(s))): c sits two binades under s, so f32 resolves the
residue there, and the result leaves the midpoint on the residue's side -- for about half of the elements towards the odd neighbour.

Cases: the construction on one group of linears (`qkv`, `o`, `gate_up`, `down`; every other linear without a bias), and `all`: on every group, each
against the inputs the oracle produces with the groups before it already biased.  What each site shows itself in (position 0 of a one-layer model):
  qkv      the K and V rows of position 0: RoPE at position 0 is the identity, so the cache holds R(k), R(v) themselves.  q is computed by the same source line of
           every kernel and is biased the same way, but with one key the softmax is 1 whatever q is: q is not separately observable.
  o        attention over one key returns v exactly, so o_proj reads v repeated over its group; observable: `hidden` = R(h + R(o)) out of layers 0..1.
  gate_up  `prev_mlp`, through SiLU * up and the down sums.
  down     `prev_mlp` directly.
Inputs of the later linears come from the oracle's own pieces (orc_llama_embed, orc_rms_norm, orc_linear_forward, orc_silu), never from the library, and
test_linear_bias.py checks that the staged pipeline reproduces orc_llama_layers_range bit for bit.
"""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np

from blazr_amd import synth
from oracle import orc_py

WIDTHS = {
    "h2048": dict(hidden=2048, n_heads=16, n_kv_heads=4, inter=384),
    "h4096": dict(hidden=4096, n_heads=32, n_kv_heads=8, inter=384),
    # the multi-row int4 forms (k_gemm_q4g_rows, k_gemm_q4g_i8) take linears whose K is a multiple of 256: with inter 384 down_proj is not, and every prompt
    # and decode batch of the two widths above runs on the decode step.  Same model with inter 512: prompts and batches reach those forms.
    "h2048-i512": dict(hidden=2048, n_heads=16, n_kv_heads=4, inter=512),
}
ROWS_WIDTH = "h2048-i512"
SITES = ("qkv", "o", "gate_up", "down")
CASES = SITES + ("all",)
GROUPS = {"qkv": ("q", "k", "v"), "o": ("o",), "gate_up": ("gate", "up"), "down": ("down",)}
# what a site's bias order shows itself in (names of Case.want / Stage fields)
OBSERVABLE = {"qkv": ("k0", "v0"), "o": ("hidden",), "gate_up": ("prev_mlp",), "down": ("prev_mlp",)}
T0 = 3
ACT = "f16"


def make_model(width):
    """the bias-free one-layer GPTQ model of a width (no act-order)"""
    return synth.make_llama("llama3-8b-awq-2l", quant="gptq", n_layers=1, vocab=512, max_seq_len=64, **WIDTHS[width])


def _r16(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------
# exact sums
# ---------------------------------------------------------------------------------------------------------
def gptq_ints(spec):
    """(q - z) as int64 [K, N] and the f16 scales [G, N] of a GPTQ linear without act-order (AutoGPTQ v1: stored zero point + 1)"""
    K, N, gs = spec["K"], spec["N"], spec["group_size"]
    assert spec.get("g_idx") is None
    sh = 4 * np.arange(8, dtype=np.uint32)
    q = ((spec["qweight"].astype(np.uint32)[:, None, :] >> sh[None, :, None]) & 0xF).reshape(K, N).astype(np.int64)
    z = ((spec["qzeros"].astype(np.uint32)[:, :, None] >> sh[None, None, :]) & 0xF).reshape(K // gs, N).astype(np.int64) + 1
    return q - np.repeat(z, gs, axis=0), spec["scales"].astype(np.float16)


def exact_sums(spec, x):
    """sum_k x[k] (q[k, n] - z) s as exact Fractions, n = 0 .. N-1.  x and s are f16 values, i.e. integers times 2^-24: the sum over a group of
    (q - z) . (x 2^24) fits an int64 (2^5 . 2^7 . 2^31), the groups are joined in Python integers."""
    qz, sc = gptq_ints(spec)
    K, N, gs = spec["K"], spec["N"], spec["group_size"]
    x = np.asarray(x, dtype=np.float32).reshape(K)
    assert np.array_equal(_r16(x), x), "the activations must be f16 values"
    mx = np.rint(x.astype(np.float64) * 2.0 ** 24).astype(np.int64)
    assert np.array_equal(mx.astype(np.float64) * 2.0 ** -24, x.astype(np.float64)) and np.abs(mx).max() < 2 ** 31
    ms = np.rint(sc.astype(np.float64) * 2.0 ** 24).astype(np.int64)
    assert np.array_equal(ms.astype(np.float64) * 2.0 ** -24, sc.astype(np.float64))
    part = np.einsum("gkn,gk->gn", qz.reshape(K // gs, gs, N), mx.reshape(K // gs, gs))   # [G, N], exact
    tot = [sum(int(p) * int(m) for p, m in zip(part[:, n], ms[:, n])) for n in range(N)]
    return [Fraction(t, 1 << 48) for t in tot]


def rn32(fr):
    """exact Fractions -> the nearest f32 values, ties to even (through the correctly rounded double, with the rare double rounding decided exactly)"""
    out = np.empty(len(fr), dtype=np.float32)
    for i, v in enumerate(fr):
        f = np.float32(float(v))
        cand = (f, np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf)))
        err = [abs(v - Fraction(float(c))) for c in cand]
        best = min(range(3), key=lambda j: (err[j], int(np.float32(cand[j]).view(np.uint32)) & 1))
        out[i] = cand[best]
    return out


def cancelling_bias(r):
    """r = RN32(s) -> (bias f32, c f32): c on an f16 midpoint two binades under r, bias = c - r exact in f32.  Elements whose quarter falls under the
    f16 normals keep bias 0 (they are few and simply not sensitised)."""
    r = np.asarray(r, dtype=np.float32)
    t = (np.abs(r) * np.float32(0.25)).astype(np.float16)
    up = (t.view(np.uint16) + np.uint16(1)).view(np.float16)
    c = (np.sign(r) * ((t.astype(np.float64) + up.astype(np.float64)) * 0.5)).astype(np.float32)
    ok = t.astype(np.float32) >= np.float32(2.0 ** -14)
    c = np.where(ok, c, np.float32(0)).astype(np.float32)
    b = np.where(ok, c - r, np.float32(0)).astype(np.float32)
    assert np.array_equal((r + b)[ok], c[ok]) and np.array_equal(b.astype(np.float64)[ok], (c.astype(np.float64) - r.astype(np.float64))[ok])
    return b, c


# ---------------------------------------------------------------------------------------------------------
# the layer, stage by stage, from the oracle's pieces
# ---------------------------------------------------------------------------------------------------------
def _rms(x, w, eps):
    x = np.ascontiguousarray(x, dtype=np.float32)
    w = np.ascontiguousarray(w, dtype=np.float32)
    out = np.empty_like(x)
    orc_py.lib().orc_rms_norm(orc_py._p(x), orc_py._p(w), len(x), C.c_float(eps), orc_py.F16, orc_py._p(out))
    return out


def _silu_mul(g, u):
    s = np.array([orc_py.lib().orc_silu(C.c_float(float(v))) for v in g], dtype=np.float32)
    return _r16(_r16(s) * u)


class Stage:
    """T0 at position 0 through the one layer.  `lin(name, x)` returns a linear's f32 output before its rounding; the default is the oracle's.
    Fields: x_qkv, q, k0, v0, x_o, o, hidden, x_gu, gate, up, x_down, prev_mlp."""

    def __init__(self, model, lin=None):
        cfg, lay = model["config"], model["layers"][0]
        lin = lin or (lambda name, x: orc_py.OrcLinear(lay[name]).forward(x)[0])
        emb = model["embed"][T0].astype(np.float32)
        rep = cfg["n_heads"] // cfg["n_kv_heads"]
        self.h0 = _r16(emb)
        self.x_qkv = _rms(self.h0, lay["attn_norm"], cfg["rms_eps"])
        self.q, self.k0, self.v0 = (_r16(lin(n, self.x_qkv)) for n in ("q", "k", "v"))
        self.x_o = np.repeat(self.v0.reshape(cfg["n_kv_heads"], 1, cfg["head_dim"]), rep, axis=1).reshape(-1)   # one key: softmax = 1, out = v
        self.o = _r16(lin("o", self.x_o))
        self.hidden = _r16(self.h0 + self.o)
        self.x_gu = _rms(self.hidden, lay["ffn_norm"], cfg["rms_eps"])
        self.gate, self.up = _r16(lin("gate", self.x_gu)), _r16(lin("up", self.x_gu))
        self.x_down = _silu_mul(self.gate, self.up)
        self.prev_mlp = _r16(lin("down", self.x_down))

    def input_of(self, name):
        return {"q": self.x_qkv, "k": self.x_qkv, "v": self.x_qkv, "o": self.x_o, "gate": self.x_gu, "up": self.x_gu, "down": self.x_down}[name]


class Case:
    """model: the synth dict with the case's f32 biases;  sums[name] / rsum[name]: exact sums (Fractions) / RN32 of them for every biased linear;
    want: the oracle's k0, v0 [n_kv * hd], hidden, prev_mlp [H] and logits [V] for T0 at position 0;  folded[site]: the same observables with the bias
    of that ONE site folded into the exact sum (the other sites in the oracle's order)."""

    def __init__(self, width, case):
        self.width, self.case = width, case
        self.sites = SITES if case == "all" else (case,)
        model = make_model(width)
        lay = model["layers"][0]
        self.model, self.cfg = model, model["config"]
        self.sums, self.rsum = {}, {}
        for site in self.sites:                      # in layer order: a later group sees the earlier groups' biases
            st = Stage(model)
            for name in GROUPS[site]:
                self.sums[name] = exact_sums(lay[name], st.input_of(name))
                self.rsum[name] = rn32(self.sums[name])
                lay[name]["bias"] = cancelling_bias(self.rsum[name])[0]
        self.stage = Stage(model)
        om = orc_py.OrcLlama(model)
        kv = om.new_kv(4)
        logits = np.asarray(om.forward_kv([T0], kv, 0), dtype=np.float32).reshape(-1)
        k, v = orc_py.kv_rows(kv)
        kv2 = om.new_kv(4)
        hid, pm = om.layers_range(om.embed([T0]), None, kv2, 0, 1, 0)
        self.want = dict(k0=k[0, :, 0, :].reshape(-1).copy(), v0=v[0, :, 0, :].reshape(-1).copy(), hidden=hid.reshape(-1), prev_mlp=pm.reshape(-1), logits=logits)
        orc_py.lib().orc_kv_free(kv)
        orc_py.lib().orc_kv_free(kv2)
        self.folded = {site: self._fold(site) for site in self.sites}
        for a in self.want.values():
            a.setflags(write=False)

    def _fold(self, site):
        lay = self.model["layers"][0]

        def lin(name, x):
            if name not in GROUPS[site]:
                return orc_py.OrcLinear(lay[name]).forward(x)[0]
            assert np.array_equal(x, self.stage.input_of(name))       # upstream is in the oracle's order: the sums are the ones the bias was built from
            return rn32([s + Fraction(float(b)) for s, b in zip(self.sums[name], lay[name]["bias"])])
        st = Stage(self.model, lin)
        return {k: getattr(st, k) for k in ("k0", "v0", "hidden", "prev_mlp")}

    def biases(self):
        """{linear name: f32 bias} of the case (what a child process needs next to make_model to rebuild the model)"""
        return {n: b for n, b in ((n, self.model["layers"][0][n].get("bias")) for n in ("q", "k", "v", "o", "gate", "up", "down")) if b is not None}


@functools.lru_cache(maxsize=None)
def get(width, case):
    return Case(width, case)


def with_biases(width, biases):
    """make_model(width) with the given {linear name: f32 bias}"""
    model = make_model(width)
    for n, b in biases.items():
        model["layers"][0][n]["bias"] = np.asarray(b, dtype=np.float32)
    return model
