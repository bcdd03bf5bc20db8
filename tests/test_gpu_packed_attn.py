"""Segment-masked prompt attention on its own (bz_attn_packed: k_pf_attn_mfma / k_pf_attn, the SEG forms) over the length sets of packed_cases.py.
Isolation is bit for bit: no row of another input can change a row.  The exact scalar form equals, bit for bit, a call holding the input alone.  The MFMA and
plain scalar forms are measured against float64 masked attention (packed_ref) on the same rounded inputs, and held to twice the error of the SAME kernel run on
each input alone (n_seq = 1: the plain, unmasked prompt launch at position 0) -- the key tiles of a packed input start at another phase, which changes the order
of the online-softmax rescalings but not their number.  Every figure is printed ("PACKED_ATTN_ERR ...") before it is asserted."""
import json

import numpy as np
import pytest

import packed_cases as PC
import packed_ref as PR
from blazr_amd import _lib as L
from blazr_amd import runtime

pytestmark = pytest.mark.gpu
DT = {"f16": L.F16, "bf16": L.BF16, "f32": L.F32}
NKV = 2
MFMA_SWEEP = [(dt, hd, rep) for dt in ("f16", "bf16") for hd in (64, 128) for rep in (1, 2, 4, 8)]
SCALAR_SWEEP = [("f32", L.PF_ATTN_SCALAR_EXACT), ("f32", L.PF_ATTN_SCALAR), ("f16", L.PF_ATTN_SCALAR), ("bf16", L.PF_ATTN_SCALAR), ("f16", L.PF_ATTN_SCALAR_EXACT)]
S_HD, S_REP = 64, 2                                             # the scalar forms' one shape
_REF = {}


def _case(name, dt, hd, rep, window=0):
    """(lens, rounded rows, float64 reference), computed once"""
    key = (name, dt, hd, rep, window)
    if key not in _REF:
        lens = PC.SETS[name]
        x = PC.qkv_rows(lens, NKV * rep, NKV, hd, dt, seed=ord(name) * 10000 + hd * 10 + rep)
        x.setflags(write=False)
        _REF[key] = (lens, x, PR.attention(x, lens, NKV * rep, NKV, hd, window))
    return _REF[key]


def _run(device, x, lens, dt, hd, rep, form, window=0):
    return runtime.attn_packed(device, x, lens, NKV * rep, NKV, hd, DT[dt], form, window)


def _alone(device, x, lens, dt, hd, rep, form, window=0):
    """every input in a call of its own, stacked"""
    off = PC.offsets(lens)
    return np.concatenate([_run(device, x[off[i]:off[i + 1]], [lens[i]], dt, hd, rep, form, window) for i in range(len(lens))])


def _isolation(device, dt, hd, rep, form):
    for name in ("B", "C"):
        lens, x, _ = _case(name, dt, hd, rep)
        base = _run(device, x, lens, dt, hd, rep, form)
        off = PC.offsets(lens)
        rng = np.random.default_rng(9)
        for i in range(len(lens)):
            y = x.copy()
            y[off[i]:off[i + 1]] = PC.round_to(rng.standard_normal((lens[i], x.shape[1])) * 3.0, dt)
            got = _run(device, y, lens, dt, hd, rep, form)
            keep = np.ones(len(x), dtype=bool)
            keep[off[i]:off[i + 1]] = False
            assert np.array_equal(got[keep], base[keep]), "set %s: input %d leaks into another input's rows" % (name, i)
            assert not np.array_equal(got[~keep], base[~keep])


def _own_v_rows(device, dt, hd, rep, form):
    """set A, one token per input: softmax over one key is exp(0) / exp(0), so a row is its own V row's bits"""
    one = np.zeros(1, dtype=np.float32)
    out = np.empty(1, dtype=np.float32)
    L.check(L.lib().bz_expf_spec(one.ctypes.data, 1, out.ctypes.data))
    assert out[0] == 1.0
    lens, x, _ = _case("A", dt, hd, rep)
    got = _run(device, x, lens, dt, hd, rep, form)
    nq = NKV * rep
    v = x[:, (nq + NKV) * hd:].reshape(len(x), NKV, hd)
    want = np.repeat(v, rep, axis=1).reshape(len(x), nq * hd)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _errors(device, dt, hd, rep, form, sets=PC.OP_SETS, window=0):
    """largest element error against the float64 reference: (packed call, every input alone), over the sets"""
    ep = ea = 0.0
    for name in sets:
        lens, x, ref = _case(name, dt, hd, rep, window)
        ep = max(ep, float(np.abs(_run(device, x, lens, dt, hd, rep, form, window) - ref).max()))
        ea = max(ea, float(np.abs(_alone(device, x, lens, dt, hd, rep, form, window) - ref).max()))
    print("PACKED_ATTN_ERR " + json.dumps(dict(dt=dt, hd=hd, rep=rep, form=int(form), window=window, sets="".join(sets), packed=ep, alone=ea)))
    return ep, ea


@pytest.mark.parametrize("dt,hd,rep", MFMA_SWEEP, ids=["%s-hd%d-g%d" % c for c in MFMA_SWEEP])
def test_mfma_form(device, dt, hd, rep):
    _isolation(device, dt, hd, rep, L.PF_ATTN_MFMA)
    _own_v_rows(device, dt, hd, rep, L.PF_ATTN_MFMA)
    ep, ea = _errors(device, dt, hd, rep, L.PF_ATTN_MFMA)
    assert ea > 0.0 and ep <= 2.0 * ea, (ep, ea)


@pytest.mark.parametrize("dt,form", SCALAR_SWEEP, ids=["%s-form%d" % c for c in SCALAR_SWEEP])
def test_scalar_forms(device, dt, form):
    _isolation(device, dt, S_HD, S_REP, form)
    _own_v_rows(device, dt, S_HD, S_REP, form)
    if form == L.PF_ATTN_SCALAR_EXACT:
        # exactly rounded sums: where an input's keys sit in the packed batch cannot matter
        for name in PC.OP_SETS:
            lens, x, _ = _case(name, dt, S_HD, S_REP)
            got, want = _run(device, x, lens, dt, S_HD, S_REP, form), _alone(device, x, lens, dt, S_HD, S_REP, form)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
    ep, ea = _errors(device, dt, S_HD, S_REP, form)
    assert ea > 0.0 and ep <= 2.0 * ea, (ep, ea)


@pytest.mark.parametrize("dt,hd,rep,form", [("f16", 128, 4, L.PF_ATTN_MFMA), ("bf16", 64, 1, L.PF_ATTN_MFMA), ("f16", S_HD, S_REP, L.PF_ATTN_SCALAR)],
                         ids=["mfma-f16-hd128-g4", "mfma-bf16-hd64-g1", "scalar-f16"])
def test_window_and_segments(device, dt, hd, rep, form):
    """window = 48 on set B: both masks, lo = max(the input's first row, the window's first key)"""
    ep, ea = _errors(device, dt, hd, rep, form, sets=("B",), window=48)
    assert ea > 0.0 and ep <= 2.0 * ea, (ep, ea)
    lens, x, _ = _case("B", dt, hd, rep, 48)
    full = PR.attention(x, lens, NKV * rep, NKV, hd, 0)
    assert np.abs(_run(device, x, lens, dt, hd, rep, form, 48) - full).max() > 10 * ep      # the window is really applied


def test_refusals(device):
    x = device.tensor(np.zeros((8, 4 * 64), dtype=np.float32))
    out = device.zeros((8, 2 * 64), L.F32)

    def call(lens, nq=2, nkv=1, hd=64, dt=L.F16, form=L.PF_ATTN_MFMA, window=0):
        sl = np.asarray(lens, dtype=np.int32)
        rc = L.lib().bz_attn_packed(device.h, x.h, sl.ctypes.data if len(sl) else None, len(sl), nq, nkv, hd, dt, form, window, out.h)
        return rc, L.lib().bz_last_error()
    assert call([5, 3])[0] == L.OK
    for kw, figure in ((dict(lens=[]), b"n_seq = 0"), (dict(lens=[5, 0, 3]), b"seq_lens[1] = 0"), (dict(lens=[5, 4]), b"[9, 256]"), (dict(lens=[5, 3], form=L.PF_ATTN_ROWS), b"form = 4"),
                       (dict(lens=[5, 3], window=-1), b"window = -1"), (dict(lens=[5, 3], dt=L.I64), b"dt = 3"), (dict(lens=[5, 3], nq=3, nkv=2), b"3 query heads")):
        rc, msg = call(**kw)
        assert rc == L.E_INVALID and figure in msg, (kw, msg)
    assert call([5, 3], dt=L.F32)[0] == L.E_UNSUPPORTED         # the MFMA form takes 16-bit rows
