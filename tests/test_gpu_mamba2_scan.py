"""The Mamba2 prompt kernels on their own (bz_ssm_scan_rows: k_pf_conv + k_pf_conv_state, k_ssm_scan, k_pf_gnorm -- what one layer of mamba_prefill launches between its
two GEMMs), token for token against the oracle's conv1d_step + ssm_step applied to the same rows, and the gated norm restated in numpy as orc_mamba2_forward writes it.
Both sides see the same input bits, so what is measured is the kernels' arithmetic alone.

Shapes: one-layer models, hidden 64, vocab 64, 8 heads (a head is a workgroup, a group an index: nothing wider is needed).  Bars: the conv window is data movement
(array_equal); xbc, y, the SSM state and yn within two rounding intervals of the activation dtype at the reference element's magnitude, at most 1 % of the elements not
the same bits (the op bar, with a second interval for yn's two roundings after an rsqrt); f32 the bars of
test_gpu_ops_state.py::test_conv1d_step_and_ssm_step_follow_the_oracle_state_for_state.  Splitting a call in two is an identity, bit for bit.

MEASURED on an MI355X, all shapes and lengths, N(0, 1) rows and rows with the edge tokens alike: xbc, y and the SSM state are the oracle's bits (0 of 494208, 289536
and 2506752 16-bit elements differ; f32: xbc and state 0, y 9.4e-8 of the range); yn 4 of 289536 elements, one interval each (the norm's sum of squares is an f32
tree where the oracle sums in double).  The conv window's dot product, the state update and the C dot are exactly rounded sums, as in the step kernel.  They were
f32 chains when this test was written, and the test then failed: a chain rounds a state element to the other 16-bit neighbour about once in 2^13 (f16) / 2^16
(bf16) updates, the carried state keeps that interval in absolute terms while later tokens cancel most of the element, and small elements ended up to 21 (f16) /
3 (bf16) intervals of their own magnitude away, y up to 7 (43 after an x row scaled by 50).
"""
import numpy as np
import pytest

from blazr_amd import _lib as L
from blazr_amd import runtime, synth
from oracle import orc_py
from test_gpu_fp8_weights import _ulp
from test_gpu_ops_state import _round

pytestmark = pytest.mark.gpu

SHAPES = {   # head_dim, d_state, n_groups, conv_kernel, act
    "hd64-ns128-g1-k4-bf16": (64, 128, 1, 4, "bf16"),     # the Mamba2-2.7B head (NQ = 8, padded LDS stride), 4 pieces
    "hd64-ns64-g2-k4-f16": (64, 64, 2, 4, "f16"),         # NQ = 4, two groups
    "hd32-ns16-g4-k2-bf16": (32, 16, 4, 2, "bf16"),       # NQ = 1, scalar LDS reads, shortest window
    "hd24-ns64-g1-k4-bf16": (24, 64, 1, 4, "bf16"),       # head_dim not a multiple of 16: masked rows in the last piece
    "hd40-ns128-g2-k3-f16": (40, 128, 2, 3, "f16"),       # the same with 3 pieces and two groups
    "hd8-ns16-g1-k9-bf16": (8, 16, 1, 9, "bf16"),         # one half-empty piece, longest admitted window
    "hd64-ns64-g2-k4-f32": (64, 64, 2, 4, "f32"),         # the f32 instantiations, reachable only through this entry; no yn
}
LENGTHS = [1, 3, 7, 8, 9, 16, 17, 23]     # below one chunk of 8, S < kc - 1, exactly one and two chunks, tails of 1 and 7
MORE = 9                                  # every case goes on for 9 rows from the carried state
NH = 8

_FIX, _ROWS, _REF, _FULL = {}, {}, {}, {}


def _config(sid, n_layers=1):
    hd, ns, g, kc, act = SHAPES[sid]
    return dict(arch="mamba2", hidden=64, n_layers=n_layers, vocab=64, d_inner=NH * hd, n_heads=NH, head_dim=hd, d_state=ns, n_groups=g, conv_kernel=kc,
                rms_eps=1e-5, act_dtype=act, tie_embeddings=True, max_seq_len=1 << 20)


def _fixture(device, sid):
    if sid not in _FIX:
        model = synth.make_mamba2(_config(sid))
        _FIX[sid] = (model, runtime.LoadedModel.from_synth(device, model), orc_py.OrcMamba2(model))
    return _FIX[sid]


def _dims(cfg):
    DI, G, NS = cfg["d_inner"], cfg["n_groups"], cfg["d_state"]
    return DI, DI + 2 * G * NS, 2 * DI + 2 * G * NS + cfg["n_heads"]


def _rows(sid, S, edges):
    """S + MORE in_proj rows [z | x B C | dt]: N(0, 1) rounded to the activation dtype.  edges: two hand-written tokens in each call -- one whose dt column is +30 in
    head 1 (softplus takes its x > 20 branch, dA underflows towards 0) and -30 in head 6 (dt -> 0, dA -> 1), one whose x row is scaled by 50"""
    if (sid, S, edges) not in _ROWS:
        cfg = _config(sid)
        DI, conv_dim, d_in = _dims(cfg)
        rng = np.random.default_rng(1000 * list(SHAPES).index(sid) + S)
        zx = rng.normal(0.0, 1.0, (S + MORE, d_in)).astype(np.float32)
        if edges:
            for t_dt, t_x in ((S - 1, S // 2), (S + MORE - 1, S + 3)):     # the last token of each call (the chunk tail), and one in the middle
                zx[t_dt, DI + conv_dim + 1] = 30.0
                zx[t_dt, DI + conv_dim + 6] = -30.0
                zx[t_x, DI:2 * DI] *= 50.0
        zx = _round(zx, cfg["act_dtype"])
        zx.setflags(write=False)
        _ROWS[sid, S, edges] = zx
    return _ROWS[sid, S, edges]


def _gnorm(y, w, G, eps, act):
    """orc_mamba2_forward's gated norm, row by row: a double sum of the f32 squares, 1 / sqrtf((float)ss / gsz + eps), R(w . R(y . rs))"""
    n, DI = y.shape
    gsz = DI // G
    yg = y.reshape(n, G, gsz)
    ss = (yg * yg).astype(np.float64).sum(axis=2)
    rs = np.float32(1.0) / np.sqrt(ss.astype(np.float32) / np.float32(gsz) + np.float32(eps), dtype=np.float32)
    return _round(w.reshape(1, G, gsz) * _round(yg * rs[:, :, None], act), act).reshape(n, DI)


def _reference(device, sid, S, edges):
    """the oracle's conv1d_step + ssm_step token by token over _rows(sid, S, edges); the state after S rows and after all S + MORE.  Computed once, read-only."""
    if (sid, S, edges) not in _REF:
        model, _, om = _fixture(device, sid)
        cfg = model["config"]
        DI, conv_dim, d_in = _dims(cfg)
        zx = _rows(sid, S, edges)
        n = zx.shape[0]
        cs = np.zeros((conv_dim, cfg["conv_kernel"] - 1), dtype=np.float32)
        ss = np.zeros((NH, cfg["head_dim"], cfg["d_state"]), dtype=np.float32)
        xbc, y = np.empty((n, conv_dim), dtype=np.float32), np.empty((n, DI), dtype=np.float32)
        mid = None
        for t in range(n):
            xbc[t] = om.conv1d_step(0, zx[t], cs)
            y[t] = om.ssm_step(0, zx[t], xbc[t], ss)
            if t == S - 1:
                mid = (cs.copy(), ss.copy())
        w = np.ascontiguousarray(model["layers"][0]["gnorm"], dtype=np.float32)
        yn = _gnorm(y, w, cfg["n_groups"], cfg["rms_eps"], cfg["act_dtype"])
        ref = dict(xbc=xbc, y=y, yn=yn, win=(mid[0], cs), ssm=(mid[1], ss))
        for v in (xbc, y, yn, mid[0], mid[1], cs, ss):
            v.setflags(write=False)
        _REF[sid, S, edges] = ref
    return _REF[sid, S, edges]


def _call(lm, cfg, st, rows):
    """one bz_ssm_scan_rows call on layer 0, then the state it left: dict(xbc, y, yn (None for f32), ssm, win)"""
    DI, conv_dim, _ = _dims(cfg)
    xbc, y, yn = lm.ssm_scan_rows(0, st, rows, norm=cfg["act_dtype"] != "f32")
    ssm = st.read(0, 0, NH * cfg["head_dim"] * cfg["d_state"]).reshape(NH, cfg["head_dim"], cfg["d_state"])
    win = st.read(0, 1, conv_dim * (cfg["conv_kernel"] - 1)).reshape(conv_dim, cfg["conv_kernel"] - 1)
    return dict(xbc=xbc, y=y, yn=yn, ssm=ssm, win=win)


def _hold(tag, name, got, want, act, lines):
    """the bar of one tensor; the measured count of differing elements and the largest distance go to `lines`.  16-bit: every element within two rounding intervals
    at the reference element's magnitude, at most 1 % not the same bits (the rows with the hand-written edge tokens meet it like the others: no bar of their own).
    f32: the state within 4e-6 of the range, y and xbc within 8e-6."""
    assert got.shape == want.shape and np.isfinite(got).all(), (tag, name)
    nd = int((got != want).sum())
    err = float(np.abs(got - want).max()) / max(float(np.abs(want).max()), 1e-6)
    if act == "f32":
        tol = 4e-6 if name == "ssm" else 8e-6
        lines.append("%s %s: %d of %d differ, max %.2e of the range" % (tag, name, nd, want.size, err))
        return [] if err <= tol else ["%s %s: %.2e of the range > %.0e" % (tag, name, err, tol)]
    dist = np.abs(got.astype(np.float64) - want.astype(np.float64)) / _ulp(want, act)
    lines.append("%s %s: %d of %d differ (%.3f %%), max %.3g intervals, %.2e of the range" % (tag, name, nd, want.size, 100.0 * nd / want.size, float(dist.max()), err))
    bad = []
    if dist.max() > 2.0:
        i = np.unravel_index(int(dist.argmax()), got.shape)
        bad.append("%s %s: %.3g intervals at %s (got %r, want %r)" % (tag, name, float(dist.max()), tuple(int(j) for j in i), float(got[i]), float(want[i])))
    if nd > 0.01 * want.size:
        bad.append("%s %s: %d of %d elements differ (> 1 %%)" % (tag, name, nd, want.size))
    return bad


@pytest.mark.parametrize("S", LENGTHS)
@pytest.mark.parametrize("sid", list(SHAPES))
def test_prompt_kernels_follow_the_oracle_token_for_token(device, sid, S):
    """S rows from the zero state, then 9 more from the carried one; after each call the outputs, the SSM state and the conv window against the oracle -- on N(0, 1)
    rows, and on the same rows with the edge tokens written in"""
    model, lm, _ = _fixture(device, sid)
    cfg = model["config"]
    act = cfg["act_dtype"]
    lines, bad = [], []
    for edges in (False, True):
        zx, ref = _rows(sid, S, edges), _reference(device, sid, S, edges)
        st = runtime.LayeredSsmState(lm)
        for k, (lo, hi) in enumerate(((0, S), (S, S + MORE))):
            got = _call(lm, cfg, st, zx[lo:hi])
            tag = "%s S=%d %s call %d" % (sid, S, "edges" if edges else "plain", k)
            assert np.array_equal(got["win"], ref["win"][k]), tag                 # pure data movement
            bad += _hold(tag, "xbc", got["xbc"], ref["xbc"][lo:hi], act, lines)
            bad += _hold(tag, "y", got["y"], ref["y"][lo:hi], act, lines)
            bad += _hold(tag, "ssm", got["ssm"], ref["ssm"][k], act, lines)
            if act != "f32":
                bad += _hold(tag, "yn", got["yn"], ref["yn"][lo:hi], act, lines)
    print("\n".join(lines))
    assert not bad, "\n".join(bad)


def _full(device, sid):
    """the first 23 rows of this shape (edge tokens included) in one call from the zero state (shared by the split cases)"""
    if sid not in _FULL:
        model, lm, _ = _fixture(device, sid)
        _FULL[sid] = _call(lm, model["config"], runtime.LayeredSsmState(lm), _rows(sid, 23, True)[:23])
    return _FULL[sid]


@pytest.mark.parametrize("S1", [1, 2, 3, 8, 15])
@pytest.mark.parametrize("sid", list(SHAPES))
def test_splitting_a_call_changes_no_bit(device, sid, S1):
    """23 rows in one call == S1 rows, then 23 - S1 from the carried state.  A token's arithmetic does not depend on where a call starts, so any difference is a staging,
    prefetch or late-store defect; S1 < kc - 1 takes a window partly from the carried state and partly from the rows (k_pf_conv and k_pf_conv_state)"""
    model, lm, _ = _fixture(device, sid)
    cfg = model["config"]
    zx, one = _rows(sid, 23, True)[:23], _full(device, sid)
    st = runtime.LayeredSsmState(lm)
    a = _call(lm, cfg, st, zx[:S1])
    b = _call(lm, cfg, st, zx[S1:])
    for name in ("xbc", "y", "yn"):
        if one[name] is not None:
            assert np.array_equal(np.concatenate([a[name], b[name]]), one[name]), (sid, S1, name)
    assert np.array_equal(b["ssm"], one["ssm"]) and np.array_equal(b["win"], one["win"]), (sid, S1)


def test_another_layers_state_is_untouched(device):
    sid = next(iter(SHAPES))
    cfg = _config(sid, n_layers=2)
    lm = runtime.LoadedModel.from_synth(device, synth.make_mamba2(cfg))
    DI, conv_dim, _ = _dims(cfg)
    n_ssm, n_win = NH * cfg["head_dim"] * cfg["d_state"], conv_dim * (cfg["conv_kernel"] - 1)
    for layer in (0, 1):
        st = runtime.LayeredSsmState(lm)
        lm.ssm_scan_rows(layer, st, _rows(sid, 9, True)[:9])
        assert st.read(layer, 0, n_ssm).any() and st.read(layer, 1, n_win).any()
        assert not st.read(1 - layer, 0, n_ssm).any() and not st.read(1 - layer, 1, n_win).any()


def test_bad_arguments_are_refused_with_an_error_code(device):
    sid = next(iter(SHAPES))
    model, lm, _ = _fixture(device, sid)
    cfg = model["config"]
    DI, conv_dim, d_in = _dims(cfg)
    S = 4
    st = runtime.LayeredSsmState(lm)
    f32 = lambda *shape: device.zeros(shape, L.F32)
    zx, xbc, y, yn = f32(S, d_in), f32(S, conv_dim), f32(S, DI), f32(S, DI)
    run = lambda m=lm, layer=0, s=st, zx=zx, S=S, xbc=xbc, y=y, yn=yn: L.lib().bz_ssm_scan_rows(m.h, layer, s.h, zx.h, S, xbc.h, y.h, None if yn is None else yn.h)
    assert run() == L.OK and run(yn=None) == L.OK                                    # the arguments the refusals below vary are good ones
    llama = runtime.LoadedModel.from_synth(device, synth.make_llama("tiny-bf16"))
    assert run(m=llama) == L.E_INVALID                                               # not a Mamba2 model
    assert run(layer=-1) == L.E_INVALID and run(layer=1) == L.E_INVALID              # layer out of range
    other = runtime.LoadedModel.from_synth(device, synth.make_mamba2(_config("hd64-ns64-g2-k4-f16")))
    assert run(s=runtime.LayeredSsmState(other)) == L.E_INVALID                      # state of another model
    assert run(S=0) == L.E_INVALID and run(S=S + 1) == L.E_INVALID and run(S=S - 1) == L.E_INVALID     # tensors of another size than S rows
    assert run(zx=f32(S, d_in - 1)) == L.E_INVALID and run(xbc=f32(S, conv_dim + 1)) == L.E_INVALID
    assert run(y=f32(S - 1, DI)) == L.E_INVALID and run(yn=f32(S, DI + 8)) == L.E_INVALID
    for name in ("zx", "xbc", "y", "yn"):                                            # 16-bit tensors of the right byte count
        cols = {"zx": d_in, "xbc": conv_dim, "y": DI, "yn": DI}[name]
        assert run(**{name: device.zeros((2 * S, cols), L.BF16)}) == L.E_INVALID, name
    # an f32 model has no 16-bit norm rows
    _, lm32, _ = _fixture(device, "hd64-ns64-g2-k4-f32")
    c32 = lm32.mamba_config()
    cd32 = c32["d_inner"] + 2 * c32["n_groups"] * c32["d_state"]
    args32 = dict(m=lm32, s=runtime.LayeredSsmState(lm32), zx=f32(S, c32["d_inner"] + cd32 + NH), xbc=f32(S, cd32), y=f32(S, c32["d_inner"]))
    assert run(yn=f32(S, c32["d_inner"]), **args32) == L.E_UNSUPPORTED and run(yn=None, **args32) == L.OK
    # a state shape bzk_ssm_scan_ok refuses (d_state 32): the model loads and steps, the scan is not for it
    odd = dict(_config(sid), d_state=32)
    lmo = runtime.LoadedModel.from_synth(device, synth.make_mamba2(odd))
    cdo = odd["d_inner"] + 2 * 32
    assert run(m=lmo, s=runtime.LayeredSsmState(lmo), zx=f32(S, odd["d_inner"] + cdo + NH), xbc=f32(S, cdo), y=f32(S, odd["d_inner"]), yn=None) == L.E_UNSUPPORTED
    assert b"scan" in L.lib().bz_last_error()
