"""GPU parity for the Mamba2 path: forward_with_ssm_state, the recurrent state, the
generate loop (executor_generate.rs:123-181) and the hipGraph decode, against oracle/orc_mamba2.c.

The recurrence lives in the absent boostr crate; the oracle restates the public Mamba2 single-token step (parity unpinned, see
oracle/orc_mamba2.c).  Bars as in test_gpu_llama.py: relative L2 of the logits, greedy ids bit-exact on fair prefixes.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from blazr_amd import _lib as L
from blazr_amd import runtime, synth
from mamba2_carry_probe import carry, read_state as _read_state
from oracle import orc_py
from test_gpu_llama import REL, TINY, _check_logits, _fair_prefix

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["tiny-mamba2", "tiny-mamba2-g2"])
def pair(request, device):
    model = synth.make_mamba2(request.param)
    return model, runtime.LoadedModel.from_synth(device, model), orc_py.OrcMamba2(model)


def test_accessors(pair):
    model, lm, _ = pair
    assert lm.needs_ssm_state() and not lm.needs_kv_cache()
    assert lm.mamba_config()["d_state"] == model["config"]["d_state"]
    resident, per_token = lm.weight_bytes()
    assert per_token == synth.mamba2_bytes_per_token(model["config"])[0]


def test_prefill_and_decode_logits(pair, device):
    model, lm, om = pair
    cfg = model["config"]
    p = synth.prompt_tokens(7, cfg["vocab"])
    st, ost = runtime.LayeredSsmState(lm), om.new_state()
    got = lm.forward_with_ssm_state(p, st, all_logits=True).to_numpy()
    want = om.forward(p, ost, all_logits=True)
    _check_logits(got, want, cfg["act_dtype"])
    tok = int(want[-1].argmax())
    for _ in range(24):   # the state keeps evolving: errors must not accumulate
        lg = lm.forward_with_ssm_state([tok], st).to_numpy()
        lo = om.forward([tok], ost)
        _check_logits(lg, lo, cfg["act_dtype"])
        tok = int(lo[0].argmax())
    orc_py.lib().orc_ssm_state_free(ost)


def test_state_reset_restarts_the_sequence(pair):
    model, lm, _ = pair
    p = synth.prompt_tokens(5, model["config"]["vocab"], seed=3)
    st = runtime.LayeredSsmState(lm)
    a = lm.forward_with_ssm_state(p, st).to_numpy()
    b = lm.forward_with_ssm_state(p, st).to_numpy()      # continues from the evolved state
    st.reset()
    c = lm.forward_with_ssm_state(p, st).to_numpy()
    assert np.array_equal(a, c) and not np.array_equal(a, b)


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_generate_greedy_token_parity(pair, mode):
    model, lm, om = pair
    cfg = model["config"]
    for seed in range(3, 40):
        p = synth.prompt_tokens(12, cfg["vocab"], seed=seed)
        want, trace = om.generate(p, 24, trace=True)
        n = _fair_prefix(trace)
        if n >= 8:
            break
    assert n >= 8, "no prompt seed gives a fair fixture"
    got = runtime.Executor(lm).generate(p, 24, use_graph=mode == "graph")
    assert got[:n].tolist() == want[:n].tolist(), (mode, got.tolist(), want.tolist(), n)


def test_graph_replay_equals_eager(pair):
    model, lm, _ = pair
    p = synth.prompt_tokens(6, model["config"]["vocab"], seed=5)
    ex = runtime.Executor(lm)
    assert ex.generate(p, 16, use_graph=True).tolist() == ex.generate(p, 16).tolist()


@pytest.mark.parametrize("pair", ["tiny-mamba2-g2"], indirect=True)
def test_profile_step_ssm_reports_the_launches_of_one_step(pair):
    """bz_profile_step_ssm, one step (iters=1) of tiny-mamba2-g2 (2 layers, f32, untied lm_head) after 8 tokens: the kernel names and their launch counts.
    Per layer mamba_step launches in_proj (norm prologue), the fused conv + SSM step and out_proj (gated-norm prologue); the embedding, the lm_head with its
    argmax partials and argmax_final launch once each -- the tail every architecture's step shares.  The values are those the library of the commit before
    the shared tail reported on an MI355X for this fixture:

    | name                      | launches |
    |---------------------------|----------|
    | embed                     | 1        |
    | gemv_rows<norm>           | 2        |  in_proj, one per layer
    | mamba2_ssm_step           | 2        |  conv1d step + SiLU + recurrence + gate, one per layer
    | gemv_rows<gated>          | 2        |  out_proj, one per layer
    | gemv_rows<lm_head+argmax> | 1        |
    | argmax_final              | 1        |
    """
    model, lm, _ = pair
    want = {"embed": 1, "gemv_rows<norm>": 2, "mamba2_ssm_step": 2, "gemv_rows<gated>": 2, "gemv_rows<lm_head+argmax>": 1, "argmax_final": 1}
    assert model["config"]["n_layers"] == 2
    st = runtime.LayeredSsmState(lm)
    lm.forward_with_ssm_state(synth.prompt_tokens(8, model["config"]["vocab"]), st)
    got = {r["name"]: r["launches"] for r in lm.profile_step_ssm(st, 5, iters=1)}
    print(got)
    assert got == want


def test_error_behaviour(pair, device):
    model, lm, _ = pair
    cfg = model["config"]
    kv = runtime.LayeredKvCache(device, cfg["n_layers"], 1, 1, 8, 64, 64, L.F16)
    with pytest.raises(L.BlazrHipError):
        lm.forward_with_kv_cache([1, 2], kv, 0)                       # no KV cache on an SSM model
    with pytest.raises(L.BlazrHipError):
        runtime.DecodeGraph(lm, kv)
    other = runtime.LoadedModel.from_synth(device, synth.make_mamba2("tiny-mamba2", n_layers=1))
    st = runtime.LayeredSsmState(other)
    with pytest.raises(L.BlazrHipError):
        lm.forward_with_ssm_state([1], st)                            # state of another model
    with pytest.raises(L.BlazrHipError):
        L.check(L.lib().bz_ssm_state_create(lm.h, 2, lm.c.act_dtype, C.byref(C.c_void_p())))   # batch 1 only


def test_llama_model_rejects_ssm_calls(device):
    lm = runtime.LoadedModel.from_synth(device, synth.make_llama("tiny-bf16"))
    with pytest.raises(L.BlazrHipError):
        runtime.LayeredSsmState(lm)


@pytest.mark.parametrize("over", [dict(d_state=16), dict(conv_kernel=2), dict(n_groups=4, d_state=32), dict(act_dtype="f16"), dict(head_dim=32, n_heads=16)],
                         ids=["state16", "conv2", "groups4", "f16", "headdim32"])
def test_config_variants(device, over):
    model = synth.make_mamba2("tiny-mamba2", **over)
    cfg = model["config"]
    lm, om = runtime.LoadedModel.from_synth(device, model), orc_py.OrcMamba2(model)
    p = synth.prompt_tokens(6, cfg["vocab"], seed=19)
    st, ost = runtime.LayeredSsmState(lm), om.new_state()
    _check_logits(lm.forward_with_ssm_state(p, st, all_logits=True).to_numpy(), om.forward(p, ost, all_logits=True), cfg["act_dtype"])
    tok = 7
    for _ in range(6):
        lo = om.forward([tok], ost)
        _check_logits(lm.forward_with_ssm_state([tok], st).to_numpy(), lo, cfg["act_dtype"])
        tok = int(lo[0].argmax())
    orc_py.lib().orc_ssm_state_free(ost)


@pytest.mark.parametrize("over", [dict(), dict(d_state=16), dict(conv_kernel=2), dict(n_groups=4, d_state=64), dict(act_dtype="f16"), dict(head_dim=32, n_heads=16)],
                         ids=["base", "state16", "conv2", "groups4", "f16", "headdim32"])
@pytest.mark.parametrize("S", [8, 21, 70])
def test_batched_prefill_scan_matches_oracle_and_steps(device, over, S):
    """prompts of >= 8 tokens take the batched path (rows through the MFMA GEMMs, conv as a map over (token, channel), the recurrence as an
    in-kernel scan over the tokens); 21 and 70 leave a partial chunk of the scan's 8-token staging.  Checked against the oracle (every
    position's logits), and the state it leaves must continue exactly like the state the token-by-token path leaves: decode steps after the
    prompt are compared with the oracle too."""
    model = synth.make_mamba2("tiny-mamba2", **over)
    cfg = model["config"]
    lm, om = runtime.LoadedModel.from_synth(device, model), orc_py.OrcMamba2(model)
    p = synth.prompt_tokens(S, cfg["vocab"], seed=23 + S)
    st, ost = runtime.LayeredSsmState(lm), om.new_state()
    got = lm.forward_with_ssm_state(p, st, all_logits=True).to_numpy()
    want = om.forward(p, ost, all_logits=True)
    _check_logits(got, want, cfg["act_dtype"])
    # a second prompt continues from the carried conv window and SSM state
    p2 = synth.prompt_tokens(9, cfg["vocab"], seed=5)
    _check_logits(lm.forward_with_ssm_state(p2, st).to_numpy(), om.forward(p2, ost), cfg["act_dtype"])
    tok = int(want[-1].argmax())
    for _ in range(8):
        lo = om.forward([tok], ost)
        _check_logits(lm.forward_with_ssm_state([tok], st).to_numpy(), lo, cfg["act_dtype"])
        tok = int(lo[0].argmax())
    orc_py.lib().orc_ssm_state_free(ost)


def test_batched_prefill_crosses_the_row_chunk(device):
    """prompts longer than the 512-row workspace chunk: the conv window and the SSM state carry from one chunk of rows to the next"""
    model = synth.make_mamba2("tiny-mamba2")
    cfg = model["config"]
    lm, om = runtime.LoadedModel.from_synth(device, model), orc_py.OrcMamba2(model)
    p = synth.prompt_tokens(530, cfg["vocab"], seed=77)
    st, ost = runtime.LayeredSsmState(lm), om.new_state()
    got = lm.forward_with_ssm_state(p, st).to_numpy()
    want = om.forward(p, ost)
    _check_logits(got, want, cfg["act_dtype"])
    tok = int(want[-1].argmax())
    for _ in range(4):
        lo = om.forward([tok], ost)
        _check_logits(lm.forward_with_ssm_state([tok], st).to_numpy(), lo, cfg["act_dtype"])
        tok = int(lo[0].argmax())
    orc_py.lib().orc_ssm_state_free(ost)


# ---- the batched prompt path at its chunk edges, and the state it leaves ---------------------------------------------------------------------------
def _orc_state(cfg, ost):
    """the oracle's state as two float32 views: ssm [L, n_heads * head_dim * d_state], conv [L, conv_dim * (k - 1)]"""
    conv_dim = cfg["d_inner"] + 2 * cfg["n_groups"] * cfg["d_state"]
    n_ssm, n_win = cfg["n_heads"] * cfg["head_dim"] * cfg["d_state"], conv_dim * (cfg["conv_kernel"] - 1)
    view = lambda p, n: np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), (cfg["n_layers"], n))
    return view(ost.contents.ssm, n_ssm), view(ost.contents.conv, n_win)


_TINY = {}


def _tiny(device):
    if not _TINY:
        model = synth.make_mamba2("tiny-mamba2")
        _TINY["pair"] = (model, runtime.LoadedModel.from_synth(device, model), orc_py.OrcMamba2(model))
    return _TINY["pair"]


@pytest.mark.parametrize("r", [8, 18])
def test_chunk_carry_is_an_identity(device, r, tmp_path):
    """512 + r tokens in one call == a call of 512 and a call of r on the same state, bit for bit: both sides launch the same GEMMs on the same row counts (the
    workspace chunk is 512 rows), so nothing but a defect in what is carried from chunk to chunk can differ.  (Other splits are not comparable exactly: the GEMM
    chooses its K split from the row count.)  By default a prompt of up to 16 rows stays on the decode kernels (BZ_EXACT_PREFILL_MAX), so the call of 8 rows takes
    the batched route -- what the long call's last chunk runs -- only with BZ_EXACT_PREFILL=0: that case runs in a process of its own (the switches are read once)."""
    if r > 16:
        model, lm, _ = _tiny(device)
        d = carry(lm, model["config"]["vocab"], r)
    else:
        out = tmp_path / "carry.npz"
        env = dict(os.environ, BZ_EXACT_PREFILL="0")
        run = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "mamba2_carry_probe.py"), str(r), str(out)],
                             env=env, capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
        d = np.load(out)
    names = sorted(k[2:] for k in d.keys() if k.startswith("a_"))
    assert len(names) == 1 + 2 * 3
    for k in names:
        assert np.array_equal(d["a_" + k], d["b_" + k]), k


def _edge_reference(device):
    """the oracle over one 520-token prompt, stopped at 512, 513 and 520 tokens: the last row's logits and a copy of the state at each stop (computed once)"""
    if "edges" not in _TINY:
        model, _, om = _tiny(device)
        cfg = model["config"]
        p = synth.prompt_tokens(520, cfg["vocab"], seed=91)
        ost = om.new_state()
        stops, lo = {}, 0
        for S in (512, 513, 520):
            logits = om.forward(p[lo:S], ost)
            stops[S] = (logits, tuple(a.copy() for a in _orc_state(cfg, ost)))
            lo = S
        orc_py.lib().orc_ssm_state_free(ost)
        _TINY["edges"] = (p, stops)
    return _TINY["edges"]


@pytest.mark.parametrize("S", [512, 513, 520])
def test_batched_prefill_at_the_row_chunk_edges(device, S):
    """exactly one workspace chunk, a final chunk of ONE row (in_proj GEMM, conv, scan, gated norm and out_proj with n = 1) and one of 8: the last row's logits against
    the oracle, then four decode steps from the state the prompt left"""
    model, lm, om = _tiny(device)
    cfg = model["config"]
    p, stops = _edge_reference(device)
    want, (ssm, conv) = stops[S]
    st, ost = runtime.LayeredSsmState(lm), om.new_state()
    _check_logits(lm.forward_with_ssm_state(p[:S], st).to_numpy(), want, cfg["act_dtype"])
    for dst, src in zip(_orc_state(cfg, ost), (ssm, conv)):
        dst[...] = src
    tok = int(want[-1].argmax())
    for _ in range(4):
        lo = om.forward([tok], ost)
        _check_logits(lm.forward_with_ssm_state([tok], st).to_numpy(), lo, cfg["act_dtype"])
        tok = int(lo[0].argmax())
    orc_py.lib().orc_ssm_state_free(ost)


def _interval(v, act):
    """one rounding interval of the activation dtype at |v| (floor: the smallest normal)"""
    e = np.floor(np.log2(np.maximum(np.abs(np.asarray(v, dtype=np.float64)), 1e-300)))
    return np.exp2(np.maximum(e, -14.0) - 10.0) if act == "f16" else np.exp2(np.maximum(e, -126.0) - 7.0)


@pytest.mark.parametrize("over", [dict(), dict(d_state=16), dict(conv_kernel=2), dict(n_groups=4, d_state=64), dict(act_dtype="f16"), dict(head_dim=32, n_heads=16)],
                         ids=["base", "state16", "conv2", "groups4", "f16", "headdim32"])
@pytest.mark.parametrize("S", [8, 21])
def test_state_after_a_batched_prompt_matches_the_oracle(device, over, S):
    """every layer's SSM state and conv window after a batched prompt, against the oracle's: per layer a relative L2 within the bar of the logits these states produce
    (REL * TINY), and layer 0's window -- the rounded in_proj output and nothing else -- within one rounding interval, at most 1 % of its elements not the same bits.
    (With the default switches the 8-token prompts stay on the decode kernels, token by token; the 21-token ones take the batched route.)  Measured: DESIGN 5."""
    model = synth.make_mamba2("tiny-mamba2", **over)
    cfg = model["config"]
    act = cfg["act_dtype"]
    lm, om = runtime.LoadedModel.from_synth(device, model), orc_py.OrcMamba2(model)
    p = synth.prompt_tokens(S, cfg["vocab"], seed=23 + S)
    st, ost = runtime.LayeredSsmState(lm), om.new_state()
    lm.forward_with_ssm_state(p, st)
    om.forward(p, ost)
    want = [a.copy() for a in _orc_state(cfg, ost)]
    orc_py.lib().orc_ssm_state_free(ost)
    rel = lambda g, w: float(np.linalg.norm(g.astype(np.float64) - w) / max(np.linalg.norm(w.astype(np.float64)), 1e-30))
    bad = []
    for l, (ssm, win) in enumerate(_read_state(lm, st)):
        e_ssm, e_win = rel(ssm, want[0][l]), rel(win, want[1][l])
        print("S=%d layer %d: ssm rel L2 %.2e (%d of %d differ), window rel L2 %.2e (%d of %d differ)"
              % (S, l, e_ssm, int((ssm != want[0][l]).sum()), ssm.size, e_win, int((win != want[1][l]).sum()), win.size))
        if max(e_ssm, e_win) > REL[act] * TINY:
            bad.append((l, e_ssm, e_win))
        if l == 0:
            dist = np.abs(win.astype(np.float64) - want[1][0]) / _interval(want[1][0], act)
            print("S=%d layer 0 window: max %.3g intervals" % (S, float(dist.max())))
            assert dist.max() <= 1.0 and (win != want[1][0]).mean() <= 0.01, (float(dist.max()), float((win != want[1][0]).mean()))
    assert not bad, bad
