"""Biased int4 linears against the oracle, bit for bit, on every form the library has for them.

The oracle's linear is R(RN32(sum) + bias); an int4 kernel that adds the bias into its exact fixed-point sum gives R(RN32(sum + bias)), which an ordinary
model shows in one output of 10^5.  tests/bias_cases.py builds one-layer GPTQ models (hidden 2048 and 4096, inter 384) whose biases put every output of
token T0 at position 0 on an f16 midpoint, where the wrong order flips more than a third of them (tests/test_linear_bias.py holds that on the CPU), one case
per group of linears and one with every group.  Every comparison here is np.array_equal against the oracle.

Routes: the default decode step (slim q/k/v, attention + o_proj, fused MLP), its three fallbacks and the two forms only an environment switch reaches
(one child process each: tests/bias_probe.py), the multi-row form as a decode batch and as a prompt.  The multi-row forms need K % 256 == 0 in every linear, which
inter 384 is not: a third width, h2048-i512, is there so that batches and prompts reach them (at the other two they run on the decode step).  Split-KV decode starts at position 4 at the earliest
and the construction does not reach past position 0: that route walks the `all` models over 10 positions and holds hidden, prev_mlp and the logits of
every position to the oracle's bits, unsensitised.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import bias_cases as bc
import bias_probe as bp
from blazr_amd import _lib as L
from blazr_amd import runtime
from oracle import orc_py

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PAIRS = [(w, c) for w in bc.WIDTHS for c in bc.CASES]
OBS = ("k0", "v0", "hidden", "prev_mlp", "logits")
MLP_LAUNCH, ATTN_LAUNCH, QKV_LAUNCH, BIAS_LAUNCH = "mlp_q4g<norm+gate/up+silu+down>", "attn+o_proj", "gemv_q4g<norm>", "fix_bias<f32 after the sum>"


def _diff(got, want, names, tag):
    """every named array equal; the message counts the differing elements of each"""
    bad = {}
    for k in names:
        n = int((np.asarray(got[k]) != np.asarray(want[k])).sum())
        print("%s %-8s %d of %d elements differ" % (tag, k, n, np.asarray(want[k]).size))
        if n:
            bad[k] = n
    assert not bad, (tag, bad)


@pytest.fixture(scope="module", params=PAIRS, ids=["%s-%s" % p for p in PAIRS])
def loaded(request, device):
    case = bc.get(*request.param)
    return case, runtime.LoadedModel.from_synth(device, case.model)


def test_default_decode_step(loaded, device):
    """T0 at position 0: K / V rows, hidden, prev_mlp and the logits row -- and the step's census names the launches this is about"""
    case, lm = loaded
    _diff(bp.run_step(device, lm, case.cfg), case.want, OBS, "%s %s step" % (case.width, case.case))
    kv = bp.new_kv(device, case.cfg)
    census = {r["name"]: r["launches"] for r in lm.profile_step(kv, bc.T0, 0, iters=1)}
    assert census.get(QKV_LAUNCH) == 1 and census.get(ATTN_LAUNCH) == 1 and census.get(MLP_LAUNCH) == 1, census
    # one pass per biased accumulator (gate / up's bias is added inside the fused MLP, where their sums are rounded)
    assert census.get(BIAS_LAUNCH, 0) == len([s for s in case.sites if s != "gate_up"]), census


def _route(lm, kind, rows):
    return runtime.prompt_plan(runtime.prompt_traits(lm), kind, rows, rows if kind == L.PLAN_PROMPT else 1)


_LMS = {}


def _lm(device, width, name):
    if (width, name) not in _LMS:
        case = bc.get(width, name)
        _LMS[width, name] = (case, runtime.LoadedModel.from_synth(device, case.model))
    return _LMS[width, name]


# With inter 384 down_proj's K is no multiple of 256 and a batch or prompt runs on the decode step; at h2048-i512 they take the multi-row int4 form
# (k_gemm_q4g_rows and its finish: asserted from the route plan).  From 5 rows on a decode batch takes the f16 MFMA GEMMs, whose f32 sums are held to a tolerance
# elsewhere: 8 rows are asked of the inter-384 widths, where they are 8 decode steps, and 3 and 4 (the last size of the multi-row form) of h2048-i512.
BATCHES = [(w, c, n) for w, c in PAIRS for n in ((3, 4) if w == bc.ROWS_WIDTH else (3, 8))]


@pytest.mark.parametrize("width,name,n", BATCHES, ids=["%s-%s-%d" % b for b in BATCHES])
def test_decode_batch_rows(device, width, name, n):
    """bz_forward_paged_batch, n sequences that all feed T0 at position 0: every row is sensitised; K / V rows out of the pool's blocks, logits rows"""
    case, lm = _lm(device, width, name)
    cfg = case.cfg
    if width == bc.ROWS_WIDTH:
        assert _route(lm, L.PLAN_DECODE_BATCH, n)["route"] == L.ROUTE_ROWS
    pool = runtime.LayeredPagedKvCache(device, 1, n, 16, cfg["n_kv_heads"], cfg["head_dim"], L.F16)
    got = lm.forward_paged_batch([bc.T0] * n, pool, [16 * b for b in range(n)], [[b] for b in range(n)], [1] * n).to_numpy()
    bad = []
    for b in range(n):
        k = pool.read_block(0, b, 0, cfg["n_kv_heads"], cfg["head_dim"], L.F16)[:, 0, :].reshape(-1).view(np.float16).astype(np.float32)
        v = pool.read_block(0, b, 1, cfg["n_kv_heads"], cfg["head_dim"], L.F16)[:, 0, :].reshape(-1).view(np.float16).astype(np.float32)
        d = [int((a != w).sum()) for a, w in ((k, case.want["k0"]), (v, case.want["v0"]), (got[b], case.want["logits"]))]
        print("%s %s batch %d row %d: k %d, v %d, logits %d elements differ" % (case.width, case.case, n, b, *d))
        if any(d):
            bad.append((b, d))
    assert not bad, bad


@pytest.mark.parametrize("S", [9, 16])
def test_prompt_rows(loaded, device, S):
    """a prompt starting with T0: row 0 is the oracle's, every row the token-by-token step's.  h2048-i512: on the exact rows (the multi-row form, 8 rows per
    pass; asserted from the route plan); the inter-384 widths: on the decode step"""
    case, lm = loaded
    if case.width == bc.ROWS_WIDTH:
        plan = _route(lm, L.PLAN_PROMPT, S)
        assert plan["route"] == L.ROUTE_ROWS and plan["exact"] == 1, plan
    got = bp.run_prompt(device, lm, case.cfg, S)
    _diff(got, case.want, ("k0", "v0", "logits"), "%s %s prompt %d row 0" % (case.width, case.case, S))
    kv = bp.new_kv(device, case.cfg)
    steps = np.concatenate([lm.forward_with_kv_cache([t], kv, i).to_numpy() for i, t in enumerate(bp.prompt(S))])
    assert np.array_equal(got["rows"], steps), [int((a != b).sum()) for a, b in zip(got["rows"], steps)]


# ---------------------------------------------------------------------------------------------------------
# routes behind a run-time switch: one fresh process each
# ---------------------------------------------------------------------------------------------------------
def _child(tmp_path, env, mode, pairs):
    src, dst = tmp_path / "biases.npz", tmp_path / "out.npz"
    arrs = {}
    for w, c in pairs:
        bs = bc.get(w, c).biases()
        for name, b in bs.items():
            arrs["%s/%s/%s" % (w, c, name)] = b
    np.savez(src, **arrs)
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(HERE, "bias_probe.py"), mode, str(src), str(dst)], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (env, mode, r.stdout[-2000:], r.stderr[-2000:])
    d = np.load(dst)
    return {(w, c): {k: d["%s/%s/%s" % (w, c, k)] for k in OBS if "%s/%s/%s" % (w, c, k) in d} for w, c in pairs}


def _all_pairs(got, names, tag):
    bad = {}
    for (w, c), g in got.items():
        want = bc.get(w, c).want
        for k in names:
            n = int((g[k] != want[k]).sum())
            print("%s %s %-7s %-8s %d of %d elements differ" % (tag, w, c, k, n, want[k].size))
            if n:
                bad[(w, c, k)] = n
    assert not bad, (tag, bad)


@pytest.mark.parametrize("switch", ["BZ_NO_SLIM_QKV", "BZ_NO_ATTN_FUSION", "BZ_NO_MLP_FUSION"])
def test_fallback_routes(tmp_path, switch):
    """the generic q/k/v GEMV, attention and o_proj as two launches, gate / up and down as two launches: the decode step of every case again"""
    _all_pairs(_child(tmp_path, {switch: "1"}, "step", PAIRS), OBS, switch)


def test_exact_integer_mfma_prompt(tmp_path):
    """BZ_EXACT_PREFILL=2: a 20-row prompt starting with T0 -- through k_gemm_q4g_i8 at h2048-i512 (on the decode step at the inter-384 widths); row 0's K / V and
    logits are the oracle's"""
    _all_pairs(_child(tmp_path, {"BZ_EXACT_PREFILL": "2"}, "prompt20", PAIRS), ("k0", "v0", "logits"), "BZ_EXACT_PREFILL=2")


_WALKS = {}


def _walk(tmp_path, env):
    key = tuple(sorted(env.items()))
    if key not in _WALKS:
        _WALKS[key] = _child(tmp_path, env, "walk10", [(w, "all") for w in bc.WIDTHS])
    return _WALKS[key]


def test_split_kv_merge_with_o_proj_is_merge_then_o_proj(tmp_path):
    """BZ_SPLIT_MIN=4: k_attn_merge_oproj (its own o_proj sums, the bias behind them) against the same split attention followed by the generic o_proj GEMV
    (BZ_NO_ATTN_FUSION=1), whose bias handling the step tests above hold to the oracle: the same bits at every position.  This pins the bias of the merged form
    without the split merge's own f32 rescaling, which the oracle does not share, in the way."""
    a, b = _walk(tmp_path, {"BZ_SPLIT_MIN": "4"}), _walk(tmp_path, {"BZ_SPLIT_MIN": "4", "BZ_NO_ATTN_FUSION": "1"})
    bad = {(w, k): int((a[w, c][k] != b[w, c][k]).sum()) for (w, c) in a for k in ("hidden", "prev_mlp", "logits") if not np.array_equal(a[w, c][k], b[w, c][k])}
    assert not bad, bad


def test_split_kv_decode_walk(tmp_path):
    """BZ_SPLIT_MIN=4: split-KV attention merged with the o_proj from position 4 on.  The construction does not reach past position 0, so this route is held
    unsensitised: the `all` models, 10 positions token by token, hidden / prev_mlp / logits of every position equal to the oracle's.

    This walk found a defect that is no bias: with f32 dot products and f32 P.V sums inside a slice, k_attn_split rounded an attention output element the
    other way at some positions from 4 on (elements of hidden / prev_mlp / logits off: h2048 position 5: 14 / 532 / 236; h4096 position 4: 91 / 1573 / 330;
    the same without any bias, and on the library before).  A slice now carries the oracle's sums (double over exact products, one rounding to f32), so a
    context that one slice covers -- these 10 positions -- has the oracle's bits.  Across slices (beyond 128 positions) the merge still rescales f32 partials:
    those contexts keep the tolerances of test_gpu_long_context.py and test_gpu_workloads.py, and this test does not speak for them."""
    got = _walk(tmp_path, {"BZ_SPLIT_MIN": "4"})
    bad = {}
    for (w, c), g in got.items():
        om = orc_py.OrcLlama(bc.get(w, c).model)
        okv = om.new_kv(16)
        for i, t in enumerate(bp.WALK):
            h, pm = om.layers_range(om.embed([t]), None, okv, 0, 1, i)
            want = dict(hidden=h.reshape(-1), prev_mlp=pm.reshape(-1), logits=om.head(h, pm).reshape(-1))
            for k, a in want.items():
                n = int((g[k][i] != a).sum())
                if n:
                    print("%s position %d %-8s %d of %d elements differ" % (w, i, k, n, a.size))
                    bad[(w, i, k)] = n
        orc_py.lib().orc_kv_free(okv)
    assert not bad, bad
