"""The numpy restatement of the device logprobs / logit bias (tests/logprobs_ref.py) against the host routines the single-sequence loop uses
(bz_compute_logprobs, bz_apply_logit_bias: sampling.rs:197-256, 464-480), against the Python restatement of the reference (test_sampler_host.py:
py_logprobs), and against a float64 log-softmax -- no GPU.  The GPU tests then hold the kernels to the restatement exactly."""
import ctypes as C

import numpy as np
import pytest

import logprobs_ref as R
from blazr_amd import _lib as L
from test_sampler_host import py_logprobs

F = np.float32
VS = (7, 1001, 32003)


def _decided_rows(V):
    x = R.make_rows(V)
    for k, kind in enumerate(R.ROW_KINDS):
        yield kind, x[k]


@pytest.mark.parametrize("V", VS)
def test_ids_and_n_top_equal_the_host_routine(V):
    checked = 0
    for kind, x in _decided_rows(V):
        for top_n in (0, 1, 5, 20, 50):
            want = R.logprobs_row(x, top_n)
            chosen = int(np.argmax(x))
            clp, ids, lps = R.host_logprobs(x, chosen, top_n)
            assert want["n_top"] == len(ids) == min(top_n, V, 20), (kind, top_n)
            host_lse = F(x[chosen] - clp)
            # the reference orders by logprob; where distinct logits give distinct logprobs (under either lse) that is the order by logit, lower id first on ties
            if R.order_is_decided(x, want["lse"], want["n_top"]) and R.order_is_decided(x, host_lse, want["n_top"]) and np.isfinite(x).all():
                assert want["top_ids"].tolist() == ids.tolist(), (kind, top_n)
                checked += 1
    assert checked >= 15, checked


def test_ids_equal_the_python_restatement_of_the_reference():
    rng = np.random.default_rng(5)
    for V in (7, 257):
        x = (rng.standard_normal(V) * 3).astype(F)
        for top_n in (1, 5, 20):
            _, ids, _ = py_logprobs(list(x), 0, top_n)
            want = R.logprobs_row(x, top_n)
            assert R.order_is_decided(x, want["lse"], want["n_top"])
            assert want["top_ids"].tolist() == list(ids), (V, top_n)


@pytest.mark.parametrize("V", VS)
def test_values_against_float64(V):
    for kind, x in _decided_rows(V):
        want = R.logprobs_row(x, 20)
        ref = R.log_softmax64(x)
        for i, lp in zip(want["top_ids"], want["top_logprobs"]):
            if np.isfinite(lp):
                assert abs(float(lp) - ref[i]) <= R.value_bound(x, lp), (kind, int(i), float(lp), ref[i])
            else:
                assert x[i] == -np.inf and lp == -np.inf, (kind, int(i))


def test_known_rows():
    M, S, Lg, lse = R.lse_parts(np.full(8, 1.25, dtype=F))
    assert S == 8 << 40 and lse == F(F(np.log(8.0)) + F(1.25))
    x = R.make_rows(1001)[4]                                         # one dominant logit: every other q_i is 0
    M, S, Lg, lse = R.lse_parts(x)
    assert S == 1 << 40 and Lg == 0 and lse == M == F(140.0)
    assert R.logprobs_row(np.full(1001, 0.5, dtype=F), 20)["top_ids"].tolist() == list(range(20))      # an all-equal row: ids 0 .. n-1
    assert R.logprobs_row(np.full(7, 0.5, dtype=F), 20)["n_top"] == 7
    z = np.array([0.0, -0.0, 0.0, -1.0], dtype=F)                    # signed zeros tie: the id decides
    assert R.order(z, 3).tolist() == [0, 1, 2]


def _dedupe_lib(V, ids, vals):
    ids = np.ascontiguousarray(ids, dtype=np.uint32); vals = np.ascontiguousarray(vals, dtype=F)
    oi, ov, n = np.zeros(max(len(ids), 1), np.uint32), np.zeros(max(len(ids), 1), F), C.c_int()
    rc = L.lib().bz_logit_bias_dedupe(V, ids.ctypes.data_as(C.c_void_p) if len(ids) else None, vals.ctypes.data_as(C.c_void_p) if len(vals) else None, len(ids),
                                      oi.ctypes.data_as(C.c_void_p), ov.ctypes.data_as(C.c_void_p), C.byref(n))
    return rc, oi[:n.value], ov[:n.value]


def test_bias_dedupe_against_apply_logit_bias():
    rng = np.random.default_rng(9)
    V = 1001
    x = (rng.standard_normal(V) * 2).astype(F)
    x[[5, 900]] = -np.inf
    cases = {"empty": ([], []),
             "duplicates_last_wins": ([4, 17, 4, 900, 17, 4], [1.0, -2.5, 3.0, 7.0, 0.25, -100.0]),
             "out_of_range": ([V, 3, V + 5, 2 ** 32 - 1, V - 1], [9.0, 1.5, 9.0, 9.0, -4.0]),
             "many": (rng.integers(0, V + 50, size=2000), (rng.standard_normal(2000) * 5))}
    for name, (ids, vals) in cases.items():
        rc, oi, ov = _dedupe_lib(V, ids, vals)
        assert rc == L.OK, name
        ri, rv = R.dedupe(V, ids, vals)
        assert oi.tolist() == ri.tolist() and ov.view(np.uint32).tolist() == rv.view(np.uint32).tolist(), name
        assert len(set(oi.tolist())) == len(oi) and (oi < V).all(), name                                   # unique, in range: the device add is race-free
        want = R.host_apply_bias(x, ids, vals)
        got = R.apply_bias(x, ids, vals)
        assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist(), name
    assert _dedupe_lib(V, [4, 17, 4], [1.0, 2.0, 3.0])[2].tolist() == [3.0, 2.0]
    assert len(_dedupe_lib(V, [V, V + 1], [1.0, 2.0])[1]) == 0
    assert np.isneginf(R.apply_bias(x, [5], [1000.0])[5])                                                  # -inf + bias stays -inf
    for bad in (np.nan, np.inf, -np.inf):
        rc, _, _ = _dedupe_lib(V, [3, 4], [1.0, bad])
        assert rc == L.E_INVALID and b"not a finite number" in L.lib().bz_last_error(), bad
