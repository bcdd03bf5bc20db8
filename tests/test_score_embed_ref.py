"""The definitions of prompt scoring and pooling, pinned without a device: the library's host evaluations (bz_score_row_spec, bz_pool_spec -- the expressions the
kernels of bz_score.hip run) against the numpy restatement in score_ref.py, and the reference's own test vectors (server/pooling.rs, server/rerank.rs:260-281)
restated as data."""
import numpy as np
import pytest

import score_ref as SR
from blazr_amd import _lib as L
from blazr_amd import runtime

F = np.float32


@pytest.mark.parametrize("V", SR.VS)
def test_score_row_spec_matches_numpy(V):
    rows = SR.make_rows(V)
    for r in range(len(rows)):
        for t in SR.targets_for(V):
            for top_n in SR.TOP_NS if V < 33025 or r == 0 else (20,):
                rec = runtime.score_row_spec(rows[r], t, top_n)
                SR.check_record(rec, rows[r], t, top_n, "V=%d row=%d t=%d top_n=%d" % (V, r, t, top_n))


@pytest.mark.parametrize("V", (255, 1003))
def test_score_row_spec_nan_logits(V):
    """NaN logits are never counted and never listed; a NaN target has rank -1"""
    x = SR.nan_row(V)
    for t in (0, V - 1, int(np.nonzero(~np.isnan(x))[0][3])):
        rec = runtime.score_row_spec(x, t, 20)
        SR.check_record(rec, x, t, 20, "V=%d t=%d" % (V, t))
    assert int(runtime.score_row_spec(x, 0, 0)["rank"]) == -1


def test_rank_ties_and_zeros():
    x = np.array([1.0, -0.0, 0.0, 1.0, -np.inf, 0.0, 2.0], dtype=F)
    assert [int(runtime.score_row_spec(x, t, 0)["rank"]) for t in range(len(x))] == [1, 3, 4, 2, 6, 5, 0]
    rec = runtime.score_row_spec(x, 2, 20)
    assert list(rec["top_ids"][:int(rec["n_top"])]) == [6, 0, 3, 1, 2, 5, 4]


def test_score_spec_refusals():
    x = np.zeros(8, dtype=F)
    for t, n in ((8, 0), (-2, 0), (0, 21), (0, -1)):
        with pytest.raises(L.BlazrHipError) as e:
            runtime.score_row_spec(x, t, n)
        assert e.value.code == L.E_INVALID and str(t if n in (0,) else n) in str(e.value)


@pytest.mark.parametrize("S", SR.POOL_S)
@pytest.mark.parametrize("H", SR.POOL_H)
def test_pool_spec_matches_numpy(S, H):
    h = SR.pool_rows_case(S, H)
    for p in SR.POOLINGS:
        assert np.array_equal(runtime.pool_spec(h, p), SR.pool(h, p)), p
        got, want = runtime.pool_spec(h, p, normalize=True), SR.pool(h, p, normalize=True)
        assert got.shape == want.shape and SR.within_ulp(got, want), p
    if S > 1:
        assert not runtime.pool_spec(h, "none", normalize=True)[1].any()      # the zero vector stays zero
    assert not runtime.pool_spec(np.zeros((S, H), F), "mean", normalize=True).any()


def test_pool_spec_unknown_pooling():
    cfg = L.EmbedConfig(pooling=4)
    h, out = np.zeros((1, 8), F), np.zeros(8, F)
    assert L.lib().bz_pool_spec(h.ctypes.data, 1, 8, cfg, out.ctypes.data) == L.E_INVALID
    assert b"pooling = 4" in L.lib().bz_last_error()


def test_reference_pooling_vectors():
    """server/pooling.rs's own cases"""
    h = np.array([[1, 2, 3], [4, 5, 6]], dtype=F)
    assert np.array_equal(runtime.pool_spec(h, "mean"), F([2.5, 3.5, 4.5]))
    assert np.array_equal(runtime.pool_spec(h, "cls"), F([1, 2, 3]))
    assert np.array_equal(runtime.pool_spec(h, "last"), F([4, 5, 6]))
    n = runtime.pool_spec(np.array([[3, 4]], dtype=F), "last", normalize=True)
    assert abs(float(n[0]) - 0.6) < 1e-6 and abs(float(n[1]) - 0.8) < 1e-6


def test_reference_cosine_vectors():
    """server/rerank.rs:260-281"""
    assert abs(runtime.cosine_similarity([1, 2, 3], [1, 2, 3]) - 1.0) < 1e-6
    assert abs(runtime.cosine_similarity([1, 0], [0, 1])) < 1e-6
    assert abs(runtime.cosine_similarity([1, 0], [-1, 0]) + 1.0) < 1e-6
    assert runtime.cosine_similarity([1, 0], [1, 0, 0]) == 0.0 and runtime.cosine_similarity([0, 0], [1, 0]) == 0.0


def test_struct_layouts():
    import ctypes as C
    assert C.sizeof(L.ScoreRow) == runtime.SCORE_ROW.itemsize == 192
    assert C.sizeof(L.ScoreConfig) == 32 and C.sizeof(L.EmbedConfig) == 32 and C.sizeof(L.ScoreTotal) == 16
