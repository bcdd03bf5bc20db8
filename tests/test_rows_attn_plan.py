"""The host side of the batched decode attention at long contexts (bz_rows_attn_plan, bz_rows_attn_slice_len): which kernel a decode batch launches, the
slice rule the device applies, and the workspace formula of DESIGN section 4.  No device is needed."""
import pytest

from blazr_amd import _lib as L
from blazr_amd import runtime

LIMITS = {1: 38888, 2: 18416, 4: 8180, 8: 3062}         # last context the scalar kernel holds: (8 REP + 2048 REP) 4 + REP len 4 + 64 <= 160 KiB
MAX_SLICES, SLICE_MIN, WS_CAP = 64, 128, 128 << 20


@pytest.fixture(autouse=True)
def _no_switch(monkeypatch):
    monkeypatch.delenv("BZ_ROWS_SPLIT_MIN", raising=False)


def _plan(rep, hd, dt=L.F16, window=0, n=4, cap=1024, nkv=2):
    return runtime.rows_attn_plan(nkv * rep, nkv, hd, dt, window, n, cap)


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("rep", [1, 2, 4, 8])
def test_scalar_limit_and_switch_one_position_beyond(rep, hd):
    lim = LIMITS[rep]
    assert 4 * (8 * rep + (256 // (hd // 8)) * rep * hd) + 4 * rep * lim + 64 <= 160 * 1024 < 4 * (8 * rep + (256 // (hd // 8)) * rep * hd) + 4 * rep * (lim + 1) + 64
    for dt in (L.F16, L.BF16):
        at, beyond = _plan(rep, hd, dt, cap=lim), _plan(rep, hd, dt, cap=lim + 1)
        assert at["scalar_limit"] == beyond["scalar_limit"] == lim
        assert at["kernel"] == 0 and at["grid_slices"] == 0 and at["ws_bytes"] == 0
        assert beyond["kernel"] == 1 and beyond["grid_slices"] == min(-(-(lim + 1) // SLICE_MIN), MAX_SLICES)


def test_window_decides_not_the_capacity():
    for cap in (4096, 8181, 131072, 1 << 30):
        assert _plan(4, 128, window=4096, cap=cap)["kernel"] == 0          # a window that fits keeps the scalar kernel at any capacity
        assert _plan(4, 128, window=8180, cap=cap)["kernel"] == 0
    assert _plan(4, 128, window=8181, cap=8180)["kernel"] == 0             # ... and so does a capacity inside a window that does not
    p = _plan(4, 128, window=8181, cap=131072)
    assert p["kernel"] == 1 and p["grid_slices"] == 64                     # 8 181 keys at most: 64 slices of 128
    assert _plan(8, 128, window=4096, cap=131072)["grid_slices"] == 32


@pytest.mark.parametrize("kw", [dict(hd=128, dt=L.F32), dict(hd=64, dt=L.F32), dict(hd=96), dict(hd=96, dt=L.BF16)], ids=["f32-128", "f32-64", "hd96", "hd96-bf16"])
def test_refused_beyond_the_limit(kw):
    inside = _plan(4, cap=4096, **kw)
    assert inside["kernel"] == 0 and inside["code"] == L.OK
    p = _plan(4, cap=20000, **kw)
    assert p["kernel"] == -1 and p["code"] == L.E_UNSUPPORTED
    assert str(p["scalar_limit"]) in p["error"] and "20000" in p["error"], p["error"]
    if kw["hd"] != 96:
        assert p["scalar_limit"] == LIMITS[4]


def test_switch_lowers_the_threshold(monkeypatch):
    monkeypatch.setenv("BZ_ROWS_SPLIT_MIN", "100")          # read per call
    assert _plan(4, 128, cap=99)["kernel"] == 0 and _plan(4, 128, cap=100)["kernel"] == 1
    assert _plan(4, 128, dt=L.F32, cap=100)["kernel"] == 0   # where the pair is not built the scalar kernel stays, inside its limit
    monkeypatch.setenv("BZ_ROWS_SPLIT_MIN", "1")
    assert _plan(4, 128, cap=1)["kernel"] == 1 and _plan(4, 128, cap=1)["grid_slices"] == 1


def _lens():
    out = set(range(1, 4097)) | {70001}
    p = 1
    while p <= 131072:
        out |= {p - 1, p, p + 1}
        p *= 2
    return sorted(x for x in out if x >= 1)


def test_slice_rule_sweep():
    """every len: the slices cover [0, len), the last one is not empty, and their count stays within the grid of every capacity >= len"""
    prev = 0
    for n in _lens():
        spl = runtime.rows_attn_slice_len(n)
        ref = SLICE_MIN
        while -(-n // ref) > MAX_SLICES:
            ref *= 2
        assert spl == ref, (n, spl)
        assert spl >= prev                                   # monotone: a longer row never gets shorter slices
        prev = spl
        ns = -(-n // spl)
        assert 1 <= ns <= MAX_SLICES
        assert (ns - 1) * spl < n <= ns * spl                # cover, last slice non-empty
        for cap in {n, n + 1, 2 * n, 131072, 1 << 20}:
            if cap >= n:
                assert ns <= min(-(-cap // SLICE_MIN), MAX_SLICES), (n, cap)
    # the plan's grid is that bound (Llama-3-8B heads; any capacity beyond the limit)
    for cap in (8181, 16384, 70001, 131072):
        assert _plan(4, 128, nkv=8, cap=cap)["grid_slices"] == min(-(-cap // SLICE_MIN), MAX_SLICES)


@pytest.mark.parametrize("n,cap,want_rows,want_bytes", [(64, 16384, 64, 64 * 32 * 64 * 132 * 4), (512, 16384, 124, 124 * 32 * 64 * 132 * 4), (4, 8181, 4, 4 * 32 * 64 * 132 * 4)])
def test_workspace_formula_llama3_8b(n, cap, want_rows, want_bytes):
    """ws_bytes = rows_per_pass x n_heads x slices x (HD + 4) x 4, rows_per_pass = min(N, 512, 128 MiB // (n_heads x slices x (HD + 4) x 4)), at least 1"""
    p = _plan(4, 128, nkv=8, n=n, cap=cap)
    per_row = 32 * p["grid_slices"] * (128 + 4) * 4
    assert p["rows_per_pass"] == max(1, min(n, 512, WS_CAP // per_row)) == want_rows
    assert p["ws_bytes"] == p["rows_per_pass"] * per_row == want_bytes
    assert p["ws_bytes"] <= WS_CAP


def test_workspace_formula_other_shapes():
    for rep, hd, nkv, n, cap in [(8, 64, 1, 3, 3328), (8, 128, 8, 512, 131072), (1, 128, 8, 2, 40000), (2, 64, 4, 17, 20000)]:
        p = _plan(rep, hd, nkv=nkv, n=n, cap=cap)
        per_row = rep * nkv * p["grid_slices"] * (hd + 4) * 4
        assert p["kernel"] == 1
        assert p["rows_per_pass"] == max(1, min(n, 512, WS_CAP // per_row))
        assert p["ws_bytes"] == p["rows_per_pass"] * per_row
