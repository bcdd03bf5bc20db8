"""Batched device sampler, CPU side: the C-ABI surface, and the numpy restatement of the per-row semantics (tests/batch_sampler_ref.py) against the oracle
on every case the GPU tests use -- with the decision margin of every case above the bound, so the GPU comparison excludes none."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from blazr_amd import _lib as L
from oracle import orc_py

import batch_sampler_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bz_batch_sampler_create", "bz_batch_sampler_free", "bz_batch_sampler_set_row", "bz_batch_sampler_sample", "bz_decode_batch_graph_capture_sampled"]


def test_symbols_declared_mirrored_and_exported():
    header = open(os.path.join(ROOT, "include", "blazr_hip.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in L.SYMBOLS, name
    assert "#define BZ_SAMPLER_WINDOW_MAX 256" in header and L.SAMPLER_WINDOW_MAX == 256
    assert "#define BZ_ABI_VERSION 4" in header and L.ABI_VERSION == 4
    assert C.sizeof(L.RowSampling) == 56                     # 8 x 4 bytes, the 64-bit seed, 4 reserved words
    lib = L.lib()                                            # binds every entry of SYMBOLS: a missing export raises here
    for name in NEW:
        assert getattr(lib, name) is not None
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r" T %s$" % name, out, re.M), name


def test_create_without_a_device_is_refused():
    h = C.c_void_p()
    rc = L.lib().bz_batch_sampler_create(None, 4, 1000, C.byref(h))
    assert rc in (L.E_NODEVICE, L.E_INVALID) and not h.value
    assert b"device" in L.lib().bz_last_error()
    assert L.lib().bz_batch_sampler_free(None) == L.OK
    p = L.RowSampling(temperature=1.0)
    assert L.lib().bz_batch_sampler_set_row(None, 0, C.byref(p), None, 0, 0) == L.E_INVALID
    assert L.lib().bz_batch_sampler_sample(None, None, None) == L.E_INVALID
    assert L.lib().bz_decode_batch_graph_capture_sampled(None, None, 4, 1, None, C.byref(h)) == L.E_INVALID


def test_expf_restatement_is_the_oracles_bits():
    rng = np.random.default_rng(3)
    x = np.concatenate([-(rng.random(4000) * 90).astype(np.float32), np.float32([0.0, -0.0, -86.0, -86.5, -100.0, -np.inf, np.nan])])
    got = R.expf_spec(x)
    lib = orc_py.lib()
    want = np.float32([lib.orc_expf(float(v)) for v in x])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_penalty_window_restatement():
    from blazr_amd import runtime
    rng = np.random.default_rng(5)
    for n, last in ((0, 64), (3, 1), (300, 256), (70, 64), (10, 4)):
        h = rng.integers(0, 9, size=n).tolist()
        a, b = R.penalty_window(h, last), runtime.penalty_window(h, last)
        assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist()


@pytest.mark.parametrize("N,V", R.GRID)
def test_restatement_equals_oracle_and_no_case_is_marginal(N, V):
    logits, rows = R.make_case(N, V, R.case_id(N, V))
    low = []
    for r, kw in enumerate(rows):
        tok, margin = R.sample_row(logits[r], **kw)
        assert tok == R.oracle_row(logits[r], kw), (N, V, r, kw)
        if margin < R.MARGIN:
            low.append((N, V, r, margin))
    assert not low, "replace these seeds (batch_sampler_ref.SEED_SHIFT): %s" % low


def test_degenerate_rows_restatement_equals_oracle():
    for name, (logits, rows) in R.degenerate_cases().items():
        for r, kw in enumerate(rows):
            tok, _ = R.sample_row(logits[r], **kw)
            if tok < 0:
                continue                                     # a row without mass: the oracle's id is not specified either
            assert tok == R.oracle_row(logits[r], kw), (name, r)
