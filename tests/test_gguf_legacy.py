"""CPU checks of the GGUF legacy-quant additions (Q4_0, Q4_1, Q5_0, Q5_1): the numpy reference against hand-packed blocks with known answers,
the block sizes, and the ABI's ggml type ids."""
import os
import re

import numpy as np
import pytest

import legacy_quant_ref as lq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _raw(size, d, m=None, qh=None, qs=None):
    """a block packed byte by byte, independently of legacy_quant_ref.pack_block"""
    b = np.zeros(size, np.uint8)
    b[0:2] = np.array([d], np.float16).view(np.uint8)
    at = 2
    if m is not None:
        b[2:4] = np.array([m], np.float16).view(np.uint8)
        at = 4
    if qh is not None:
        b[at:at + 4] = [qh & 255, (qh >> 8) & 255, (qh >> 16) & 255, (qh >> 24) & 255]
        at += 4
    b[at:at + 16] = qs
    return b


def test_q4_0_nibble_order_and_offset():
    """low nibble of qs[j] is weight j, high nibble weight j + 16; y = (q - 8) d"""
    qs = np.full(16, 0x88, np.uint8)                      # every weight 8 -> 0
    qs[3] = 0x8F                                          # weight 3 -> 15, weight 19 -> 8
    qs[5] = 0x28                                          # weight 5 -> 8, weight 21 -> 2
    y = lq.dequant_blocks(lq.GGML_Q4_0, _raw(18, 0.5, qs=qs), 1, 32)[0]
    want = np.zeros(32, np.float32)
    want[3] = 7 * 0.5
    want[21] = -6 * 0.5
    assert np.array_equal(y, want)
    y0 = lq.dequant_blocks(lq.GGML_Q4_0, _raw(18, 0.25, qs=np.zeros(16, np.uint8)), 1, 32)[0]
    assert np.array_equal(y0, np.full(32, -8 * 0.25, np.float32))


def test_q4_1_offset_is_added_after_the_product():
    """y = q d + m, two float32 roundings in that order"""
    d, m = np.float32(np.float16(0.1)), np.float32(np.float16(-0.7))
    qs = np.zeros(16, np.uint8)
    qs[0] = 0x3F                                          # weight 0 -> 15, weight 16 -> 3
    y = lq.dequant_blocks(lq.GGML_Q4_1, _raw(20, 0.1, m=-0.7, qs=qs), 1, 32)[0]
    assert y[0] == np.float32(np.float32(15) * d) + m
    assert y[16] == np.float32(np.float32(3) * d) + m
    assert y[1] == m and y[31] == m


def test_q5_0_high_bit_mapping():
    """bit j of qh (little-endian u32) is the 5th bit of weight j, bit j + 16 that of weight j + 16; y = (q - 16) d"""
    for j in (0, 7, 8, 15, 16, 23, 24, 31):
        y = lq.dequant_blocks(lq.GGML_Q5_0, _raw(22, 1.0, qh=1 << j, qs=np.zeros(16, np.uint8)), 1, 32)[0]
        want = np.full(32, -16.0, np.float32)
        want[j] = 0.0
        assert np.array_equal(y, want), j
    qs = np.zeros(16, np.uint8)
    qs[2] = 0x5A                                          # weight 2 -> 10, weight 18 -> 5
    y = lq.dequant_blocks(lq.GGML_Q5_0, _raw(22, 0.5, qh=(1 << 2) | (1 << 18), qs=qs), 1, 32)[0]
    assert y[2] == (26 - 16) * 0.5 and y[18] == (21 - 16) * 0.5 and y[0] == -8.0


def test_q5_1_high_bit_and_offset():
    d, m = np.float32(np.float16(0.03)), np.float32(np.float16(-0.5))
    qs = np.zeros(16, np.uint8)
    qs[15] = 0xF1                                         # weight 15 -> 1, weight 31 -> 15
    y = lq.dequant_blocks(lq.GGML_Q5_1, _raw(24, 0.03, m=-0.5, qh=(1 << 31) | (1 << 15), qs=qs), 1, 32)[0]
    assert y[15] == np.float32(np.float32(17) * d) + m
    assert y[31] == np.float32(np.float32(31) * d) + m
    assert y[0] == m


@pytest.mark.parametrize("t", lq.LEGACY)
def test_pack_block_round_trips(t):
    rng = np.random.default_rng(t)
    q = rng.integers(0, 32 if t in (lq.GGML_Q5_0, lq.GGML_Q5_1) else 16, 32)
    d, m = np.float16(0.0123), np.float16(-0.21)
    y = lq.dequant_blocks(t, lq.pack_block(t, d, q, m), 1, 32)[0]
    d32, m32 = np.float32(d), np.float32(m)
    if t == lq.GGML_Q4_0:
        want = (q - 8).astype(np.float32) * d32
    elif t == lq.GGML_Q5_0:
        want = (q - 16).astype(np.float32) * d32
    else:
        want = q.astype(np.float32) * d32 + m32
    assert np.array_equal(y, want)


def test_block_sizes():
    assert lq.BLOCK_BYTES == {2: 18, 3: 20, 6: 22, 7: 24}
    for t, size in lq.BLOCK_BYTES.items():
        spec = lq.legacy_blocks("t", t, 64, 512)
        assert spec["blocks"].shape == (64, 512 // 32 * size)
        assert lq.row_bytes(t, 4096) * 8 == 4096 // 256 * {2: 144, 3: 160, 6: 176, 7: 192}[t] * 8
        w = lq.dequant(spec)
        assert w.dtype == np.float32 and np.isfinite(w).all() and 0 < np.abs(w).max() < 0.1


def test_mixed_layout_types():
    model = lq.make_model("mixed", n_layers=2)
    lay = model["layers"][0]
    assert lay["q"]["ggml_type"] == 12 and lay["v"]["ggml_type"] == lq.GGML_Q5_0 and lay["down"]["ggml_type"] == lq.GGML_Q5_1
    om = lq.oracle_model(model)
    assert om["layers"][0]["v"]["kind"] == "dense" and om["layers"][0]["q"]["kind"] == "gguf"


def test_header_declares_legacy_types():
    text = open(os.path.join(ROOT, "include", "blazr_hip.h")).read()
    enum = re.search(r"enum\s*\{([^}]*BZ_GGML_F32[^}]*)\}", text).group(1)
    vals = dict((k, int(v)) for k, v in re.findall(r"(BZ_GGML_\w+)\s*=\s*(\d+)", enum))
    assert vals.get("BZ_GGML_Q4_0") == 2
    assert vals.get("BZ_GGML_Q4_1") == 3
    assert vals.get("BZ_GGML_Q5_0") == 6
    assert vals.get("BZ_GGML_Q5_1") == 7
