"""CPU checks of the GGUF k-quant additions: the numpy Q5_K reference against hand-built blocks with known answers, and the ABI's ggml type id."""
import os
import re

import numpy as np

import kquant_ref as kq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _block(d, dmin, scales12, qh, qs):
    b = np.zeros(176, dtype=np.uint8)
    b[0:2] = np.array([d], np.float16).view(np.uint8)
    b[2:4] = np.array([dmin], np.float16).view(np.uint8)
    b[4:16], b[16:48], b[48:176] = scales12, qh, qs
    return b


def test_q5k_high_bit_selects_sub_block():
    """bit j of qh[l] is the 5th bit of element l of sub-block j (and only of that one)"""
    sc = np.zeros(12, np.uint8)
    sc[0:4] = 1                                  # sub-blocks 0..3: scale 1, min 0
    sc[8:12] = 1                                 # sub-blocks 4..7: scale (s[j+4] & 15) = 1, min (s[j+4] >> 4) = 0
    for j in range(8):
        qh = np.zeros(32, np.uint8)
        qh[5] = 1 << j
        y = kq.q5k_dequant(_block(1.0, 0.0, sc, qh, np.zeros(128, np.uint8)), 1, 256)[0]
        want = np.zeros(256, np.float32)
        want[32 * j + 5] = 16.0
        assert np.array_equal(y, want), j


def test_q5k_nibbles_and_scale_min_packing():
    """low nibbles of qs[32 (j/2) + l] (even j) / high nibbles (odd j); 6-bit scale / min for j < 4 and the split packing for j >= 4"""
    sc = np.zeros(12, np.uint8)
    sc[0], sc[4] = 3 | (1 << 6), 2 | (2 << 6)     # j = 0: sc 3, m 2 ; high bits feed j = 4 (sc += 16) and j = 4's min (+= 32)
    sc[8] = 5 | (7 << 4)                          # j = 4: sc = 5 | (s[0] >> 6) << 4 = 21, m = 7 | (s[4] >> 6) << 4 = 39
    qs = np.zeros(128, np.uint8)
    qs[0], qs[1] = 0x9 | (0x4 << 4), 0xF          # element 0 of j = 0 -> 9, of j = 1 -> 4 ; element 1 of j = 0 -> 15
    qs[64] = 0x6                                  # element 0 of j = 4 -> 6
    qh = np.zeros(32, np.uint8)
    qh[0] = 1 | (1 << 4)                          # +16 on element 0 of j = 0 and of j = 4
    y = kq.q5k_dequant(_block(0.5, 0.25, sc, qh, qs), 1, 256)[0]
    assert y[0] == np.float32(0.5 * 3) * 25 - np.float32(0.25 * 2)
    assert y[1] == np.float32(0.5 * 3) * 15 - np.float32(0.25 * 2)
    assert y[32] == 0.0 * 4 - 0.0                 # j = 1: scale 0, min 0
    assert y[128] == np.float32(0.5 * 21) * 22 - np.float32(0.25 * 39)
    assert y[129] == -np.float32(0.25 * 39)


def test_q5k_generator_is_well_conditioned():
    spec = kq.q5k_blocks("t", 64, 512)
    assert spec["blocks"].shape == (64, 2 * 176)
    w = kq.q5k_dequant(spec["blocks"], 64, 512)
    assert np.isfinite(w).all() and 0 < np.abs(w).max() < 0.3


def test_header_declares_q5_k():
    text = open(os.path.join(ROOT, "include", "blazr_hip.h")).read()
    enum = re.search(r"enum\s*\{([^}]*BZ_GGML_F32[^}]*)\}", text).group(1)
    vals = dict((k, int(v)) for k, v in re.findall(r"(BZ_GGML_\w+)\s*=\s*(\d+)", enum))
    assert vals.get("BZ_GGML_Q5_K") == 13
