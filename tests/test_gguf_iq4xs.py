"""CPU: the IQ4_XS reference dequantiser on a hand-built block with known answers, and the new enum values."""
import os
import re

import numpy as np

import iq4xs_ref as iq
from blazr_amd import _lib as L

LS = [0, 32, 63, 17, 47, 1, 62, 33]      # the extremes, the zero point, and both halves of every scales_h / scales_l byte


def test_dequant_hand_built_block():
    codes = np.concatenate([np.concatenate([np.arange(16), 15 - np.arange(16)]) for _ in range(8)])     # low nibble j, high nibble 15 - j
    b = iq.pack_block(2.0 ** -10, LS, codes)
    assert b[2:4].view("<u2")[0] == 45688 and list(b[4:8]) == [0, 31, 31, 30] and b[8] == 0xF0 and b[8 + 15] == 0x0F    # worked out by hand from LS
    y = iq.dequant_blocks(b, 1, 256)[0]
    for ib, ls in enumerate(LS):
        for j in range(16):      # exact: small integers times a power of two
            assert y[32 * ib + j] == 2.0 ** -10 * (ls - 32) * iq.KV[j] and y[32 * ib + j + 16] == 2.0 ** -10 * (ls - 32) * iq.KV[15 - j], (ib, j)
    assert not y[32:64].any() and y[64] == 2.0 ** -10 * 31 * -127 and y[0] == 2.0 ** -10 * 32 * 127


def test_enum_values():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "blazr_hip.h")).read()
    assert re.search(r"\bBZ_GGML_IQ4_XS = 23\b", hdr) and re.search(r"\bBZ_LIN_IQ4XS = 15\b", hdr) and L.LIN_IQ4XS == 15
