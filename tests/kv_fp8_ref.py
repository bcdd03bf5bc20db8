"""Reference side of the E4M3 quantiser (OCP e4m3fn; groundwork for an FP8 paged KV pool): a numpy quantiser / dequantiser that restates the library's rule
independently.

The rule (include/blazr_hip.h, bz_fp8_e4m3_spec): stored byte = e4m3(x * 2^-exp), value read = e4m3 * 2^exp.  The quantiser multiplies by 2^-exp (exact),
clamps to +-448, rounds to nearest even -- below 2^-6 onto the subnormal grid of 2^-9 -- and maps NaN to 0x7F.  Every one of the 256 values times 2^e,
e in [-5, 7], is exact in f16 and in bf16, so a 16-bit row can hold a dequantised row exactly."""
import numpy as np

EXP_RANGE = range(-5, 8)


def _decode_table():
    t = np.zeros(256, np.float64)
    for b in range(256):
        e, m = (b >> 3) & 15, b & 7
        if (b & 0x7F) == 0x7F:
            v = np.nan
        elif e == 0:
            v = m * 2.0 ** -9
        else:
            v = (1.0 + m / 8.0) * 2.0 ** (e - 7)
        t[b] = -v if b & 0x80 else v
    return t


TABLE = _decode_table()                     # byte -> value (float64; NaN at 0x7F / 0xFF)
_POS = TABLE[:0x7F].copy()                  # the 127 non-negative finite values, ascending: 0 .. 448


def quant(x, exp=0):
    """float array -> uint8 E4M3 bytes of x * 2^-exp.  Nearest value of the 127-entry magnitude grid by search, ties to the even code: no bit tricks shared
    with the library's quantiser."""
    x = np.asarray(x, np.float64)
    y = np.abs(x) * 2.0 ** -exp
    y = np.minimum(np.where(np.isnan(y), 0.0, y), 448.0)
    hi = np.clip(np.searchsorted(_POS, y, side="left"), 1, 126)          # _POS[hi - 1] <= y <= _POS[hi] (or y == 0)
    lo = hi - 1
    dl, dh = y - _POS[lo], _POS[hi] - y
    code = np.where(dl < dh, lo, np.where(dh < dl, hi, np.where(lo % 2 == 0, lo, hi)))
    out = (code | np.where(np.signbit(x), 0x80, 0)).astype(np.uint8)
    return np.where(np.isnan(x), np.uint8(0x7F), out).astype(np.uint8)


def dequant(b, exp=0):
    """uint8 E4M3 bytes -> float32 values times 2^exp (exact)"""
    return (TABLE[np.asarray(b, np.uint8)] * 2.0 ** exp).astype(np.float32)


def roundtrip(x, exp=0):
    return dequant(quant(x, exp), exp)


def from16(u16, act):
    """the 16-bit patterns a pool stores -> float32"""
    u16 = np.ascontiguousarray(u16, np.uint16)
    if act == "f16":
        return u16.view(np.float16).astype(np.float32)
    return (u16.astype(np.uint32) << 16).view(np.float32)
