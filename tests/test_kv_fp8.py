"""The E4M3 quantiser (groundwork for an FP8 KV pool), on the CPU: the numpy reference quantiser (tests/kv_fp8_ref.py) against a hand table and, where torch has
the type, against torch.float8_e4m3fn on every f16 and bf16 bit pattern; the library's quantiser -- a host-and-device function body, evaluated on the host through
bz_fp8_e4m3_spec -- against that reference on the same patterns; exactness of every dequantised value in 16 bits."""
import ctypes as C

import numpy as np
import pytest

import kv_fp8_ref as F8
from blazr_amd import _lib as L

# value -> byte, written out by hand from the format (4 exponent bits, bias 7, 3 mantissa bits, subnormals in units of 2^-9, largest finite value 448)
HAND = [(1.0, 0x38), (1.0625, 0x38), (1.1875, 0x3A), (1.125, 0x39), (2.0 ** -10, 0x00), (1.01 * 2.0 ** -10, 0x01), (1.5 * 2.0 ** -9, 0x02), (2.0 ** -9, 0x01),
        (2.0 ** -6, 0x08), (7.5 * 2.0 ** -9, 0x08), (448.0, 0x7E), (449.0, 0x7E), (1000.0, 0x7E), (-1000.0, 0xFE), (np.inf, 0x7E), (-np.inf, 0xFE), (0.0, 0x00),
        (-0.0, 0x80), (np.nan, 0x7F), (-1.0625, 0xB8), (240.0, 0x77), (464.0, 0x7E)]


def _all16(act):
    u = np.arange(1 << 16, dtype=np.uint16)
    return F8.from16(u, act)


def _lib_quant(x, exp):
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    b, v = np.empty(x.size, np.uint8), np.empty(x.size, np.float32)
    L.check(L.lib().bz_fp8_e4m3_spec(x.ctypes.data_as(C.c_void_p), x.size, int(exp), b.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p)))
    return b, v


def test_reference_quantiser_hand_table():
    for x, want in HAND:
        got = int(F8.quant(np.float32(x))[()])
        assert got == want, (x, hex(got), hex(want))
    assert int(F8.quant(np.float32(2.125), 1)[()]) == 0x38 and int(F8.quant(np.float32(0.59375), -1)[()]) == 0x3A      # the same ties under a scale
    assert int(F8.quant(np.float32(900.0), 1)[()]) == 0x7E and int(F8.quant(np.float32(57344.0), 7)[()]) == 0x7E


def test_decode_table():
    t = F8.TABLE
    assert t[0x38] == 1.0 and t[0x7E] == 448.0 and t[0x01] == 2.0 ** -9 and t[0x08] == 2.0 ** -6 and t[0xFE] == -448.0 and np.isnan(t[0x7F]) and np.isnan(t[0xFF])
    fin = np.delete(np.arange(256), [0x7F, 0xFF])
    assert np.array_equal(F8.quant(t[fin]), fin.astype(np.uint8))                    # every finite code is a fixed point (the sign of -0 included)
    assert (np.diff(t[:0x7F]) > 0).all()


@pytest.mark.parametrize("act", ["f16", "bf16"])
def test_reference_quantiser_against_torch(act):
    torch = pytest.importorskip("torch")
    if not hasattr(torch, "float8_e4m3fn"):
        pytest.skip("this torch has no float8_e4m3fn")
    x = _all16(act)
    ok = np.isfinite(x) & (np.abs(x) <= 448.0)             # torch does not saturate: beyond 448 it gives NaN, which is the library's clamp's business
    want = torch.from_numpy(x[ok]).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert np.array_equal(F8.quant(x[ok]), want)
    back = torch.from_numpy(want).view(torch.float8_e4m3fn).to(torch.float32).numpy()
    assert np.array_equal(F8.dequant(want), back)


@pytest.mark.parametrize("act", ["f16", "bf16"])
@pytest.mark.parametrize("exp", [-5, -3, 0, 1, 6, 7])
def test_library_quantiser_equals_the_reference(act, exp):
    """every 16-bit pattern (NaNs, infinities, subnormals and both zeros included) through the library's quantiser on the host"""
    x = _all16(act)
    b, v = _lib_quant(x, exp)
    want = F8.quant(x, exp)
    bad = np.nonzero(b != want)[0]
    assert bad.size == 0, [(float(x[i]), hex(b[i]), hex(want[i])) for i in bad[:8]]
    fin = ~np.isnan(x)
    assert np.array_equal(v[fin], F8.dequant(want[fin], exp)) and np.isnan(v[~fin]).all()


def test_library_quantiser_hand_table_and_f32_inputs():
    xs = np.array([h[0] for h in HAND], np.float32)
    b, _ = _lib_quant(xs, 0)
    assert b.tolist() == [h[1] for h in HAND]
    rng = np.random.default_rng(8)
    x = np.concatenate([rng.standard_normal(20000) * s for s in (1e-3, 0.02, 1.0, 40.0, 600.0)]).astype(np.float32)    # f32 values, not 16-bit ones
    x = np.concatenate([x, np.float32([1e-45, -1e-45, 1e-38, 3e38, -3e38])])
    for exp in (-5, 0, 7):
        assert np.array_equal(_lib_quant(x, exp)[0], F8.quant(x, exp)), exp
    for bad in (-6, 8):
        with pytest.raises(L.BlazrHipError) as e:
            _lib_quant(xs, bad)
        assert e.value.code == L.E_INVALID


def test_every_dequantised_value_is_exact_in_16_bits():
    fin = np.delete(np.arange(256), [0x7F, 0xFF]).astype(np.uint8)
    for e in F8.EXP_RANGE:
        v = F8.dequant(fin, e)
        assert np.array_equal(v.astype(np.float16).astype(np.float32), v), e
        assert np.array_equal(((v.view(np.uint32) >> 16) << 16).view(np.float32), v), e            # bf16: the low 16 bits are zero
        nz = v[v != 0]
        assert np.abs(nz).min() >= 2.0 ** -14 and np.abs(v).max() < 65504.0, e                      # normal f16 numbers: no kernel's denormal mode matters
