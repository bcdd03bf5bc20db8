"""Fused MLP kernel alone (bz_tune_mlp): mean dispatch time on cold weights.
usage: python scripts/tune_mlp.py"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from blazr_amd import _lib as L, runtime  # noqa: E402

dev = runtime.Device(0)
us = C.c_double()
for rep in range(3):
    L.check(L.lib().bz_tune_mlp(dev.h, 4096, 14336, 6, 40, 0, C.byref(us), None))
    print("mlp H=4096 I=14336: %.2f us per launch (91.52 MB -> %.0f GB/s)" % (us.value, 91.521024e6 / us.value / 1e3))
dev.close()
