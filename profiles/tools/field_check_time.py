"""Time of the host-side field check of the byte entry points, alone: the check reads every input symbol on the
calling thread before anything is staged.  A GF(2^7) code whose LAST input symbol is 128 makes cc_correct_hard_batch and
cc_encode_batch read the whole input and answer CC_ERR_NOT_IN_FIELD, so nothing reaches the device.  The input has the
size of the RS(255,223) inputs of host_path_bench.py (2^20 x 255 and 2^20 x 223 bytes)."""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import channelcoding_amd as cc
from channelcoding_amd import capi

NOT_IN_FIELD = 7
lib = capi.lib()
rs = cc.rs(7, cc.errors(4), cc.berlekamp_massey_tag())
P = lambda a: a.ctypes.data_as(C.c_void_p)


def timed(call, reps=5):
    assert call() == NOT_IN_FIELD
    best = 1e9
    for _ in range(reps):
        t0 = time.perf_counter()
        assert call() == NOT_IN_FIELD
        best = min(best, time.perf_counter() - t0)
    return best


for name, width, total in (("cc_correct_hard_batch", rs.n, (1 << 20) * 255), ("cc_encode_batch", rs.l, (1 << 20) * 223)):
    B = total // width
    x = np.zeros((B, width), np.uint8)
    x[-1, -1] = 128
    out = np.ones((B, rs.n), np.uint8)
    if name == "cc_encode_batch":
        dt = timed(lambda: lib.cc_encode_batch(rs._h, P(x), P(out), B))
    else:
        dt = timed(lambda: lib.cc_correct_hard_batch(rs._h, P(x), None, None, P(out), None, None, B))
    print("field check of %s, %d bytes: %.2f ms  (%.2f GB/s, best of 5)" % (name, B * width, dt * 1e3, B * width / dt / 1e9),
          flush=True)
