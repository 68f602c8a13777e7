"""PCIe-inclusive rates of the host-pointer entry points (never the headline `value`): caller-owned, pre-touched
buffers passed straight to the C ABI.  cc_correct_soft_batch with pageable and page-locked buffers, then the byte paths
cc_correct_hard_batch and cc_encode_batch of RS(255,223) with pageable buffers."""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
import channelcoding_amd as cc
from channelcoding_amd import capi

code = cc.primitive_bch(8, cc.errors(3), cc.min_sum_tag(20))
lib = capi.lib()
rng = np.random.default_rng(0)
P = lambda a: a.ctypes.data_as(C.c_void_p)


def run(y, hard, iters, status, B, reps=3):
    lib.cc_correct_soft_batch(code._h, P(y), None, None, P(hard), None, P(iters), P(status), B)
    t0 = time.perf_counter()
    for _ in range(reps):
        rc = lib.cc_correct_soft_batch(code._h, P(y), None, None, P(hard), None, P(iters), P(status), B)
        assert rc == 0
    return (time.perf_counter() - t0) / reps


for log2b, ebno in ((10, 4.0), (14, 4.0), (16, 4.0), (18, 4.0), (20, 4.0), (20, 8.0)):
    B = 1 << log2b
    y = (1.0 + code.sigma(ebno) * rng.standard_normal((B, 255), dtype=np.float32)).astype(np.float32)
    hard = np.ones((B, 255), np.uint8)
    iters = np.ones(B, np.uint16)
    status = np.ones(B, np.int32)
    dt = run(y, hard, iters, status, B)
    print("pageable buffers, B=2^%d, %.0f dB: %.2f M frames/s  (%.2f ms, %.2f GB/s of LLR in)" % (
        log2b, ebno, B / dt / 1e6, dt * 1e3, B * 1020 / dt / 1e9), flush=True)
    if log2b == 20:
        yp = torch.from_numpy(y).pin_memory().numpy()
        hp = torch.from_numpy(hard).pin_memory().numpy()
        ip = torch.from_numpy(iters.view(np.int16)).pin_memory().numpy()
        sp = torch.from_numpy(status).pin_memory().numpy()
        dt = run(yp, hp, ip, sp, B)
        print("page-locked buffers, B=2^%d, %.0f dB: %.2f M frames/s  (%.2f ms, %.2f GB/s of LLR in)" % (
            log2b, ebno, B / dt / 1e6, dt * 1e3, B * 1020 / dt / 1e9), flush=True)


# the byte paths: RS(255,223) BM, 2^20 frames, 0..16 symbol errors per frame (4096 distinct frames, tiled)
rs = cc.rs(8, cc.errors(16), cc.berlekamp_massey_tag())
B = 1 << 20
msg = np.tile(rng.integers(0, 256, (4096, rs.l)).astype(np.uint8), (B // 4096, 1))
cw = np.ones((B, rs.n), np.uint8)
noise = np.zeros((4096, rs.n), np.uint8)
for f in range(4096):
    pos = rng.choice(rs.n, int(rng.integers(0, 17)), replace=False)
    noise[f, pos] = rng.integers(1, 256, len(pos))


def timed(call, reps=3):
    assert call() == 0
    t0 = time.perf_counter()
    for _ in range(reps):
        assert call() == 0
    return (time.perf_counter() - t0) / reps


dt = timed(lambda: lib.cc_encode_batch(rs._h, P(msg), P(cw), B))
print("pageable buffers, B=2^20, RS(255,223) cc_encode_batch: %.2f M frames/s  (%.2f ms, %.2f GB/s of codewords out)" % (
    B / dt / 1e6, dt * 1e3, B * rs.n / dt / 1e9), flush=True)
rx = cw ^ np.tile(noise, (B // 4096, 1))
out = np.ones((B, rs.n), np.uint8)
nerr = np.ones(B, np.int32)
status = np.ones(B, np.int32)
dt = timed(lambda: lib.cc_correct_hard_batch(rs._h, P(rx), None, None, P(out), P(nerr), P(status), B))
assert (status == 0).all() and np.array_equal(out, cw)
print("pageable buffers, B=2^20, RS(255,223) BM cc_correct_hard_batch, 0..16 errors: %.2f M frames/s  (%.2f ms, %.2f GB/s of words in)" % (
    B / dt / 1e6, dt * 1e3, B * rs.n / dt / 1e9), flush=True)
