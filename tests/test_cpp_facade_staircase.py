"""Staircase codes through the C++ facade (cyclic::staircase_code of include/channelcoding_amd/cyclic.hpp):
tests/cpp/facade_staircase.cpp compiles as plain C++14 with g++ against the C ABI, refuses to run without a GPU, and on
one decodes BCH(14,10) and eBCH(16,11) streams to the bytes of the Python call."""
import os
import subprocess

import numpy as np
import pytest

from test_cpp_facade import ROOT, build

BIN = os.path.join(ROOT, "tests", "cpp", "facade_staircase")


def test_staircase_facade_compiles_and_fails_loudly_without_gpu():
    build("facade_staircase")
    import torch
    if not torch.cuda.is_available():
        out = subprocess.run([BIN], capture_output=True, text=True)
        assert out.returncode == 1 and "no usable HIP device" in out.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("extended", [False, True], ids=["plain", "ext"])
def test_staircase_facade_equals_the_python_call(tmp_path, extended):
    import channelcoding_amd as cc
    build("facade_staircase")
    if not extended:
        out = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr
    kw = {} if extended else {"n": 14}
    sc = cc.staircase_code(cc.primitive_bch(4, cc.errors(1), cc.berlekamp_massey_tag(), **kw), 9, 4, 2, extended=extended)
    rng = np.random.default_rng(15)
    B = 50
    cw = sc.encode_batch(rng.integers(0, 2, (B, sc.blocks, sc.m, sc.k_b)).astype(np.uint8))
    z = cw ^ (rng.random(cw.shape) < 0.04).astype(np.uint8)
    z.tofile(str(tmp_path / "z.u8"))
    out = subprocess.run([BIN, str(tmp_path), "9", "4", "2"] + (["ext"] if extended else []), capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr
    want_out, want_nflip, want_status = sc.correct_batch(z)
    assert (want_out != z).any() and len(set(want_status.tolist())) == 2  # errors were corrected, not in every stream
    load = lambda name, dtype: np.fromfile(str(tmp_path / name), dtype)
    assert np.array_equal(load("out.u8", np.uint8), want_out.reshape(-1))
    assert np.array_equal(load("nflip.i32", np.int32), want_nflip)
    assert np.array_equal(load("status.i32", np.int32), want_status)
