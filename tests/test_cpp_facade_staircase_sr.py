"""The soft-aided staircase decoder through the C++ facade (cyclic::staircase_code::correct_sr of
include/channelcoding_amd/cyclic.hpp): tests/cpp/facade_staircase_sr.cpp compiles as plain C++14 with g++ against the C ABI,
refuses to run without a GPU, and on one decodes BCH(14,10) and eBCH(16,11) streams to the bytes of the Python call."""
import math
import os
import subprocess

import numpy as np
import pytest

from test_cpp_facade import ROOT, build

BIN = os.path.join(ROOT, "tests", "cpp", "facade_staircase_sr")


def test_staircase_sr_facade_compiles_and_fails_loudly_without_gpu():
    build("facade_staircase_sr")
    import torch
    if not torch.cuda.is_available():
        out = subprocess.run([BIN], capture_output=True, text=True)
        assert out.returncode == 1 and "no usable HIP device" in out.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("extended", [False, True], ids=["plain", "ext"])
def test_staircase_sr_facade_equals_the_python_call(tmp_path, extended):
    import channelcoding_amd as cc
    build("facade_staircase_sr")
    if not extended:
        out = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr
    kw = {} if extended else {"n": 14}
    sc = cc.staircase_code(cc.primitive_bch(4, cc.errors(1), cc.berlekamp_massey_tag(), **kw), 9, 4, 2, extended=extended)
    rng = np.random.default_rng(15)
    B = 50
    cw = sc.encode_batch(rng.integers(0, 2, (B, sc.blocks, sc.m, sc.k_b)).astype(np.uint8))
    y = ((1.0 - 2.0 * cw) + 0.55 * rng.standard_normal(cw.shape)).astype(np.float32)
    w = np.array([0.5, 0.9, 1.3, math.inf], np.float32)
    y.tofile(str(tmp_path / "y.f32"))
    w.tofile(str(tmp_path / "w.f32"))
    out = subprocess.run([BIN, str(tmp_path), "9", "4", "2"] + (["ext"] if extended else []), capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr
    want = sc.correct_sr_batch(y, w)
    assert want["nflip"].any() and len(set(want["status"].tolist())) == 2  # errors were corrected, not in every stream
    load = lambda name, dtype: np.fromfile(str(tmp_path / name), dtype)
    assert np.array_equal(load("out.u8", np.uint8), want["out"].reshape(-1))
    assert np.array_equal(load("nflip.i32", np.int32), want["nflip"])
    assert np.array_equal(load("status.i32", np.int32), want["status"])
