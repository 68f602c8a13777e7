"""Product codes through the C++ facade (cyclic::product_code of include/channelcoding_amd/cyclic.hpp):
tests/cpp/facade_product.cpp compiles as plain C++14 with g++ against the C ABI, refuses to run without a GPU, and on one
encodes and decodes BCH(15,11)^2 blocks, plain and extended, to the bits of the Python call."""
import os
import subprocess

import numpy as np
import pytest

from test_cpp_facade import ROOT, build

BIN = os.path.join(ROOT, "tests", "cpp", "facade_product")


def test_product_facade_compiles_and_fails_loudly_without_gpu():
    build("facade_product")
    import torch
    if not torch.cuda.is_available():
        out = subprocess.run([BIN], capture_output=True, text=True)
        assert out.returncode == 1 and "no usable HIP device" in out.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("extended", [False, True], ids=["plain", "ext"])
def test_product_facade_equals_the_python_call(tmp_path, extended):
    import channelcoding_amd as cc
    build("facade_product")
    if not extended:
        out = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr
    make = lambda: cc.primitive_bch(4, cc.errors(1), cc.berlekamp_massey_tag())
    pc = cc.product_code(make(), make(), extended=extended)
    rng = np.random.default_rng(15)
    B = 50
    msg = rng.integers(0, 2, (B, pc.k2, pc.k1)).astype(np.uint8)
    cw = pc.encode_batch(msg)
    y = ((1.0 - 2.0 * cw) + 0.75 * rng.standard_normal(cw.shape)).astype(np.float32)
    msg.tofile(str(tmp_path / "msg.u8"))
    y.tofile(str(tmp_path / "y.f32"))
    out = subprocess.run([BIN, str(tmp_path)] + (["ext"] if extended else []), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr
    alpha, beta = (0.0, 0.3, 0.5), (0.2, 0.4, 0.6)
    want = pc.correct_batch(y, 4, alpha, beta)
    assert (want["out"] != cw).any() and (want["out"] != (y < 0)).any()  # errors are left, errors were corrected
    load = lambda name, dtype: np.fromfile(str(tmp_path / name), dtype)
    assert np.array_equal(load("cw.u8", np.uint8), cw.reshape(-1))
    assert np.array_equal(load("out.u8", np.uint8), want["out"].reshape(-1))
    assert np.array_equal(load("hard.u8", np.uint8), want["out"].reshape(-1))
    assert np.array_equal(load("status.i32", np.int32), want["status"].reshape(-1))
    assert np.array_equal(load("ext.f32", np.float32).view(np.uint32), want["ext"].reshape(-1).view(np.uint32))
