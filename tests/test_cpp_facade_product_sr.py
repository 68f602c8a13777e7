"""iBDD with scaled reliability of product codes through the C++ facade (cyclic::product_code::correct_sr of
include/channelcoding_amd/cyclic.hpp): tests/cpp/facade_product_sr.cpp compiles as plain C++14 with g++ against the C
ABI, refuses to run without a GPU, and on one decodes BCH(15,11)^2 blocks, plain and extended, to the bytes of the Python
call."""
import os
import subprocess

import numpy as np
import pytest

from test_cpp_facade import ROOT, build

BIN = os.path.join(ROOT, "tests", "cpp", "facade_product_sr")


def test_product_sr_facade_compiles_and_fails_loudly_without_gpu():
    build("facade_product_sr")
    import torch
    if not torch.cuda.is_available():
        out = subprocess.run([BIN], capture_output=True, text=True)
        assert out.returncode == 1 and "no usable HIP device" in out.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("extended", [False, True], ids=["plain", "ext"])
def test_product_sr_facade_equals_the_python_call(tmp_path, extended):
    import channelcoding_amd as cc
    build("facade_product_sr")
    if not extended:
        out = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr
    make = lambda: cc.primitive_bch(4, cc.errors(1), cc.berlekamp_massey_tag())
    pc = cc.product_code(make(), make(), extended=extended)
    rng = np.random.default_rng(15)
    B = 50
    weights = (0.5, 0.8, 1.2, float("inf"), float("inf"))
    cw = pc.encode_batch(rng.integers(0, 2, (B, pc.k2, pc.k1)).astype(np.uint8))
    y = ((1.0 - 2.0 * cw) + 0.55 * rng.standard_normal(cw.shape)).astype(np.float32)
    y.tofile(str(tmp_path / "y.f32"))
    np.array(weights, np.float32).tofile(str(tmp_path / "w.f32"))
    out = subprocess.run([BIN, str(tmp_path)] + (["ext"] if extended else []), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr
    want = pc.correct_sr_batch(y, weights)
    assert want["nflip"].any() and len(set(want["last"].tolist())) > 1  # errors were corrected, not all at once
    load = lambda name, dtype: np.fromfile(str(tmp_path / name), dtype)
    assert np.array_equal(load("out.u8", np.uint8), want["out"].reshape(-1))
    for k in ("nflip", "last", "status"):
        assert np.array_equal(load(k + ".i32", np.int32), want[k]), k
