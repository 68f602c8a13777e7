"""Anchor decoding of product codes through the C++ facade (cyclic::product_code::correct_anchor of
include/channelcoding_amd/cyclic.hpp): tests/cpp/facade_product_anchor.cpp compiles as plain C++14 with g++ against the C
ABI, refuses to run without a GPU, and on one decodes BCH(15,11)^2 blocks, plain and extended, to the bytes of the Python
call."""
import os
import subprocess

import numpy as np
import pytest

from test_cpp_facade import ROOT, build

BIN = os.path.join(ROOT, "tests", "cpp", "facade_product_anchor")


def test_product_anchor_facade_compiles_and_fails_loudly_without_gpu():
    build("facade_product_anchor")
    import torch
    if not torch.cuda.is_available():
        out = subprocess.run([BIN], capture_output=True, text=True)
        assert out.returncode == 1 and "no usable HIP device" in out.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("extended", [False, True], ids=["plain", "ext"])
def test_product_anchor_facade_equals_the_python_call(tmp_path, extended):
    import channelcoding_amd as cc
    build("facade_product_anchor")
    if not extended:
        out = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr
    make = lambda: cc.primitive_bch(4, cc.errors(1), cc.berlekamp_massey_tag())
    pc = cc.product_code(make(), make(), extended=extended)
    rng = np.random.default_rng(15)
    B = 50
    cw = pc.encode_batch(rng.integers(0, 2, (B, pc.k2, pc.k1)).astype(np.uint8))
    z = cw ^ (rng.random(cw.shape) < 0.06).astype(np.uint8)
    z.tofile(str(tmp_path / "z.u8"))
    out = subprocess.run([BIN, str(tmp_path), "1", "6"] + (["ext"] if extended else []), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr
    want = pc.correct_anchor_batch(z, 1, 6)
    assert (want["out"] != z).any() and len(set(want["last"].tolist())) > 1 and want["nconf"].any() and want["nback"].any()
    load = lambda name, dtype: np.fromfile(str(tmp_path / name), dtype)
    assert np.array_equal(load("out.u8", np.uint8), want["out"].reshape(-1))
    for k in ("nflip", "last", "status", "nback", "nconf"):
        assert np.array_equal(load(k + ".i32", np.int32), want[k]), k
