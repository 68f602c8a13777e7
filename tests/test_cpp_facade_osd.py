"""Ordered-statistics decoding through the C++ facade (primitive_bch::correct_osd / correct_osd_batch of
include/channelcoding_amd/cyclic.hpp): tests/cpp/facade_osd.cpp compiles as plain C++14 with g++ against the C ABI,
refuses to run without a GPU, and passes on one."""
import os
import subprocess

import pytest

from test_cpp_facade import ROOT, build

BIN = os.path.join(ROOT, "tests", "cpp", "facade_osd")


def test_osd_facade_compiles_and_fails_loudly_without_gpu():
    build("facade_osd")
    import torch
    if not torch.cuda.is_available():
        out = subprocess.run([BIN], capture_output=True, text=True)
        assert out.returncode == 1 and "no usable HIP device" in out.stderr


@pytest.mark.gpu
def test_osd_facade_on_gpu():
    build("facade_osd")
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL OK" in out.stdout and out.stdout.count("ok ") >= 10
