"""The C++ facade with RS roots other than alpha^1 .. alpha^2t: tests/cpp/facade_rs_roots.cpp, the DVB RS(204,188)
code as cyclic::rs<8, errors<8>, berlekamp_massey_tag, 204, division_tag, 0, 1>.  Compiles as plain C++14 anywhere, refuses
to run without a GPU, passes on one."""
import os
import subprocess

import pytest

from test_cpp_facade import ROOT, build

BIN = os.path.join(ROOT, "tests", "cpp", "facade_rs_roots")


def test_facade_rs_roots_compiles_and_fails_loudly_without_gpu():
    build("facade_rs_roots")
    import torch
    if not torch.cuda.is_available():
        out = subprocess.run([BIN], capture_output=True, text=True)
        assert out.returncode == 1 and "no usable HIP device" in out.stderr


@pytest.mark.gpu
def test_facade_rs_roots_on_gpu():
    build("facade_rs_roots")
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL OK" in out.stdout and out.stdout.count("ok ") >= 7
