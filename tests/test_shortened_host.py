"""Shortened codes (cc_desc.n = N < 2^q - 1) on the host: descriptors, matrices and invalid lengths on CC_DEVICE_NONE
handles, the model of tests/shortened_model.py against the oracle, and the C++ facade's spelling of N."""
import os
import subprocess

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import capi
from checkers import BCH, BM, EUKLID, PGZ, RS, Oracle
import shortened_model as S

NONE = capi.DEVICE_NONE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make(family, q, t, n=None, alg=None, **kw):
    cls = cc.primitive_bch if family == BCH else cc.rs
    return cls(q, cc.errors(t), alg or cc.berlekamp_massey_tag(), device=NONE, n=n, **kw)


CASES = [(BCH, 4, 2, 12), (BCH, 6, 3, 40), (BCH, 8, 3, 200), (BCH, 8, 3, 254), (RS, 8, 8, 204), (RS, 5, 4, 9),
         (RS, 3, 1, 3)]


@pytest.mark.parametrize("family,q,t,N", CASES)
def test_descriptors(family, q, t, N):
    full = make(family, q, t)
    for same in (make(family, q, t, 0), make(family, q, t, (1 << q) - 1)):
        assert (same.n, same.k, same.l, same.dmin, same.rate, same.to_string()) == \
               (full.n, full.k, full.l, full.dmin, full.rate, full.to_string())
    s = make(family, q, t, N)
    assert (s.n, s.k, s.l, s.t, s.dmin) == (N, full.k, N - full.k, full.t, full.dmin)
    assert s.rate == (N - full.k) / N
    assert s.to_string() == "(%d, %d, %d)-BM" % (N, N - full.k, full.dmin)


@pytest.mark.parametrize("family,q,t,N", CASES)
def test_matrices_and_polynomials(family, q, t, N):
    full, s = make(family, q, t), make(family, q, t, N)
    for a, b in ((s.g, full.g), (s.h, full.h), (s.roots, full.roots)):
        assert np.array_equal(a, b)
    assert np.array_equal(s.H_alt(), full.H_alt()[:, :N])
    if family == BCH:
        assert np.array_equal(s.H(), full.H()[:, :N])
        o = Oracle(family, q, t)
        assert np.array_equal(full.H(), o.H())  # the full H is unchanged by the banded getter
        soft = cc.primitive_bch(q, cc.errors(t), cc.min_sum_tag(10), device=NONE, n=N)
        assert np.array_equal(soft.H(), full.H()[:, :N])
        assert soft.kernel_info()["kernel"].startswith("minsum_generic_kernel")


def test_full_length_H_unchanged_for_rs():
    full = make(RS, 4, 2)
    o = Oracle(RS, 4, 2)
    assert np.array_equal(full.H(), o.H())


def test_wide_descriptors():
    full = cc.primitive_bch(14, cc.errors(12), cc.berlekamp_massey_tag(), device=NONE, modular_polynomial=0x402B)
    s = cc.primitive_bch(14, cc.errors(12), cc.berlekamp_massey_tag(), device=NONE, modular_polynomial=0x402B, n=4000)
    assert (s.n, s.k, s.l, s.dmin) == (4000, full.k, 4000 - full.k, full.dmin)
    assert s.to_string() == "(4000, %d, %d)-BM" % (4000 - full.k, full.dmin)
    assert np.array_equal(s.g, full.g)


@pytest.mark.parametrize("family,q,t", [(BCH, 8, 3), (RS, 8, 8), (BCH, 4, 2)])
def test_invalid_lengths(family, q, t):
    k = make(family, q, t).k
    for N in (1, k, (1 << q), (1 << q) + 5):
        with pytest.raises(cc.CcError) as e:
            make(family, q, t, N)
        assert e.value.status == capi.ERR_INVALID_ARGUMENT
    make(family, q, t, k + 1)


def test_diag_table_refused_for_a_shortened_code():
    """BCH(31,21) shortened to 15 has (n, k) = (15, 10) of geometry g15_10: it must not match it"""
    import ctypes as C
    s = cc.primitive_bch(5, cc.errors(2), cc.min_sum_tag(10), device=NONE, n=15)
    assert (s.n, s.k) == (15, 10)
    out = np.zeros(4096, np.uint16)
    assert capi.lib().cc_diag_table(s._h, out.ctypes.data_as(C.c_void_p), out.size, None, None, None) == 0
    h = cc.primitive_bch(5, cc.errors(2), cc.berlekamp_massey_tag(), device=NONE, n=15)
    assert capi.lib().cc_diag_table(h._h, out.ctypes.data_as(C.c_void_p), out.size, None, None, None) == 0


# ---- the model on the oracle ----
@pytest.mark.parametrize("family,q,t,N", [(BCH, 8, 3, 200), (RS, 8, 8, 204), (BCH, 6, 3, 40), (RS, 4, 2, 11)])
def test_model_decodes_and_fails_virtual_frames(family, q, t, N):
    rng = np.random.default_rng(N)
    m = S.oracle(family, q, t, N)
    msg = rng.integers(0, 2 if family == BCH else 1 << q, (20, m.l)).astype(np.uint8)
    cw = m.encode(msg)
    assert cw.shape == (20, N) and np.array_equal(m.extract(cw), msg)
    rx = cw.copy()
    for f in range(20):
        for p in rng.choice(N, f % (t + 1), replace=False):
            rx[f, p] ^= 1 if family == BCH else int(rng.integers(1, 1 << q))
    for alg in (BM, EUKLID, PGZ):
        out, nerr, st = m.correct_hard(alg, rx)
        assert (st == 0).all() and np.array_equal(out, cw)
        assert np.array_equal(nerr, np.arange(20) % (t + 1))
    v = S.virtual_frame(m, (1 << q) - 2)
    full = Oracle(family, q, t)
    fo, _, fs, _ = full.correct_hard(BM, S.pad(v[None], full.n))
    assert fs[0] == 0 and fo[0, (1 << q) - 2] != 0  # the mother corrects the virtual position
    out, nerr, st = m.correct_hard(BM, v[None])
    assert st[0] == S.FRAME_LOCATOR and nerr[0] == -1 and np.array_equal(out[0], v)


def test_model_two_trials_differ_from_the_mother():
    """BCH PGZ with erasures: a trial landing in a virtual position fails, so the other trial may win"""
    m = S.oracle(BCH, 4, 2, 12)
    full = Oracle(BCH, 4, 2)
    hits = 0
    rng = np.random.default_rng(5)
    for _ in range(300):
        w = rng.integers(0, 2, 12).astype(np.uint8)
        er = sorted(rng.choice(12, int(rng.integers(1, 4)), replace=False).tolist())
        out, nerr, st = m.correct_hard(PGZ, w[None], [er])
        if st[0] == 0:
            assert not S.pad(out, 15)[0, 12:].any()
            w2 = out[0].copy()
            assert (full.syndromes(S.pad(w2[None], 15)[0]) == 0).all()
            hits += 1
    assert hits > 0


# ---- C++ facade ----
def build_facade():
    lib = os.path.join(ROOT, "channelcoding_amd")
    exe = os.path.join(ROOT, "tests", "cpp", "facade_shortened")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "facade_shortened.cpp"), "-o", exe, "-L" + lib, "-lchannelcoding_amd",
           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe


def test_facade_shortened_compiles_and_fails_loudly_without_gpu():
    exe = build_facade()
    import torch
    if not torch.cuda.is_available():
        out = subprocess.run([exe], capture_output=True, text=True)
        assert out.returncode == 1 and "no usable HIP device" in out.stderr


@pytest.mark.gpu
def test_facade_shortened_on_gpu():
    exe = build_facade()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL OK" in out.stdout and out.stdout.count("ok ") >= 8
