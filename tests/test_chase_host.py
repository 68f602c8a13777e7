"""CPU tests of Chase-II decoding (cc_correct_chase_batch, cc_correct_chase_batch_dev, cc_mc_run_chase_dev): the model
of tests/chase_model.py against a brute force over the 128 words of BCH(15,7) in which nothing of the library takes part,
the refusals and their order on CC_DEVICE_NONE handles, and the bindings.  tests/test_gpu_chase.py holds the device
against the model."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import benchmark, capi
from channelcoding_amd.montecarlo import ChaseBackend, awgn_simulation
import chase_model as M
from checkers import BCH, Oracle, awgn_llr
from test_discrete_host import StubBackend, StubCode

NONE = dict(device=capi.DEVICE_NONE)
BM = cc.berlekamp_massey_tag
NAMES = ("cc_correct_chase_batch", "cc_correct_chase_batch_dev", "cc_mc_run_chase_dev")


# ---- the model against brute force ----
def brute_force(words, t, y, p):
    """every codeword within t of some test pattern is a candidate; smallest metric wins, equal metrics to the pattern
    with the smallest j.  Float32 sums in ascending position, written out."""
    n = y.size
    z = (y < 0).astype(np.uint8)
    keys = [int(v) & 0x7FFFFFFF for v in y.view(np.uint32)]
    order = sorted(range(n), key=lambda i: (keys[i], i))[:p]
    best = None
    ncand = 0
    for j in range(1 << p):
        pat = z.copy()
        for i in range(p):
            if (j >> i) & 1:
                pat[order[i]] ^= 1
        near = np.flatnonzero((words != pat[None, :]).sum(axis=1) <= t)
        assert near.size <= 1  # dmin = 2t + 1
        if near.size == 0:
            continue
        ncand += 1
        c = words[near[0]]
        m = np.float32(0.0)
        for i in range(n):
            if c[i] != z[i]:
                m = np.float32(m + np.float32(abs(y[i])))
        if best is None or m < best[0]:
            best = (m, j, c)
    return z, best, ncand


def brute_frames():
    orc = Oracle(BCH, 4, 2)
    assert (orc.n, orc.l, orc.t) == (15, 7, 2)
    msgs = ((np.arange(128)[:, None] >> np.arange(7)[None, :]) & 1).astype(np.uint8)
    words = orc.encode(msgs)
    assert len({w.tobytes() for w in words}) == 128
    rng = np.random.default_rng(1507)
    sent = words[rng.integers(0, 128, 400)]
    y = awgn_llr(rng, sent, orc.l / orc.n, 3.0)
    q = np.clip(np.round(y[300:] * 2) / 2, -1.5, 1.5).astype(np.float32)  # values in {+-0.5, +-1, +-1.5} and 0
    q[q == 0] = np.float32(0.5)
    q[::7, 3] = np.float32(0.0)
    q[::5, 9] = np.float32(-0.0)
    q[1::11, 0] = np.float32(-0.0)
    y[300:] = q
    return orc, words, y


def test_model_against_brute_force():
    orc, words, y = brute_frames()
    assert np.isin(np.abs(y[300:]), [0.0, 0.5, 1.0, 1.5]).all() and (y[300:] == 0).sum() > 20
    cand = M.candidates(orc, y, 4)
    ties = won_late = failures = 0
    for p in (0, 2, 4):
        got = M.pick(cand, p)
        for f in range(y.shape[0]):
            z, best, ncand = brute_force(words, orc.t, y[f], p)
            assert np.array_equal(cand["z"][f], z)
            if best is None:
                assert got["status"][f] == M.FRAME_LOCATOR and got["nerr"][f] == -1, (p, f)
                assert np.array_equal(got["out"][f], z) and got["metric"][f].view(np.uint32) == 0, (p, f)
                failures += 1
                continue
            m, j, c = best
            assert got["status"][f] == M.FRAME_OK and np.array_equal(got["out"][f], c), (p, f)
            assert got["metric"][f].view(np.uint32) == m.view(np.uint32), (p, f)
            assert got["nerr"][f] == int((c != z).sum()) and got["winner"][f] == j, (p, f)
            won_late += j > 0
            js = np.flatnonzero(cand["ok"][f, : 1 << p])
            ties += np.unique(cand["M"][f, js]).size < np.unique(cand["words"][f, js], axis=0).shape[0]
    assert won_late > 20 and failures > 0
    assert ties > 0  # two different candidates of one frame with one metric: the rule "smallest j" decided


@pytest.mark.parametrize("N", [5, 6])
def test_model_on_frames_of_at_most_six_positions(N):
    """BCH(7,4) shortened to N = 5 and 6: p runs up to N, where the selection takes every position and the 2^N test
    patterns are all words of length N"""
    dec = M.decoder(3, 1, N)
    assert (dec.n, dec.l, dec.t) == (N, N - 3, 1)
    msgs = ((np.arange(1 << dec.l)[:, None] >> np.arange(dec.l)[None, :]) & 1).astype(np.uint8)
    words = dec.encode(msgs)
    assert len({w.tobytes() for w in words}) == 1 << dec.l
    rng = np.random.default_rng(310 + N)
    y = awgn_llr(rng, words[rng.integers(0, 1 << dec.l, 200)], dec.l / dec.n, 2.0)
    y[150:] = rng.choice(np.array([-1.0, -0.5, -0.0, 0.0, 0.5, 0.5, 1.0], np.float32), (50, N))
    cand = M.candidates(dec, y)
    assert cand["L"].shape == (200, N) and cand["ok"].shape == (200, 1 << N)
    assert all(sorted(row) == list(range(N)) for row in cand["L"].tolist())  # p = n consumes every key
    if N < M.MAX_P:
        with pytest.raises(ValueError, match="test patterns"):
            M.pick(cand, N + 1)
    won_late = failures = 0
    for p in (0, 1, 3, N):
        got = M.pick(cand, p)
        whole = M.chase(dec, y, p)
        assert all(np.array_equal(got[k], whole[k]) for k in got)
        for f in range(y.shape[0]):
            z, best, ncand = brute_force(words, dec.t, y[f], p)
            if best is None:
                assert got["status"][f] == M.FRAME_LOCATOR and got["nerr"][f] == -1 and got["winner"][f] == -1, (p, f)
                assert np.array_equal(got["out"][f], z) and got["metric"][f].view(np.uint32) == 0, (p, f)
                failures += 1
                continue
            m, j, c = best
            assert got["status"][f] == M.FRAME_OK and np.array_equal(got["out"][f], c), (p, f)
            assert got["metric"][f].view(np.uint32) == m.view(np.uint32), (p, f)
            assert got["nerr"][f] == int((c != z).sum()) and got["winner"][f] == j, (p, f)
            won_late += j > 0
    assert won_late > 20 and failures > 0
    assert (M.pick(cand, N)["status"] == M.FRAME_OK).all()  # some pattern of p = n is a codeword


def test_reliability_order_ties_and_zeros():
    y = np.array([[0.5, -0.5, 0.0, 1.0, -0.0, 0.5, -1.5, 1e-40, -1e-40]], np.float32)
    assert M.least_reliable(y, 6).tolist() == [[2, 4, 7, 8, 0, 1]]
    assert M.hard(y).tolist() == [[0, 1, 0, 0, 0, 0, 1, 0, 1]]


# ---- the C interface on handles without a device ----
def _correct(code, p, llr=True, out=True, dev=False, B=4):
    n = code.n if code is not None else 15
    y = np.ones((B, n), np.float32)
    o = np.zeros((B, n), np.uint8)
    args = [code._h if code is not None else None, y.ctypes.data_as(C.c_void_p) if llr else None, p,
            o.ctypes.data_as(C.c_void_p) if out else None, None, None, None, B]
    if dev:
        return capi.lib().cc_correct_chase_batch_dev(*args, None)
    return capi.lib().cc_correct_chase_batch(*args)


def _run(code, p, counters=True):
    buf = np.zeros(capi.MC_NCOUNTERS, np.uint64)
    return capi.lib().cc_mc_run_chase_dev(code._h if code is not None else None, p, 4.0, 0, 0, 16, 1,
                                          buf.ctypes.data_as(C.c_void_p) if counters else None, None)


def calls():
    return [lambda c, p: _correct(c, p), lambda c, p: _correct(c, p, dev=True), _run]


def served():
    return [cc.primitive_bch(3, cc.errors(1), BM(), **NONE),
            cc.primitive_bch(6, cc.errors(3), cc.peterson_gorenstein_zierler_tag(), **NONE),
            cc.primitive_bch(8, cc.errors(16), cc.euklid_tag(), **NONE),
            cc.primitive_bch(8, cc.errors(3), BM(), n=200, **NONE)]


def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(os.path.dirname(capi.__file__), "..", "include", "channelcoding_amd.h")).read()
    raw = C.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capi.exported_symbols() and hasattr(capi.lib(), name) and hasattr(raw, name)
    assert re.search(r"#define CC_CHASE_MAX_P 6\b", header) and capi.CHASE_MAX_P == 6
    for name in NAMES:
        assert "pack" not in name and "interleave" not in name


def test_valid_calls_reach_the_device_check():
    for code in served():
        for p in range(capi.CHASE_MAX_P + 1):
            for call in calls():
                assert call(code, p) == capi.ERR_NO_DEVICE, (code.to_string(), p)


def test_refusals_and_their_order():
    lib = capi.lib()
    ok = served()[1]
    bch_ms = cc.primitive_bch(5, cc.errors(2), cc.min_sum_tag(10), **NONE)
    matrix = cc.min_sum_decoder(bch_ms.H(), cc.min_sum_tag(10), **NONE)
    # 1. null pointers, whatever else is wrong with the call
    for p in (0, 99):
        assert _correct(None, p) == capi.ERR_INVALID_ARGUMENT
        assert _correct(None, p, dev=True) == capi.ERR_INVALID_ARGUMENT
        assert _run(None, p) == capi.ERR_INVALID_ARGUMENT
        for code in (ok, matrix, bch_ms):
            for dev in (False, True):
                assert _correct(code, p, llr=False, dev=dev) == capi.ERR_INVALID_ARGUMENT
                assert _correct(code, p, out=False, dev=dev) == capi.ERR_INVALID_ARGUMENT
            assert _run(code, p, counters=False) == capi.ERR_INVALID_ARGUMENT
    # 2. a parity-check matrix without a code: invalid, before anything the code or p would be refused for
    for call in calls():
        for p in (0, 99):
            assert call(matrix, p) == capi.ERR_INVALID_ARGUMENT
            assert "cc_minsum_create" in lib.cc_last_error().decode()
    # 3. unsupported, with a text that names the reason
    refused = [(cc.rs(8, cc.errors(16), BM(), **NONE), 2, "Reed-Solomon"),
               (bch_ms, 2, "min-sum"),
               (cc.primitive_bch(10, cc.errors(2), BM(), modular_polynomial=0x409, **NONE), 2, "q <= 8"),
               (cc.primitive_bch(8, cc.errors(17), BM(), **NONE), 2, "2t <= 32"),
               (ok, capi.CHASE_MAX_P + 1, "CC_CHASE_MAX_P"),
               (ok, 0xFFFFFFFF, "CC_CHASE_MAX_P")]
    for code, p, text in refused:
        for call in calls():
            assert call(code, p) == capi.ERR_UNSUPPORTED, text
            assert text in lib.cc_last_error().decode(), text
    # p beyond the frame length, after CC_CHASE_MAX_P: BCH(7,4) shortened to five positions
    short = cc.primitive_bch(3, cc.errors(1), BM(), n=5, **NONE)
    for call in calls():
        assert call(short, 6) == capi.ERR_UNSUPPORTED and "frame length" in lib.cc_last_error().decode()
        assert call(short, 5) == capi.ERR_NO_DEVICE
        assert call(short, 7) == capi.ERR_UNSUPPORTED and "CC_CHASE_MAX_P" in lib.cc_last_error().decode()
    # the handle is looked at before p
    rs = refused[0][0]
    for call in calls():
        assert call(rs, 99) == capi.ERR_UNSUPPORTED and "Reed-Solomon" in lib.cc_last_error().decode()
    # and only a call that passes all of this asks for a device
    for call in calls():
        assert call(ok, 6) == capi.ERR_NO_DEVICE
    # an empty batch needs no pointers
    assert _correct(ok, 3, llr=False, out=False, B=0) == capi.ERR_NO_DEVICE


# ---- Python ----
def test_correct_batch_refuses_combinations():
    code = served()[1]
    y = np.ones((2, code.n), np.float32)
    for kw in (dict(erasures=[[1], []]), dict(want_L=True), dict(packed=True), dict(interleave=2),
               dict(out=np.zeros((2, code.n), np.uint8))):
        with pytest.raises(TypeError, match="chase="):
            code.correct_batch(y, chase=2, **kw)
    with pytest.raises(TypeError, match="chase="):
        code.decode_batch(y, chase=2, packed=True)
    with pytest.raises(TypeError, match="float32"):
        code.correct_batch(np.ones((2, code.n), np.uint8), chase=2)
    with pytest.raises(cc.CcError):
        code.correct_batch(np.ones((2, code.n + 1), np.float32), chase=2)
    with pytest.raises(cc.CcError) as e:
        code.correct_batch(y, chase=2)
    assert e.value.status == capi.ERR_NO_DEVICE
    with pytest.raises(cc.CcError) as e:
        code.correct_batch(y, chase=7)
    assert e.value.status == capi.ERR_UNSUPPORTED


def test_simulation_log_name_and_cli(tmp_path, monkeypatch):
    sim = awgn_simulation(StubCode(), backend=StubBackend(), max_samples=1000, start=4.0, stop=5.0, log_dir=str(tmp_path),
                          chase=4)
    sim()
    assert (tmp_path / "(255, 223, 33)-STUB-chase4.log").exists()
    plain = awgn_simulation(StubCode(), backend=StubBackend(), max_samples=1000, start=4.0, stop=5.0, log_dir=str(tmp_path))
    plain()
    assert (tmp_path / "(255, 223, 33)-STUB.log").exists() and plain.chase is None
    assert ChaseBackend.run is not None and "--chase" in benchmark.usage_text()
    assert benchmark.main(["--simulation", "bsc", "--chase", "2"]) == 1
    assert benchmark.main(["--chase", "7"]) == 1
    assert benchmark.main(["--chase", "2", "--algorithm", "ms"]) == 1  # no hard-tag decoder left in the selection
