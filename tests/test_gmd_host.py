"""CPU tests of GMD decoding (cc_correct_gmd_batch, cc_correct_gmd_batch_dev, cc_awgn_symbols_dev, cc_mc_run_gmd_dev):
the model of tests/gmd_model.py against a brute force over all codewords in which nothing of the library takes part,
the reliability order, the refusals and their order on CC_DEVICE_NONE handles, and the bindings.
tests/test_gpu_gmd.py holds the device against the model."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import capi
from channelcoding_amd.montecarlo import GmdBackend, awgn_simulation
import gmd_model as M
from test_discrete_host import StubBackend, StubCode

NONE = dict(device=capi.DEVICE_NONE)
BM = cc.berlekamp_massey_tag
NAMES = ("cc_correct_gmd_batch", "cc_correct_gmd_batch_dev", "cc_awgn_symbols_dev", "cc_mc_run_gmd_dev")


# ---- the model against brute force ----
def all_words(dec):
    msgs = np.array(list(itertools.product(range(1 << dec.q), repeat=dec.l)), np.uint8)
    words = dec.encode(msgs)
    assert len({w.tobytes() for w in words}) == (1 << dec.q) ** dec.l
    return words


def make_frames(dec, words, B, seed):
    """0 .. 2t + 1 symbol errors per frame; reliabilities low on the erroneous symbols in most frames, uninformative in
    others, a fifth of the frames with all reliabilities equal; ties, zeros and negative values throughout"""
    rng = np.random.default_rng(seed)
    w = words[rng.integers(0, words.shape[0], B)].copy()
    r = rng.choice(np.array([0.25, 0.5, 0.5, 1.0, 1.5, 2.0], np.float32), (B, dec.n))
    for f in range(B):
        ne = min(int(rng.integers(0, 2 * dec.t + 2)), dec.n)
        pos = rng.choice(dec.n, ne, replace=False)
        for p in pos:
            w[f, p] ^= int(rng.integers(1, 1 << dec.q))
        if f % 3:
            r[f, pos] = rng.choice(np.array([0.0, 0.125, 0.25], np.float32), ne)
        if f % 5 == 0:
            r[f] = np.float32(0.75)
    r *= rng.choice(np.array([-1.0, 1.0], np.float32), r.shape)  # the sign is ignored
    return w, r


def brute_force(words, t, w, r, m):
    """per trial the codewords within t - tau of w outside the erased set; smallest metric wins, ties to the smallest
    tau.  Float32 sums in ascending position, written out."""
    n = w.size
    keys = [int(v) & 0x7FFFFFFF for v in r.view(np.uint32)]
    order = sorted(range(n), key=lambda i: (keys[i], i))[: 2 * t]
    diff = words != w[None, :]
    best, have = None, []
    for tau in range(m):
        outside = np.ones(n, bool)
        outside[order[: 2 * tau]] = False
        near = np.flatnonzero(diff[:, outside].sum(axis=1) <= t - tau)
        assert near.size <= 1  # two would differ in <= 2t < d positions
        have.append(near.size == 1)
        if near.size == 0:
            continue
        c = words[near[0]]
        met = np.float32(0.0)
        for i in range(n):
            if c[i] != w[i]:
                met = np.float32(met + np.float32(abs(r[i])))
        if best is None or met < best[0]:
            best = (met, tau, c)
    return best, have


CASES = [(3, 2, None, 1, 300), (3, 1, None, 1, 200), (3, 2, 6, 1, 250), (3, 2, 5, 1, 250), (3, 1, 4, 1, 200),
         (4, 6, 14, 1, 200), (3, 2, None, 0, 300)]


@pytest.mark.parametrize("q,t,N,mu,B", CASES)
def test_model_against_brute_force(q, t, N, mu, B):
    dec = M.Decoder(q, t, N, mu)
    words = all_words(dec)
    w, r = make_frames(dec, words, B, 100 * q + 10 * t + (N or 0) + mu)
    cand = M.candidates(dec, w, r)
    assert cand["ok"][:, t].all()  # trial t decodes on erasures alone
    won_late = failures = 0
    for m in sorted({1, (t + 2) // 2, t + 1}):
        got = M.pick(cand, m)
        for f in range(B):
            best, have = brute_force(words, t, w[f], r[f], m)
            assert have == cand["ok"][f, :m].tolist(), (m, f)
            if best is None:
                assert got["status"][f] == M.FRAME_LOCATOR and got["nerr"][f] == -1 and got["winner"][f] == -1, (m, f)
                assert np.array_equal(got["out"][f], w[f]) and got["metric"][f].view(np.uint32) == 0, (m, f)
                failures += 1
                continue
            met, tau, c = best
            assert got["status"][f] == M.FRAME_OK and np.array_equal(got["out"][f], c), (m, f)
            assert got["metric"][f].view(np.uint32) == met.view(np.uint32), (m, f)
            assert got["nerr"][f] == int((c != w[f]).sum()) and got["winner"][f] == tau, (m, f)
            won_late += tau > 0
    assert won_late > 10 and failures > 0
    assert (M.pick(cand, t + 1)["status"] == M.FRAME_OK).all()


def test_reliability_order_ties_zeros_denormals_and_signs():
    r = np.array([[0.5, -0.5, 0.0, 1.0, -0.0, 0.5, -1.5, 1e-40, -1e-40, -0.25]], np.float32)
    assert M.least_reliable(r, 8).tolist() == [[2, 4, 7, 8, 9, 0, 1, 5]]
    assert M.metric(r, np.zeros((1, 10), np.uint8), np.array([[0, 1, 0, 0, 0, 0, 1, 0, 0, 1]], np.uint8)).tolist() == [2.25]


def test_frames_per_wave():
    assert M.frames_per_wave(32, 255, 17) == 2 and M.frames_per_wave(32, 255, 1) == 2  # LDS caps the widest code
    assert M.frames_per_wave(16, 255, 9) == 7 and M.frames_per_wave(4, 7, 3) == 21 and M.frames_per_wave(4, 7, 1) == 64


# ---- the C interface on handles without a device ----
def _correct(code, m, words=True, rel=True, out=True, dev=False, B=4):
    n = code.n if code is not None else 15
    w = np.zeros((B, n), np.uint8)
    r = np.ones((B, n), np.float32)
    o = np.zeros((B, n), np.uint8)
    args = [code._h if code is not None else None, w.ctypes.data_as(C.c_void_p) if words else None,
            r.ctypes.data_as(C.c_void_p) if rel else None, m, o.ctypes.data_as(C.c_void_p) if out else None, None, None,
            None, B]
    if dev:
        return capi.lib().cc_correct_gmd_batch_dev(*args, None)
    return capi.lib().cc_correct_gmd_batch(*args)


def _run(code, m, counters=True):
    buf = np.zeros(capi.MC_NCOUNTERS, np.uint64)
    return capi.lib().cc_mc_run_gmd_dev(code._h if code is not None else None, m, 5.0, 0, 0, 16, 1,
                                        buf.ctypes.data_as(C.c_void_p) if counters else None, None)


def _channel(code, words=True, rel=True):
    n = code.n if code is not None else 15
    w, r = np.zeros((4, n), np.uint8), np.zeros((4, n), np.float32)
    return capi.lib().cc_awgn_symbols_dev(code._h if code is not None else None, 5.0, 0, 0, 4, 1,
                                          w.ctypes.data_as(C.c_void_p) if words else None,
                                          r.ctypes.data_as(C.c_void_p) if rel else None, None, None)


def calls():
    return [lambda c, m: _correct(c, m), lambda c, m: _correct(c, m, dev=True), _run]


def served():
    return [cc.rs(3, cc.errors(2), BM(), **NONE),
            cc.rs(8, cc.errors(16), cc.peterson_gorenstein_zierler_tag(), **NONE),
            cc.rs(8, cc.errors(8), cc.euklid_tag(), mu=0, **NONE),
            cc.rs(8, cc.errors(8), BM(), mu=0, n=204, **NONE),
            cc.rs(3, cc.errors(2), BM(), n=5, **NONE)]


def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(os.path.dirname(capi.__file__), "..", "include", "channelcoding_amd.h")).read()
    raw = C.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capi.exported_symbols() and hasattr(capi.lib(), name) and hasattr(raw, name)
        assert "pack" not in name and "interleave" not in name
    assert re.search(r"#define CC_GMD_ALL 0u\b", header) and capi.GMD_ALL == 0


def test_valid_calls_reach_the_device_check():
    for code in served():
        for m in (1, code.t + 1, capi.GMD_ALL):
            for call in calls():
                assert call(code, m) == capi.ERR_NO_DEVICE, (code.to_string(), m)
        assert _channel(code) == capi.ERR_NO_DEVICE


def test_refusals_and_their_order():
    lib = capi.lib()
    ok = served()[1]
    bch = cc.primitive_bch(6, cc.errors(3), BM(), **NONE)
    bch_ms = cc.primitive_bch(5, cc.errors(2), cc.min_sum_tag(10), **NONE)
    matrix = cc.min_sum_decoder(bch_ms.H(), cc.min_sum_tag(10), **NONE)
    # 1. null pointers, whatever else is wrong with the call
    for m in (1, 99):
        assert _correct(None, m) == capi.ERR_INVALID_ARGUMENT
        assert _correct(None, m, dev=True) == capi.ERR_INVALID_ARGUMENT
        assert _run(None, m) == capi.ERR_INVALID_ARGUMENT
        for code in (ok, matrix, bch):
            for dev in (False, True):
                assert _correct(code, m, words=False, dev=dev) == capi.ERR_INVALID_ARGUMENT
                assert _correct(code, m, rel=False, dev=dev) == capi.ERR_INVALID_ARGUMENT
                assert _correct(code, m, out=False, dev=dev) == capi.ERR_INVALID_ARGUMENT
            assert _run(code, m, counters=False) == capi.ERR_INVALID_ARGUMENT
    assert _channel(None) == capi.ERR_INVALID_ARGUMENT
    assert _channel(ok, words=False) == capi.ERR_INVALID_ARGUMENT and _channel(ok, rel=False) == capi.ERR_INVALID_ARGUMENT
    # 2. a parity-check matrix without a code: invalid, before anything the code or m would be refused for
    for call in calls() + [lambda c, m: _channel(c)]:
        for m in (1, 99):
            assert call(matrix, m) == capi.ERR_INVALID_ARGUMENT
            assert "cc_minsum_create" in lib.cc_last_error().decode()
    # 3. .. 8. unsupported, with a text that names the reason
    refused = [(bch, 1, "BCH"),
               (bch_ms, 1, "BCH"),  # a BCH handle before a min-sum handle
               (cc.rs(10, cc.errors(2), BM(), modular_polynomial=0x409, **NONE), 1, "q <= 8"),
               (cc.rs(8, cc.errors(17), BM(), **NONE), 1, "2t <= 32"),
               (cc.rs(8, cc.errors(4), BM(), mu=3, step=2, **NONE), 1, "step = 1"),
               (ok, ok.t + 2, "t + 1"),
               (ok, 0xFFFFFFFF, "t + 1")]
    for code, m, text in refused:
        for call in calls():
            assert call(code, m) == capi.ERR_UNSUPPORTED, text
            assert text in lib.cc_last_error().decode(), text
    for code, m, text in refused[:5]:
        assert _channel(code) == capi.ERR_UNSUPPORTED and text in lib.cc_last_error().decode(), text
    # the handle is looked at before the trials, and the earlier reason wins
    for call in calls():
        assert call(bch, 99) == capi.ERR_UNSUPPORTED and "BCH" in lib.cc_last_error().decode()
        assert call(refused[3][0], 99) == capi.ERR_UNSUPPORTED and "2t <= 32" in lib.cc_last_error().decode()
        assert call(refused[4][0], 99) == capi.ERR_UNSUPPORTED and "step = 1" in lib.cc_last_error().decode()
    wide_long = cc.rs(10, cc.errors(17), BM(), modular_polynomial=0x409, **NONE)
    for call in calls():
        assert call(wide_long, 1) == capi.ERR_UNSUPPORTED and "q <= 8" in lib.cc_last_error().decode()
    # and only a call that passes all of this asks for a device
    for call in calls():
        assert call(ok, ok.t + 1) == capi.ERR_NO_DEVICE
    # an empty batch needs no pointers
    assert _correct(ok, 3, words=False, rel=False, out=False, B=0) == capi.ERR_NO_DEVICE
    # Chase keeps refusing RS handles with its own text
    y = np.ones((1, ok.n), np.float32)
    assert lib.cc_correct_chase_batch(ok._h, y.ctypes.data_as(C.c_void_p), 2, y.ctypes.data_as(C.c_void_p), None, None, None,
                                      1) == capi.ERR_UNSUPPORTED
    assert "Reed-Solomon" in lib.cc_last_error().decode()


# ---- Python ----
def test_correct_batch_refuses_combinations():
    code = served()[1]
    w, r = np.zeros((2, code.n), np.uint8), np.ones((2, code.n), np.float32)
    for kw in (dict(erasures=[[1], []]), dict(want_L=True), dict(packed=True), dict(interleave=2),
               dict(out=np.zeros((2, code.n), np.uint8)), dict(chase=2)):
        with pytest.raises(TypeError, match="gmd="):
            code.correct_batch(w, gmd=2, reliability=r, **kw)
    with pytest.raises(TypeError, match="gmd="):
        code.decode_batch(w, gmd=2, reliability=r, packed=True)
    with pytest.raises(TypeError, match="go together"):
        code.correct_batch(w, gmd=2)
    with pytest.raises(TypeError, match="go together"):
        code.correct_batch(w, reliability=r)
    with pytest.raises(TypeError, match="uint8"):
        code.correct_batch(w.astype(np.float32), gmd=2, reliability=r)
    with pytest.raises(ValueError, match="gmd="):
        code.correct_batch(w, gmd=0, reliability=r)
    with pytest.raises(cc.CcError):
        code.correct_batch(w, gmd=2, reliability=r[:, :-1])
    for m in (1, 2, True):
        with pytest.raises(cc.CcError) as e:
            code.correct_batch(w, gmd=m, reliability=r)
        assert e.value.status == capi.ERR_NO_DEVICE
    with pytest.raises(cc.CcError) as e:
        code.correct_batch(w, gmd=code.t + 2, reliability=r)
    assert e.value.status == capi.ERR_UNSUPPORTED


def test_symbol_reliability_against_a_loop():
    import torch
    rng = np.random.default_rng(5)
    for q in (3, 5, 8):
        y = rng.normal(0.3, 1.0, (6, 9 * q)).astype(np.float32)
        y[0, :4] = [0.0, -0.0, 1e-40, -1e-40]
        y[1, q: 2 * q] = np.float32(-0.5)
        w, rel = cc.symbol_reliability(y, q)
        assert w.dtype == np.uint8 and rel.dtype == np.float32 and w.shape == rel.shape == (6, 9)
        for f in range(6):
            for i in range(9):
                bits = y[f, i * q: (i + 1) * q]
                assert w[f, i] == sum(int(bits[b] < 0) << b for b in range(q))
                keys = [int(v) & 0x7FFFFFFF for v in bits.view(np.uint32)]
                assert rel[f, i].view(np.uint32) == min(keys)
        tw, trel = cc.symbol_reliability(torch.from_numpy(y), q)
        assert np.array_equal(tw.numpy(), w) and np.array_equal(trel.numpy().view(np.uint32), rel.view(np.uint32))
    with pytest.raises(cc.CcError):
        cc.symbol_reliability(np.zeros((2, 10), np.float32), 3)


def test_simulation_log_name(tmp_path):
    sim = awgn_simulation(StubCode(), backend=StubBackend(), max_samples=1000, start=4.0, stop=5.0, log_dir=str(tmp_path),
                          gmd=17)
    sim()
    assert (tmp_path / "(255, 223, 33)-STUB-gmd17.log").exists() and sim.gmd == 17 and sim.chase is None
    plain = awgn_simulation(StubCode(), backend=StubBackend(), max_samples=1000, start=4.0, stop=5.0, log_dir=str(tmp_path))
    plain()
    assert (tmp_path / "(255, 223, 33)-STUB.log").exists() and plain.gmd is None
    assert GmdBackend.run is not None
    with pytest.raises(TypeError, match="gmd="):
        awgn_simulation(StubCode(), backend=StubBackend(), gmd=2, chase=2)
