"""CPU-side checks of the soft-aided staircase decoder (cc_staircase_decode_sr) on CC_DEVICE_NONE handles: the
symbols are declared, bound and exported; every refusal in the order the header states, with its text; the LDS formula
of the layout; the model of tests/staircase_sr_model.py -- weights 0 return z, the toy of tests/test_staircase_host.py
against enumeration, weights all infinite against staircase_model.decode where no line fails; staircase_code's errors,
the benchmark's --weights option and staircase_sr_simulation over a stub; what the batches of
tests/test_gpu_staircase_sr.py hold, decoded by the model alone (CASES, SCHEDULES, SWEEP); and the gain over the
hard-decision window on eBCH(64,51) at 3.9 dB."""
import ctypes as C
import functools
import math
import os
import re
from statistics import NormalDist

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import benchmark, capi, montecarlo
import staircase_model as SM
import staircase_sr_model as SR
from test_staircase_host import StubBackend, toy_streams

NONE = dict(device=capi.DEVICE_NONE)
BM = cc.berlekamp_massey_tag
NAMES = ("cc_staircase_decode_sr", "cc_staircase_decode_sr_dev", "cc_staircase_sr_lds_bytes", "cc_awgn_staircase_values_dev",
         "cc_mc_run_staircase_sr_dev")
INF = math.inf

# the schedules every GPU tile runs (tests/test_gpu_staircase_sr.py); iters = len / 2
SCHEDULES = {
    "rising": (0.5, 0.9, 1.3, INF),
    "constant": (1.0,) * 4,
    "nonmonotone": (1.2, 0.4, 0.4, 1.2, INF, 0.3),                       # falling within the even and the odd half-passes
    "late": (0.0, 0.0, INF, INF),
    "single": (0.8, INF),                                                # I = 1
    "fifteen": tuple(0.25 + 0.125 * i for i in range(14)) + (INF, INF),  # 15 distinct weights at I = 8
    "pool": (0.6,) * 64 + (1.1,) * 64 + (INF, INF),                      # 130 half-passes: the levels leave the arguments
}

# name: (q, t, N or None), extended, window, blocks, streams, seed, and the probability p with which a hard decision of the
# channel is wrong at the tile's sigma (that of tests/test_staircase_host.py's tile of the same name, m64e apart).  The
# streams of a tile run from SPREAD[0] to SPREAD[1] times that sigma, and the last two carry rows that the B_0 rule holds
# (case, below): chosen with the model so that every batch holds what test_model_batches_are_not_degenerate asks of it.
# The tiles are those of tests/test_gpu_staircase.py; the last one asks for more LDS than the default limit of a workgroup.
CASES = {
    "m7": ((4, 1, 14), False, 4, 12, 64, 7, 0.05),
    "m8e": ((4, 1, None), True, 4, 12, 64, 7, 0.045),
    "m15": ((5, 2, 30), False, 3, 7, 24, 7, 0.05),
    "m16e": ((5, 2, None), True, 4, 9, 24, 7, 0.05),
    "m31": ((6, 2, 62), False, 4, 9, 12, 7, 0.02),
    "m32e": ((6, 2, None), True, 3, 7, 12, 7, 0.02),
    "m63": ((7, 2, 126), False, 4, 9, 8, 7, 0.009),
    "m64e": ((7, 2, None), True, 2, 5, 8, 7, 0.004),
    "m127": ((8, 2, 254), False, 4, 9, 8, 7, 0.0033),
    "m128e": ((8, 2, None), True, 3, 4, 4, 7, 0.003),
    "m128e_t15_w4": ((8, 15, None), True, 4, 5, 4, 7, 0.04),
    # block sides between the chunk boundaries of a line (tests/test_staircase_host.py says what each is there for)
    "m40": ((7, 2, 80), False, 4, 9, 8, 7, 0.015),
    "m80": ((8, 2, 160), False, 4, 9, 8, 7, 0.008),
    "m48e": ((7, 2, 95), True, 4, 9, 8, 11, 0.014),
}
SWEEP_TILES = {"m7": ((4, 1, 14), False, 0.05), "m8e": ((4, 1, None), True, 0.045)}
SWEEP_WINDOWS = (2, 3, 4, 16)
SWEEP_SCHEDULES = {1: (0.7, INF), 2: (0.5, 0.9, 0.3, INF), 3: (0.4, 0.4, 0.9, 0.9, INF, INF)}  # by iters
SWEEP_STREAMS = 12


def sweep_lengths(W):
    return sorted({max(1, W - 2), W - 1, W, 2 * W + 1})


def channel(dec, extended, L, p, streams, seed):
    """code streams and their channel values at the sigma whose hard decisions flip with probability p"""
    e, m, r, kb = SM.shape(dec, extended)
    rng = np.random.default_rng(seed)
    sent = SM.encode(dec, rng.integers(0, 2, (streams, L, m, kb)).astype(np.uint8), extended)
    s = -1.0 / NormalDist().inv_cdf(p)
    y = ((1.0 - 2.0 * sent) + s * rng.standard_normal(sent.shape)).astype(np.float32)
    return sent, y


SPREAD = (0.55, 1.15)  # the sigma of a tile's streams runs from the first factor to the second: quiet streams and noisy ones
PLANTED = 3           # rows of block 1 of the last two streams that the B_0 rule has to hold


def plant_zero_rule_lines(dec, extended, y, rng):
    """rows 0 .. PLANTED - 1 of block 1 of the last two streams of y get the signs of the row half of a word of the
    component code whose column half, which lies in block 0, holds one or two ones (at most t): the line is within t of
    that word, and the word differs from the line in block 0 alone.  The magnitudes stay."""
    e, m, r, kb = SM.shape(dec, extended)
    for b in (-2, -1):
        for j in range(PLANTED):
            info = np.zeros((1, dec.l), np.uint8)
            info[0, :kb] = rng.integers(0, 2, kb)
            info[0, kb + rng.choice(m, min(dec.t, 1 + j % 2), replace=False)] = 1
            word = np.asarray(dec.encode(info), np.uint8)[0]
            row = np.zeros(m, np.uint8)
            row[: m - e] = word[: m - e]
            if e:
                row[m - 1] = word.sum() & 1
            y[b, 0, j] = np.abs(y[b, 0, j]) * (1.0 - 2.0 * row)


@functools.lru_cache(maxsize=None)
def case(name):
    (q, t, N), extended, W, L, streams, seed, p = CASES[name]
    dec = SM.decoder(q, t, N)
    e, m, r, kb = SM.shape(dec, extended)
    rng = np.random.default_rng(seed)
    sent = SM.encode(dec, rng.integers(0, 2, (streams, L, m, kb)).astype(np.uint8), extended)
    s = -1.0 / NormalDist().inv_cdf(p) * np.linspace(SPREAD[0], SPREAD[1], streams)[:, None, None, None]
    y = ((1.0 - 2.0 * sent) + s * rng.standard_normal(sent.shape)).astype(np.float32)
    plant_zero_rule_lines(dec, extended, y, rng)
    sent.setflags(write=False)
    y.setflags(write=False)
    return dec, extended, sent, y


def batch(name, schedule):
    """the channel values a tile decodes under a schedule: the 130 half-passes of "pool" run on the quietest stream of the
    tile and the noisiest, which has the planted rows, cut after the first slide"""
    y = case(name)[3]
    return np.ascontiguousarray(y[[0, -1], : CASES[name][2] + 1]) if schedule == "pool" else y


@functools.lru_cache(maxsize=None)
def model(name, schedule, trace=False):
    """(the model's outputs, its trace or None) of a tile under a schedule, made once"""
    dec, extended = case(name)[:2]
    w = SCHEDULES[schedule]
    tr = [] if trace else None
    want = SR.decode(dec, batch(name, schedule), w, CASES[name][2], len(w) // 2, extended, tr)
    for a in want.values():
        a.setflags(write=False)
    return want, tr


@functools.lru_cache(maxsize=None)
def sweep_case(tile, W, I, L):
    (q, t, N), extended, p = SWEEP_TILES[tile]
    dec = SM.decoder(q, t, N)
    sent, y = channel(dec, extended, L, p, SWEEP_STREAMS, 1000 * W + 10 * I + L)
    want = SR.decode(dec, y, SWEEP_SCHEDULES[I], W, I, extended)
    for a in [y] + list(want.values()):
        a.setflags(write=False)
    return y, want


def bch(q, t, **kw):
    return cc.primitive_bch(q, cc.errors(t), BM(), **dict(NONE, **kw))


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(os.path.dirname(capi.__file__), "..", "include", "channelcoding_amd.h")).read()
    raw = C.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b(int|size_t) %s\(" % name, header), name
        assert name in capi.exported_symbols() and hasattr(capi.lib(), name) and hasattr(raw, name)
    assert "No staircase codes yet" not in header and "no soft information" not in header
    assert callable(montecarlo.StaircaseSrBackend) and callable(montecarlo.staircase_sr_simulation)
    assert montecarlo.StaircaseSrBackend.symbol == "cc_mc_run_staircase_sr_dev"
    for name in ("correct_sr_batch", "decode_sr_batch", "lds_bytes", "channel"):
        assert callable(getattr(cc.staircase_code, name))
    facade = open(os.path.join(os.path.dirname(capi.__file__), "..", "include", "channelcoding_amd", "cyclic.hpp")).read()
    assert "cc_staircase_decode_sr(" in facade


class Call:
    """one cc_staircase_decode_sr(_dev) call on host arrays, every piece of it replaceable"""

    def __init__(self, code, extended=False, blocks=3, window=3, iters=2, weights=(0.5, 1.0, INF, INF), B=2):
        self.desc = capi.Staircase(code._h, int(bool(extended)), blocks, window, iters)
        self.w = np.array(weights, np.float32)
        m = (code.n + (1 if extended else 0)) // 2
        self.B, self.N = B, blocks * m * m
        self.y, self.out = np.zeros(B * self.N, np.float32), np.zeros(B * self.N, np.uint8)
        self.nflip, self.status = np.zeros(B, np.int32), np.zeros(B, np.int32)

    def __call__(self, dev=False, **replace):
        a = dict(desc=C.byref(self.desc), w=vp(self.w), y=vp(self.y), out=vp(self.out), nflip=vp(self.nflip),
                 status=vp(self.status), B=self.B)
        a.update(replace)
        lib = capi.lib()
        if dev:
            return lib.cc_staircase_decode_sr_dev(a["desc"], a["w"], a["y"], a["out"], a["nflip"], a["status"], a["B"], None)
        return lib.cc_staircase_decode_sr(a["desc"], a["w"], a["y"], a["out"], a["nflip"], a["status"], a["B"])


FIFTEEN = tuple(0.25 * (i + 1) for i in range(14)) + (INF,)


def test_refusals_and_their_order():
    lib = capi.lib()
    text = lambda: lib.cc_last_error().decode()
    good_code = bch(4, 1, n=14)
    rs = cc.rs(8, cc.errors(16), BM(), **NONE)
    ms = cc.primitive_bch(5, cc.errors(2), cc.min_sum_tag(10), **NONE)
    matrix = cc.min_sum_decoder(ms.H(), cc.min_sum_tag(10), **NONE)
    odd, tight = bch(4, 1), bch(4, 3)  # n + e odd as a plain code; BCH(15, 5) extended: m = 8, r = 11
    big = bch(8, 2)                    # eBCH(256, 239): m = 128
    good = Call(good_code)
    nan, neg = np.array([0.5, np.nan, -1.0, 1.0], np.float32), np.array([0.5, 1.0, -1.0, np.nan], np.float32)
    for dev in (False, True):
        # a call with nothing wrong reaches the device check; the two per-stream outputs may be NULL
        assert good(dev) == capi.ERR_NO_DEVICE
        assert good(dev, nflip=None, status=None) == capi.ERR_NO_DEVICE
        assert Call(bch(4, 1), extended=True)(dev) == capi.ERR_NO_DEVICE
        # 1. null pointers, whatever else is wrong with the call
        for call in (good, Call(rs, blocks=0, window=1, iters=0)):
            assert call(dev, desc=None) == capi.ERR_INVALID_ARGUMENT
            for name in ("w", "y", "out"):
                assert call(dev, **{name: None}) == capi.ERR_INVALID_ARGUMENT, name
        c = Call(rs, blocks=0)
        c.desc.code = None
        assert c(dev) == capi.ERR_INVALID_ARGUMENT
        # 2. the numbers of the struct, before the handle and the weights are looked at
        for kw in (dict(blocks=0), dict(window=1), dict(window=17), dict(iters=0)):
            assert Call(rs, **kw)(dev, w=vp(nan)) == capi.ERR_INVALID_ARGUMENT, kw
        c = Call(rs, B=0)
        c.desc.iters = 1 << 31  # 2 * iters is no 32-bit number
        assert c(dev, w=vp(nan)) == capi.ERR_INVALID_ARGUMENT
        c = Call(rs, B=0)
        c.desc.blocks = (1 << 32) // (127 * 127) + 1  # L m m >= 2^32 at m = 127
        assert c(dev, w=vp(nan)) == capi.ERR_INVALID_ARGUMENT
        # 3. what the Chase call refuses at p = 0, before the shape, the weights and the buffers are looked at
        for code, what in ((rs, "Reed-Solomon"), (ms, "min-sum"), (bch(8, 17), "2t <= 32")):
            c = Call(code)
            assert c(dev, w=vp(nan), out=vp(c.y.view(np.uint8)[1:])) == capi.ERR_UNSUPPORTED, what
            assert what in text(), what
        c = Call(good_code)
        c.desc.code = matrix._h
        assert c(dev, w=vp(nan)) == capi.ERR_INVALID_ARGUMENT and "cc_minsum_create" in text()
        # 4. the shape, with a text naming which, before the weights are looked at
        for code, extended, what in ((odd, False, "n + e is odd"), (bch(4, 1, n=14), True, "n + e is odd"),
                                     (tight, True, "r = (n - l) + e"), (bch(4, 2, n=14), False, "r = (n - l) + e")):
            c = Call(code, extended)
            assert c(dev, w=vp(nan), out=vp(c.y.view(np.uint8)[1:])) == capi.ERR_INVALID_ARGUMENT, what
            assert what in text(), what
        # 5. the weights, before the LDS and the overlap: the first bad one is named; -0.0 is not negative; 15 distinct
        # values pass, 16 do not
        c = Call(big, True, window=16)
        over = vp(c.y.view(np.uint8)[1:])
        assert c(dev, w=vp(nan), out=over) == capi.ERR_INVALID_ARGUMENT and "weights[1] is NaN" in text()
        assert c(dev, w=vp(neg), out=over) == capi.ERR_INVALID_ARGUMENT and "weights[2] is negative" in text()
        assert good(dev, w=vp(np.array([-np.inf] * 4, np.float32))) == capi.ERR_INVALID_ARGUMENT and "weights[0] is negative" in text()
        assert good(dev, w=vp(np.array([-0.0, 0.0, INF, INF], np.float32))) == capi.ERR_NO_DEVICE
        sixteen = Call(big, True, window=16, iters=8, weights=np.arange(16))
        assert sixteen(dev) == capi.ERR_INVALID_ARGUMENT and "more than 15 distinct weights" in text()
        assert Call(good_code, iters=8, weights=FIFTEEN + (INF,))(dev) == capi.ERR_NO_DEVICE
        assert Call(good_code, iters=30, weights=FIFTEEN * 4)(dev) == capi.ERR_NO_DEVICE  # 60 half-passes, 15 values
        # 6. a window that does not fit the LDS of a workgroup: decided here, on a handle without a device, before the
        # overlap is looked at; eBCH(256,239) through W = 8 under 15 levels is admitted
        for weights in ((1.0,) * 4, (0.5, 1.0, INF, INF)):
            c = Call(big, True, window=16, weights=weights)
            assert c(dev, out=vp(c.y.view(np.uint8)[1:])) == capi.ERR_UNSUPPORTED
            asked = lib.cc_staircase_sr_lds_bytes(C.byref(c.desc), vp(c.w))
            assert asked > 160 * 1024 and str(asked) in text() and "LDS" in text()
        assert Call(big, True, window=16, B=0)(dev, y=None, out=None) == capi.ERR_UNSUPPORTED
        deployed = Call(big, True, blocks=2, window=8, iters=8, weights=FIFTEEN + (INF,), B=1)
        assert deployed(dev) == capi.ERR_NO_DEVICE
        assert lib.cc_staircase_sr_lds_bytes(C.byref(deployed.desc), vp(deployed.w)) == 160272
        # 7. out overlapping y, by any byte
        c = good
        whole = np.zeros(5 * c.B * c.N + 4, np.uint8)
        fl = lambda a: a[: 4 * c.B * c.N].view(np.float32)
        for out in (whole[1:], whole[4 * c.B * c.N - 1:]):
            assert c(dev, y=vp(fl(whole)), out=vp(out)) == capi.ERR_INVALID_ARGUMENT
        assert c(dev, y=vp(fl(whole[4:])), out=vp(whole)) == capi.ERR_INVALID_ARGUMENT
        assert c(dev, y=vp(fl(whole)), out=vp(whole[4 * c.B * c.N:])) == capi.ERR_NO_DEVICE  # adjacent is not overlapping
        # B = 0 answers after these checks: the device check is one of them
        assert good(dev, B=0, y=None, out=None) == capi.ERR_NO_DEVICE
        assert good(dev, B=0, y=None, out=None, w=vp(nan)) == capi.ERR_INVALID_ARGUMENT
        assert good(dev, B=0, y=None, out=None, w=None) == capi.ERR_INVALID_ARGUMENT
        assert Call(rs)(dev, B=0, y=None, out=None) == capi.ERR_UNSUPPORTED
    # the Monte-Carlo call: NULL sc / code / weights / counters first, then the same order
    counters = np.zeros(capi.MC_NCOUNTERS, np.uint64)
    run = lambda desc, w, c: lib.cc_mc_run_staircase_sr_dev(desc, vp(w), 3.0, 1, 0, 16, 1, vp(c), None)
    assert run(C.byref(good.desc), good.w, counters) == capi.ERR_NO_DEVICE
    worst = Call(rs, blocks=0, window=1, iters=0)
    assert run(None, good.w, counters) == capi.ERR_INVALID_ARGUMENT
    assert run(C.byref(worst.desc), None, counters) == capi.ERR_INVALID_ARGUMENT
    assert run(C.byref(worst.desc), nan, None) == capi.ERR_INVALID_ARGUMENT
    assert run(C.byref(worst.desc), nan, counters) == capi.ERR_INVALID_ARGUMENT
    assert run(C.byref(Call(rs).desc), nan, counters) == capi.ERR_UNSUPPORTED and "Reed-Solomon" in text()
    assert run(C.byref(good.desc), nan, counters) == capi.ERR_INVALID_ARGUMENT and "weights[1] is NaN" in text()
    assert run(C.byref(Call(big, True, window=16).desc), good.w, counters) == capi.ERR_UNSUPPORTED and "LDS" in text()
    assert not counters.any()
    # the channel of values reads code, extended and blocks alone
    sc = capi.Staircase(good_code._h, 0, 3, 0, 0)
    y = np.zeros(2 * 3 * 7 * 7, np.float32)
    assert lib.cc_awgn_staircase_values_dev(C.byref(sc), 3.0, 1, 0, 2, 1, vp(y), None, None) == capi.ERR_NO_DEVICE
    assert lib.cc_awgn_staircase_values_dev(C.byref(sc), 3.0, 1, 0, 2, 1, None, None, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.cc_awgn_staircase_values_dev(None, 3.0, 1, 0, 2, 1, vp(y), None, None) == capi.ERR_INVALID_ARGUMENT


def lds_formula(m, t, W, D):
    P, pitch = ((m + 31) // 32) | 1, (t + 4) & ~3
    planes = max(1, int(D).bit_length())  # the levels 0 .. D
    return (1536 + 4 * (2 * 2 * t * 64 + 4 * (2 * t + 1) * 64)
            + 4 * (4 + W * ((3 + planes) * m * P + 2 * (m * pitch // 4))))


def test_lds_bytes_equal_the_layout():
    lib = capi.lib()
    ladders = {1: (1.0,) * 4, 2: (0.5, 1.0) * 2, 3: (0.5, 1.0, INF, INF), 4: (0.25, 0.5, 1.0, INF), 15: None}
    for q, t, N, extended in ((8, 15, None, True), (8, 16, 254, False), (8, 2, None, True), (7, 5, None, True), (4, 1, 14, False)):
        for W in (2, 4, 8, 16):
            for D, weights in ladders.items():
                iters = 8 if weights is None else 2
                weights = FIFTEEN + (INF,) if weights is None else weights
                sc = cc.staircase_code(bch(q, t, **({} if N is None else {"n": N})), 3, W, iters, extended=extended)
                assert sc.lds_bytes(weights) == lds_formula(sc.m, t, W, D), (q, t, N, W, D)
                assert sc.lds_bytes(weights) > sc.lds_bytes()
    assert lds_formula(128, 2, 8, 15) == 160272 <= 160 * 1024 < lds_formula(128, 2, 16, 1)
    assert lds_formula(128, 15, 4, 15) > 64 * 1024  # the launcher has to raise the limit of a workgroup's dynamic LDS
    # 0 for what it cannot read
    sc = cc.staircase_code(bch(4, 1, n=14), 3, 3, 2)
    w = np.array([0.5, 1.0, INF, INF], np.float32)
    assert lib.cc_staircase_sr_lds_bytes(C.byref(sc._sc()), vp(w)) == lds_formula(7, 1, 3, 3)
    assert lib.cc_staircase_sr_lds_bytes(C.byref(sc._sc()), None) == 0 and lib.cc_staircase_sr_lds_bytes(None, vp(w)) == 0
    assert lib.cc_staircase_sr_lds_bytes(C.byref(sc._sc()), vp(np.array([0.5, np.nan, 1.0, 1.0], np.float32))) == 0
    for kw in (dict(window=17), dict(window=1), dict(iters=0)):
        desc = capi.Staircase(sc.code._h, 0, *(dict(dict(blocks=3, window=3, iters=2), **kw)[k] for k in ("blocks", "window", "iters")))
        assert lib.cc_staircase_sr_lds_bytes(C.byref(desc), vp(w)) == 0, kw


# ---- the model ----
def test_all_weights_zero_return_the_hard_decisions():
    for name in ("m7", "m16e"):
        dec, extended, sent, y = case(name)
        got = SR.decode(dec, y, (0.0,) * 4, CASES[name][2], 2, extended)
        z = SR.hard(y)
        assert np.array_equal(got["out"], z) and not got["nflip"].any()
        assert np.array_equal(got["status"], SM.status(dec, z, extended))


def test_model_against_exhaustive_search_on_the_toy():
    """BCH(10,6), t = 1, m = 5, k_b = 1, L = 2 (tests/test_staircase_host.py): 2^10 code streams.  One hard error of small
    magnitude: with every weight infinite, or any weight above that magnitude, the model returns the unique nearest code
    stream; with every weight below it the correction reverts and the stream stays z."""
    dec = SM.decoder(4, 1, 10)
    L = 2
    book = toy_streams(dec, L)
    flat = book.reshape(book.shape[0], -1)
    rng = np.random.default_rng(5)
    sent = book[rng.integers(0, book.shape[0], 50)]
    y = (1.0 - 2.0 * sent).astype(np.float32).reshape(50, -1)
    at = rng.integers(0, y.shape[1], 50)
    y[np.arange(50), at] *= -0.25
    y = y.reshape(sent.shape)
    z = SR.hard(y)
    assert ((z != sent).reshape(50, -1).sum(axis=1) == 1).all()
    for b in range(50):  # the nearest code stream is the one sent, and it is alone
        d = (flat != z[b].reshape(-1)).sum(axis=1)
        assert d.min() == 1 and (d == 1).sum() == 1 and np.array_equal(book[d.argmin()], sent[b])
    for weights in ((INF,) * 4, (0.3,) * 4, (0.0, 0.0, 0.3, 0.3)):
        got = SR.decode(dec, y, weights, 3, 2, False)
        assert np.array_equal(got["out"], sent) and (got["nflip"] == 1).all() and (got["status"] == SM.FRAME_OK).all()
    for weights in ((0.25,) * 4, (0.1, 0.2, 0.0, 0.25)):  # the tie |y| == w reverts
        got = SR.decode(dec, y, weights, 3, 2, False)
        assert np.array_equal(got["out"], z) and not got["nflip"].any() and (got["status"] == SM.FRAME_NOT_CONVERGED).all()


def test_infinite_weights_equal_the_hard_window_where_no_line_fails():
    """every bit weak: a taken word is taken whole, as in cc_staircase_decode; the two decoders part only at a line
    without a taken word (it returns to z here and stays there) or one the B_0 rule holds"""
    seen = 0
    for name in ("m7", "m8e", "m15", "m32e"):
        (q, t, N), extended, W, L = CASES[name][:4]
        dec = SM.decoder(q, t, N)
        sent, y = channel(dec, extended, L, CASES[name][6] / 3, 48, 21)
        trace = []
        got = SR.decode(dec, y, (INF,) * 4, W, 2, extended, trace)
        calm = sum(r["fallback"] + r["zero_rule"] for r in trace) == 0
        hard = SM.decode(dec, SR.hard(y), W, 2, extended)
        assert calm.sum() >= 8 and got["nflip"][calm].any(), (name, int(calm.sum()))
        for k in ("out", "nflip", "status"):
            assert np.array_equal(got[k][calm], hard[k][calm]), (name, k)
        assert not sum(r["reverted"] for r in trace).any()
        seen += int((~calm).sum())
    assert seen > 0


def test_special_values_follow_the_comparisons():
    """-0.0 decides as 0, a NaN decides as 0 and is never weak, +-inf is weak under no weight, |y| equal to the weight is
    strong; block 0 is never weak, so a word that would set one of its bits is no taken word"""
    dec = SM.decoder(4, 1, 14)
    y = np.ones((1, 2, 7, 7), np.float32)
    y[0, 1, 0, 3] = -1.0     # one error in row 0 of block 2 (line 0 of step 2): the candidate flips it
    y[0, 1, 1, 4] = -0.5     # the same in row 1, at exactly the weight: reverted
    y[0, 1, 2, 5] = -0.25    # weak: corrected
    y[0, 1, 3, 0], y[0, 1, 3, 1], y[0, 1, 3, 2], y[0, 1, 3, 6] = -0.0, np.nan, np.inf, -np.inf
    z = SR.hard(y)
    assert z[0, 1, 3].tolist() == [0, 0, 0, 0, 0, 0, 1]
    # W = 2: position 0 holds step 1 alone, position 1 step 2 alone, and only even half-passes have a step
    x = SR.decode(dec, y, (0.5, 0.5), 2, 1, False)["out"]
    assert x[0, 1, 0, 3] == 1 and x[0, 1, 1, 4] == 1 and x[0, 1, 2, 5] == 0 and x[0, 1, 3, 6] == 1
    x = SR.decode(dec, y, (INF, INF), 2, 1, False)["out"]
    assert x[0, 1, 0, 3] == 0 and x[0, 1, 1, 4] == 0 and x[0, 1, 3, 6] == 1  # -inf is not below inf


# ---- the Python layer ----
def test_python_errors():
    sc = cc.staircase_code(bch(4, 1, n=14), 3, 3, 2)
    y = np.zeros((2, 3, 7, 7), np.float32)
    w = (0.5, 1.0, INF, INF)
    for call in (sc.correct_sr_batch, sc.decode_sr_batch):
        with pytest.raises(cc.CcError) as e:  # no CPU fallback
            call(y, w)
        assert e.value.status == capi.ERR_NO_DEVICE
        for shape in ((2, 3, 7, 8), (3, 7, 7), (2, 4, 7, 7)):
            with pytest.raises(cc.CcError) as e:
                call(np.zeros(shape, np.float32), w)
            assert e.value.status == capi.ERR_LENGTH
        with pytest.raises(TypeError, match="float32"):
            call(np.zeros((2, 3, 7, 7), np.uint8), w)
        for bad in ((0.5,), (0.5, 1.0, INF), (0.5,) * 5):  # exactly 2 * iters
            with pytest.raises(ValueError, match="2 \\* iters = 4"):
                call(y, bad)
        with pytest.raises(ValueError):
            call(y, ())
        for weights, what in (((0.5, math.nan, 1, 1), "NaN"), ((0.5, -0.25, 1, 1), "negative")):
            with pytest.raises(cc.CcError) as e:
                call(y, weights)
            assert e.value.status == capi.ERR_INVALID_ARGUMENT and what in capi.lib().cc_last_error().decode()
    with pytest.raises(ValueError):
        sc.lds_bytes((0.5,))
    big = cc.staircase_code(bch(8, 2), 3, 16, 2, extended=True)
    with pytest.raises(cc.CcError) as e:
        big.correct_sr_batch(np.zeros((1, 3, 128, 128), np.float32), w)
    assert e.value.status == capi.ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        montecarlo.staircase_sr_simulation(sc, (0.5, 1.0), backend=object())


def test_simulation_log_name_ladder_and_sharding(tmp_path, monkeypatch):
    sc = cc.staircase_code(bch(6, 2), 12, 5, 2, extended=True)
    w = (0.5, 1.0, 1.5, INF)
    stub = StubBackend()
    sim = montecarlo.staircase_sr_simulation(sc, w, backend=stub, max_samples=1000, log_dir=str(tmp_path))
    hard = montecarlo.staircase_simulation(sc, backend=StubBackend())
    assert sim.start == hard.start and sim.points() == hard.points() and sim.counted_blocks == 8 and sim.weights == list(w)
    res = sim()
    path = tmp_path / "staircase((63, 51, 5)-BM-ext, L=12, W=5, I=2)-sr.log"
    assert path.exists() and len(res) == len(sim.points()) == len(stub.calls)
    # wer, and ber over the counted blocks alone: 8 of the 12 blocks of 32 x 32
    assert res[0]["frames"] == 1000 and res[0]["wer"] == 0.01 and res[0]["ber"] == 20 / (1000 * 8 * 32 * 32)
    assert [c[2] for c in stub.calls[:3]] == [0, 1 << 40, 2 << 40] and all(c[1] == 0 for c in stub.calls)

    class Dist:
        def get_rank(self):
            return 1

        def get_world_size(self):
            return 3

        def all_reduce(self, counters, op=None):
            pass

        class ReduceOp:
            SUM = None

    stub2 = StubBackend()
    sim2 = montecarlo.staircase_sr_simulation(sc, w, backend=stub2)
    monkeypatch.setattr(sim2, "_dist", lambda: Dist())
    sim2.run_point(3.0, 1000, 2)
    lo, count = montecarlo.shard(1000, 1, 3)
    assert stub2.calls == [(3.0, 0, (2 << 40) + lo, count)]


def test_benchmark_options():
    usage = benchmark.usage_text()
    assert "--weights" in usage and "2 * iters" in usage
    full = ["--simulation", "staircase", "--k", "8", "--dmin", "5", "--blocks", "8", "--window", "4", "--iters", "2"]
    assert benchmark.main(full + ["--weights", "0.5,x,1,1"]) == 1
    assert benchmark.main(full + ["--weights", "0.5,-1,1,1"]) == 1
    assert benchmark.main(full + ["--weights", "0.5,nan,1,1"]) == 1
    assert benchmark.main(full + ["--weights", "0.5,inf"]) == 1          # exactly 2 * iters entries
    assert benchmark.main(full + ["--weights", "0.5,1,1.5,2,inf"]) == 1
    assert benchmark.main(full[:-2] + ["--weights", "0.5,inf"]) == 1     # no --iters
    assert benchmark.main(full + ["--weights", "0.5,1,2,inf", "--halves", "4"]) == 1

    def parsed(extra):
        import argparse
        ap = argparse.ArgumentParser()
        ap.add_argument("--simulation")
        for name in ("--k", "--dmin"):
            ap.add_argument(name, action="append")
        for name in ("--cols-k", "--cols-dmin", "--chase", "--osd", "--halves", "--blocks", "--window", "--iters"):
            ap.add_argument(name, type=int, default=None)
        for name in ("--alpha", "--beta", "--weights"):
            ap.add_argument(name)
        return benchmark.staircase_sr_arguments(ap.parse_args(full + extra))

    assert parsed(["--weights", "0.6,1,2,inf"]) == (8, 5, 8, 4, 2, [0.6, 1.0, 2.0, INF])
    assert parsed(["--weights", "0,0,0,0"])[5] == [0.0] * 4
    assert isinstance(parsed(["--weights", "1,1,1"]), str) and "2 * iters = 4" in parsed(["--weights", "1,1,1"])


# ---- what the GPU batches hold ----
def test_model_batches_are_not_degenerate():
    """every batch the GPU decodes, tile by tile and schedule by schedule: both statuses, bits that a taken word leaves
    to the channel, a fallback line that changes the stream, a line the B_0 rule holds (the long schedules "fifteen" and
    "pool" add levels and half-passes only: their outputs alone are looked at)"""
    for name in sorted(CASES):
        for schedule in sorted(SCHEDULES):
            traced = schedule not in ("fifteen", "pool")
            want, trace = model(name, schedule, traced)
            ok = want["status"] == SR.FRAME_OK
            sums = {k: int(sum(r[k].sum() for r in trace or ())) for k in ("reverted", "fallback", "fallback_changed", "zero_rule", "clean_changed")}
            print(name, schedule, "streams", len(ok), "converged", int(ok.sum()), "nflip max", int(want["nflip"].max()), sums)
            assert 0 < ok.sum() < len(ok), (name, schedule)  # both statuses
            assert want["nflip"].max() > 0, (name, schedule)
            if not traced:
                continue
            assert sums["reverted"] > 0 and sums["fallback_changed"] > 0 and sums["zero_rule"] > 0, (name, schedule, sums)
            if schedule == "nonmonotone":
                assert sums["clean_changed"] > 0, name  # a word of the code that a lower weight takes apart again
            if schedule == "late":  # nothing is weak in the first two half-passes: the stream is z until half-pass 2
                early = sum(r["changed"] for r in trace if r["position"] == 0 and r["half"] < 2)
                later = sum(r["changed"] for r in trace if r["position"] == 0 and r["half"] >= 2)
                assert not early.any() and later.any(), name


def test_sweep_batches_hold_both_statuses():
    for tile in SWEEP_TILES:
        seen = set()
        for W in SWEEP_WINDOWS:
            for I in SWEEP_SCHEDULES:
                for L in sweep_lengths(W):
                    seen |= set(sweep_case(tile, W, I, L)[1]["status"].tolist())
        assert seen == {SR.FRAME_OK, SR.FRAME_NOT_CONVERGED}


def test_the_gain_over_the_hard_window():
    """eBCH(64,51), m = 32, L = 12, W = 6, I = 3 on 64 all-zero streams at 3.9 dB, wrong bits over the 7 counted blocks:
    fewer than half as many as cc_staircase_decode's model leaves (the prototype of the contract measured 665 against
    2733 on this seed)"""
    dec = SM.decoder(6, 2, None)
    e, m, r, kb = SM.shape(dec, True)
    s = 1 / np.sqrt(2 * (1 - r / m) * 10 ** (3.9 / 10))
    y = (1 + s * np.random.default_rng(1).standard_normal((64, 12, 32, 32))).astype(np.float32)
    Lc = SM.counted_blocks(12, 6)
    hard = int(SM.decode(dec, SR.hard(y), 6, 3, True)["out"][:, :Lc].sum())
    sr = int(SR.decode(dec, y, (0.6, 0.95, 1.3, 1.65, 2.0, INF), 6, 3, True)["out"][:, :Lc].sum())
    print("wrong bits over the counted blocks: iBDD-SR", sr, "hard window", hard)
    assert hard > 0 and 2 * sr < hard
