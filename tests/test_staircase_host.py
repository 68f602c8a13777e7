"""CPU-side checks of the staircase calls (cc_staircase) on CC_DEVICE_NONE handles: the symbols are declared,
bound and exported; every refusal in the order the header states, with its text; the model of tests/staircase_model.py --
its encoder's lines are component words, extract inverts it, it agrees with exhaustive nearest-stream search on a toy,
a decoded stream is a fixed point; staircase_code's errors; the LDS bound of the decoder's layout; and what the batches of
tests/test_gpu_staircase.py are chosen for, decoded by the model alone (CASES, SWEEP)."""
import ctypes as C
import functools
import itertools
import os
import re

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import capi
import staircase_model as SM
from shortened_model import Shortened

NONE = dict(device=capi.DEVICE_NONE)
BM = cc.berlekamp_massey_tag
NAMES = ("cc_staircase_encode_batch", "cc_staircase_encode_batch_dev", "cc_staircase_extract_batch",
         "cc_staircase_extract_batch_dev", "cc_staircase_decode", "cc_staircase_decode_dev", "cc_staircase_sigma",
         "cc_staircase_lds_bytes", "cc_awgn_staircase_dev")

# name: (q, t, N or None), extended, window, iters, blocks, BSC flip probability chosen with the model, streams, seed.
# The GPU tests decode the same batches on the device (tests/test_gpu_staircase.py says what each tile is there for).
CASES = {
    "m7": ((4, 1, 14), False, 4, 2, 12, 0.05, 64, 7),
    "m8e": ((4, 1, None), True, 4, 2, 12, 0.045, 64, 7),
    "m15": ((5, 2, 30), False, 3, 2, 7, 0.05, 24, 7),
    "m16e": ((5, 2, None), True, 4, 3, 9, 0.05, 24, 7),
    "m31": ((6, 2, 62), False, 4, 2, 9, 0.02, 12, 7),
    "m32e": ((6, 2, None), True, 3, 2, 7, 0.02, 12, 7),
    "m63": ((7, 2, 126), False, 4, 2, 9, 0.009, 8, 7),
    "m64e": ((7, 2, None), True, 2, 3, 5, 0.008, 8, 7),
    "m127": ((8, 2, 254), False, 4, 1, 9, 0.0033, 8, 7),
    "m128e": ((8, 2, None), True, 3, 2, 4, 0.003, 4, 7),
    "m128e_t15_w16": ((8, 15, None), True, 16, 1, 17, 0.04, 2, 7),
    # block sides between the chunk boundaries of a line: a 64-bit chunk holds bits of both halves, and the row half ends
    # inside a dword.  m40: chunk 0 is 40 row + 24 column bits, the second dword of a row 8 bits wide; m80: three dwords
    # per row, chunk 1 is 16 row + 48 column bits; m48e (shortened and extended, m - e = 47): the parity position n = 95
    # is bit 31 of chunk 1
    "m40": ((7, 2, 80), False, 4, 2, 9, 0.015, 8, 7),
    "m80": ((8, 2, 160), False, 4, 2, 9, 0.008, 8, 7),
    "m48e": ((7, 2, 95), True, 4, 2, 9, 0.014, 8, 11),
}
# the two smallest tiles through every window, iteration count and stream length: L < W - 1 (one position, a short
# window), L = W - 1, L = W (the first slide), L = 2W + 1 (the ring wraps twice)
SWEEP_TILES = {"m7": ((4, 1, 14), False, 0.05), "m8e": ((4, 1, None), True, 0.045)}
SWEEP_WINDOWS = (2, 3, 4, 16)
SWEEP_ITERS = (1, 2, 3)
SWEEP_STREAMS = 12


def sweep_lengths(W):
    return sorted({max(1, W - 2), W - 1, W, 2 * W + 1})


def make_batch(dec, extended, L, p, streams, seed):
    e, m, r, kb = SM.shape(dec, extended)
    rng = np.random.default_rng(seed)
    sent = SM.encode(dec, rng.integers(0, 2, (streams, L, m, kb)).astype(np.uint8), extended)
    z = sent ^ (rng.random(sent.shape) < p).astype(np.uint8)
    return sent, z


@functools.lru_cache(maxsize=None)
def case(name):
    """the model decoder, the streams sent and received, the model's outputs and its trace, made once"""
    (q, t, N), extended, W, I, L, p, streams, seed = CASES[name]
    dec = SM.decoder(q, t, N)
    sent, z = make_batch(dec, extended, L, p, streams, seed)
    trace = []
    want = SM.decode(dec, z, W, I, extended, trace)
    for a in [sent, z] + list(want.values()):
        a.setflags(write=False)
    return dec, extended, sent, z, want, trace


@functools.lru_cache(maxsize=None)
def sweep_case(tile, W, I, L):
    (q, t, N), extended, p = SWEEP_TILES[tile]
    dec = SM.decoder(q, t, N)
    sent, z = make_batch(dec, extended, L, p, SWEEP_STREAMS, 1000 * W + 10 * I + L)
    want = SM.decode(dec, z, W, I, extended)
    for a in [z] + list(want.values()):
        a.setflags(write=False)
    return z, want


def bch(q, t, **kw):
    return cc.primitive_bch(q, cc.errors(t), BM(), **dict(NONE, **kw))


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(os.path.dirname(capi.__file__), "..", "include", "channelcoding_amd.h")).read()
    raw = C.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b(int|double|size_t) %s\(" % name, header), name
        assert name in capi.exported_symbols() and hasattr(capi.lib(), name) and hasattr(raw, name)
    assert C.sizeof(capi.Staircase) == C.sizeof(C.c_void_p) + 4 + 4 + 4 + 4
    assert "#define CC_STAIRCASE_MAX_WINDOW 16" in header and capi.STAIRCASE_MAX_WINDOW == 16
    assert "staircase_code" in cc.__all__
    for name in ("encode_batch", "extract_batch", "correct_batch", "decode_batch", "channel", "sigma", "to_string"):
        assert callable(getattr(cc.staircase_code, name))


class Call:
    """one cc_staircase_decode(_dev) call on host arrays, every piece of it replaceable"""

    def __init__(self, code, extended=False, blocks=3, window=3, iters=2, B=2):
        self.code = code
        self.desc = capi.Staircase(code._h, int(bool(extended)), blocks, window, iters)
        m = (code.n + (1 if extended else 0)) // 2
        self.B, N = B, blocks * m * m
        self.inp, self.out = np.zeros(B * N + 1, np.uint8), np.zeros(B * N + 1, np.uint8)
        self.nflip, self.status = np.zeros(B, np.int32), np.zeros(B, np.int32)

    def __call__(self, dev=False, **replace):
        a = dict(desc=C.byref(self.desc), inp=vp(self.inp), out=vp(self.out), nflip=vp(self.nflip), status=vp(self.status),
                 B=self.B)
        a.update(replace)
        lib = capi.lib()
        if dev:
            return lib.cc_staircase_decode_dev(a["desc"], a["inp"], a["out"], a["nflip"], a["status"], a["B"], None)
        return lib.cc_staircase_decode(a["desc"], a["inp"], a["out"], a["nflip"], a["status"], a["B"])


def test_refusals_and_their_order():
    lib = capi.lib()
    good_code = bch(4, 1, n=14)
    rs = cc.rs(8, cc.errors(16), BM(), **NONE)
    ms = cc.primitive_bch(5, cc.errors(2), cc.min_sum_tag(10), **NONE)
    matrix = cc.min_sum_decoder(ms.H(), cc.min_sum_tag(10), **NONE)
    odd = bch(4, 1)        # n = 15, plain: n + e odd
    tight = bch(4, 3)      # BCH(15, 5) extended: m = 8, r = 11
    good = Call(good_code)
    for dev in (False, True):
        # a call with nothing wrong reaches the device check; the two per-stream outputs may be NULL, out == in is allowed
        assert good(dev) == capi.ERR_NO_DEVICE
        assert good(dev, nflip=None, status=None) == capi.ERR_NO_DEVICE
        assert good(dev, out=vp(good.inp)) == capi.ERR_NO_DEVICE
        assert Call(bch(4, 1), extended=True)(dev) == capi.ERR_NO_DEVICE
        # 1. null pointers, whatever else is wrong with the call
        for call in (good, Call(rs, blocks=0, window=1, iters=0)):
            assert call(dev, desc=None) == capi.ERR_INVALID_ARGUMENT
            for name in ("inp", "out"):
                assert call(dev, **{name: None}) == capi.ERR_INVALID_ARGUMENT, name
        c = Call(rs, blocks=0)
        c.desc.code = None
        assert c(dev) == capi.ERR_INVALID_ARGUMENT
        # 2. the numbers of the struct, before the handle is looked at
        for kw in (dict(blocks=0), dict(window=1), dict(window=17), dict(iters=0)):
            c = Call(rs, **kw)
            assert c(dev) == capi.ERR_INVALID_ARGUMENT, kw
        c = Call(rs, B=0)
        c.desc.blocks = (1 << 32) // (127 * 127) + 1  # L m m >= 2^32 at m = 127
        assert c(dev) == capi.ERR_INVALID_ARGUMENT
        # 3. what the Chase call refuses at p = 0, before the shape and the buffers are looked at
        for code, text in ((rs, "Reed-Solomon"), (ms, "min-sum"), (bch(8, 17), "2t <= 32")):
            c = Call(code)
            assert c(dev, out=vp(c.inp[1:])) == capi.ERR_UNSUPPORTED, text
            assert text in lib.cc_last_error().decode(), text
        c = Call(good_code)
        c.desc.code = matrix._h
        assert c(dev, out=vp(c.inp[1:])) == capi.ERR_INVALID_ARGUMENT and "cc_minsum_create" in lib.cc_last_error().decode()
        # 4. the shape, with a text naming which, before the buffers are looked at
        for code, extended, text in ((odd, False, "n + e is odd"), (bch(4, 1, n=14), True, "n + e is odd"),
                                     (tight, True, "r = (n - l) + e"), (bch(4, 2, n=14), False, "r = (n - l) + e")):
            c = Call(code, extended)
            assert c(dev, out=vp(c.inp[1:])) == capi.ERR_INVALID_ARGUMENT, text
            assert text in lib.cc_last_error().decode(), text
        # 5. overlap other than out == in
        assert good(dev, out=vp(good.inp[1:])) == capi.ERR_INVALID_ARGUMENT
        n_bytes = good.B * 3 * 7 * 7
        both = np.zeros(2 * n_bytes, np.uint8)
        assert good(dev, inp=vp(both), out=vp(both[n_bytes - 1:])) == capi.ERR_INVALID_ARGUMENT
        assert good(dev, inp=vp(both), out=vp(both[n_bytes:])) == capi.ERR_NO_DEVICE
        # B = 0: no buffers needed, and every check is still made (CC_OK takes a device, tests/test_gpu_staircase.py)
        assert good(dev, B=0, inp=None, out=None) == capi.ERR_NO_DEVICE
        assert Call(rs)(dev, B=0) == capi.ERR_UNSUPPORTED
    # encode, extract and the channel read code, extended and blocks alone: window = 0 and iters = 0 do not matter
    sc = capi.Staircase(good_code._h, 0, 3, 0, 0)
    msg, cw = np.zeros(2 * 3 * 7 * 3, np.uint8), np.zeros(2 * 3 * 7 * 7, np.uint8)
    assert lib.cc_staircase_encode_batch(C.byref(sc), vp(msg), vp(cw), 2) == capi.ERR_NO_DEVICE
    assert lib.cc_staircase_extract_batch(C.byref(sc), vp(cw), vp(msg), 2) == capi.ERR_NO_DEVICE
    assert lib.cc_staircase_encode_batch_dev(C.byref(sc), vp(msg), vp(cw), 2, None) == capi.ERR_NO_DEVICE
    assert lib.cc_staircase_extract_batch_dev(C.byref(sc), vp(cw), vp(msg), 2, None) == capi.ERR_NO_DEVICE
    assert lib.cc_staircase_encode_batch(C.byref(sc), None, vp(cw), 2) == capi.ERR_INVALID_ARGUMENT
    assert lib.cc_staircase_encode_batch(C.byref(sc), None, None, 0) == capi.ERR_NO_DEVICE
    assert lib.cc_awgn_staircase_dev(C.byref(sc), 3.0, 1, 0, 2, 1, vp(cw), None, None) == capi.ERR_NO_DEVICE
    assert lib.cc_awgn_staircase_dev(C.byref(sc), 3.0, 1, 0, 2, 1, None, None, None) == capi.ERR_INVALID_ARGUMENT
    sc.blocks = 0
    assert lib.cc_staircase_encode_batch(C.byref(sc), vp(msg), vp(cw), 2) == capi.ERR_INVALID_ARGUMENT


def test_sigma_and_rate():
    lib = capi.lib()
    code = bch(8, 2)
    sc = cc.staircase_code(code, 32, 8, 4, extended=True)
    assert (sc.m, sc.k_b) == (128, 111) and abs(sc.rate - (1 - 17 / 128)) < 1e-15
    assert sc.to_string() == "staircase((255, 239, 5)-BM-ext, L=32, W=8, I=4)"
    for ebno in (0.0, 4.5):
        assert abs(sc.sigma(ebno) - 1 / np.sqrt(2 * sc.rate * 10 ** (ebno / 10))) < 1e-12
    # the stream length plays no part: the zero block is not counted
    assert cc.staircase_code(code, 1, 2, 1, extended=True).sigma(3.0) == sc.sigma(3.0)
    assert lib.cc_staircase_sigma(None, 3.0) == 0.0
    assert lib.cc_staircase_sigma(C.byref(capi.Staircase(code._h, 0, 4, 2, 1)), 3.0) == 0.0  # n + e odd
    assert lib.cc_staircase_sigma(C.byref(capi.Staircase(code._h, 1, 0, 2, 1)), 3.0) == 0.0  # no block


def test_python_errors():
    code = bch(4, 1, n=14)
    with pytest.raises(TypeError):
        cc.staircase_code("code", 3, 3, 1)
    for kw in (dict(blocks=0), dict(window=1), dict(window=17), dict(iters=0)):
        with pytest.raises(ValueError):
            cc.staircase_code(code, **dict(dict(blocks=3, window=3, iters=1), **kw))
    with pytest.raises(ValueError):
        cc.staircase_code(bch(4, 1), 3, 3, 1)  # n + e odd
    with pytest.raises(ValueError):
        cc.staircase_code(bch(4, 3), 3, 3, 1, extended=True)  # r >= m
    sc = cc.staircase_code(code, 3, 3, 1)
    assert (sc.m, sc.k_b, sc.n, sc.l) == (7, 3, 3 * 49, 3 * 21)
    with pytest.raises(cc.CcError) as err:
        sc.correct_batch(np.zeros((2, 3, 7, 8), np.uint8))
    assert err.value.status == capi.ERR_LENGTH
    with pytest.raises(cc.CcError) as err:
        sc.encode_batch(np.zeros((2, 3, 7, 4), np.uint8))
    assert err.value.status == capi.ERR_LENGTH
    with pytest.raises(TypeError):
        sc.correct_batch(np.zeros((2, 3, 7, 7), np.float32))
    for call, arg in ((sc.correct_batch, np.zeros((2, 3, 7, 7), np.uint8)), (sc.encode_batch, np.zeros((2, 3, 7, 3), np.uint8)),
                      (sc.extract_batch, np.zeros((2, 3, 7, 7), np.uint8))):
        with pytest.raises(cc.CcError) as err:  # no CPU fallback
            call(arg)
        assert err.value.status == capi.ERR_NO_DEVICE


def lds_formula(m, t, W):
    P, pitch = ((m + 31) // 32) | 1, (t + 4) & ~3
    return 1536 + 4 * (2 * 2 * t * 64 + 4 * (2 * t + 1) * 64) + 4 * (4 + W * (m * P + m * pitch // 4))


def test_lds_layout_bound():
    """tables + four sets of Berlekamp-Massey columns + the ring + the line states stay under the 160 KiB of a workgroup
    for everything the interface admits: q = 8, t = 15, extended, m = 128, W = 16, and the largest 2t = 32 at m = 127"""
    limit = 160 * 1024
    seen = []
    for q, t, N, extended in ((8, 15, None, True), (8, 16, 254, False), (8, 2, None, True), (7, 5, None, True), (4, 1, 14, False)):
        for W in (2, 16):
            sc = cc.staircase_code(bch(q, t, **({} if N is None else {"n": N})), 3, W, 1, extended=extended)
            lds = sc.lds_bytes()
            assert lds == lds_formula(sc.m, t, W) and 0 < lds <= limit, (q, t, N, W, lds)
            seen.append(lds)
    assert max(seen) > 64 * 1024  # the launcher has to raise the limit of a workgroup's dynamic LDS
    assert lds_formula(128, 16, 16) <= limit  # no admitted shape exceeds this one
    assert capi.lib().cc_staircase_lds_bytes(C.byref(capi.Staircase(bch(8, 2)._h, 1, 3, 17, 1))) == 0


@pytest.mark.parametrize("q,t,N,extended", [(4, 1, 14, False), (4, 1, None, True), (5, 2, 30, False), (6, 2, None, True),
                                             (6, 3, 50, False), (8, 2, None, True)])
def test_encoder_lines_are_component_words_and_extract_inverts(q, t, N, extended):
    dec = SM.decoder(q, t, N)
    e, m, r, kb = SM.shape(dec, extended)
    rng = np.random.default_rng(3)
    msg = rng.integers(0, 2, (3, 5, m, kb)).astype(np.uint8)
    cw = SM.encode(dec, msg, extended)
    assert cw.shape == (3, 5, m, m) and cw.any()
    assert (SM.status(dec, cw, extended) == SM.FRAME_OK).all()
    assert np.array_equal(SM.extract(dec, cw, extended), msg)
    # one flipped bit breaks exactly the two lines it lies on (one where it lies in the last block)
    bad = cw.copy()
    bad[0, 1, 2, 3] ^= 1
    assert SM.status(dec, bad, extended)[0] == SM.FRAME_NOT_CONVERGED
    # a clean stream is a fixed point with nothing flipped
    res = SM.decode(dec, cw, 3, 2, extended)
    assert np.array_equal(res["out"], cw) and not res["nflip"].any() and (res["status"] == SM.FRAME_OK).all()


def toy_streams(dec, L):
    e, m, r, kb = SM.shape(dec, False)
    msgs = np.array(list(itertools.product((0, 1), repeat=L * m * kb)), np.uint8).reshape(-1, L, m, kb)
    return SM.encode(dec, msgs, False)


def test_model_against_exhaustive_search():
    """The toy: BCH(15,11) shortened to (10,6), t = 1, m = 5, k_b = 1, L = 2 -- 2^10 code streams.  (A (6,3) component
    has r = 3 = m: no message bit in a row, which the calls refuse; (10,6) is the smallest t = 1 component with one.)
    One error anywhere is within the radius of both of its lines, the unique nearest code stream is the one sent, and the
    model, with the whole stream in its window, must return it.  Under heavier noise: the model reports FRAME_OK exactly
    where its output is one of the 2^10 code streams."""
    dec = SM.decoder(4, 1, 10)
    e, m, r, kb = SM.shape(dec, False)
    assert (m, kb) == (5, 1)
    L = 2
    book = toy_streams(dec, L)
    assert book.shape[0] == 1 << (L * m * kb) and (SM.status(dec, book, False) == SM.FRAME_OK).all()
    flat = book.reshape(book.shape[0], -1)
    rng = np.random.default_rng(5)
    sent = book[rng.integers(0, book.shape[0], 50)]
    z = sent.copy().reshape(50, -1)
    z[np.arange(50), rng.integers(0, z.shape[1], 50)] ^= 1
    z = z.reshape(sent.shape)
    res = SM.decode(dec, z, 3, 2, False)
    nearest = np.array([np.flatnonzero((flat != s.reshape(-1)).sum(axis=1) == (flat != s.reshape(-1)).sum(axis=1).min())
                        for s in z], dtype=object)
    unique = np.array([len(c) == 1 for c in nearest])
    assert unique.sum() >= 40
    for b in np.flatnonzero(unique):
        assert np.array_equal(book[nearest[b][0]], sent[b])
        assert np.array_equal(res["out"][b], sent[b]) and res["status"][b] == SM.FRAME_OK and res["nflip"][b] == 1
    # heavier noise: FRAME_OK means a code stream came out, whichever
    z2 = sent ^ (rng.random(sent.shape) < 0.08).astype(np.uint8)
    res2 = SM.decode(dec, z2, 3, 3, False)
    members = np.array([(flat == o.reshape(-1)).all(axis=1).any() for o in res2["out"]])
    assert np.array_equal(members, res2["status"] == SM.FRAME_OK) and members.any() and not members.all()


def test_fixed_point():
    """what the decoder returns with FRAME_OK decodes to itself; more iterations after a position's fixed point change
    nothing (the device's early stop cannot show)"""
    dec, extended, sent, z, want, trace = case("m8e")
    ok = want["status"] == SM.FRAME_OK
    again = SM.decode(dec, want["out"][ok], 4, 2, extended)
    assert np.array_equal(again["out"], want["out"][ok]) and not again["nflip"].any()
    # per position: after two successive half-passes without a change nothing changes any more
    for rec in trace:
        if "position" in rec:
            ch = np.array(rec["changed"])  # (half-passes, streams)
            for s in range(ch.shape[1]):
                quiet = [h for h in range(1, ch.shape[0]) if not ch[h, s] and not ch[h - 1, s]]
                if quiet:
                    assert not ch[quiet[0]:, s].any()


def summary(name):
    dec, extended, sent, z, want, trace = case(name)
    W, L = CASES[name][2], CASES[name][4]
    Lc = SM.counted_blocks(L, W)
    wrong = (want["out"][:, :Lc] != sent[:, :Lc]).any(axis=(1, 2, 3))
    ok = want["status"] == SM.FRAME_OK
    steps = [r for r in trace if "step" in r]
    zero = sum(int(r["zero"].sum()) for r in steps)
    refused = sum(int((r["cand"] & ~r["take"]).sum()) for r in steps)
    stuck = sum(int((~r["cand"]).sum()) for r in steps)
    virtual = 0
    if isinstance(dec, Shortened):
        for r in steps:
            lines = r["before"].reshape(-1, r["before"].shape[-1])
            virtual += int((SM.PH.rejected_for_a_virtual_root(dec, lines) & ~r["cand"].reshape(-1)).sum())
    last = sum(int(np.array(r["changed"])[-1].sum()) for r in trace if "position" in r)
    return dict(converged=int(ok.sum()), wrong=int(wrong.sum()), undetected=int((wrong & ok).sum()), zero_rule=zero,
                refused=refused, stuck=stuck, virtual=virtual, last_half_pass=last, streams=len(ok))


def test_model_batches_are_not_degenerate():
    """what the GPU batches are chosen for, by the model alone"""
    stats = {name: summary(name) for name in CASES}
    for name, s in stats.items():
        print(name, s)
    # the first batch in numbers: its seed is this file's
    assert {k: stats["m7"][k] for k in ("converged", "wrong", "undetected")} == M7_NUMBERS, stats["m7"]
    for name, s in stats.items():
        if name != "m128e_t15_w16":
            assert 0 < s["converged"] < s["streams"], (name, s)  # both statuses in one batch
        if CASES[name][2] > 2:  # (W = 2: the last half-pass of a position is odd and has no step)
            assert s["last_half_pass"] > 0, (name, s)  # a stream that changes in the last half-pass of a position
        if CASES[name][1]:
            assert s["refused"] > 0, (name, s)  # an extended line whose candidate d <= t refuses
        else:
            assert s["refused"] == 0
            if name in ("m7", "m15", "m31"):  # plain cases shortened by one: a root at the virtual position
                assert s["virtual"] > 0, (name, s)
    assert stats["m7"]["zero_rule"] > 0 and stats["m8e"]["zero_rule"] > 0  # a line the B_0 rule keeps, plain and extended
    assert sum(s["zero_rule"] for s in stats.values()) >= 5
    for name in ("m40", "m80", "m48e"):  # and where a chunk of the line holds both halves
        assert stats[name]["zero_rule"] > 0, (name, stats[name])
    assert stats["m128e_t15_w16"]["converged"] >= 1


M7_NUMBERS = dict(converged=36, wrong=20, undetected=1)  # of 64 streams; wrong: in a block decoded with a full window


def test_sweep_batches_hold_both_statuses():
    for tile in SWEEP_TILES:
        seen = set()
        for W in SWEEP_WINDOWS:
            for I in SWEEP_ITERS:
                for L in sweep_lengths(W):
                    seen |= set(sweep_case(tile, W, I, L)[1]["status"].tolist())
        assert seen == {SM.FRAME_OK, SM.FRAME_NOT_CONVERGED}


class StubBackend:
    """counts what it is asked for: one stream error in a hundred, two wrong bits in a hundred streams"""

    def __init__(self):
        self.calls = []

    def run(self, point, seed, first, streams):
        self.calls.append((point, seed, first, streams))
        c = np.zeros(capi.MC_NCOUNTERS, np.int64)
        c[capi.MC_FRAMES], c[capi.MC_WORD_ERRORS], c[capi.MC_BIT_ERRORS] = streams, streams // 100, streams // 50
        return c


def test_simulation_log_name_ladder_and_counted_blocks(tmp_path, monkeypatch):
    from channelcoding_amd import montecarlo
    assert callable(montecarlo.StaircaseBackend) and montecarlo.StaircaseBackend.symbol == "cc_mc_run_staircase_dev"
    sc = cc.staircase_code(bch(6, 2), 12, 5, 3, extended=True)
    stub = StubBackend()
    sim = montecarlo.staircase_simulation(sc, backend=stub, max_samples=1000, log_dir=str(tmp_path))
    start, _ = montecarlo.ladder(sc.rate, 0.5)
    assert sim.start == start and sim.counted_blocks == 8
    res = sim()
    path = tmp_path / "staircase((63, 51, 5)-BM-ext, L=12, W=5, I=3).log"
    assert path.exists() and len(res) == len(sim.points()) == len(stub.calls)
    # ber over the counted blocks alone: 8 of the 12 blocks of 32 x 32
    assert res[0]["frames"] == 1000 and res[0]["wer"] == 0.01 and res[0]["ber"] == 20 / (1000 * 8 * 32 * 32)
    assert [c[2] for c in stub.calls[:3]] == [0, 1 << 40, 2 << 40] and all(c[1] == 0 for c in stub.calls)
    # a stream shorter than the window: every block counts
    assert montecarlo.staircase_simulation(cc.staircase_code(bch(6, 2), 3, 5, 1, extended=True), backend=stub).counted_blocks == 3

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
    sim2 = montecarlo.staircase_simulation(sc, backend=stub2)
    monkeypatch.setattr(sim2, "_dist", lambda: Dist())
    sim2.run_point(3.0, 1000, 2)
    lo, count = montecarlo.shard(1000, 1, 3)
    assert stub2.calls == [(3.0, 0, (2 << 40) + lo, count)]


def test_benchmark_options():
    from channelcoding_amd import benchmark
    usage = benchmark.usage_text()
    assert all(opt in usage for opt in ("--blocks", "--window", "--iters", "staircase"))
    base = ["--simulation", "staircase", "--k", "8", "--dmin", "5"]
    full = base + ["--blocks", "8", "--window", "4", "--iters", "2"]
    assert benchmark.main(base) == 1  # no default for the three
    assert benchmark.main(base + ["--blocks", "8", "--window", "4"]) == 1
    assert benchmark.main(base + ["--blocks", "0", "--window", "4", "--iters", "2"]) == 1
    assert benchmark.main(base + ["--blocks", "8", "--window", "1", "--iters", "2"]) == 1
    assert benchmark.main(base + ["--blocks", "8", "--window", "17", "--iters", "2"]) == 1
    assert benchmark.main(base + ["--blocks", "8", "--window", "4", "--iters", "0"]) == 1
    assert benchmark.main(["--simulation", "staircase", "--blocks", "8", "--window", "4", "--iters", "2"]) == 1
    assert benchmark.main(["--simulation", "staircase", "--k", "9", "--dmin", "5"] + full[6:]) == 1
    assert benchmark.main(["--simulation", "staircase", "--k", "8", "--dmin", "4"] + full[6:]) == 1
    for extra in (["--halves", "4"], ["--alpha", "0.3"], ["--beta", "0.3"], ["--cols-k", "5"], ["--chase", "2"], ["--osd", "1"]):
        assert benchmark.main(full + extra) == 1, extra
    # what is refused today stays refused
    assert benchmark.main(["--simulation", "fading"]) == 1 and benchmark.main(["--bogus"]) == 1
    assert benchmark.main(["--simulation", "product", "--k", "6", "--dmin", "7"]) == 1
    # the codes the options name: extended as it is, plain shortened by one position
    sc = benchmark.build_staircase(8, 5, 32, 8, 4, True, device=capi.DEVICE_NONE)
    assert (sc.m, sc.k_b, sc.extended) == (128, 111, True) and sc.to_string() == "staircase((255, 239, 5)-BM-ext, L=32, W=8, I=4)"
    sc = benchmark.build_staircase(8, 5, 32, 8, 4, False, device=capi.DEVICE_NONE)
    assert (sc.m, sc.k_b, sc.code.n) == (127, 111, 254)
