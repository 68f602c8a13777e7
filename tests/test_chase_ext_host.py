"""CPU tests of Chase decoding of extended BCH codes (cc_correct_chase_extended_batch(_dev)): the model of
tests/chase_ext_model.py against the full list of extended codewords of small codes, the parity position at work on a
frame built by hand, the refusals and their order on CC_DEVICE_NONE handles, the bindings, the keyword, cc.extend and
cc.unextend, and product decoding of an extended product code over the model.
tests/test_gpu_chase_ext.py holds the device against the model."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import capi
import chase_ext_model as E
import chase_model as M
from checkers import awgn_llr
from test_chase_soft_host import ALPHA, BETA, P, all_words, hard_rows_then_columns

NONE = dict(device=capi.DEVICE_NONE)
BM = cc.berlekamp_massey_tag
NAMES = ("cc_correct_chase_extended_batch", "cc_correct_chase_extended_batch_dev", "cc_chase_extended_frames_per_wavefront")


def full_metrics(words, y):
    """(B, words) float32 sums in ascending position over all columns of y, written out with nothing of the model"""
    z = (y < 0).astype(np.uint8)
    Mw = np.zeros((y.shape[0], words.shape[0]), np.float32)
    for i in range(y.shape[1]):
        Mw = (Mw + np.where(words[None, :, i] != z[:, None, i], np.abs(y[:, None, i]), np.float32(0))).astype(np.float32)
    return Mw


def parity_check(q, t, N=None):
    return np.asarray(cc.primitive_bch(q, cc.errors(t), BM(), **dict(NONE, **({} if N is None else {"n": N}))).H(), np.int64)


def is_extended_codeword(H, words):
    inner = words[:, :-1].astype(np.int64)
    return ~((inner @ H.T) % 2).any(axis=1) & (words.sum(axis=1) % 2 == 0)


# ---- the model against the full list ----
def test_model_on_the_extended_15_7_code_against_all_128_codewords():
    """eBCH(16,7), p = 6: the winner is an extended codeword with the metric the model states, never nearer than the
    nearest codeword, and it is the nearest one in most frames"""
    dec = M.decoder(4, 2)
    words = E.extend(all_words(dec))
    assert words.shape == (128, 16) and (words.sum(axis=1) % 2 == 0).all() and words.sum(axis=1)[1:].min() == 6  # d = 5 + 1
    rng = np.random.default_rng(1614)
    y = awgn_llr(rng, words[rng.integers(0, 128, 300)], 7 / 16, 2.0)
    full = full_metrics(words, y)
    H = parity_check(4, 2)
    for p in (0, 3, 6):
        got = E.chase(dec, y, p)
        ok = got["status"] == E.FRAME_OK
        assert ok.sum() > 200 and is_extended_codeword(H, got["out"][ok]).all()
        idx = np.array([np.flatnonzero((words == w[None, :]).all(axis=1))[0] for w in got["out"][ok]])
        mine = full[np.flatnonzero(ok), idx]
        assert np.array_equal(mine.view(np.uint32), got["metric"][ok].view(np.uint32)), p
        assert (got["nerr"][ok] == (got["out"][ok] != (y[ok] < 0)).sum(axis=1)).all()
        assert (full.min(axis=1)[ok] <= mine).all()
        assert (full.min(axis=1)[ok] == mine).mean() > (0.9 if p == 6 else 0.5), p
        lost = ~ok
        assert np.array_equal(got["out"][lost], (y[lost] < 0).astype(np.uint8)) and (got["nerr"][lost] == -1).all()
        assert (got["metric"][lost].view(np.uint32) == 0).all()


@pytest.mark.parametrize("N", [5, 6])
def test_every_inner_word_a_test_pattern_gives_maximum_likelihood(N):
    """BCH(15,11) shortened to N = 5 and 6 with p = N: every codeword is the candidate of some pattern, so out is the
    maximum-likelihood word of the extended code in the extended metric: the metric to the bit, the word wherever the
    minimum is unique"""
    dec = M.decoder(4, 1, N)
    words = E.extend(all_words(dec))
    rng = np.random.default_rng(510 + N)
    y = awgn_llr(rng, words[rng.integers(0, words.shape[0], 200)], dec.l / (N + 1), 1.0)
    y[150:] = rng.choice(np.array([-1.0, -0.5, -0.0, 0.0, 0.5, 0.5, 1.0], np.float32), (50, N + 1))
    got = E.chase(dec, y, N)
    full = full_metrics(words, y)
    best = full.min(axis=1)
    assert (got["status"] == E.FRAME_OK).all()
    assert np.array_equal(got["metric"].view(np.uint32), best.view(np.uint32))
    unique = (full == best[:, None]).sum(axis=1) == 1
    assert unique.sum() > 150 and not unique.all()
    assert np.array_equal(got["out"][unique], words[full.argmin(axis=1)][unique])
    assert is_extended_codeword(parity_check(4, 1, N), got["out"]).all()
    soft = E.chase_soft(dec, y, N, 0.25)
    # the parity position has a competitor in every frame: the code holds words of odd weight, all of them candidates
    assert words[:, N].any() and soft["has"][:, N].all()


@pytest.mark.parametrize("q,t,N,ebno", [(3, 1, None, 2.0), (5, 2, None, 3.0), (6, 3, 50, 3.0)])
def test_every_ok_word_has_even_weight_and_a_codeword_inside(q, t, N, ebno):
    dec = M.decoder(q, t, N)
    rng = np.random.default_rng(77 + q)
    sent = E.extend(dec.encode(rng.integers(0, 2, (120, dec.l)).astype(np.uint8)))
    y = awgn_llr(rng, sent, dec.l / (dec.n + 1), ebno)
    H = parity_check(q, t, N)
    cand = E.candidates(dec, y)
    assert (cand["L"] < dec.n).all()  # the parity position is never a test position
    for p in (0, 2, 6):
        got = M.pick(cand, p)
        ok = got["status"] == E.FRAME_OK
        assert ok.sum() > 60 and is_extended_codeword(H, got["out"][ok]).all()
        assert np.array_equal(got["out"][~ok], cand["z"][~ok])


def test_the_parity_value_decides_between_two_inner_words():
    """BCH(7,4), p = 2.  z = e_0 with |y_0| = 0.5, positions 1 and 3 at +0.3, the rest at +2: pattern 0 decodes to the
    zero word (inner metric 0.5), pattern 1 flips position 1 and decodes to 1 + x + x^3 (inner metric 0.3 + 0.3).  The
    plain call picks the zero word.  With y_7 = -0.4 the zero word pays for the parity position (0.5 + 0.4) and the
    weight-3 word, whose parity bit is 1, does not: 0.1 between the inner metrics, 0.4 at stake."""
    dec = M.decoder(3, 1)
    inner = np.array([[-0.5, 0.3, 2.0, 0.3, 2.0, 2.0, 2.0]], np.float32)
    w3 = np.array([1, 1, 0, 1, 0, 0, 0], np.uint8)
    assert np.array_equal(dec.correct_hard(M.BM, w3[None, :])[0][0], w3)  # a codeword
    plain = M.chase(dec, inner, 2)
    assert not plain["out"].any() and plain["metric"][0] == np.float32(0.5)
    y = np.concatenate([inner, np.array([[-0.4]], np.float32)], axis=1)
    cand = E.candidates(dec, y, 2)
    assert cand["L"][0].tolist() == [1, 3]
    assert cand["M"][0, 0] == np.float32(np.float32(0.5) + np.float32(0.4)) and cand["M"][0, 1] == np.float32(0.6)
    got = E.chase(dec, y, 2)
    assert got["out"][0].tolist() == [1, 1, 0, 1, 0, 0, 0, 1] and got["winner"][0] == 1 and got["nerr"][0] == 2
    assert got["metric"][0] == np.float32(np.float32(0.3) + np.float32(0.3))
    soft = E.chase_soft(dec, y, 2, 0.5)
    assert soft["has"][0].tolist() == [True, True, False, True, False, False, False, True]
    gap = np.float32(np.float32(0.9) - np.float32(0.6))
    assert soft["ext"][0, 7] == np.float32(-gap - np.float32(-0.4))  # s = -1 at the parity position
    # the other sign of the same magnitude: both words keep their order, the zero word wins with nothing added
    y[0, 7] = np.float32(0.4)
    got = E.chase(dec, y, 2)
    assert not got["out"].any() and got["metric"][0] == np.float32(0.5) and got["nerr"][0] == 1
    # and with +0.0 at the parity position the inner words and metrics are the plain call's
    y[0, 7] = np.float32(0.0)
    got = E.chase(dec, y, 2)
    assert np.array_equal(got["out"][:, :7], plain["out"]) and got["metric"][0] == plain["metric"][0]


# ---- the C interface on handles without a device ----
def _call(code, p, beta=0.5, llr=True, out=True, ext=True, dev=False, B=4, overlap=None):
    w = code.n + 1 if code is not None else 16
    buf = np.ones(2 * B * w + 8, np.float32)
    y, e = buf[: B * w], buf[B * w + 4: 2 * B * w + 4]
    if overlap is not None:
        e = buf[overlap: overlap + B * w]
    o = np.zeros((B, w), np.uint8)
    ptr = lambda a, on: a.ctypes.data_as(C.c_void_p) if on else None
    args = [code._h if code is not None else None, ptr(y, llr), p, C.c_float(beta), ptr(o, out), ptr(e, ext), None, None,
            None, B]
    if dev:
        return capi.lib().cc_correct_chase_extended_batch_dev(*args, None)
    return capi.lib().cc_correct_chase_extended_batch(*args)


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
    for name in ("extend", "unextend", "product_decode"):
        assert callable(getattr(cc, name)) and name in cc.__all__


def test_frames_per_wavefront():
    """rows of n + 1 values under the same 16 000 bytes per wavefront: F of the plain calls wherever 64 >> p or the
    per-frame share leaves room for one more value per row, fewer where it does not"""
    F, plain = capi.lib().cc_chase_extended_frames_per_wavefront, capi.lib().cc_chase_frames_per_wavefront
    want = {(8, 3): ([12, 12, 12, 8, 4, 2, 1], [6, 6, 6, 6, 4, 2, 1]), (7, 3): ([24, 24, 16, 8, 4, 2, 1], [12, 12, 12, 8, 4, 2, 1]),
            (4, 2): ([64, 32, 16, 8, 4, 2, 1],) * 2, (8, 16): ([3, 3, 3, 3, 3, 2, 1], [1, 1, 1, 1, 1, 1, 1])}
    for (q, t), (hard, soft) in want.items():
        code = cc.primitive_bch(q, cc.errors(t), BM(), **NONE)
        assert [F(code._h, p, 0) for p in range(7)] == hard, (q, t)
        assert [F(code._h, p, 1) for p in range(7)] == soft, (q, t)
    for q, t in ((6, 3), (5, 2), (8, 8)):
        code = cc.primitive_bch(q, cc.errors(t), BM(), **NONE)
        for soft in (0, 1):
            for p in range(7):
                assert 1 <= F(code._h, p, soft) <= plain(code._h, p, soft)
    ok = served()[1]
    assert F(None, 2, 1) == 0 and F(ok._h, 7, 1) == 0 and F(cc.rs(8, cc.errors(16), BM(), **NONE)._h, 2, 0) == 0
    assert F(cc.primitive_bch(3, cc.errors(1), BM(), n=5, **NONE)._h, 6, 1) == 0


def test_valid_calls_reach_the_device_check():
    for code in served():
        for p in range(capi.CHASE_MAX_P + 1):
            for dev in (False, True):
                for beta in (0.0, 0.5, 3e38):
                    assert _call(code, p, beta, dev=dev) == capi.ERR_NO_DEVICE, (code.to_string(), p, beta)
                # ext == NULL: the hard output, beta is not examined
                for beta in (0.5, -1.0, float("nan"), float("inf")):
                    assert _call(code, p, beta, ext=False, dev=dev) == capi.ERR_NO_DEVICE, (code.to_string(), p, beta)


def test_refusals_and_their_order():
    lib = capi.lib()
    ok = served()[1]
    w = ok.n + 1
    bch_ms = cc.primitive_bch(5, cc.errors(2), cc.min_sum_tag(10), **NONE)
    matrix = cc.min_sum_decoder(bch_ms.H(), cc.min_sum_tag(10), **NONE)
    rs = cc.rs(8, cc.errors(16), BM(), **NONE)
    bad_betas = (-1.0, -1e-45, float("inf"), float("-inf"), float("nan"))
    for dev in (False, True):
        # 1. null pointers (ext is optional), whatever else is wrong with the call
        for p, beta in ((0, 0.5), (99, -1.0)):
            assert _call(None, p, beta, dev=dev) == capi.ERR_INVALID_ARGUMENT
            for code in (ok, matrix, bch_ms, rs):
                for missing in ("llr", "out"):
                    assert _call(code, p, beta, dev=dev, **{missing: False}) == capi.ERR_INVALID_ARGUMENT, missing
        # 2. what cc_correct_chase_batch refuses, in its order, before beta and the overlap are looked at
        for beta, overlap in ((0.5, None), (-1.0, None), (float("nan"), 0)):
            assert _call(matrix, 2, beta, dev=dev, overlap=overlap) == capi.ERR_INVALID_ARGUMENT
            assert "cc_minsum_create" in lib.cc_last_error().decode()
            refused = [(rs, 2, "Reed-Solomon"), (bch_ms, 2, "min-sum"),
                       (cc.primitive_bch(10, cc.errors(2), BM(), modular_polynomial=0x409, **NONE), 2, "q <= 8"),
                       (cc.primitive_bch(8, cc.errors(17), BM(), **NONE), 2, "2t <= 32"),
                       (ok, capi.CHASE_MAX_P + 1, "CC_CHASE_MAX_P"), (rs, 99, "Reed-Solomon"),
                       (cc.primitive_bch(3, cc.errors(1), BM(), n=5, **NONE), 6, "frame length")]
            for code, p, text in refused:
                for ext in (True, False):
                    assert _call(code, p, beta, ext=ext, dev=dev, overlap=overlap) == capi.ERR_UNSUPPORTED, text
                    assert text in lib.cc_last_error().decode(), text
        # 3. with ext, beta negative, infinite or NaN: invalid, before the device is asked for
        for beta in bad_betas:
            assert _call(ok, 3, beta, dev=dev) == capi.ERR_INVALID_ARGUMENT, beta
        for beta in (0.0, -0.0, 1e-45, 3.4e38):
            assert _call(ok, 3, beta, dev=dev) == capi.ERR_NO_DEVICE, beta
        # 4. ext overlapping llr by any byte of the B (n + 1) floats: invalid; next to it: served
        B = 4
        for off in (0, 1, B * w - 1):
            assert _call(ok, 3, dev=dev, B=B, overlap=off) == capi.ERR_INVALID_ARGUMENT, off
        assert _call(ok, 3, dev=dev, B=B, overlap=B * w) == capi.ERR_NO_DEVICE
        # 5. and only a call that passes all of this asks for a device; an empty batch needs no pointers
        assert _call(ok, 6, dev=dev) == capi.ERR_NO_DEVICE
        assert _call(ok, 3, llr=False, out=False, ext=False, dev=dev, B=0) == capi.ERR_NO_DEVICE
        assert _call(ok, 99, llr=False, out=False, ext=False, dev=dev, B=0) == capi.ERR_UNSUPPORTED


# ---- Python ----
def test_the_keyword_and_what_it_refuses():
    code = served()[1]
    w = code.n + 1
    y = np.ones((2, w), np.float32)
    for call in (code.correct_batch, code.decode_batch):
        with pytest.raises(TypeError, match="extended="):
            call(y, extended=True)
        with pytest.raises(TypeError, match="extended="):
            call(np.ones((2, code.n), np.uint8), extended=True)
    rs = cc.rs(8, cc.errors(16), BM(), **NONE)
    with pytest.raises(TypeError, match="extended="):
        rs.correct_batch(np.ones((2, rs.n), np.uint8), gmd=2, reliability=np.ones((2, rs.n), np.float32), extended=True)
    for kw in (dict(erasures=[[1], []]), dict(want_L=True), dict(packed=True), dict(interleave=2),
               dict(out=np.zeros((2, w), np.uint8))):
        with pytest.raises(TypeError, match="chase="):
            code.correct_batch(y, chase=2, extended=True, **kw)
    with pytest.raises(TypeError, match="float32"):
        code.correct_batch(np.ones((2, w), np.uint8), chase=2, extended=True)
    with pytest.raises(TypeError, match="soft="):
        code.correct_batch(y, chase=2, extended=True, soft="0.5")
    for width in (code.n, code.n + 2):  # rows of n + 1 and nothing else
        with pytest.raises(cc.CcError) as e:
            code.correct_batch(np.ones((2, width), np.float32), chase=2, extended=True)
        assert e.value.status == capi.ERR_LENGTH
    for kw, status in ((dict(chase=2), capi.ERR_NO_DEVICE), (dict(chase=0), capi.ERR_NO_DEVICE),
                       (dict(chase=2, soft=0.5), capi.ERR_NO_DEVICE), (dict(chase=7), capi.ERR_UNSUPPORTED),
                       (dict(chase=7, soft=0.5), capi.ERR_UNSUPPORTED), (dict(chase=2, soft=-0.5), capi.ERR_INVALID_ARGUMENT),
                       (dict(chase=2, soft=float("nan")), capi.ERR_INVALID_ARGUMENT)):
        for call in (code.correct_batch, code.decode_batch):
            with pytest.raises(cc.CcError) as e:
                call(y, extended=True, **kw)
            assert e.value.status == status, kw
    # without the keyword nothing has changed: rows of n + 1 are a wrong length
    with pytest.raises(cc.CcError) as e:
        code.correct_batch(y, chase=2)
    assert e.value.status == capi.ERR_LENGTH


def test_extend_and_unextend_round_trip():
    import torch
    rng = np.random.default_rng(5)
    words = rng.integers(0, 2, (3, 7, 15)).astype(np.uint8)
    ext = cc.extend(words)
    assert ext.shape == (3, 7, 16) and ext.dtype == np.uint8 and ext.flags.c_contiguous
    assert np.array_equal(ext, E.extend(words)) and (ext.sum(axis=-1) % 2 == 0).all()
    back = cc.unextend(ext)
    assert np.array_equal(back, words) and back.flags.c_contiguous
    t = torch.from_numpy(words)
    te = cc.extend(t)
    assert te.dtype == torch.uint8 and np.array_equal(te.numpy(), ext)
    tb = cc.unextend(te)
    assert tb.is_contiguous() and torch.equal(tb, t)
    one = cc.extend(np.array([1, 1, 1], np.uint8))
    assert one.tolist() == [1, 1, 1, 1] and cc.unextend(one).tolist() == [1, 1, 1]
    # a codeword of BCH(15,11) extended is a word of eBCH(16,11): every nonzero weight is even and at least 4
    dec = M.decoder(4, 1)
    w = cc.extend(all_words(dec)).sum(axis=1)
    assert (w % 2 == 0).all() and w[w > 0].min() == 4


# ---- product decoding over the model ----
class ModelCode:
    """what product_decode(extended=True) needs of a code, answered by the model"""

    def __init__(self, dec):
        self.dec, self.n, self.calls = dec, dec.n, []

    def correct_batch(self, X, chase=None, soft=None, extended=False):
        assert extended is True
        assert isinstance(X, np.ndarray) and X.dtype == np.float32 and X.flags.c_contiguous and X.shape[1] == self.n + 1
        self.calls.append((chase, soft))
        r = E.chase_soft(self.dec, X, chase, soft)
        return dict(out=r["out"], ext=r["ext"], status=r["status"], nerr=r["nerr"], metric=r["metric"])


PRODUCT_EBNO, PRODUCT_BLOCKS = 3.0, 300


@functools.lru_cache(maxsize=None)
def extended_product_batch(rq=4, rt=1, cq=4, ct=1, ebno=PRODUCT_EBNO, blocks=PRODUCT_BLOCKS, seed=2016):
    """random words of eBCH x eBCH (rows encoded and extended, then the columns of that), BPSK plus Gaussian noise"""
    rows, cols = M.decoder(rq, rt), M.decoder(cq, ct)
    rng = np.random.default_rng(seed)
    info = rng.integers(0, 2, (blocks, cols.l, rows.l)).astype(np.uint8)
    wide = E.extend(rows.encode(info.reshape(-1, rows.l))).reshape(blocks, cols.l, rows.n + 1)
    tall = E.extend(cols.encode(np.ascontiguousarray(wide.transpose(0, 2, 1)).reshape(-1, cols.l)))
    sent = np.ascontiguousarray(tall.reshape(blocks, rows.n + 1, cols.n + 1).transpose(0, 2, 1))  # (blocks, n2 + 1, n1 + 1)
    rate = rows.l * cols.l / ((rows.n + 1) * (cols.n + 1))
    y = awgn_llr(rng, sent, rate, ebno)
    y.setflags(write=False)
    return rows, cols, sent, y


def test_product_decode_of_an_extended_product_code_over_the_model():
    """eBCH(16,11) x eBCH(16,11), 300 blocks at Eb/N0 = 3.0 dB, seed 2016, p = 4, alpha = 0, 0.3, 0.5, 0.7, beta = 0.2,
    0.4, 0.6, 0.8.  Blocks in error over the 16 x 16 positions: hard decoding (inner rows, then inner columns, each word's
    parity bit recomputed) 289; after the four half-iterations 285, 142, 28, 5.  The assertion is the direction only."""
    rows, cols, sent, y = extended_product_batch()
    H = parity_check(4, 1)
    for words in (sent.reshape(-1, 16), sent.transpose(0, 2, 1).reshape(-1, 16)):
        assert is_extended_codeword(H, words).all()  # rows and columns, the parity row and column among them
    inner = hard_rows_then_columns(rows, cols, np.ascontiguousarray(y[:, :15, :15]))
    hard = E.extend(np.ascontiguousarray(E.extend(inner).transpose(0, 2, 1))).transpose(0, 2, 1)
    hard_errors = int((hard != sent).any(axis=(1, 2)).sum())
    steps = E.product_decode(rows, cols, y, P, ALPHA, BETA)
    soft_errors = [int((s["out"] != sent).any(axis=(1, 2)).sum()) for s in steps]
    print("eBCH(16,11)^2 hard", hard_errors, "after each half-iteration", soft_errors)
    assert soft_errors[-1] < hard_errors, (hard_errors, soft_errors)
    # cc.product_decode(extended=True) is the same loop: with the model as its component decoder, the model's last step
    r, c = ModelCode(rows), ModelCode(cols)
    for halves in (1, 2, 3, 4):
        got = cc.product_decode(r, c, y[:40], P, ALPHA[:halves], BETA[:halves], extended=True)
        want = steps[halves - 1]
        assert sorted(got) == ["ext", "out", "status"]
        assert np.array_equal(got["out"], want["out"][:40]) and np.array_equal(got["status"], want["status"][:40])
        assert np.array_equal(got["ext"].view(np.uint32), want["ext"][:40].view(np.uint32))
        assert got["out"].shape == (40, 16, 16) and got["status"].shape == (40, 16)
    assert r.calls == [(P, np.float32(b)) for b in (0.2, 0.2, 0.2, 0.6, 0.2, 0.6)]
    assert c.calls == [(P, np.float32(b)) for b in (0.4, 0.4, 0.4, 0.8)]
    with pytest.raises(cc.CcError):
        cc.product_decode(r, c, np.ones((2, 15, 15), np.float32), 2, (0.0,), (0.5,), extended=True)
    with pytest.raises(ValueError, match="half-iteration"):
        cc.product_decode(r, c, np.ones((2, 16, 16), np.float32), 2, (0.0, 0.5), (0.5,), extended=True)
    with pytest.raises(TypeError, match="float32"):
        cc.product_decode(r, c, np.ones((2, 16, 16), np.uint8), 2, (0.0,), (0.5,), extended=True)
