"""CPU tests of the Chase-Pyndiah soft output (cc_correct_chase_soft_batch(_dev)): the model of
tests/chase_soft_model.py against the full-list (max-log-MAP) value over every codeword of small codes, the refusals and
their order on CC_DEVICE_NONE handles, the bindings, and product decoding over the model.
tests/test_gpu_chase_soft.py holds the device against the model."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import capi
import chase_model as M
import chase_soft_model as S
from checkers import BCH, Oracle, awgn_llr

NONE = dict(device=capi.DEVICE_NONE)
BM = cc.berlekamp_massey_tag
NAMES = ("cc_correct_chase_soft_batch", "cc_correct_chase_soft_batch_dev", "cc_chase_frames_per_wavefront")


# ---- the model against the full list ----
def all_words(dec):
    msgs = ((np.arange(1 << dec.l)[:, None] >> np.arange(dec.l)[None, :]) & 1).astype(np.uint8)
    words = dec.encode(msgs)
    assert len({w.tobytes() for w in words}) == 1 << dec.l
    return words


def full_list(words, y, D=None):
    """per frame, over every codeword, written out with nothing of the model: the metrics (float32 sums in ascending
    position), the nearest codeword D (the first of equals; or the codewords D given, one of several equally near where
    metrics tie), and per position the smallest metric among the codewords that differ from D there (inf: none) with the
    value s (K - M_D) - y"""
    B, n = y.shape
    z = (y < 0).astype(np.uint8)
    Mw = np.zeros((B, words.shape[0]), np.float32)
    for i in range(n):
        Mw = (Mw + np.where(words[None, :, i] != z[:, None, i], np.abs(y[:, None, i]), np.float32(0))).astype(np.float32)
    best = Mw.argmin(axis=1)
    if D is not None:
        best = np.array([np.flatnonzero((words == D[f][None, :]).all(axis=1))[0] for f in range(B)])
    D, MD = words[best], Mw[np.arange(B), best]
    differs = words[None, :, :] != D[:, None, :]
    K = np.where(differs, Mw[:, :, None], np.float32(np.inf)).min(axis=1).astype(np.float32)
    s = np.where(D == 0, np.float32(1), np.float32(-1))
    with np.errstate(invalid="ignore"):
        value = ((s * (K - MD[:, None]).astype(np.float32)).astype(np.float32) - y).astype(np.float32)
    return dict(M=Mw, D=D, MD=MD, K=K, s=s, value=value)


def test_model_never_below_the_full_list_and_equal_where_the_competitor_is_a_candidate():
    orc = Oracle(BCH, 4, 2)
    assert (orc.n, orc.l, orc.t) == (15, 7, 2)
    words = all_words(orc)
    rng = np.random.default_rng(1508)
    y = awgn_llr(rng, words[rng.integers(0, 128, 300)], orc.l / orc.n, 2.0)
    full = full_list(words, y)
    cand = M.candidates(orc, y)
    beta = np.float32(0.5)
    checked = equal = above = without = 0
    for p in (2, 4, 6):
        got = S.soft(cand, p, beta)
        for f in range(y.shape[0]):
            if got["winner"][f] < 0:
                assert (got["ext"][f].view(np.uint32) == 0).all()
                continue
            if not np.array_equal(got["out"][f], full["D"][f]):
                continue  # the winner is not the nearest codeword: the full list says nothing about this frame
            assert got["metric"][f].view(np.uint32) == full["MD"][f].view(np.uint32)
            s = full["s"][f]
            js = np.flatnonzero(cand["ok"][f, : 1 << p])
            mine = {cand["words"][f, j].tobytes() for j in js}
            for i in range(orc.n):
                if not got["has"][f, i]:
                    assert got["ext"][f, i].view(np.uint32) == (s[i] * beta).view(np.uint32)
                    without += 1
                    continue
                checked += 1
                # rounding is monotone: K >= K_full gives s ext >= s value, in float32, exactly
                assert s[i] * got["ext"][f, i] >= s[i] * full["value"][f, i], (p, f, i)
                rivals = np.flatnonzero((words[:, i] != full["D"][f, i]) & (full["M"][f] == full["K"][f, i]))
                if any(words[r].tobytes() in mine for r in rivals):
                    assert got["ext"][f, i].view(np.uint32) == full["value"][f, i].view(np.uint32), (p, f, i)
                    equal += 1
                else:
                    above += s[i] * got["ext"][f, i] > s[i] * full["value"][f, i]
    assert checked > 2000 and equal > 500 and above > 100 and without > 500, (checked, equal, above, without)


@pytest.mark.parametrize("N", [5, 6])
def test_every_word_a_test_pattern_gives_the_full_list(N):
    """BCH(15,11) shortened to N = 5 and 6 with p = n: every word of length N is a test pattern and every codeword a
    candidate, so ext is the full-list value wherever some codeword differs from the decision, and +-beta elsewhere"""
    dec = M.decoder(4, 1, N)
    assert (dec.n, dec.l, dec.t) == (N, N - 4, 1)
    words = all_words(dec)
    rng = np.random.default_rng(410 + N)
    y = awgn_llr(rng, words[rng.integers(0, 1 << dec.l, 200)], dec.l / dec.n, 1.0)
    y[150:] = rng.choice(np.array([-1.0, -0.5, -0.0, 0.0, 0.5, 0.5, 1.0], np.float32), (50, N))
    beta = np.float32(0.25)
    got = S.chase_soft(dec, y, N, beta)
    full = full_list(words, y, got["out"])  # (the quantised frames have equally near codewords: the winner is one of them)
    assert (got["status"] == M.FRAME_OK).all() and np.array_equal(got["metric"], full["M"].min(axis=1))
    assert (full_list(words, y)["D"] != got["out"]).any(axis=1).sum() < 25
    has = np.isfinite(full["K"])
    assert np.array_equal(got["has"], has) and has.any() and not has.all()
    want = np.where(has, full["value"], full["s"] * beta).astype(np.float32)
    assert np.array_equal(got["ext"].view(np.uint32), want.view(np.uint32))


def test_the_three_cases_on_one_frame_by_hand():
    """BCH(7,4), p = 1: y decides z = 0000000 with position 2 the weakest.  Pattern 0 gives the zero word with M = 0,
    pattern 1 decodes z ^ e_2 back to it: no competitor, ext = +beta everywhere.  With more patterns other codewords
    appear and a position where one of them differs has a competitor; a frame without a candidate has ext = +0.0"""
    dec = M.decoder(3, 1)
    y = np.array([[1.0, 0.9, 0.1, 0.8, 1.1, 1.2, 0.7]], np.float32)
    got = S.chase_soft(dec, y, 1, 0.5)
    assert got["winner"][0] == 0 and not got["has"].any() and (got["ext"] == np.float32(0.5)).all()
    y2 = y.copy()
    y2[0, 2] = np.float32(-0.1)  # z = e_2: pattern 0 decodes to 0 (M = 0.1), pattern 1 is the zero word itself
    got = S.chase_soft(dec, y2, 1, 0.5)
    assert not got["out"].any() and got["metric"][0] == np.float32(0.1) and not got["has"].any()
    assert (got["ext"] == np.float32(0.5)).all()  # the decision is 0 at position 2 as well: s = +1 there
    # p = 3 over the weakest positions 2, 6, 3: z ^ e_2 ^ e_6 ^ e_3 is within one position of a weight-3 or -4 codeword
    got = S.chase_soft(dec, y2, 3, 0.5)
    assert got["has"].any() and not got["out"].any()
    i = int(np.flatnonzero(got["has"])[0])
    cand = M.candidates(dec, y2, 3)
    rival = min((cand["M"][0, j] for j in range(8) if cand["ok"][0, j] and cand["words"][0, j, i]), default=None)
    assert got["ext"][0, i] == np.float32(np.float32(rival - np.float32(0.1)) - y2[0, i])
    # BCH(7,4) cut to five positions, p = 0: where the Hamming decoder corrects a position the frame does not have there
    # is no candidate, and ext is +0.0 whatever beta
    short = M.decoder(3, 1, 5)
    none = S.chase_soft(short, awgn_llr(np.random.default_rng(3), np.zeros((64, 5), np.uint8), 0.4, 0.0), 0, 0.5)
    lost = none["status"] == M.FRAME_LOCATOR
    assert lost.any() and not lost.all() and (none["ext"][lost].view(np.uint32) == 0).all()
    assert (np.abs(none["ext"][~lost]) == np.float32(0.5)).all()  # one pattern: no competitor anywhere


# ---- the C interface on handles without a device ----
def _call(code, p, beta=0.5, llr=True, out=True, ext=True, dev=False, B=4, overlap=None):
    n = code.n if code is not None else 15
    buf = np.ones(2 * B * n + 8, np.float32)
    y, e = buf[: B * n], buf[B * n + 4: 2 * B * n + 4]
    if overlap is not None:
        e = buf[overlap: overlap + B * n]
    o = np.zeros((B, n), np.uint8)
    ptr = lambda a, on: a.ctypes.data_as(C.c_void_p) if on else None
    args = [code._h if code is not None else None, ptr(y, llr), p, C.c_float(beta), ptr(o, out), ptr(e, ext), None, None,
            None, B]
    if dev:
        return capi.lib().cc_correct_chase_soft_batch_dev(*args, None)
    return capi.lib().cc_correct_chase_soft_batch(*args)


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
    assert callable(cc.product_decode) and "product_decode" in cc.__all__


def test_frames_per_wavefront():
    """64 >> p, fewer where a wavefront's 16 000 bytes of LDS bound it: the figures of DESIGN 4.11 and 4.13; K doubles what
    a frame holds, so the soft output runs half the frames where the bound applies"""
    F = capi.lib().cc_chase_frames_per_wavefront
    want = {(8, 3): ([12, 12, 12, 8, 4, 2, 1], [6, 6, 6, 6, 4, 2, 1]), (7, 3): ([24, 24, 16, 8, 4, 2, 1], [12, 12, 12, 8, 4, 2, 1]),
            (6, 3): ([45, 32, 16, 8, 4, 2, 1], [24, 24, 16, 8, 4, 2, 1]), (4, 2): ([64, 32, 16, 8, 4, 2, 1],) * 2,
            (8, 16): ([3, 3, 3, 3, 3, 2, 1], [1, 1, 1, 1, 1, 1, 1])}
    for (q, t), (hard, soft) in want.items():
        code = cc.primitive_bch(q, cc.errors(t), BM(), **NONE)
        assert [F(code._h, p, 0) for p in range(7)] == hard, (q, t)
        assert [F(code._h, p, 1) for p in range(7)] == soft, (q, t)
    ok = served()[1]
    assert F(None, 2, 1) == 0 and F(ok._h, 7, 1) == 0 and F(cc.rs(8, cc.errors(16), BM(), **NONE)._h, 2, 0) == 0
    assert F(cc.primitive_bch(3, cc.errors(1), BM(), n=5, **NONE)._h, 6, 1) == 0


def test_valid_calls_reach_the_device_check():
    for code in served():
        for p in range(capi.CHASE_MAX_P + 1):
            for dev in (False, True):
                for beta in (0.0, 0.5, 3e38):
                    assert _call(code, p, beta, dev=dev) == capi.ERR_NO_DEVICE, (code.to_string(), p, beta)


def test_refusals_and_their_order():
    lib = capi.lib()
    ok = served()[1]
    n = ok.n
    bch_ms = cc.primitive_bch(5, cc.errors(2), cc.min_sum_tag(10), **NONE)
    matrix = cc.min_sum_decoder(bch_ms.H(), cc.min_sum_tag(10), **NONE)
    rs = cc.rs(8, cc.errors(16), BM(), **NONE)
    bad_betas = (-1.0, -1e-45, float("inf"), float("-inf"), float("nan"))
    for dev in (False, True):
        # 1. null pointers, ext among them, whatever else is wrong with the call
        for p, beta in ((0, 0.5), (99, -1.0)):
            assert _call(None, p, beta, dev=dev) == capi.ERR_INVALID_ARGUMENT
            for code in (ok, matrix, bch_ms, rs):
                for missing in ("llr", "out", "ext"):
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
                assert _call(code, p, beta, dev=dev, overlap=overlap) == capi.ERR_UNSUPPORTED, text
                assert text in lib.cc_last_error().decode(), text
        # 3. beta negative, infinite or NaN: invalid, before the device is asked for
        for beta in bad_betas:
            assert _call(ok, 3, beta, dev=dev) == capi.ERR_INVALID_ARGUMENT, beta
        for beta in (0.0, -0.0, 1e-45, 3.4e38):
            assert _call(ok, 3, beta, dev=dev) == capi.ERR_NO_DEVICE, beta
        # 4. ext overlapping llr by any byte: invalid; next to it on either side: served
        B = 4
        for off in (0, 1, B * n - 1):
            assert _call(ok, 3, dev=dev, B=B, overlap=off) == capi.ERR_INVALID_ARGUMENT, off
        assert _call(ok, 3, dev=dev, B=B, overlap=B * n) == capi.ERR_NO_DEVICE
        # 5. and only a call that passes all of this asks for a device; an empty batch needs no pointers
        assert _call(ok, 6, dev=dev) == capi.ERR_NO_DEVICE
        assert _call(ok, 3, llr=False, out=False, ext=False, dev=dev, B=0) == capi.ERR_NO_DEVICE
        assert _call(ok, 3, -1.0, llr=False, out=False, ext=False, dev=dev, B=0) == capi.ERR_INVALID_ARGUMENT


# ---- Python ----
def test_correct_batch_refuses_combinations():
    code = served()[1]
    rs = cc.rs(8, cc.errors(16), BM(), **NONE)
    y = np.ones((2, code.n), np.float32)
    with pytest.raises(TypeError, match="soft="):
        code.correct_batch(y, soft=0.5)
    with pytest.raises(TypeError, match="soft="):
        code.decode_batch(y, soft=0.5)
    with pytest.raises(TypeError, match="soft="):
        rs.correct_batch(np.ones((2, rs.n), np.uint8), gmd=2, reliability=np.ones((2, rs.n), np.float32), soft=0.5)
    with pytest.raises(TypeError, match="soft="):
        code.correct_batch(y, chase=2, gmd=2, reliability=y, soft=0.5)
    for kw in (dict(erasures=[[1], []]), dict(want_L=True), dict(packed=True), dict(interleave=2),
               dict(out=np.zeros((2, code.n), np.uint8))):
        with pytest.raises(TypeError, match="chase="):
            code.correct_batch(y, chase=2, soft=0.5, **kw)
    with pytest.raises(TypeError, match="chase="):
        code.decode_batch(y, chase=2, soft=0.5, packed=True)
    with pytest.raises(TypeError, match="float32"):
        code.correct_batch(np.ones((2, code.n), np.uint8), chase=2, soft=0.5)
    for beta in ("0.5", None.__class__, [0.5], True):
        with pytest.raises(TypeError, match="soft="):
            code.correct_batch(y, chase=2, soft=beta)
    with pytest.raises(cc.CcError):
        code.correct_batch(np.ones((2, code.n + 1), np.float32), chase=2, soft=0.5)
    for kw, status in ((dict(chase=2, soft=0.5), capi.ERR_NO_DEVICE), (dict(chase=2, soft=0), capi.ERR_NO_DEVICE),
                       (dict(chase=7, soft=0.5), capi.ERR_UNSUPPORTED), (dict(chase=2, soft=-0.5), capi.ERR_INVALID_ARGUMENT),
                       (dict(chase=2, soft=float("nan")), capi.ERR_INVALID_ARGUMENT),
                       (dict(chase=2, soft=1e39), capi.ERR_INVALID_ARGUMENT)):  # 1e39 is +inf as a float32
        for call in (code.correct_batch, code.decode_batch):
            with pytest.raises(cc.CcError) as e:
                call(y, **kw)
            assert e.value.status == status, kw


# ---- product decoding over the model ----
class ModelCode:
    """what product_decode needs of a code, answered by the model: n and correct_batch(X, chase=, soft=)"""

    def __init__(self, dec):
        self.dec, self.n, self.calls = dec, dec.n, []

    def correct_batch(self, X, chase=None, soft=None):
        assert isinstance(X, np.ndarray) and X.dtype == np.float32 and X.flags.c_contiguous and X.shape[1] == self.n
        self.calls.append((chase, soft))
        r = S.chase_soft(self.dec, X, chase, soft)
        return dict(out=r["out"], ext=r["ext"], status=r["status"], nerr=r["nerr"], metric=r["metric"])


# rows x columns, Eb/N0 of the product code, blocks; the schedule is the same for both
PRODUCTS = {"15_11x15_11": ((4, 1), (4, 1), 4.5, 300), "15_7x15_11": ((4, 2), (4, 1), 3.5, 300)}
P, ALPHA, BETA = 4, (0.0, 0.3, 0.5, 0.7), (0.2, 0.4, 0.6, 0.8)


@functools.lru_cache(maxsize=None)
def product_batch(name):
    """random product codewords (rows encoded, then columns), BPSK plus Gaussian noise from a fixed seed"""
    (rq, rt), (cq, ct), ebno, blocks = PRODUCTS[name]
    rows, cols = M.decoder(rq, rt), M.decoder(cq, ct)
    rng = np.random.default_rng(1998)
    info = rng.integers(0, 2, (blocks, cols.l, rows.l)).astype(np.uint8)
    wide = rows.encode(info.reshape(-1, rows.l)).reshape(blocks, cols.l, rows.n)  # every information row encoded
    sent = cols.encode(np.ascontiguousarray(wide.transpose(0, 2, 1)).reshape(-1, cols.l)).reshape(blocks, rows.n, cols.n)
    sent = np.ascontiguousarray(sent.transpose(0, 2, 1))  # (blocks, n2, n1): every column a word of cols
    rate = rows.l * cols.l / (rows.n * cols.n)
    y = awgn_llr(rng, sent, rate, ebno)
    y.setflags(write=False)
    return rows, cols, sent, y


def hard_rows_then_columns(rows, cols, y):
    """bounded-distance hard decoding of the rows, then of the columns of what that left (a failed word stays)"""
    from checkers import BM as ORACLE_BM
    B, n2, n1 = y.shape
    z = (y < 0).astype(np.uint8)
    z = np.asarray(rows.correct_hard(ORACLE_BM, z.reshape(-1, n1))[0]).reshape(B, n2, n1)
    zt = np.ascontiguousarray(z.transpose(0, 2, 1)).reshape(-1, n2)
    return np.ascontiguousarray(np.asarray(cols.correct_hard(ORACLE_BM, zt)[0]).reshape(B, n1, n2).transpose(0, 2, 1))


@pytest.mark.parametrize("name", sorted(PRODUCTS))
def test_product_decode_over_the_model(name):
    """Noise level and schedule were chosen on the model alone.  Block (word) errors out of 300 blocks, seed 1998,
    p = 4, alpha = 0, 0.3, 0.5, 0.7, beta = 0.2, 0.4, 0.6, 0.8:
        BCH(15,11) x BCH(15,11) at 4.5 dB: hard rows then columns 130, after the half-iterations 153, 21, 1, 0
        BCH(15,7)  x BCH(15,11) at 3.5 dB: hard rows then columns 235, after the half-iterations 193, 155, 6, 2
    (at 3.5 dB and 2.0 dB: 237 against 256, 118, 18, 3 and 299 against 282, 279, 122, 59.)
    The assertion is the issue's: at least 20 after hard decoding, at most half as many after the schedule."""
    rows, cols, sent, y = product_batch(name)
    for dec, words in ((rows, sent.reshape(-1, 15)), (cols, sent.transpose(0, 2, 1).reshape(-1, 15))):
        H = np.asarray(cc.primitive_bch(4, cc.errors(dec.t), BM(), **NONE).H(), np.int64)
        assert dec.n == 15 and not (words.astype(np.int64) @ H.T % 2).any()  # rows and columns are codewords
    hard = hard_rows_then_columns(rows, cols, y)
    hard_errors = int((hard != sent).any(axis=(1, 2)).sum())
    steps = S.product_decode(rows, cols, y, P, ALPHA, BETA)
    soft_errors = [int((s["out"] != sent).any(axis=(1, 2)).sum()) for s in steps]
    print(name, "hard", hard_errors, "after each half-iteration", soft_errors)
    assert hard_errors >= 20 and 2 * soft_errors[-1] <= hard_errors, (hard_errors, soft_errors)
    # cc.product_decode is the same loop: with the model as its component decoder it returns the model's last step
    r, c = ModelCode(rows), ModelCode(cols)
    for halves in (1, 2, 3, 4):
        got = cc.product_decode(r, c, y[:40], P, ALPHA[:halves], BETA[:halves])
        want = S.product_decode(rows, cols, y[:40], P, ALPHA[:halves], BETA[:halves])[-1]
        assert sorted(got) == ["ext", "out", "status"]
        assert np.array_equal(got["out"], want["out"]) and np.array_equal(got["status"], want["status"])
        assert np.array_equal(got["ext"].view(np.uint32), want["ext"].view(np.uint32))
        assert got["out"].shape == (40, 15, 15) and got["status"].shape == (40, 15)
    assert r.calls == [(P, np.float32(b)) for b in (0.2, 0.2, 0.2, 0.6, 0.2, 0.6)]
    assert c.calls == [(P, np.float32(b)) for b in (0.4, 0.4, 0.4, 0.8)]


def test_product_decode_refuses_what_it_cannot_loop_over():
    rows, cols = ModelCode(M.decoder(4, 1)), ModelCode(M.decoder(4, 2))
    y = np.ones((2, 15, 15), np.float32)
    with pytest.raises(ValueError, match="half-iteration"):
        cc.product_decode(rows, cols, y, 2, (0.0, 0.5), (0.5,))
    with pytest.raises(ValueError, match="half-iteration"):
        cc.product_decode(rows, cols, y, 2, (), ())
    with pytest.raises(cc.CcError):
        cc.product_decode(rows, cols, np.ones((2, 15, 14), np.float32), 2, (0.0,), (0.5,))
    with pytest.raises(cc.CcError):
        cc.product_decode(rows, cols, np.ones((30, 15), np.float32), 2, (0.0,), (0.5,))
    with pytest.raises(TypeError, match="float32"):
        cc.product_decode(rows, cols, np.ones((2, 15, 15), np.uint8), 2, (0.0,), (0.5,))
