"""The buffer contract of the soft-decision calls -- cc_correct_chase_batch_dev, cc_correct_chase_soft_batch_dev,
cc_correct_chase_extended_batch_dev (without and with soft output), cc_correct_gmd_batch_dev, cc_product_decode_dev,
cc_product_encode_batch_dev and cc_product_extract_batch_dev -- under the harness of tests/guarded_buffers.py: inputs of
exactly the stated extent at the least alignment of their element type in the middle of poison (NaN, then +3e38 / zeros),
outputs between sentinel guards, every optional output absent in turn, and the results of the two poisons equal bit for bit.
These decoders search rows of floats for their least reliable positions and sum metrics over them: a value fetched from
past the end of a row's buffer would enter the search, and the poison shows it.

The expected arrays are those of the models (chase_model, chase_soft_model, chase_ext_model, gmd_model and the product loop
over them); every comparison is exact, floats as their bytes.  Batches sit on both sides of what a wavefront takes at
once (cc_chase_frames_per_wavefront, asserted), and every batch of more than a few frames holds frames that decode and
frames without a candidate (asserted where the code allows it: a full-length t = 1 code is perfect and always has one,
BCH(255,239) at p = 6 has one in practice, and so has GMD at the full trial count, whose last trial decodes on erasures
alone)."""
import ctypes as C
import functools

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import capi
import chase_ext_model as E
import chase_model as M
import chase_soft_model as S
import gmd_model as G
from checkers import awgn_llr
from guarded_buffers import check_call
from test_chase_soft_host import ALPHA, BETA, P
from test_gpu_product import encode_blocks, model_steps

pytestmark = pytest.mark.gpu

BETA_ONE = 0.4


def lib():
    return capi.lib()


def bch(q, t, N=None):
    return cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag(), n=N)


# ------------------------------------------------ the Chase family ------------------------------------------------
# (q, t, N, p, Eb/N0): BCH(7,4), BCH(63,45) (odd n: every second row of floats sits at 4 mod 8), BCH(255,239), and
# BCH(63,45) shortened to 50
CHASE = {"bch7": (3, 1, None, 2, 2.0), "bch63": (6, 3, None, 3, 3.0), "bch255": (8, 2, None, 6, 4.5), "bch50": (6, 3, 50, 3, 3.0)}
FRAMES = 200


@functools.lru_cache(maxsize=None)
def chase_batch(name, extended):
    """200 frames of one code -- random codewords over AWGN, signed zeros among them, the last forty at -2 dB -- and the
    model's candidates of the 2^p test patterns, made once for the plain, soft and extended calls"""
    q, t, N, p, ebno = CHASE[name]
    dec = M.decoder(q, t, N)
    rng = np.random.default_rng(100 * q + t + (N or 0) + (7 if extended else 0))
    words = dec.encode(rng.integers(0, 2, (FRAMES, dec.l)).astype(np.uint8))
    if extended:
        words = E.extend(words)
    rate = dec.l / words.shape[1]
    y = np.concatenate([awgn_llr(rng, words[:160], rate, ebno), awgn_llr(rng, words[160:], rate, -2.0)])
    y[::7, 1] = np.float32(0.0)
    y[3::11, words.shape[1] - 1] = np.float32(-0.0)
    y = np.ascontiguousarray(y, np.float32)
    y.setflags(write=False)
    return dec, y, (E if extended else M).candidates(dec, y, p)


def chase_sizes(code, p, soft, extended):
    fn = lib().cc_chase_extended_frames_per_wavefront if extended else lib().cc_chase_frames_per_wavefront
    per = fn(code._h, p, int(soft))
    assert 1 <= per <= 64 >> p, (per, p)
    return (1, per + 1, FRAMES)


def outcomes(want, B, name):
    if B == FRAMES:
        assert (want["status"][:B] == M.FRAME_OK).any()
        # (a Hamming code always has a candidate; of BCH(255,239) half the syndromes decode, and 64 patterns never all fail)
        assert (want["status"][:B] == M.FRAME_LOCATOR).any() or name in ("bch7", "bch255")


@pytest.mark.parametrize("name", list(CHASE))
def test_chase(name):
    q, t, N, p, _ = CHASE[name]
    dec, y, cand = chase_batch(name, False)
    want = M.pick(cand, p)
    code = bch(q, t, N)
    n = code.n
    assert n == dec.n and (n % 2 == 1) == (name != "bch50")
    for B in chase_sizes(code, p, False, False):
        outcomes(want, B, name)

        def call(a):
            return lib().cc_correct_chase_batch_dev(code._h, a["llr"], p, a["out"], a["nerr"], a["metric"], a["status"], B, a["stream"])
        outputs = {"out": (np.uint8, B * n), "nerr": (np.int32, B), "metric": (np.float32, B), "status": (np.int32, B)}
        expected = {k: want[k][:B] for k in outputs}
        check_call(call, {"llr": y[:B]}, outputs, expected, optional=("nerr", "metric", "status"), what=(name, p, B))


@pytest.mark.parametrize("name", list(CHASE))
def test_chase_soft(name):
    q, t, N, p, _ = CHASE[name]
    dec, y, cand = chase_batch(name, False)
    want = S.soft(cand, p, BETA_ONE)
    code = bch(q, t, N)
    n = code.n
    for B in chase_sizes(code, p, True, False):
        outcomes(want, B, name)
        if B == FRAMES:
            assert want["has"][:B].any() and (not want["has"][:B].all() or name == "bch7")  # competitors, and +-beta

        def call(a):
            return lib().cc_correct_chase_soft_batch_dev(code._h, a["llr"], p, BETA_ONE, a["out"], a["ext"], a["nerr"], a["metric"],
                                                         a["status"], B, a["stream"])
        outputs = {"out": (np.uint8, B * n), "ext": (np.float32, B * n), "nerr": (np.int32, B), "metric": (np.float32, B),
                   "status": (np.int32, B)}
        expected = {k: want[k][:B] for k in outputs}
        check_call(call, {"llr": y[:B]}, outputs, expected, optional=("nerr", "metric", "status"), what=(name, p, B))


@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("name", list(CHASE))
def test_chase_extended(name, soft):
    """rows of n + 1 values; ext absent is the hard-output call, ext present the soft one"""
    q, t, N, p, _ = CHASE[name]
    dec, y, cand = chase_batch(name, True)
    want = S.soft(cand, p, BETA_ONE) if soft else M.pick(cand, p)
    code = bch(q, t, N)
    n = code.n + 1
    assert y.shape[1] == n
    for B in chase_sizes(code, p, soft, True):
        outcomes(want, B, name)

        def call(a):
            return lib().cc_correct_chase_extended_batch_dev(code._h, a["llr"], p, BETA_ONE, a["out"],
                                                             a["ext"], a["nerr"], a["metric"], a["status"], B, a["stream"])
        outputs = {"out": (np.uint8, B * n), "ext": (np.float32, B * n), "nerr": (np.int32, B), "metric": (np.float32, B),
                   "status": (np.int32, B)}
        expected = {k: want[k][:B] for k in outputs if k in want}
        check_call(call, {"llr": y[:B]}, outputs, expected, optional=("nerr", "metric", "status"),
                   absent=() if soft else ("ext",), what=(name, p, B, soft))


# ------------------------------------------------ GMD ------------------------------------------------
@pytest.mark.parametrize("q,t", [(3, 2), (4, 3), (8, 8)], ids=["rs7-3", "rs15-9", "rs255-239"])
def test_gmd(q, t):
    """the full trial count; both inputs in poison, the words as bytes and the reliabilities as floats"""
    from test_gpu_gmd import batches
    bt = batches(q, t, None, 1)
    want = G.pick(bt["cand"], t + 1)
    code = cc.rs(q, cc.errors(t), cc.berlekamp_massey_tag())
    n = code.n
    for B in (1, 5, 130):
        assert (want["status"][:B] == G.FRAME_OK).all()  # (trial t decodes on erasures alone)
        assert B < 130 or ((want["nerr"][:B] > 0).any() and (want["winner"][:B] > 0).any())

        def call(a):
            return lib().cc_correct_gmd_batch_dev(code._h, a["words"], a["rel"], capi.GMD_ALL, a["out"], a["nerr"], a["metric"],
                                                  a["status"], B, a["stream"])
        outputs = {"out": (np.uint8, B * n), "nerr": (np.int32, B), "metric": (np.float32, B), "status": (np.int32, B)}
        expected = {k: want[k][:B] for k in outputs}
        check_call(call, {"words": bt["w"][:B], "rel": bt["r"][:B]}, outputs, expected, optional=("nerr", "metric", "status"),
                   what=(q, t, B))


# ------------------------------------------------ product codes ------------------------------------------------
# rows (q, t), cols (q, t), extended, Eb/N0, seed.  255 x 255 is the only shape here whose mix-and-turn tiles (33 rows) do
# not divide the rows: a remainder of 24.
PRODUCTS = {"7x7": ((3, 1), (3, 1), False, 2.0, 21), "15x7": ((4, 1), (3, 1), False, 2.0, 22), "7x15": ((3, 1), (4, 1), False, 2.0, 23),
            "e64x64": ((6, 2), (6, 2), True, 3.0, 24), "255x255": ((8, 2), (8, 2), False, 4.5, 25)}


@functools.lru_cache(maxsize=None)
def product_batch(name, blocks):
    (rq, rt), (cq, ct), extended, ebno, seed = PRODUCTS[name]
    rows, cols = M.decoder(rq, rt), M.decoder(cq, ct)
    rng = np.random.default_rng(seed)
    msg = rng.integers(0, 2, (blocks, cols.l, rows.l)).astype(np.uint8)
    sent = encode_blocks(rows, cols, msg, extended)
    y = awgn_llr(rng, sent, rows.l * cols.l / sent[0].size, ebno)
    y.setflags(write=False)
    return rows, cols, msg, sent, y


def product_handle(name):
    (rq, rt), (cq, ct), extended = PRODUCTS[name][:3]
    return cc.product_code(bch(rq, rt), bch(cq, ct), extended=extended)


@pytest.mark.parametrize("name,halves", [("7x7", h) for h in (1, 2, 3, 4)] + [("15x7", 2), ("7x15", 2), ("e64x64", 2), ("255x255", 2)])
def test_product_decode(name, halves):
    """a last pass over rows (halves odd) or columns changes which kernels write out, ext and status; ext absent swaps the
    last decoder for the hard-output one"""
    pc = product_handle(name)
    extended = PRODUCTS[name][2]
    for B in (1,) if name == "255x255" else (1, 3):
        rows, cols, _, _, y = product_batch(name, B)
        assert y.shape == (B, pc.n2, pc.n1)
        last = model_steps(rows, cols, y, extended, P, ALPHA[:halves], BETA[:halves])[-1]
        lines = pc.n2 if halves % 2 else pc.n1
        assert last["status"].shape == (B, lines)
        desc = pc._pc(P, ALPHA[:halves], BETA[:halves])

        def call(a):
            return lib().cc_product_decode_dev(C.byref(desc), a["y"], a["out"], a["ext"], a["status"], B, a["stream"])
        outputs = {"out": (np.uint8, B * pc.n), "ext": (np.float32, B * pc.n), "status": (np.int32, B * lines)}
        expected = {k: last[k] for k in outputs}
        check_call(call, {"y": y}, outputs, expected, optional=("ext",), what=(name, halves, B))


def message_positions(dec):
    """the positions of a word that extraction reads: those whose unit vector extracts to something"""
    unit = np.eye(dec.n, dtype=np.uint8)
    return np.flatnonzero(dec.extract(unit).any(axis=1))


@pytest.mark.parametrize("name", list(PRODUCTS))
def test_product_encode_and_extract(name):
    """extract from blocks whose other positions hold random bits, no codeword's: only the message positions may reach
    the result"""
    pc = product_handle(name)
    for B in (1,) if name == "255x255" else (1, 5):
        rows, cols, msg, sent, _ = product_batch(name, B)
        desc = pc._pc()

        def encode(a):
            return lib().cc_product_encode_batch_dev(C.byref(desc), a["msg"], a["cw"], B, a["stream"])
        check_call(encode, {"msg": msg}, {"cw": (np.uint8, B * pc.n)}, {"cw": sent}, what=(name, "encode", B))
        at_r, at_c = message_positions(cols), message_positions(rows)
        assert at_r.size == pc.k2 and at_c.size == pc.k1
        carries = np.zeros((pc.n2, pc.n1), bool)
        carries[np.ix_(at_r, at_c)] = True
        assert np.array_equal(sent[:, carries].reshape(msg.shape), msg)
        dirty = np.where(carries[None], sent, np.random.default_rng(B).integers(0, 2, sent.shape).astype(np.uint8))
        assert (dirty != sent).any()

        def extract(a):
            return lib().cc_product_extract_batch_dev(C.byref(desc), a["cw"], a["msg"], B, a["stream"])
        check_call(extract, {"cw": dirty}, {"msg": (np.uint8, msg.size)}, {"msg": msg}, what=(name, "extract", B))
