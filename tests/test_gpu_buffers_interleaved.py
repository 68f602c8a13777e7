"""The buffer contract of the symbol-interleaved entry points -- cc_interleave_dev, cc_deinterleave_dev and
the interleaved encode, correct, extract and decode calls, bytes and 16-bit symbols -- under the harness of
tests/guarded_buffers.py.  tests/test_gpu_buffers.py runs RS(255,223) at depths 2, 16 and 33; here are the other paths of
the loader (bitslice.hip, interleaved_load_run: 16-byte, 8-byte, dword and 16-bit runs, the byte-by-byte branch of the
depths that do not divide 32, where a group of 32 frames starts inside a block, and the exit of a shortened code), the
tiles of interleave_tile_kernel with a ragged last one, the dword runs and byte tail of interleaved_extract_kernel, erasure
lists, out == in and the host form.

Expected arrays: the plain-C oracle's words laid out by interleave_model.interleave, bit for bit; no frame is left out.
The tables and builders need no device: tests/test_buffer_cases_host.py checks every batch on the CPU."""
import functools

import numpy as np
import pytest

import channelcoding_amd as cc
import shortened_model as S
from checkers import BCH, BM, RS, Oracle, WideOracle
from guarded_buffers import check_call
from interleave_model import deinterleave, interleave
from test_gpu_buffers import HARD_TAGS, corrupted, erased, hard_expected, lib, map_check, messages, symbol_type
from test_gpu_buffers_packed import status_rule

pytestmark = pytest.mark.gpu

# name -> (family, q, t, modular polynomial, N, mu, coding)
CODES = {
    "RS(255,223)": (RS, 8, 16, None, None, 1, 0),
    "RS(204,188)": (RS, 8, 8, None, 204, 0, 0),  # DVB: first root alpha^0, shortened
    "RS(15,9)": (RS, 4, 3, None, None, 1, 0),
    "RS(7,3)": (RS, 3, 2, None, None, 1, 0),
    "BCH(63,45)": (BCH, 6, 3, None, None, 1, 0),
    "BCH(63,45) c = a g": (BCH, 6, 3, None, None, 1, 1),
    "BCH(511,484)": (BCH, 9, 3, 0x211, None, 1, 0),
    "RS(1023,1015)": (RS, 10, 4, 0x409, None, 1, 0),
}


@functools.lru_cache(maxsize=None)
def model_of(name):
    family, q, t, poly, N, mu, coding = CODES[name]
    if q <= 8 and mu == 1:
        m = Oracle(family, q, t, coding=coding)
    else:  # (the 16-bit build serves q <= 8 too, and decodes other first roots through rs_roots_model)
        m = WideOracle(family, q, t, poly or 0, mu, 1, coding)
    return S.Shortened(m, N) if N else m


def handle_of(name):
    family, q, t, poly, N, mu, coding = CODES[name]
    kw = dict(mu=mu, step=1) if family == RS else {}
    code = (cc.primitive_bch if family == BCH else cc.rs)(q, cc.errors(t), HARD_TAGS[BM](), modular_polynomial=poly, n=N,
                                                          coding="multiplication" if coding else "division", **kw)
    m = model_of(name)
    assert (code.n, code.l) == (m.n, m.l), name
    return code


def seed_of(name, *more):
    return 1000 * list(CODES).index(name) + sum((i + 3) * int(v) for i, v in enumerate(more))


# ------------------------------------------------ the layout itself ------------------------------------------------
# (63, 256): two tiles per block, the second ragged
LAYOUTS = [(width, n, I, B) for width in (1, 2) for n, I in ((1, 2), (7, 3), (255, 16), (63, 256), (300, 5)) for B in (I, 3 * I)]


@functools.lru_cache(maxsize=None)
def layout_batch(width, n, I, B):
    """random symbols, frame-major (B, n), and the same as blocks (B / I, n, I)"""
    rng = np.random.default_rng(10000 * width + 100 * n + I + B)
    x = rng.integers(0, 1 << (8 * width), (B, n)).astype(np.uint8 if width == 1 else np.uint16)
    return x, interleave(x, I)


@pytest.mark.parametrize("width,n,I,B", LAYOUTS)
def test_interleave(width, n, I, B):
    x, blocks = layout_batch(width, n, I, B)

    def call(p):
        return lib().cc_interleave_dev(p["in"], width, n, I, p["out"], B, p["stream"])
    check_call(call, {"in": x}, {"out": (x.dtype, x.size)}, {"out": blocks}, what=("interleave", width, n, I, B))


@pytest.mark.parametrize("width,n,I,B", LAYOUTS)
def test_deinterleave(width, n, I, B):
    x, blocks = layout_batch(width, n, I, B)
    assert np.array_equal(deinterleave(blocks, I), x)

    def call(p):
        return lib().cc_deinterleave_dev(p["in"], width, n, I, p["out"], B, p["stream"])
    check_call(call, {"in": blocks}, {"out": (x.dtype, x.size)}, {"out": x}, what=("deinterleave", width, n, I, B))


# ------------------------------------------------ correct ------------------------------------------------
# (code, I, B, route of cc_interleaved_route, erasure list?, out == in?)
# I = 3 and 5 with 43 and 27 blocks: groups of 32 frames start inside a block and the last group is partial
CORRECT_CASES = ([("RS(255,223)", I, B, 1, False, False) for I in (4, 8) for B in (I, 3 * I)] +
                 [("RS(255,223)", 3, 43 * 3, 1, False, False), ("RS(255,223)", 5, 27 * 5, 1, False, False)] +
                 [("RS(204,188)", 4, B, 1, False, False) for B in (4, 12)] +
                 [("RS(255,223)", 16, 48, 1, False, True)] +
                 [("RS(15,9)", 3, 9, 0, False, False), ("RS(255,223)", 4, 12, 0, True, False),
                  ("RS(255,223)", 4, 12, 0, True, True)])
WIDE_CORRECT_CASES = [("BCH(511,484)", 3, B, 0, False, False) for B in (3, 6)]


@functools.lru_cache(maxsize=None)
def correct_batch(name, I, B, with_erasures):
    """a dict: rx (frame-major), per, csr, out / nerr / status (the oracle's, frame-major)"""
    m = model_of(name)
    seed = seed_of(name, I, B, with_erasures)
    per = csr = None
    if with_erasures:
        rx, per, csr = erased(m, B, seed, 6)
    else:
        rx = corrupted(m, B, seed)
    out, nerr, st = hard_expected(m, BM, rx, per)
    return dict(rx=rx, per=per, csr=csr, out=out, nerr=nerr, status=st)


def interleaved_correct(code, name, fn, case, I, what, in_place=False):
    B = case["rx"].shape[0]
    inputs = {"in": interleave(case["rx"], I)}
    if case["csr"] is not None:
        inputs.update(erasures=case["csr"][0], offsets=case["csr"][1])
        assert case["csr"][1].size == B + 1 and case["csr"][0].size == case["csr"][1][-1] > 0

    def call(p):
        return fn(code._h, p["in"], p.get("erasures"), p.get("offsets"), p["out"], p["nerr"], p["status"], B, I, p["stream"])
    outputs = {"out": (case["out"].dtype, case["out"].size), "nerr": (np.int32, B), "status": (np.int32, B)}
    expected = {"out": interleave(case["out"], I), "nerr": case["nerr"],
                "status": status_rule(case["status"], BM, CODES[name][4] is not None)}
    check_call(call, inputs, outputs, expected, optional=("nerr", "status"), what=what,
               in_place={"out": "in"} if in_place else None)


@pytest.mark.parametrize("name,I,B,route,with_erasures,in_place", CORRECT_CASES)
def test_correct(name, I, B, route, with_erasures, in_place):
    code = handle_of(name)
    assert code.interleaved_route(B, I, with_erasures) == route
    interleaved_correct(code, name, lib().cc_correct_hard_interleaved_batch_dev, correct_batch(name, I, B, with_erasures), I,
                        (name, I, B, with_erasures, in_place), in_place=in_place)


@pytest.mark.parametrize("name,I,B,route,with_erasures,in_place", WIDE_CORRECT_CASES)
def test_correct_16_bit_symbols(name, I, B, route, with_erasures, in_place):
    code = handle_of(name)
    assert code.wide and code.interleaved_route(B, I, with_erasures) == route
    interleaved_correct(code, name, lib().cc_correct_hard_interleaved_batch_u16_dev, correct_batch(name, I, B, with_erasures),
                        I, (name, I, B, "u16"))


# ------------------------------------------------ encode, extract ------------------------------------------------
# (code, I, B, route of cc_interleaved_map_route)
ENCODE_CASES = ([("RS(255,223)", I, B, 1) for I in (4, 8) for B in (I, 3 * I)] + [("RS(255,223)", 3, B, 1) for B in (3, 43 * 3)] +
                [("BCH(63,45)", 3, B, 0) for B in (3, 9)])
WIDE_ENCODE_CASES = [("BCH(511,484)", 3, B, 0) for B in (3, 6)]
# RS(7,3) at depth 3: a run of 9 bytes, two dwords and a one-byte tail
EXTRACT_CASES = ([("RS(7,3)", 3, B, 1) for B in (3, 9)] + [("RS(255,223)", 16, 16, 1), ("BCH(63,45) c = a g", 3, 9, 0)])
WIDE_EXTRACT_CASES = [("RS(1023,1015)", 2, B, 1) for B in (2, 6)]


@functools.lru_cache(maxsize=None)
def encode_batch(name, I, B):
    m = model_of(name)
    msg = messages(m, B, seed_of(name, I, B))
    if m.family == BCH:
        msg &= 1
    return msg, m.encode(msg).astype(symbol_type(m))


@functools.lru_cache(maxsize=None)
def extract_batch(name, I, B):
    """arbitrary field elements, not codewords"""
    m = model_of(name)
    words = np.random.default_rng(seed_of(name, I, B, 1)).integers(0, 1 << m.q, (B, m.n)).astype(symbol_type(m))
    return words, m.extract(words).astype(symbol_type(m))


def interleaved_map(name, which, fn, I, route, src, want, what):
    code = handle_of(name)
    assert code.interleaved_map_route(which, I) == route
    map_check(code, fn, interleave(src, I), interleave(want, I), what, tail=(I,))


@pytest.mark.parametrize("name,I,B,route", ENCODE_CASES)
def test_encode(name, I, B, route):
    interleaved_map(name, 0, lib().cc_encode_interleaved_batch_dev, I, route, *encode_batch(name, I, B),
                    ("interleaved encode", name, I, B))


@pytest.mark.parametrize("name,I,B,route", WIDE_ENCODE_CASES)
def test_encode_16_bit_symbols(name, I, B, route):
    interleaved_map(name, 0, lib().cc_encode_interleaved_batch_u16_dev, I, route, *encode_batch(name, I, B),
                    ("interleaved u16 encode", name, I, B))


@pytest.mark.parametrize("name,I,B,route", EXTRACT_CASES)
def test_extract(name, I, B, route):
    interleaved_map(name, 1, lib().cc_extract_interleaved_batch_dev, I, route, *extract_batch(name, I, B),
                    ("interleaved extract", name, I, B))


@pytest.mark.parametrize("name,I,B,route", WIDE_EXTRACT_CASES)
def test_extract_16_bit_symbols(name, I, B, route):
    interleaved_map(name, 1, lib().cc_extract_interleaved_batch_u16_dev, I, route, *extract_batch(name, I, B),
                    ("interleaved u16 extract", name, I, B))


# ------------------------------------------------ decode (host pointers) ------------------------------------------------
DECODE_CASES = [("RS(255,223)", 4, 12, 1)]


@pytest.mark.parametrize("name,I,B,route", DECODE_CASES)
def test_decode_is_correct_and_extract(name, I, B, route):
    """cc_decode_hard_interleaved_batch: words absent and present"""
    code = handle_of(name)
    assert code.interleaved_route(B, I) == route
    case, m = correct_batch(name, I, B, False), model_of(name)

    def call(p):
        return lib().cc_decode_hard_interleaved_batch(code._h, p["in"], None, None, p["msg"], p["words"], p["nerr"],
                                                      p["status"], B, I)
    outputs = {"msg": (np.uint8, B * m.l), "words": (np.uint8, B * m.n), "nerr": (np.int32, B), "status": (np.int32, B)}
    expected = {"msg": interleave(m.extract(case["out"]), I), "words": interleave(case["out"], I), "nerr": case["nerr"],
                "status": case["status"]}
    check_call(call, {"in": interleave(case["rx"], I)}, outputs, expected, optional=("words",), device="cpu",
               what=("interleaved decode", name, I))
