"""The buffer contract of the packed-bit entry points -- cc_pack_bits_dev, cc_unpack_bits_dev, cc_encode_packed_batch_dev,
cc_extract_packed_batch_dev, cc_correct_hard_packed_batch_dev, cc_decode_hard_packed_batch -- under the harness of
tests/guarded_buffers.py: B * P bytes and not one more at an odd address, sentinel guards round every output, poison
round every input, every optional output absent in turn, two poisons.  These are the kernels that move whole unaligned
dwords over caller memory and finish a frame byte by byte (packed_words.hpp: load_word / store_word, packed.hip: load_at),
at pitches P = ceil(n / 8) that are odd for shortened codes.

The expected arrays are the plain-C oracle's (checkers.Oracle, checkers.WideOracle, shortened_model.Shortened over them)
packed with numpy.packbits(..., bitorder="little"); every comparison is bit for bit and no frame is left out of one.  The
case tables and the batch builders below need no device: tests/test_buffer_cases_host.py checks on the CPU that every batch
holds what makes it worth running."""
import functools

import numpy as np
import pytest

import channelcoding_amd as cc
import shortened_model as S
from checkers import BCH, BM, PGZ, Oracle, WideOracle
from guarded_buffers import check_call
from test_gpu_buffers import HARD_TAGS, PLANES, TRIALS, erased, hard_expected, lib, status_check, symbol_type

pytestmark = pytest.mark.gpu

# name -> (q, t, N, modular polynomial, coding)
CODES = {
    "BCH(7,4)": (3, 1, None, None, 0),
    "BCH(15,7)": (4, 2, None, None, 0),
    "BCH(63,45)": (6, 3, None, None, 0),
    "BCH(63,45) c = a g": (6, 3, None, None, 1),
    "BCH(255,231)": (8, 3, None, None, 0),
    "BCH(100,76)": (8, 3, 100, None, 0),  # P = 13, 10 message bytes
    "BCH(255,215)": (8, 5, None, None, 0),  # 40 parity bits: beyond the packed encoder
    "BCH(511,484)": (9, 3, None, 0x211, 0),  # 27 parity bits, 61 message bytes
    "GF(2^11) t = 4 N = 70": (11, 4, 70, 0x805, 0),  # P = 9: a frame shorter than one pass of the wavefront
}
PERFECT = {"BCH(7,4)"}  # every word lies within distance t of a codeword: no frame of such a code fails


@functools.lru_cache(maxsize=None)
def model_of(name):
    q, t, N, poly, coding = CODES[name]
    m = Oracle(BCH, q, t, coding=coding) if q <= 8 else WideOracle(BCH, q, t, poly, coding=coding)
    return S.Shortened(m, N) if N else m


def handle_of(name, alg=BM):
    q, t, N, poly, coding = CODES[name]
    code = cc.primitive_bch(q, cc.errors(t), HARD_TAGS[alg](), coding="multiplication" if coding else "division", n=N,
                            modular_polynomial=poly)
    m = model_of(name)
    assert (code.n, code.l) == (m.n, m.l), name
    return code


def pack(bits):
    """(B, n) symbols 0 / 1 -> (B, ceil(n / 8)) bytes, position p in bit p & 7 of byte p >> 3, pad bits 0"""
    return np.packbits(np.ascontiguousarray(bits).astype(np.uint8), axis=1, bitorder="little")


def unpack(words, n):
    return np.unpackbits(np.ascontiguousarray(words), axis=1, bitorder="little")[:, :n]


def dirty(words, n, rng):
    """the same words with random pad bits (positions n .. 8 P - 1, ignored on input), at least one of them set"""
    words, free = words.copy(), (0xFF << (n % 8)) & 0xFF if n % 8 else 0
    if free:
        words[:, -1] |= rng.integers(0, 256, words.shape[0]).astype(np.uint8) & free
        words[0, -1] |= free
    return words


# ------------------------------------------------ pack, unpack ------------------------------------------------
LENGTHS = (1, 7, 8, 9, 31, 32, 33, 100, 255, 1000)  # P < 4, P odd, P a multiple of 4, whole dwords of symbols, the tail loop
BITS_CASES = [(width, n, B) for width in (1, 2) for n in LENGTHS for B in (1, 3)]


@functools.lru_cache(maxsize=None)
def pack_batch(width, n, B):
    """symbols with random high bits (only bit 0 counts) and the packed words numpy makes of their low bits"""
    rng = np.random.default_rng(100000 * width + 10 * n + B)
    sym = rng.integers(0, 1 << (8 * width), (B, n)).astype(np.uint8 if width == 1 else np.uint16)
    sym[0, 0] |= 0xFE
    return sym, pack(sym & 1)


@functools.lru_cache(maxsize=None)
def unpack_batch(width, n, B):
    """random packed words, pad bits included, and the symbols 0 / 1 numpy reads from them"""
    rng = np.random.default_rng(200000 * width + 10 * n + B)
    words = dirty(rng.integers(0, 256, (B, (n + 7) // 8)).astype(np.uint8), n, rng)
    return words, unpack(words, n).astype(np.uint8 if width == 1 else np.uint16)


@pytest.mark.parametrize("width,n,B", BITS_CASES)
def test_pack_bits(width, n, B):
    sym, want = pack_batch(width, n, B)

    def call(p):
        return lib().cc_pack_bits_dev(p["symbols"], width, n, p["packed"], B, p["stream"])
    check_call(call, {"symbols": sym}, {"packed": (np.uint8, want.size)}, {"packed": want}, what=("pack", width, n, B))


@pytest.mark.parametrize("width,n,B", BITS_CASES)
def test_unpack_bits(width, n, B):
    words, want = unpack_batch(width, n, B)

    def call(p):
        return lib().cc_unpack_bits_dev(p["packed"], n, p["symbols"], width, B, p["stream"])
    check_call(call, {"packed": words}, {"symbols": (want.dtype, want.size)}, {"symbols": want},
               what=("unpack", width, n, B))


# ------------------------------------------------ encode, extract ------------------------------------------------
# (code, route of cc_packed_map_route, B)
ENCODE_CASES = ([(name, 1, B) for name in ("BCH(7,4)", "BCH(15,7)", "BCH(63,45)", "BCH(255,231)", "BCH(100,76)") for B in (1, 5)] +
                [(name, 0, 5) for name in ("BCH(255,215)", "BCH(511,484)", "BCH(63,45) c = a g")])
EXTRACT_CASES = ([(name, 1, B) for name in ("BCH(63,45)", "BCH(255,231)", "BCH(100,76)", "BCH(511,484)") for B in (1, 5)] +
                 [("BCH(63,45) c = a g", 0, 5)])


@functools.lru_cache(maxsize=None)
def encode_batch(name, B):
    """packed messages (the first all zero, the second all one, pad bits dirty) and the packed words of the oracle"""
    m = model_of(name)
    rng = np.random.default_rng(31 * m.n + B)
    msg = rng.integers(0, 2, (B, m.l)).astype(symbol_type(m))
    msg[0] = 0
    if B >= 2:
        msg[1] = 1
    return dirty(pack(msg), m.l, rng), pack(m.encode(msg))


@functools.lru_cache(maxsize=None)
def extract_batch(name, B):
    """arbitrary packed words, pad bits included; their unpacked form; the packed messages the oracle extracts"""
    m = model_of(name)
    rng = np.random.default_rng(37 * m.n + B)
    words = dirty(rng.integers(0, 256, (B, (m.n + 7) // 8)).astype(np.uint8), m.n, rng)
    bits = unpack(words, m.n).astype(symbol_type(m))
    return words, bits, pack(m.extract(bits))


def packed_map(code, fn, src, want, what):
    B = src.shape[0]

    def call(p):
        return fn(code._h, p["src"], p["dst"], B, p["stream"])
    check_call(call, {"src": src}, {"dst": (np.uint8, want.size)}, {"dst": want}, what=what)


@pytest.mark.parametrize("name,route,B", ENCODE_CASES)
def test_encode(name, route, B):
    code = handle_of(name)
    assert code.packed_map_route(0) == route
    msg, want = encode_batch(name, B)
    assert msg.shape == (B, code.packed_message_bytes) and want.shape == (B, code.packed_bytes)
    packed_map(code, lib().cc_encode_packed_batch_dev, msg, want, ("packed encode", name, B))


@pytest.mark.parametrize("name,route,B", EXTRACT_CASES)
def test_extract(name, route, B):
    code = handle_of(name)
    assert code.packed_map_route(1) == route
    words, _, want = extract_batch(name, B)
    assert words.shape == (B, code.packed_bytes) and want.shape == (B, code.packed_message_bytes)
    packed_map(code, lib().cc_extract_packed_batch_dev, words, want, ("packed extract", name, B))


# ------------------------------------------------ correct ------------------------------------------------
def received(m, B, seed):
    """B codewords with 0 .. t + 2 bit errors each: the first frame clean (one error where it is the only frame, so that a
    call in place has something to change), the second t + 2 errors"""
    from test_gpu_algebraic import corrupt
    rng = np.random.default_rng(seed)
    cw = m.encode(rng.integers(0, 2, (B, m.l)).astype(symbol_type(m)))
    ne = rng.integers(0, m.t + 3, B)
    ne[0] = 0 if B >= 2 else 1
    if B >= 2:
        ne[1] = m.t + 2
    return np.stack([corrupt(rng, m, cw[f], int(ne[f])) for f in range(B)])


def two_trial_frames(m, B, seed):
    """words for the two-trial rule of the PGZ tag (bch.h:97-149), as test_hard_decoding_by_two_trials builds them: up to
    three bit errors anywhere, the erased positions keep what they held; no list for the first and the last frame, more
    than 2t positions for the second (CC_FRAME_ERASURES)"""
    from test_gpu_buffers import erasure_lists
    rng = np.random.default_rng(seed)
    rx = m.encode(rng.integers(0, 2, (B, m.l)).astype(symbol_type(m)))
    per, _, _ = erasure_lists(rng, B, m.n, 2 * m.t + 1)
    per[1] = sorted(rng.choice(m.n, 2 * m.t + 1, replace=False).tolist())
    pos = np.array([e for er in per for e in er], np.uint16)
    off = np.concatenate([[0], np.cumsum([len(er) for er in per])]).astype(np.uint32)
    for f in range(B):
        for p in rng.choice(m.n, int(rng.integers(0, 4)), replace=False):
            rx[f, p] ^= 1
    rx[1, per[1]] ^= 1  # a word that no trial brings back
    return rx, per, (pos, off)


# (code, tag, B, variant): "plain"; "dirty": pad bits set in the input; "in place": out == in; "erasures": with a CSR
NATIVE_CASES = [(name, BM, B, v) for name in ("BCH(255,231)", "BCH(100,76)") for B in (1, 31, 33, 65)
                for v in ("plain", "dirty", "in place")]
LONG_CASES = [(name, BM, 1025, v) for name in ("BCH(511,484)", "GF(2^11) t = 4 N = 70") for v in ("plain", "in place")]
GENERIC_CASES = [("BCH(15,7)", BM, 5, "plain"), ("BCH(63,45)", BM, 5, "plain"), ("BCH(255,231)", BM, 9, "erasures"),
                 ("BCH(255,231)", PGZ, 9, "erasures")]
CORRECT_CASES = NATIVE_CASES + LONG_CASES + GENERIC_CASES


@functools.lru_cache(maxsize=None)
def correct_batch(name, alg, B, variant):
    """a dict: rx (symbols), per and csr (erasures or None), words (the packed input), out / nerr / status (the oracle's, out
    packed)"""
    m = model_of(name)
    seed = 1000 * m.n + 10 * B + alg
    per = csr = None
    if variant != "erasures":
        rx = received(m, B, seed)
    elif alg == PGZ:
        rx, per, csr = two_trial_frames(m, B, seed)
    else:
        rx, per, csr = erased(m, B, seed, 4)
    out, nerr, st = hard_expected(m, alg, rx, per)
    words = pack(rx)
    if variant == "dirty":
        words = dirty(words, m.n, np.random.default_rng(seed + 1))
    return dict(rx=rx, per=per, csr=csr, words=words, out=pack(out), nerr=nerr, status=st)


def status_rule(st, alg, shortened, exact=None):
    """status_check of test_gpu_buffers.py: the exact class for the BM tag and the two-trial rule.  A shortened code has
    the one licence of shortened_model.native_status: a locator root at a position >= N fails the root count
    (CC_FRAME_LOCATOR) before the re-check that the padded full-length decode fails."""
    exact = alg == BM if exact is None else exact
    if not (exact and shortened):
        return status_check(st, exact)

    def check(view, label):
        got = view.cpu().numpy().view(np.int32)
        assert np.array_equal(got, S.native_status(st, got)), (label, got, st)
    return check


def packed_correct(code, alg, case, what, in_place=False, exact=None):
    B = case["words"].shape[0]
    inputs = {"in": case["words"]}
    if case["csr"] is not None:
        inputs.update(erasures=case["csr"][0], offsets=case["csr"][1])
        assert case["csr"][1].size == B + 1 and case["csr"][0].size == case["csr"][1][-1] > 0

    def call(p):
        return lib().cc_correct_hard_packed_batch_dev(code._h, p["in"], p.get("erasures"), p.get("offsets"), p["out"],
                                                      p["nerr"], p["status"], B, p["stream"])
    outputs = {"out": (np.uint8, case["out"].size), "nerr": (np.int32, B), "status": (np.int32, B)}
    expected = {"out": case["out"], "nerr": case["nerr"],
                "status": status_rule(case["status"], alg, CODES[what[0]][2] is not None, exact)}
    check_call(call, inputs, outputs, expected, optional=("nerr", "status"), what=what,
               in_place={"out": "in"} if in_place else None)


@pytest.mark.parametrize("name,alg,B,variant", NATIVE_CASES)
def test_correct_on_the_native_chain(name, alg, B, variant):
    """packed_syndrome_kernel / packed_fix_kernel (packed.hip), both sides of the 32-frame group and the 64-frame chunk"""
    code = handle_of(name, alg)
    assert code.packed_route(B) == 1 and not code.wide
    packed_correct(code, alg, correct_batch(name, alg, B, variant), (name, alg, B, variant), in_place=variant == "in place")


@pytest.mark.parametrize("name,alg,B,variant", LONG_CASES)
def test_correct_on_the_native_long_route(name, alg, B, variant):
    """packed_long.hip at the first call size above the default CC_AMD_PACKED_LONG_MIN_FRAMES"""
    code = handle_of(name, alg)
    assert code.wide and code.packed_route(B) == 1 and code.packed_route(B - 2) == 0
    packed_correct(code, alg, correct_batch(name, alg, B, variant), (name, alg, B, variant), in_place=variant == "in place")


@pytest.mark.parametrize("name,alg,B,variant", GENERIC_CASES)
def test_correct_on_the_generic_route(name, alg, B, variant):
    """unpack, the byte router, pack: codes the chain does not serve, and erasure lists (BM on the plane chain; the PGZ
    tag's two trials, where workspace stands in for an absent nerr / status)"""
    code = handle_of(name, alg)
    if variant == "erasures":
        assert code.hard_route(B, True) == (TRIALS if alg == PGZ else PLANES)
    else:
        assert code.packed_route(B) == 0
    packed_correct(code, alg, correct_batch(name, alg, B, variant), (name, alg, B, variant),
                   exact=True if alg == PGZ else None)


# ------------------------------------------------ decode (host pointers) ------------------------------------------------
DECODE_CASES = [("BCH(255,231)", 1, 33), ("BCH(63,45)", 0, 33)]


@functools.lru_cache(maxsize=None)
def decode_batch(name, B):
    m = model_of(name)
    rx = received(m, B, 77 * m.n + B)
    out, nerr, st = hard_expected(m, BM, rx)
    return dict(rx=rx, words=pack(rx), msg=pack(m.extract(out)), out=pack(out), nerr=nerr, status=st)


@pytest.mark.parametrize("name,route,B", DECODE_CASES)
def test_decode_is_correct_and_extract(name, route, B):
    """cc_decode_hard_packed_batch: words absent and present"""
    code = handle_of(name)
    assert code.packed_route(B) == route
    case = decode_batch(name, B)

    def call(p):
        return lib().cc_decode_hard_packed_batch(code._h, p["in"], None, None, p["msg"], p["words"], p["nerr"], p["status"], B)
    outputs = {"msg": (np.uint8, case["msg"].size), "words": (np.uint8, case["out"].size), "nerr": (np.int32, B),
               "status": (np.int32, B)}
    expected = {"msg": case["msg"], "words": case["out"], "nerr": case["nerr"], "status": case["status"]}
    check_call(call, {"in": case["words"]}, outputs, expected, optional=("words",), device="cpu", what=("packed decode", name))
