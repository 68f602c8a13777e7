"""The buffer contract of the 16-bit symbol entry points (q = 9 .. 15, csrc/wide.hip) -- cc_encode_batch_u16_dev,
cc_extract_batch_u16_dev, cc_correct_hard_batch_u16_dev and its host form -- under the harness of tests/guarded_buffers.py:
every uint16_t buffer at 2 mod 4, exactly as long as the header says, between sentinel guards or inside poison, nerr and
status absent in turn, the erasure CSR present and absent, and out == in, which the header allows and the interleaved
contract relies on.

The expected arrays are those of checkers.WideOracle, the 16-bit build of the plain-C oracle (shortened_model.Shortened
over it for the shortened handle); every comparison is bit for bit.  The tables and builders need no device:
tests/test_buffer_cases_host.py checks every batch on the CPU."""
import functools

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import capi
import shortened_model as S
from checkers import BCH, BM, EUKLID, PGZ, RS, WideOracle
from guarded_buffers import check_call
from test_gpu_buffers import HARD_TAGS, TRIALS, corrupted, erased, hard_expected, lib, map_check, messages
from test_gpu_buffers_packed import status_rule, two_trial_frames

pytestmark = pytest.mark.gpu
WIDE = capi.HARD_ROUTE_WIDE

# name -> (family, q, t, modular polynomial, N, mu)
CODES = {
    "BCH(511,484)": (BCH, 9, 3, 0x211, None, 1),
    "RS(1023,1015)": (RS, 10, 4, 0x409, None, 1),
    "RS(1023,1015) mu=0": (RS, 10, 4, 0x409, None, 0),  # first root alpha^0: wide_correct_kernel<true>
    "RS(300,292)": (RS, 10, 4, 0x409, 300, 1),  # shortened, 300 = 4 * 64 + 44: the last pass of the wavefront is ragged
}
SIZES = (1, 5)  # five: the first frame of a second workgroup of four wavefronts


@functools.lru_cache(maxsize=None)
def model_of(name):
    family, q, t, poly, N, mu = CODES[name]
    m = WideOracle(family, q, t, poly, mu, 1)
    return S.Shortened(m, N) if N else m


def handle_of(name, alg=BM):
    family, q, t, poly, N, mu = CODES[name]
    kw = dict(mu=mu, step=1) if family == RS else {}
    code = (cc.primitive_bch if family == BCH else cc.rs)(q, cc.errors(t), HARD_TAGS[alg](), modular_polynomial=poly, n=N, **kw)
    m = model_of(name)
    assert code.wide and (code.n, code.l) == (m.n, m.l), name
    return code


def seed_of(name, *more):
    return 1000 * list(CODES).index(name) + sum((i + 3) * int(v) for i, v in enumerate(more))


# ------------------------------------------------ encode, extract ------------------------------------------------
MAP_CASES = [(name, B) for name in CODES for B in SIZES]


@functools.lru_cache(maxsize=None)
def encode_batch(name, B):
    m = model_of(name)
    msg = messages(m, B, seed_of(name, B))
    if m.family == BCH:
        msg &= 1
    return msg, m.encode(msg).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def extract_batch(name, B):
    """arbitrary field elements, not codewords"""
    m = model_of(name)
    words = np.random.default_rng(seed_of(name, B, 1)).integers(0, 1 << m.q, (B, m.n)).astype(np.uint16)
    return words, m.extract(words).astype(np.uint16)


@pytest.mark.parametrize("name,B", MAP_CASES)
def test_encode(name, B):
    code = handle_of(name)
    msg, want = encode_batch(name, B)
    map_check(code, lib().cc_encode_batch_u16_dev, msg, want, ("u16 encode", name, B))


@pytest.mark.parametrize("name,B", MAP_CASES)
def test_extract(name, B):
    code = handle_of(name)
    words, want = extract_batch(name, B)
    map_check(code, lib().cc_extract_batch_u16_dev, words, want, ("u16 extract", name, B))


# ------------------------------------------------ correct ------------------------------------------------
# (code, tag, B, erasure list?, out == in?)
CORRECT_CASES = ([(name, alg, B, False, False) for name in CODES for alg in (BM, PGZ, EUKLID) for B in SIZES] +
                 [(name, alg, 5, True, False) for name in CODES for alg in (BM, EUKLID)] +
                 [("BCH(511,484)", PGZ, 5, True, False)] +  # launch_wide_pgz_erasures: the two trials
                 [(name, BM, 5, False, True) for name in CODES] +
                 [("RS(1023,1015)", EUKLID, 5, True, True), ("BCH(511,484)", PGZ, 5, True, True)])
HOST_CASES = [("BCH(511,484)", BM, 5, False, False), ("RS(1023,1015)", BM, 5, True, False)]


@functools.lru_cache(maxsize=None)
def correct_batch(name, alg, B, with_erasures):
    """a dict: rx, per and csr (None without erasures), out / nerr / status (the oracle's)"""
    m = model_of(name)
    seed = seed_of(name, alg, B, with_erasures)
    per = csr = None
    if not with_erasures:
        rx = corrupted(m, B, seed)
    elif alg == PGZ:
        rx, per, csr = two_trial_frames(m, B, seed)
    else:
        rx, per, csr = erased(m, B, seed, 4)
    out, nerr, st = hard_expected(m, alg, rx, per)
    return dict(rx=rx, per=per, csr=csr, out=out, nerr=nerr, status=st)


def wide_correct(code, name, alg, case, what, in_place=False, device="cuda"):
    B = case["rx"].shape[0]
    inputs = {"in": case["rx"]}
    if case["csr"] is not None:
        inputs.update(erasures=case["csr"][0], offsets=case["csr"][1])
        assert case["csr"][1].size == B + 1 and case["csr"][0].size == case["csr"][1][-1] > 0

    def call(p):
        args = (code._h, p["in"], p.get("erasures"), p.get("offsets"), p["out"], p["nerr"], p["status"], B)
        if device == "cpu":
            return lib().cc_correct_hard_batch_u16(*args)
        return lib().cc_correct_hard_batch_u16_dev(*args, p["stream"])
    outputs = {"out": (np.uint16, case["out"].size), "nerr": (np.int32, B), "status": (np.int32, B)}
    two_trials = alg == PGZ and case["csr"] is not None
    expected = {"out": case["out"], "nerr": case["nerr"],
                "status": status_rule(case["status"], alg, CODES[name][4] is not None, True if two_trials else None)}
    check_call(call, inputs, outputs, expected, optional=("nerr", "status"), what=what, device=device,
               in_place={"out": "in"} if in_place else None)


@pytest.mark.parametrize("name,alg,B,with_erasures,in_place", CORRECT_CASES)
def test_correct(name, alg, B, with_erasures, in_place):
    code = handle_of(name, alg)
    assert code.hard_route(B, with_erasures) == (TRIALS if alg == PGZ and with_erasures else WIDE)
    wide_correct(code, name, alg, correct_batch(name, alg, B, with_erasures), (name, alg, B, with_erasures, in_place),
                 in_place=in_place)


@pytest.mark.parametrize("name,alg,B,with_erasures,in_place", HOST_CASES)
def test_correct_on_host_memory(name, alg, B, with_erasures, in_place):
    """cc_correct_hard_batch_u16: the staged call, host buffers under the same harness"""
    code = handle_of(name, alg)
    assert code.hard_route(B, with_erasures) == WIDE
    wide_correct(code, name, alg, correct_batch(name, alg, B, with_erasures), (name, alg, B, with_erasures, "host"),
                 device="cpu")
