"""GPU tests of the native packed route of the 16-bit handles (packed_long.hip): binary BCH codes over
GF(2^9) .. GF(2^15), BM and PGZ tags, t <= 31, no erasures, calls of at least CC_AMD_PACKED_LONG_MIN_FRAMES frames.
For every frame out, nerr and status equal what the _u16 call gives for the unpacked words (the generic route's
definition) and what the 16-bit oracle gives; plus truths that need no reference: placed errors come back corrected, the
bounded-distance guarantee, H out^T = 0, untouched bytes around the words.  No frame is excluded from any comparison."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import shortened_model as S
from checkers import BCH, BM, PGZ, WideOracle
from test_gpu_packed import check_equal, make, received

import channelcoding_amd as cc
from channelcoding_amd import capi

pytestmark = pytest.mark.gpu

DEFAULT_MIN_FRAMES = 1024  # packed_long.hip: CC_AMD_PACKED_LONG_MIN_FRAMES
# (q, t, N, polynomial): polynomials of test_gpu_wide_model.POLY, 0x402B for the DVB-S2 field.
#   (9, 3)          P = 64, n % 32 = 31
#   (14, 12, 3000)  P = 375: odd pitch, most frames start on an odd byte; shortened
#   (13, 31, 1000)  the lane limit t = 31; 403 parity bits
#   (15, 2)         the largest tables, 16-bit positions (B <= 65 where the frames are drawn by sorting)
#   (11, 4, 70)     a frame shorter than one pass of 64 lanes x 32 bits
CODES = [(9, 3, None, 0x211), (10, 2, None, 0x409), (14, 12, 3000, 0x402B), (13, 31, 1000, 0x201B), (15, 2, None, 0x8003),
         (11, 4, 70, 0x805)]
SIZES = (1, 3, 4, 5, 63, 64, 65, 257, 1031)
HERE = os.path.dirname(os.path.abspath(__file__))


def in_child(call, **env):
    """runs test_gpu_packed_long.<call> in a fresh process with the given environment (the switches are read once)"""
    script = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
              "import test_gpu_packed_long as T\n"
              "T.%s\n"
              "print('CHILD OK')\n" % (HERE, os.path.dirname(HERE), call))
    out = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "CHILD OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


def flipped(code, rng, B, emin, emax, distinct=64):
    """codewords (`distinct` random ones, repeated) with emin .. emax bit errors per frame at random distinct positions,
    without sorting n numbers per frame: (sent, received, error counts)"""
    cw = code.encode_batch(rng.integers(0, 2, (min(B, distinct), code.l)).astype(np.uint16))
    cw = np.tile(cw, ((B + len(cw) - 1) // len(cw), 1))[:B]
    ne = rng.integers(emin, emax + 1, B)
    rx = cw.copy()
    if emax:
        pos = rng.integers(0, code.n, (B, emax))
        while True:
            srt = np.sort(pos, axis=1)
            bad = (srt[:, 1:] == srt[:, :-1]).any(axis=1)
            if not bad.any():
                break
            pos[bad] = rng.integers(0, code.n, (int(bad.sum()), emax))
        for j in range(emax):
            rows = np.nonzero(ne > j)[0]
            rx[rows, pos[rows, j]] ^= 1
    assert ((cw ^ rx).sum(axis=1) == ne).all()
    return cw, rx, ne


# ---------------- 1. routing ----------------
def routes_all_generic():
    for q, t, N, poly in CODES + [(10, 32, None, 0x409)]:
        for tag in ("BM", "PGZ", "EUKLID"):
            if (t, tag) == (32, "EUKLID"):
                continue  # refused (test_gpu_packed.test_refusals_of_the_16_bit_route_stay)
            code = make(q, t, N, tag, poly)
            for B in (1, 700, DEFAULT_MIN_FRAMES, 4096, 1 << 16):
                assert code.packed_route(B) == 0, (q, t, N, tag, B)


def test_routing():
    for q, t, N, poly in CODES:
        for tag in ("BM", "PGZ"):
            code = make(q, t, N, tag, poly)
            assert code.packed_route(DEFAULT_MIN_FRAMES) == 1 and code.packed_route(4096) == 1, (q, t, N, tag)
            assert code.packed_route(700) == 0 and code.packed_route(DEFAULT_MIN_FRAMES - 1) == 0
        euklid = make(q, t, N, "EUKLID", poly)
        assert [euklid.packed_route(B) for B in (700, DEFAULT_MIN_FRAMES, 4096)] == [0, 0, 0]
    for tag in ("BM", "PGZ"):  # t = 32: the locator's coefficient 64 has no lane
        code = make(10, 32, None, tag, 0x409)
        assert [code.packed_route(B) for B in (1, 700, DEFAULT_MIN_FRAMES, 4096, 1 << 16)] == [0] * 5
    assert make(8, 3).packed_route(4096) == 1  # (the GF(2^8) route as it was)
    in_child("routes_all_generic()", CC_AMD_PACKED_NATIVE="0")


# ---------------- 2. equality with the 16-bit call and the oracle at layout boundaries ----------------
def equality(q, t, N, poly):
    model = WideOracle(BCH, q, t, poly)
    model = S.Shortened(model, N) if N else model
    for tag, alg in (("BM", BM), ("PGZ", PGZ)):
        code = make(q, t, N, tag, poly)
        rng = np.random.default_rng(1000 * q + t + len(tag))
        seen = {"corrected": 0, "clean": 0, "failed": 0, "locator": 0}
        for B in SIZES:
            if q == 15 and B > 65:
                continue
            assert code.packed_route(B) == 1, (tag, B)
            # (1031 frames of a shortened code: t + 1 .. t + 3 errors, locators with a root at a position >= N)
            _, rx, _ = received(code, rng, B, t + 3, t + 1 if (N and B == 1031) else 0)
            want = check_equal(code, rx, dirty_pad=True)
            seen["corrected"] += int(((want["status"] == 0) & (want["nerr"] > 0)).sum())
            seen["clean"] += int(((want["status"] == 0) & (want["nerr"] == 0)).sum())
            seen["failed"] += int((want["status"] != 0).sum())
            seen["locator"] += int((want["status"] == capi.FRAME_LOCATOR).sum())
            if B <= 257:
                m_out, m_nerr, m_st = model.correct_hard(alg, rx)[:3]
                assert np.array_equal(want["status"] == 0, m_st == 0)
                assert np.array_equal(want["out"], np.where((m_st == 0)[:, None], m_out, rx))
                assert np.array_equal(want["nerr"], np.where(m_st == 0, m_nerr, -1))
                if alg == BM:
                    assert np.array_equal(want["status"], S.native_status(m_st, want["status"]) if N else m_st)
        assert seen["corrected"] > 0 and seen["clean"] > 0 and seen["failed"] > 0, (tag, seen)
        if N:
            assert seen["locator"] > 0, (tag, seen)


@pytest.mark.parametrize("q,t,N,poly", CODES)
def test_equal_to_the_16_bit_call_at_layout_boundaries(q, t, N, poly):
    in_child("equality(%d, %d, %r, %d)" % (q, t, N, poly), CC_AMD_PACKED_LONG_MIN_FRAMES="1")


# ---------------- 3. placed errors: two roots in one byte or dword, the first and the last positions ----------------
@pytest.mark.parametrize("tag", ["BM", "PGZ"])
@pytest.mark.parametrize("q,t,N,poly", [(9, 3, None, 0x211), (14, 12, 3000, 0x402B)])
def test_placed_errors(q, t, N, poly, tag):
    """Needs no reference: a codeword with e <= t flipped bits comes back as the codeword, nerr = e, status 0."""
    code = make(q, t, N, tag, poly)
    n = code.n
    last = 8 * (code.packed_bytes - 1)  # first position of the last byte (7 bits of it used for n = 511)
    patterns = [[0], [n - 1], [31, 32], [n - 2, n - 1], [40, 42, 47], list(range(64, 64 + t)), [last, n - 1],
                [last + 1, last + 3, n - 1], [0, 7, 8, 31, 32, 63, 64, n - 1][:t], []]
    B = DEFAULT_MIN_FRAMES
    assert code.packed_route(B) == 1
    rng = np.random.default_rng(q + t)
    cw = code.encode_batch(rng.integers(0, 2, (B, code.l)).astype(np.uint16))
    rx = cw.copy()
    ne = np.zeros(B, np.int32)
    for f in range(B):
        pat = patterns[f % len(patterns)]
        assert len(set(pat)) == len(pat) <= t and max(pat, default=0) < n
        rx[f, pat] ^= 1
        ne[f] = len(pat)
    pk = cc.pack_bits(rx)
    if n % 8:
        pk[:, -1] |= (0xFF << (n % 8)) & 0xFF
    # host arrays: the route is decided for the B frames of the call (every chunk then runs the native kernel), so
    # packed_route(B) above describes this call as well as the device call below
    res = code.correct_batch(pk, packed=True)
    assert not res["status"].any() and np.array_equal(res["nerr"], ne)
    assert np.array_equal(res["out"], cc.pack_bits(cw))
    dev = torch.from_numpy(pk).cuda()
    res = code.correct_batch(dev, packed=True, out=dev)  # in place
    assert not res["status"].any().item() and np.array_equal(res["nerr"].cpu().numpy(), ne)
    assert np.array_equal(dev.cpu().numpy(), cc.pack_bits(cw))


def test_locators_beyond_the_running_log_search():
    """The root search keeps running logs for locators up to degree 32; longer ones (BM tag only) go by Horner's rule.
    Reached on purpose: a word of the t = 30 code plus w <= 12 errors has the 60 syndromes of a w-error pattern and a
    61st that does not fit, so Berlekamp-Massey on the 62 syndromes of the t = 31 code jumps to L = 61 - w >= 49 there.
    The oracle's locator confirms the degree; every frame is compared with the 16-bit call and with the oracle."""
    q, N, poly = 13, 1000, 0x201B
    inner = make(q, 30, N, "BM", poly)
    assert inner.k < make(q, 31, N, "BM", poly).k
    B = DEFAULT_MIN_FRAMES
    rng = np.random.default_rng(31)
    _, rx, _ = flipped(inner, rng, B, 0, 12)
    mother = WideOracle(BCH, q, 31, poly)
    model = S.Shortened(mother, N)
    degs = []
    for f in range(64):
        st, sig, _ = mother.locator(BM, mother.syndromes(S.pad(rx[f], mother.n)))
        degs.append(int(np.nonzero(sig)[0].max()))
    assert min(degs) > 32, degs
    m_out, m_nerr, m_st = model.correct_hard(BM, rx[:64])[:3]
    for tag in ("BM", "PGZ"):
        code = make(q, 31, N, tag, poly)
        assert code.packed_route(B) == 1
        want = code.correct_batch(rx)
        got = code.correct_batch(torch.from_numpy(cc.pack_bits(rx)).cuda(), packed=True)
        assert np.array_equal(got["status"].cpu().numpy(), want["status"])
        assert np.array_equal(got["nerr"].cpu().numpy(), want["nerr"])
        assert np.array_equal(cc.unpack_bits(got["out"].cpu().numpy(), code.n, np.uint16), want["out"])
        assert (want["status"] != 0).any()
        if tag == "BM":
            assert np.array_equal(want["status"][:64] == 0, m_st == 0)
            assert np.array_equal(want["out"][:64], np.where((m_st == 0)[:, None], m_out, rx[:64]))
            assert np.array_equal(want["nerr"][:64], np.where(m_st == 0, m_nerr, -1))


# ---------------- 4. bounded-distance guarantee and parity ----------------
@pytest.mark.parametrize("tag", ["BM", "PGZ"])
@pytest.mark.parametrize("q,t,N,poly", CODES)
def test_bounded_distance_guarantee_and_parity(q, t, N, poly, tag):
    """Nothing here is compared with another decoder: exactly e <= t errors come back as the word sent with nerr = e, and
    every status-0 frame of a noisy batch is a codeword (H out^T = 0; for the long codes: re-encoding its message)."""
    code = make(q, t, N, tag, poly)
    B = DEFAULT_MIN_FRAMES
    assert code.packed_route(B) == 1
    rng = np.random.default_rng(50 * q + t)
    def decode(rx):  # device words: one call of B frames (a host call is cut into chunks of 32 MiB of symbols)
        res = code.correct_batch(torch.from_numpy(cc.pack_bits(rx)).cuda(), packed=True)
        return {k: v.cpu().numpy() for k, v in res.items()}

    for e in range(t + 1):
        cw, rx, ne = flipped(code, rng, B, e, e)
        res = decode(rx)
        assert (res["status"] == 0).all() and (res["nerr"] == e).all(), e
        assert np.array_equal(res["out"], cc.pack_bits(cw)), e
    _, rx, _ = flipped(code, rng, B, 0, t + 3)
    res = decode(rx)
    ok = res["status"] == 0
    assert ok.any() and (~ok).any()
    out = cc.unpack_bits(res["out"], code.n, np.uint16)
    assert np.array_equal(out[~ok], rx[~ok]) and (res["nerr"][~ok] == -1).all()
    if q <= 11:
        H = code.H().astype(np.int64)
        assert not ((out[ok].astype(np.int64) @ H.T) & 1).any()
    else:
        assert np.array_equal(code.encode_batch(code.extract_batch(out[ok])), out[ok])


# ---------------- 5. buffers: unaligned base, sentinels, side stream, in place, no nerr / status ----------------
@pytest.mark.parametrize("q,t,N,poly", [(9, 3, None, 0x211), (14, 12, 3000, 0x402B), (11, 4, 70, 0x805)])
def test_unaligned_buffers_in_place_on_a_side_stream(q, t, N, poly):
    code = make(q, t, N, "BM", poly)
    P, B = code.packed_bytes, DEFAULT_MIN_FRAMES + 3
    assert code.packed_route(B) == 1
    rng = np.random.default_rng(q)
    _, rx, _ = flipped(code, rng, B, 0, t + 3)
    want = code.correct_batch(rx)
    pk = cc.pack_bits(rx)
    if code.n % 8:
        pk[:, -1] |= (0xFF << (code.n % 8)) & 0xFF
    lib = capi.lib()
    for off in (1, 3):
        side = torch.cuda.Stream()
        big = torch.full((off + B * P + 29,), 0xA5, dtype=torch.uint8, device="cuda")
        words = big[off:off + B * P].view(B, P)
        assert words.data_ptr() % 4 == off and words.is_contiguous()
        words.copy_(torch.from_numpy(pk))
        bare = big.clone()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            res = code.correct_batch(words, packed=True, out=words)  # out is in
            # and the C call without nerr / status, on a copy of the same bytes
            rc = lib.cc_correct_hard_packed_batch_dev(code._h, C.c_void_p(bare.data_ptr() + off), None, None,
                                                      C.c_void_p(bare.data_ptr() + off), None, None, B,
                                                      C.c_void_p(side.cuda_stream))
        side.synchronize()
        assert rc == capi.OK and res["out"] is words
        assert np.array_equal(res["status"].cpu().numpy(), want["status"])
        assert np.array_equal(res["nerr"].cpu().numpy(), want["nerr"])
        for buf in (big, bare):
            host = buf.cpu().numpy()
            assert (host[:off] == 0xA5).all() and (host[off + B * P:] == 0xA5).all()
            assert np.array_equal(cc.unpack_bits(host[off:off + B * P].reshape(B, P), code.n, np.uint16), want["out"])
            assert np.array_equal(host[off:off + B * P].reshape(B, P), cc.pack_bits(want["out"]))  # pad bits written as 0
