"""GPU tests of the Monte-Carlo route on packed words (mc_packed.hip): cc_bsc_packed_channel_dev against
the numpy channel model of tests/test_discrete_host.py bit for bit, cc_mc_run_bsc_packed_dev against the byte route
(q <= 8, every counter) and against a host count over the model's flips (q > 8: frames of weight <= t decode to the word
sent, the bounded-distance guarantee; the others go through the 16-bit oracle).  Counters must not depend on chunking,
sharding or the stream.

Shapes, the smallest where the kernels can go wrong (P = bytes per packed word):
    BCH(15,7)                 P = 2     P < 4: no whole dword in a frame
    BCH(63,45)                P = 8     1 pad bit
    BCH(255,231)              P = 32
    q = 9, t = 3, n = 511     P = 64    1 pad bit
    q = 10, t = 4, N = 203    P = 26    odd pitch in dwords, 5 pad bits
    q = 13, t = 8, N = 4200   P = 525   odd pitch, more dwords than a wavefront has lanes
    q = 14, t = 12, N = 3240  P = 405
    q = 14, t = 12, N = 16383 P = 2048  eight dwords per lane (at most 64 frames)"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import shortened_model as S
from checkers import BCH, BM, PGZ, WideOracle
from test_discrete_host import MASK, bch_message_bits, channel, philox4x32_10, thresholds
from test_gpu_packed import make, pad_bits

import channelcoding_amd as cc
from channelcoding_amd import capi
from channelcoding_amd.montecarlo import DiscreteBackend, PackedBscBackend, discrete_simulation

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# (q, t, N, polynomial)
SHORT = [(4, 2, None, None), (6, 3, None, None), (8, 3, None, None)]
LONG = [(9, 3, None, 0x211), (10, 4, 203, 0x409), (13, 8, 4200, 0x201B), (14, 12, 3240, 0x402B)]
FULL14 = (14, 12, None, 0x402B)
SEED, FIRST = 0x1234567890AB, (1 << 33) + 5
# channel probabilities at which frames within t and frames beyond t both occur: about t / (2 n) .. t / n
P_MC = {4: 0.05, 6: 0.02, 8: 0.004, 9: 0.004, 10: 0.012, 13: 0.0012, 14: 0.0025}


def in_child(call, **env):
    """runs test_gpu_packed_mc.<call> in a fresh process with the given environment (the switches are read once)"""
    script = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
              "import test_gpu_packed_mc as T\n"
              "T.%s\n"
              "print('CHILD OK')\n" % (HERE, os.path.dirname(HERE), call))
    out = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "CHILD OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


def sym(code):
    return np.uint16 if code.wide else np.uint8


def flips_model(p, seed, first, frames, n):
    """the channel of test_discrete_host.channel for the BSC, one Philox call per four bits instead of one per bit:
    bit j of frame gf flips iff word (j & 3) of counter (gf_lo, gf_hi, j >> 2, 2) < llround(p 2^32)"""
    gf = np.uint64(first) + np.arange(frames, dtype=np.uint64)[:, None]
    c2 = np.arange((n + 3) // 4, dtype=np.uint64)[None, :]
    w = philox4x32_10(gf & MASK, gf >> np.uint64(32), c2, 2, seed & 0xFFFFFFFF, seed >> 32)
    u = np.stack(w, axis=-1).reshape(frames, -1)[:, :n]
    return (u < np.uint64(thresholds(p, 0.0)[1])).astype(np.uint8)


def message_model(seed, first, frames, l):
    """bch_message_bits with one Philox call per 128 bits instead of one per bit: bit j of the message is bit (j & 31) of
    word ((j >> 5) & 3) of counter (gf_lo, gf_hi, j >> 7, 1)"""
    gf = np.uint64(first) + np.arange(frames, dtype=np.uint64)[:, None]
    c2 = np.arange((l + 127) // 128, dtype=np.uint64)[None, :]
    w = philox4x32_10(gf & MASK, gf >> np.uint64(32), c2, 1, seed & 0xFFFFFFFF, seed >> 32)
    words = np.ascontiguousarray(np.stack(w, axis=-1).reshape(frames, -1).astype("<u4"))
    return np.unpackbits(words.view(np.uint8), axis=-1, bitorder="little")[:, :l]


@functools.lru_cache(maxsize=None)
def sent_model(q, t, N, poly, seed, first, frames):
    """the words sent with random codewords: the model's message bits through the device's byte / _u16 encoder"""
    code = make(q, t, N, "BM", poly)
    words = np.asarray(code.encode_batch(message_model(seed, first, frames, code.l).astype(sym(code))))
    words.setflags(write=False)
    return words


def mc(code, p, seed, first, frames, random_cw):
    return PackedBscBackend(code, random_cw).run(p, seed, first, frames).cpu().numpy()


def untouched(counters):
    return counters[capi.MC_ITER_SUM] == 0 and counters[capi.MC_CHANNEL_ERASURES] == 0 and \
        not counters[capi.MC_ITER_HIST:].any()


def test_the_fast_model_is_the_model():
    for p in (0.0, 0.03, 1.0):
        _, erased, wrong = channel(p, 0.0, SEED, FIRST, 37, 203, 2)
        assert not erased.any() and np.array_equal(flips_model(p, SEED, FIRST, 37, 203), wrong.astype(np.uint8))
    for l in (7, 128, 231, 300):
        assert np.array_equal(message_model(SEED, FIRST, 9, l), bch_message_bits(SEED, FIRST, 9, l))


# ---------------- 1. the channel, bit for bit ----------------
@pytest.mark.parametrize("random_cw", [False, True])
@pytest.mark.parametrize("q,t,N,poly", SHORT + LONG + [FULL14])
def test_channel_equals_the_numpy_model(q, t, N, poly, random_cw):
    code = make(q, t, N, "BM", poly)
    frames = 63 if (q, N) == (14, None) else 301
    P = code.packed_bytes
    assert P == (code.n + 7) // 8
    sent = sent_model(q, t, N, poly, SEED, FIRST, frames) if random_cw else np.zeros((frames, code.n), sym(code))
    if random_cw:  # the encoder's words are the model's: the oracle on the first frames
        model = WideOracle(BCH, q, t, poly or 0)
        model = S.Shortened(model, N) if N else model
        msg = bch_message_bits(SEED, FIRST, 4, code.l).astype(np.uint16)
        assert np.array_equal(model.encode(msg), sent[:4])
    for p in (0.0, 0.004, 0.5, 1.0):
        got = cc.bsc_packed_channel(code, p, SEED, FIRST, frames, random_cw)
        recv, d_sent = got if random_cw else (got, None)
        assert recv.shape == (frames, P) and recv.dtype == torch.uint8
        flips = flips_model(p, SEED, FIRST, frames, code.n)
        if p in (0.0, 1.0):
            assert (flips == int(p)).all()
        want = sent ^ flips.astype(sent.dtype)
        assert np.array_equal(recv.cpu().numpy(), cc.pack_bits(want)), p  # (pack_bits writes the pad bits as 0)
        assert not pad_bits(recv.cpu().numpy(), code.n).any()
        if random_cw:
            assert np.array_equal(d_sent.cpu().numpy(), cc.pack_bits(sent)), p
    # d_sent with the all-zero word is cleared; NULL d_sent with random codewords: the workspace holds the words
    lib = capi.lib()
    for rnd in (0, 1):
        a = torch.full((frames, P), 0xA5, dtype=torch.uint8, device="cuda")
        b = torch.full((frames, P), 0xA5, dtype=torch.uint8, device="cuda")
        capi.check(lib.cc_bsc_packed_channel_dev(code._h, 0.004, SEED, FIRST, frames, rnd, a.data_ptr(),
                                                 None if rnd else b.data_ptr(), None), "cc_bsc_packed_channel_dev")
        torch.cuda.synchronize()
        flips = flips_model(0.004, SEED, FIRST, frames, code.n)
        base = sent_model(q, t, N, poly, SEED, FIRST, frames) if rnd else np.zeros((frames, code.n), sym(code))
        assert np.array_equal(a.cpu().numpy(), cc.pack_bits(base ^ flips.astype(base.dtype)))
        assert rnd or not b.any().item()


# ---------------- 2. q <= 8: the byte route's channel and counters ----------------
def byte_route_equality(sizes, routes=None):
    for q, t, N, poly in SHORT:
        for tag in ("BM", "PGZ", "EUKLID"):
            code = make(q, t, N, tag, poly)
            for frames in sizes:
                if routes and q == 8:
                    assert code.packed_route(frames) == routes[frames], (tag, frames)
                for random_cw in (False, True):
                    p, first = P_MC[q], FIRST + 1000 * frames
                    want_ch = code.discrete_channel(p, 0.0, SEED, first, frames, random_cw)
                    got = cc.bsc_packed_channel(code, p, SEED, first, frames, random_cw)
                    recv, sent = got if random_cw else (got, None)
                    assert torch.equal(cc.unpack_bits(recv, code.n), want_ch["recv"])
                    if random_cw:
                        assert torch.equal(cc.unpack_bits(sent, code.n), want_ch["sent"])
                    want = DiscreteBackend(code, "bsc", random_cw).run(p, SEED, first, frames).cpu().numpy()
                    got = mc(code, p, SEED, first, frames, random_cw)
                    assert np.array_equal(got, want), (q, tag, frames, random_cw, got[:8], want[:8])
                    assert got[capi.MC_FRAMES] == frames and untouched(got)
                    if frames >= 4096:  # the point is inside the waterfall: both classes of frames occur
                        assert 0 < got[capi.MC_WORD_ERRORS] < frames // 2, got[:8]


def test_equal_to_the_byte_route_on_the_plane_chain():
    # (the suite runs with CC_AMD_PLANES_MIN_WORK=0: GF(2^8) calls of every size take the plane chain on packed words)
    byte_route_equality((4096, 100), {4096: 1, 100: 1})


# ---------------- 3. q > 8: counters against a host count ----------------
def host_count(q, t, N, poly, tag, p, seed, first, frames, random_cw):
    """counters from the model's flips: weight <= t decodes to the word sent, the others through the oracle"""
    model = WideOracle(BCH, q, t, poly)
    model = S.Shortened(model, N) if N else model
    n = model.n
    flips = flips_model(p, seed, first, frames, n).astype(np.uint16)
    sent = sent_model(q, t, N, poly, seed, first, frames) if random_cw else np.zeros((frames, n), np.uint16)
    weight = flips.sum(axis=1)
    beyond = np.nonzero(weight > t)[0]
    # the condition belongs to the inputs: adjust p, not the assertion
    assert len(beyond) >= 1 and (weight <= t).sum() * 2 >= frames, (len(beyond), frames)
    c = np.zeros(capi.MC_NCOUNTERS, np.int64)
    c[capi.MC_FRAMES] = frames
    c[capi.MC_CHANNEL_BIT_ERRORS] = int(weight.sum())
    c[capi.MC_WORD_ERRORS] = len(beyond)
    rx = sent[beyond] ^ flips[beyond]
    out, _, st = model.correct_hard(BM if tag == "BM" else PGZ, rx)[:3]
    out = np.where((st == 0)[:, None], out, rx)  # a failed frame counts its output, the received word
    wrong = (out ^ sent[beyond]).sum(axis=1)
    assert (wrong > 0).all()  # beyond t no bounded-distance decoder returns the word sent
    c[capi.MC_BIT_ERRORS] = int(wrong.sum())
    c[capi.MC_FAILURES] = int((st != 0).sum())
    c[capi.MC_UNDETECTED] = int((st == 0).sum())
    return c


@pytest.mark.parametrize("q,t,N,poly", LONG)
def test_long_codes_equal_a_host_count(q, t, N, poly):
    for tag, frames, route, random_cw in (("BM", 2048, 1, False), ("PGZ", 300, 0, True)):
        code = make(q, t, N, tag, poly)
        assert code.packed_route(frames) == route
        first = FIRST + frames
        got = mc(code, P_MC[q], SEED, first, frames, random_cw)
        want = host_count(q, t, N, poly, tag, P_MC[q], SEED, first, frames, random_cw)
        assert np.array_equal(got, want), (tag, frames, got[:8], want[:8])


def test_full_length_gf_2_14_equals_a_host_count():
    q, t, N, poly = FULL14
    code = make(q, t, N, "BM", poly)
    got = mc(code, 0.0006, SEED, FIRST, 64, True)
    want = host_count(q, t, N, poly, "BM", 0.0006, SEED, FIRST, 64, True)
    assert np.array_equal(got, want), (got[:8], want[:8])


# ---------------- 4. additivity and chunking ----------------
ADDITIVE = [(8, 3, None, None, 3000, 1313), (9, 3, None, 0x211, 1000, 1313), (10, 4, 203, 0x409, 7, 2222)]
# three ragged chunks at CC_AMD_PACKED_MC_CHUNK_MB=1: 1 MiB / P frames per chunk (32768, 1997, 512), twice that and a rest
CHUNKED = [(8, 3, None, None, 2 * 32768 + 777), (13, 8, 4200, 0x201B, 2 * 1997 + 500), FULL14 + (2 * 512 + 9,)]


@pytest.mark.parametrize("q,t,N,poly,A,B", ADDITIVE)
def test_counters_add_over_frame_ranges(q, t, N, poly, A, B):
    code = make(q, t, N, "BM", poly)
    for random_cw in (False, True):
        whole = mc(code, P_MC[q], SEED, FIRST, A + B, random_cw)
        parts = mc(code, P_MC[q], SEED, FIRST, A, random_cw) + mc(code, P_MC[q], SEED, FIRST + A, B, random_cw)
        assert np.array_equal(whole, parts) and whole[capi.MC_FRAMES] == A + B and whole[capi.MC_WORD_ERRORS] > 0


def chunked_counters(random_cw):
    return [mc(make(q, t, N, "BM", poly), 0.0006 if N is None and q == 14 else P_MC[q], SEED, FIRST, frames,
               random_cw).tolist() for q, t, N, poly, frames in CHUNKED]


def child_checks(want):
    """in a process with CC_AMD_PACKED_MC_CHUNK_MB=1 and CC_AMD_PLANES_MIN_WORK=2000: three chunks give the counters of
    one, and 100 frames of a GF(2^8) code take the table route (4096 the plane chain) with the byte route's results"""
    assert chunked_counters(True) == want
    byte_route_equality((4096, 100), {4096: 1, 100: 0})


def test_chunks_do_not_show_and_the_table_route_in_a_child_process():
    want = chunked_counters(True)  # here: one chunk each (32 MiB of received words)
    assert all(c[capi.MC_WORD_ERRORS] > 0 for c in want)
    in_child("child_checks(%r)" % (want,), CC_AMD_PACKED_MC_CHUNK_MB="1", CC_AMD_PLANES_MIN_WORK="2000")


# ---------------- 5. streams: the workspace fence ----------------
@pytest.mark.parametrize("q,t,N,poly", [(8, 3, None, None), (14, 12, 3240, 0x402B)])
def test_side_stream_and_calls_back_to_back(q, t, N, poly):
    code = make(q, t, N, "BM", poly)
    p, frames = P_MC[q], 3000
    want = [mc(code, p, SEED, FIRST + k * frames, frames, True) for k in range(3)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    backend = PackedBscBackend(code, True)
    with torch.cuda.stream(side):  # two calls back to back on the side stream ...
        a = backend.run(p, SEED, FIRST, frames)
        b = backend.run(p, SEED, FIRST + frames, frames)
    c = backend.run(p, SEED, FIRST + 2 * frames, frames)  # ... and one on the default stream right behind them
    recv = cc.bsc_packed_channel(code, p, SEED, FIRST, frames, True)[0]  # (the channel call shares the workspace)
    side.synchronize()
    torch.cuda.synchronize()
    for got, ref in zip((a, b, c), want):
        assert np.array_equal(got.cpu().numpy(), ref)
    sent = sent_model(q, t, N, poly, SEED, FIRST, frames)
    flips = flips_model(p, SEED, FIRST, frames, code.n)
    assert np.array_equal(recv.cpu().numpy(), cc.pack_bits(sent ^ flips.astype(sent.dtype)))


# ---------------- 6. the harness end to end ----------------
def test_discrete_simulation_packed_end_to_end(tmp_path):
    code = make(9, 3, None, "BM", 0x211)
    sim = discrete_simulation(code, "bsc", points=[0.004], seed=SEED, log_dir=str(tmp_path), samples_per_point=3000,
                              packed=True)
    assert isinstance(sim.backend, PackedBscBackend) and sim.backend.random_codewords
    res = sim()
    want = mc(code, 0.004, SEED, 0, 3000, True)
    assert len(res) == 1 and res[0]["frames"] == 3000 and res[0]["p_error"] == 0.004
    assert res[0]["word_errors"] == want[capi.MC_WORD_ERRORS] > 0
    assert res[0]["bit_errors"] == want[capi.MC_BIT_ERRORS]
    assert res[0]["channel_bit_errors"] == want[capi.MC_CHANNEL_BIT_ERRORS] and res[0]["channel_erasures"] == 0
    assert res[0]["wer"] == want[capi.MC_WORD_ERRORS] / 3000
    lines = (tmp_path / (code.to_string() + ".bsc.log")).read_text().splitlines()
    assert lines[0] == "%7s %21s" % ("p", "wer") and lines[1] == "%7s %s" % ("0.004", "%16.15e" % res[0]["wer"])
    with pytest.raises(ValueError, match="packed"):
        discrete_simulation(code, "bec", packed=True)
