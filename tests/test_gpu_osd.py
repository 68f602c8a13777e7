"""GPU tests of ordered-statistics decoding: cc_correct_osd_batch(_dev) bit for bit against
tests/osd_model.py on out, nerr, status and metric at order 0, 1 and 2, on the codes at which the kernel's layout changes
(words per row, row slots per lane, dwords per column mask, l = 1); constructed frames (equal magnitudes, zeros,
denormals, near FLT_MAX, a noiseless codeword); a wavefront's second frame; monotony in the order; the buffer contract;
cc_mc_run_osd_dev against the model, its own shards and the composition of channel, decoder and count; and order 1
against hard decoding in word errors."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import capi
from channelcoding_amd.montecarlo import OsdBackend
import osd_model as M
from checkers import awgn_llr
from guarded_buffers import check_call

pytestmark = pytest.mark.gpu

# (q, t, N, frames the model decodes): the model enumerates 1 + l + l (l - 1) / 2 candidates per frame -- 30 629 for
# BCH(255,247) -- so the large codes get fewer model frames; the other frames of a batch are held to H and to the metric
CASES = [(3, 1, None, 67), (4, 3, None, 67), (4, 2, None, 67), (4, 1, None, 67), (5, 3, None, 67), (6, 3, None, 40),
         (6, 15, None, 67),   # BCH(63,7): k = 56, l = 7
         (7, 10, None, 24),   # BCH(127,64): k = 63 against l = 64
         (7, 3, None, 16), (8, 3, None, 10),
         (8, 1, None, 10),    # BCH(255,247): l = 247, the most pairs
         (8, 18, None, 12),   # BCH(255,131): 2t = 36 > 32
         (8, 63, None, 24),   # BCH(255,9): k = 246, four rows per lane
         (8, 3, 64, 24), (8, 3, 65, 24), (8, 3, 129, 16), (8, 3, 193, 10), (8, 3, 200, 10),
         (8, 3, 25, 67)]      # N = k + 1: l = 1, no pairs
IDS = ["bch%d-t%d%s" % (q, t, "" if N is None else "-N%d" % N) for q, t, N, _ in CASES]
FRAMES = 67
ORDERS = (0, 1, 2)


def make(q, t, N=None, tag=cc.berlekamp_massey_tag):
    return cc.primitive_bch(q, cc.errors(t), tag(), **({} if N is None else {"n": N}))


def quantised(rng, shape):
    """multiples of 0.5 with a few +-0.0: equal keys in every frame, equal metrics in many"""
    y = rng.choice(np.array([-1.5, -1.0, -0.5, 0.5, 0.5, 1.0, 1.0, 1.5, 1.5, 1.5], np.float32), shape)
    y[::3, 1] = np.float32(0.0)
    y[::4, shape[1] - 1] = np.float32(-0.0)
    y[1::5, 0] = np.float32(-0.0)
    return y.astype(np.float32)


@functools.lru_cache(maxsize=None)
def batches(q, t, N, modelled):
    """67 frames of one code -- AWGN at 3 dB and quantised ones alternating -- and the model's answers at every order for
    the first `modelled` of them, made once"""
    dec = M.decoder(q, t, N)
    rng = np.random.default_rng(3000 + 100 * q + t + (N or 0))
    words = dec.encode(rng.integers(0, 2, (FRAMES, dec.l)).astype(np.uint8))
    y = awgn_llr(rng, words, dec.l / dec.n, 3.0)
    y[1::2] = quantised(rng, (FRAMES, dec.n))[1::2]
    y = np.ascontiguousarray(y, np.float32)
    y.setflags(write=False)
    return dict(dec=dec, y=y, want=M.osd(dec, y[:modelled], M.MAX_ORDER), modelled=modelled)


def to_numpy(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def same(got, want, rows, what):
    for k in ("out", "nerr", "status"):
        assert np.array_equal(got[k][:rows], want[k][:rows]), (what, k)
    assert np.array_equal(got["metric"][:rows].view(np.uint32), want["metric"][:rows].view(np.uint32)), (what, "metric")


def holds_everywhere(code, y, got, what):
    """what needs no model: every out a codeword, metric and nerr those of the contract, status CC_FRAME_OK"""
    H = np.asarray(code.H(), np.int64)
    z = M.hard(y)
    assert not ((got["out"].astype(np.int64) @ H.T) % 2).any(), what
    assert np.array_equal(M.metric(y, z, got["out"]).view(np.uint32), got["metric"].view(np.uint32)), what
    assert np.array_equal((got["out"] != z).sum(axis=1), got["nerr"]) and (got["status"] == M.FRAME_OK).all(), what


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_equals_model(case):
    import torch
    q, t, N, modelled = case
    bt = batches(*case)
    code = make(q, t, N)
    assert capi.lib().cc_osd_frames_per_wavefront(code._h, 2) >= 1
    y = torch.from_numpy(bt["y"].copy()).cuda()
    for order in ORDERS:
        want = bt["want"][("order", order)]
        for B in (1, 2, FRAMES):
            got = to_numpy(code.correct_batch(y[:B], osd=order))
            assert sorted(got) == ["metric", "nerr", "out", "status"]
            same(got, want, min(B, modelled), (case, order, B))
            holds_everywhere(code, bt["y"][:B], got, (case, order, B))
    # the comparison is worth something: in at least one frame in eight the walk along pi passed over a dependent column
    # before the basis was complete, and higher orders found closer words (a code with l = 1 has one basis position; in
    # these batches no pair wins on the three Hamming codes, t = 1)
    assert (bt["want"]["skipped"] > 0).mean() >= 0.125, (bt["want"]["skipped"] > 0).mean()
    assert (bt["want"][("order", 1)]["winner"] > 0).sum() >= 4
    if bt["dec"].l > 1 and t > 1:
        assert (bt["want"]["winner"] > bt["dec"].l).sum() >= 2


@pytest.mark.parametrize("tag", [cc.peterson_gorenstein_zierler_tag, cc.euklid_tag], ids=["pgz", "euklid"])
def test_the_tag_does_not_matter(tag):
    import torch
    case = CASES[5]
    bt = batches(*case)
    got = to_numpy(make(case[0], case[1], case[2], tag).correct_batch(torch.from_numpy(bt["y"].copy()).cuda(), osd=2))
    same(got, bt["want"], bt["modelled"], (case, "tag"))


# ---- constructed frames ----
SPECIAL = [(4, 2), (6, 3), (8, 3)]
TINY = np.finfo(np.float32).tiny


@functools.lru_cache(maxsize=None)
def special_batch(q, t):
    dec = M.decoder(q, t)
    n = dec.n
    rng = np.random.default_rng(40 + q)
    words = dec.encode(rng.integers(0, 2, (4, dec.l)).astype(np.uint8))
    sign = lambda c: (1.0 - 2.0 * c.astype(np.float32)).astype(np.float32)
    frames, names = [], []

    def add(name, f):
        names.append(name)
        frames.append(np.asarray(f, np.float32))
    # all magnitudes equal: pi is the identity, and the metrics are small integers, so that many tie
    f = sign(words[0]).copy()
    f[[2, n - 3, n // 2]] *= np.float32(-1.0)
    add("equal", f)
    add("equal-random", rng.choice(np.array([-1.0, 1.0], np.float32), n))
    # +-0.0: z = 0 everywhere (-0.0 < 0 is false), every key and every metric zero
    add("zeros", np.where(rng.integers(0, 2, n) != 0, np.float32(-0.0), np.float32(0.0)))
    # denormals only
    add("denormal", (awgn_llr(rng, words[1:2], dec.l / n, 3.0)[0] * np.float32(1e-42)).astype(np.float32))
    # magnitudes next to FLT_MAX, three errors: every candidate that differs from z twice or more has M = +inf
    f = (sign(words[2]) * np.float32(3e38)).astype(np.float32)
    f[[1, n // 3, n - 2]] *= np.float32(-1.0)
    add("top", f)
    add("top-random", (rng.choice(np.array([-1.0, 1.0], np.float32), n) * rng.uniform(2.5e38, 3.4e38, n)).astype(np.float32))
    # a noiseless codeword
    add("codeword", sign(words[3]))
    y = np.ascontiguousarray(np.array(frames, np.float32))
    assert np.isfinite(y).all()
    y.setflags(write=False)
    with np.errstate(over="ignore"):
        want = M.osd(dec, y, M.MAX_ORDER)
    return dict(dec=dec, y=y, names=names, want=want, words=words)


@pytest.mark.parametrize("q,t", SPECIAL, ids=["bch15", "bch63", "bch255"])
def test_model_special_frames_exercise_the_rules(q, t):
    bt = special_batch(q, t)
    y, want, names, n = bt["y"], bt["want"], bt["names"], bt["dec"].n
    at = names.index
    assert np.array_equal(M.order(y[at("equal")]), np.arange(n)) and np.array_equal(M.order(y[at("zeros")]), np.arange(n))
    assert want["metric"][at("zeros")].view(np.uint32) == 0 and want["winner"][at("zeros")] == 0
    assert not want["out"][at("zeros")].any()
    assert (np.abs(y[at("denormal")]) < TINY).all() and (y[at("denormal")] != 0).mean() > 0.9
    assert want[("order", 0)]["metric"][at("denormal")] < TINY
    assert np.isposinf(want["metric"][at("top-random")]) or want["nerr"][at("top-random")] <= 1
    k = at("codeword")
    for o in (0, 1, 2):
        r = want[("order", o)]
        assert r["winner"][k] == 0 and r["metric"][k].view(np.uint32) == 0 and r["nerr"][k] == 0
        assert np.array_equal(r["out"][k], bt["words"][3])
    # three errors at the top of the range: the word sent differs from z three times, so its metric is +inf, like that
    # of every other candidate further than one position from z
    assert np.isposinf(want["metric"][at("top")]) or want["nerr"][at("top")] <= 1


@pytest.mark.parametrize("q,t", SPECIAL, ids=["bch15", "bch63", "bch255"])
def test_device_equals_model_on_special_frames(q, t):
    import torch
    bt = special_batch(q, t)
    code = make(q, t)
    y = torch.from_numpy(bt["y"].copy()).cuda()
    for order in ORDERS:
        got = to_numpy(code.correct_batch(y, osd=order))
        same(got, bt["want"][("order", order)], y.shape[0], ((q, t), order))


# ---- a wavefront's second frame ----
def test_second_visit_of_a_wavefront():
    """more than twice the frames one pass of the largest grid takes, so that every wavefront meets a second and a third
    frame in the LDS region that the frame before has left"""
    import torch
    code = make(3, 1)
    dec = M.decoder(3, 1)
    n = dec.n
    # launch_osd caps the grid at num_cus * 8 workgroups of 4 wavefronts
    W = 32 * torch.cuda.get_device_properties(0).multi_processor_count
    F = capi.lib().cc_osd_frames_per_wavefront(code._h, 2)
    assert F >= 1
    B = 2 * W * F + 37 * F + 3
    rng = np.random.default_rng(7300)
    words = dec.encode(rng.integers(0, 2, (16, dec.l)).astype(np.uint8))
    y = awgn_llr(rng, words[rng.integers(0, 16, B)], dec.l / n, 3.0)
    y[W * F - 2 * F: W * F + 2 * F] = quantised(rng, (4 * F, n))
    y = np.ascontiguousarray(y, np.float32)
    dev = torch.from_numpy(y).cuda()
    res = code.correct_batch(dev, osd=2)
    got = to_numpy(res)

    pick = np.zeros(B, bool)
    pick[::97] = True
    pick[W * F - 2 * F: W * F + 4 * F] = True
    pick[2 * W * F - 2 * F: 2 * W * F + 4 * F] = True
    pick[B - 300:] = True
    idx = np.flatnonzero(pick)
    assert idx.size <= 2500
    want = M.osd(dec, y[idx], 2)
    same({k: v[idx] for k, v in got.items()}, want, idx.size, "second visit")
    later = idx >= W * F  # without these the comparison beyond the first pass proves nothing
    assert (want["winner"][later] > 0).sum() >= 5 and (want["skipped"][later] > 0).sum() >= 5

    head, tail = code.correct_batch(dev[: W * F], osd=2), code.correct_batch(dev[W * F:], osd=2)
    for k in ("out", "nerr", "status", "metric"):
        assert torch.equal(torch.cat([head[k], tail[k]]).view(torch.uint8), res[k].view(torch.uint8)), k
    holds_everywhere(code, y, got, "second visit")


def test_higher_orders_are_never_worse():
    import torch
    code = make(6, 3)
    dec = M.decoder(6, 3)
    rng = np.random.default_rng(63)
    words = dec.encode(rng.integers(0, 2, (4096, dec.l)).astype(np.uint8))
    y = awgn_llr(rng, words, dec.l / dec.n, 2.0)
    dev = torch.from_numpy(y).cuda()
    res = [to_numpy(code.correct_batch(dev, osd=o)) for o in ORDERS]
    H = np.asarray(code.H(), np.int64)
    for r in res:
        assert not ((r["out"].astype(np.int64) @ H.T) % 2).any()
    assert (res[2]["metric"] <= res[1]["metric"]).all() and (res[1]["metric"] <= res[0]["metric"]).all()
    assert (res[2]["metric"] < res[1]["metric"]).any() and (res[1]["metric"] < res[0]["metric"]).any()


# ---- the buffer contract ----
BUFFERS = {"bch7": (3, 1, None), "bch63": (6, 3, None), "bch50": (6, 3, 50), "bch255": (8, 3, None)}


@pytest.mark.parametrize("name", list(BUFFERS))
def test_buffer_contract(name):
    q, t, N = BUFFERS[name]
    dec = M.decoder(q, t, N)
    B = 10 if name == "bch255" else 40
    rng = np.random.default_rng(900 + q + (N or 0))
    y = awgn_llr(rng, dec.encode(rng.integers(0, 2, (B, dec.l)).astype(np.uint8)), dec.l / dec.n, 3.0)
    y[::7, 1] = np.float32(0.0)
    y[3::11, dec.n - 1] = np.float32(-0.0)
    y = np.ascontiguousarray(y, np.float32)
    order = 2
    want = M.osd(dec, y, order)
    code = make(q, t, N)
    n = code.n
    for frames in (1, B):
        def call(a):
            return capi.lib().cc_correct_osd_batch_dev(code._h, a["llr"], order, a["out"], a["nerr"], a["metric"], a["status"],
                                                       frames, a["stream"])
        outputs = {"out": (np.uint8, frames * n), "nerr": (np.int32, frames), "metric": (np.float32, frames),
                   "status": (np.int32, frames)}
        expected = {k: want[k][:frames] for k in outputs}
        check_call(call, {"llr": y[:frames]}, outputs, expected, optional=("nerr", "metric", "status"), what=(name, frames))


def test_host_pointers_equal_device_pointers():
    """numpy (pageable and page-locked) against torch, with the staging chunk forced small in a process of its own (the
    value is read once): 200 frames of n = 255 in chunks of 39"""
    here = os.path.dirname(os.path.abspath(__file__))
    script = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import numpy as np, torch\n"
        "import channelcoding_amd as cc\n"
        "rng = np.random.default_rng(5)\n"
        "for q, t, N in ((8, 3, None), (6, 3, 50)):\n"
        "    code = cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag(), **({} if N is None else {'n': N}))\n"
        "    y = (1.0 + 0.6 * rng.standard_normal((200, code.n))).astype(np.float32)\n"
        "    pinned = torch.from_numpy(y).pin_memory().numpy()\n"
        "    for order in (0, 1, 2):\n"
        "        dev = {k: v.cpu().numpy() for k, v in code.correct_batch(torch.from_numpy(y.copy()).cuda(), osd=order).items()}\n"
        "        assert (dev['status'] == 0).all() and (dev['nerr'] > 0).any()\n"
        "        for src in (y, pinned):\n"
        "            host = code.correct_batch(src, osd=order)\n"
        "            assert sorted(host) == ['metric', 'nerr', 'out', 'status']\n"
        "            for k in host:\n"
        "                assert host[k].dtype == dev[k].dtype and np.array_equal(host[k].view(np.uint8), dev[k].view(np.uint8)), (order, k)\n"
        "        dec = code.decode_batch(y, osd=order)\n"
        "        assert np.array_equal(dec['out'], dev['out']) and np.array_equal(dec['msg'], code.extract_batch(dev['out']))\n"
        "print('OSD HOST OK')\n" % (here, os.path.dirname(here)))
    env = dict(os.environ, CC_AMD_HOST_CHUNK_BYTES="40000")
    out = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "OSD HOST OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


# ---- Monte-Carlo ----
def channel(code, ebno, seed, first, frames, random_codewords=True):
    import torch
    llr = torch.empty((frames, code.n), dtype=torch.float32, device="cuda")
    sent = torch.empty((frames, code.n), dtype=torch.uint8, device="cuda")
    capi.check(capi.lib().cc_awgn_llr_dev(code._h, float(ebno), seed, first, frames, int(random_codewords),
                                          C.c_void_p(llr.data_ptr()), C.c_void_p(sent.data_ptr()), None), "cc_awgn_llr_dev")
    torch.cuda.synchronize()
    return llr, sent


def mc(code, order, ebno, seed, first, frames, random_codewords=True):
    return OsdBackend(code, order, random_codewords).run(ebno, seed, first, frames).cpu().numpy()


def counted(out, sent, llr):
    """the counters of the frames given, by the definitions of the header: every frame decodes"""
    wrong = (out != sent).sum(axis=1)
    c = np.zeros(capi.MC_NCOUNTERS, np.int64)
    c[capi.MC_FRAMES] = out.shape[0]
    c[capi.MC_WORD_ERRORS] = int((wrong > 0).sum())
    c[capi.MC_BIT_ERRORS] = int(wrong.sum())
    c[capi.MC_UNDETECTED] = int((wrong > 0).sum())
    c[capi.MC_CHANNEL_BIT_ERRORS] = int(((llr < 0) != (sent != 0)).sum())
    return c


@pytest.mark.parametrize("random_codewords", [True, False], ids=["random", "zero"])
@pytest.mark.parametrize("q,t,order,ebno", [(4, 2, 2, 1.0), (5, 3, 1, 1.0)], ids=["bch15-o2", "bch31-o1"])
def test_mc_counters_against_the_model_and_sharding(q, t, order, ebno, random_codewords):
    code = make(q, t)
    seed, frames = 2024 + q, 1024
    llr, sent = channel(code, ebno, seed, 0, frames, random_codewords)
    y, s = llr.cpu().numpy(), sent.cpu().numpy()
    assert s.any() == random_codewords
    want = M.osd(M.decoder(q, t), y, order)
    expect = counted(want["out"], s, y)
    got = mc(code, order, ebno, seed, 0, frames, random_codewords)
    assert np.array_equal(got, expect), (got[:8], expect[:8])
    assert expect[capi.MC_WORD_ERRORS] > 0 and got[capi.MC_FAILURES] == 0
    assert got[capi.MC_ITER_SUM] == 0 and not got[capi.MC_ITER_HIST:].any()
    halves = mc(code, order, ebno, seed, 0, 500, random_codewords)
    halves = halves + mc(code, order, ebno, seed, 500, frames - 500, random_codewords)
    assert np.array_equal(halves, got)


def test_mc_across_a_chunk_boundary_equals_the_composition():
    code = make(4, 2)
    seed, frames, order = 99, (1 << 20) + 4096, 1  # MC_CHUNK = 2^20
    got = mc(code, order, 2.0, seed, 0, frames)
    llr, sent = channel(code, 2.0, seed, 0, frames)
    res = code.correct_batch(llr, osd=order)
    wrong = (res["out"] != sent).sum(dim=1)
    expect = np.zeros(capi.MC_NCOUNTERS, np.int64)
    expect[capi.MC_FRAMES] = frames
    expect[capi.MC_WORD_ERRORS] = int((wrong > 0).sum())
    expect[capi.MC_BIT_ERRORS] = int(wrong.sum())
    expect[capi.MC_UNDETECTED] = int((wrong > 0).sum())
    expect[capi.MC_CHANNEL_BIT_ERRORS] = int(((llr < 0) != (sent != 0)).sum())
    assert np.array_equal(got, expect), (got[:8], expect[:8])
    assert expect[capi.MC_WORD_ERRORS] > 0 and int((res["status"] != 0).sum()) == 0


# ---- against hard decoding ----
# Chosen with the models on the CPU, over the frames cc_awgn_llr_dev writes for this seed: of 4096 frames of BCH(63,45) at
# 4 dB, seed 11, osd_model counts 15 word errors at order 1 and chase_model 489 at p = 0 (bounded-distance decoding,
# failures included): a factor of 32.  (3 dB: 127 against 1289; 5 dB: 1 against 80 -- too few to tell anything.)
WER_EBNO, WER_SEED, WER_FRAMES = 4.0, 11, 4096
WER_MODEL_OSD1, WER_MODEL_HARD = 15, 489


def test_order_1_has_fewer_word_errors_than_hard_decoding():
    code = make(6, 3)
    llr, sent = channel(code, WER_EBNO, WER_SEED, 0, WER_FRAMES)
    osd1 = code.correct_batch(llr, osd=1)
    hard = code.correct_batch(llr, chase=0)
    errors_osd = int(((osd1["out"] != sent).sum(dim=1) > 0).sum())
    errors_hard = int((((hard["out"] != sent).sum(dim=1) > 0) | (hard["status"] != 0)).sum())
    print("word errors of %d frames: order 1 %d, hard %d" % (WER_FRAMES, errors_osd, errors_hard))
    assert 2 * WER_MODEL_OSD1 <= WER_MODEL_HARD
    assert 0 < errors_osd < errors_hard
