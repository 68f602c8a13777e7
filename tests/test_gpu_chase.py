"""GPU tests of Chase-II decoding: cc_correct_chase_batch(_dev) bit for bit against tests/chase_model.py
on out, nerr, status and metric; p = 0 against the hard decoder; host-pointer against device entry point; properties that
need nothing but H; and cc_mc_run_chase_dev against the model, against its own shards and against the composition of the
channel call, the decoder call and a count."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import capi
from channelcoding_amd.montecarlo import ChaseBackend
import chase_model as M
from checkers import BCH, Oracle, awgn_llr

pytestmark = pytest.mark.gpu

# (q, t, N, Eb/N0 at which hard decoding fails 10 - 25 % of the frames: found with the model on the CPU)
CASES = [(4, 2, None, 3.0), (5, 3, None, 3.0), (6, 3, None, 4.0), (7, 3, None, 4.0), (8, 3, None, 5.0),
         (8, 15, None, 4.0), (8, 16, None, 4.0), (8, 3, 200, 5.0), (6, 3, 50, 4.0)]
IDS = ["bch%d-t%d%s" % (q, t, "" if N is None else "-N%d" % N) for q, t, N, _ in CASES]
PS = (0, 1, 3, 6)  # 64, 32, 8 and 1 frames per wavefront


def make(q, t, N=None, tag=cc.berlekamp_massey_tag):
    return cc.primitive_bch(q, cc.errors(t), tag(), **({} if N is None else {"n": N}))


def quantised(rng, shape):
    """values in {+-0.5, +-1, +-1.5} with a few +-0.0: equal keys in every frame, equal metrics in many"""
    y = rng.choice(np.array([-1.5, -1.0, -0.5, 0.5, 0.5, 1.0, 1.0, 1.5, 1.5, 1.5], np.float32), shape)
    y[::3, 1] = np.float32(0.0)
    y[::4, shape[1] - 1] = np.float32(-0.0)
    y[1::5, 0] = np.float32(-0.0)
    return y.astype(np.float32)


@functools.lru_cache(maxsize=None)
def batches(q, t, N, ebno):
    """the frames of one code -- AWGN, quantised, -2 dB -- and the model's candidates for all 64 patterns, made once"""
    dec = M.decoder(q, t, N)
    big = t < 15
    rng = np.random.default_rng(1000 * q + 10 * t + (N or 0))
    sizes = (1031 if big else 67, 67 if big else 30, 67 if big else 30)
    msgs = rng.integers(0, 2, (sizes[0] + sizes[2], dec.l)).astype(np.uint8)
    words = dec.encode(msgs)
    rate = dec.l / dec.n
    y_awgn = awgn_llr(rng, words[: sizes[0]], rate, ebno)
    y_quant = quantised(rng, (sizes[1], dec.n))
    y_low = awgn_llr(rng, words[sizes[0]:], rate, -2.0)
    y = np.ascontiguousarray(np.concatenate([y_awgn, y_quant, y_low]), np.float32)
    low = np.zeros(y.shape[0], bool)
    low[sizes[0] + sizes[1]:] = True
    y.setflags(write=False)
    return dict(dec=dec, y=y, low=low, cand=M.candidates(dec, y), sizes=sizes)


def frame_counts(bt):
    total = bt["y"].shape[0]
    return (1, 67, 1031, total) if total > 1031 else (1, 67, total)  # none a multiple of every frames-per-wavefront count


def same(got, want, rows, what):
    for k in ("out", "nerr", "status"):
        assert np.array_equal(np.asarray(got[k].cpu()), want[k][:rows]), (what, k)
    assert np.array_equal(got["metric"].cpu().numpy().view(np.uint32), want["metric"][:rows].view(np.uint32)), (what, "metric")


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_equals_model(case, p):
    import torch
    q, t, N, ebno = case
    bt = batches(*case)
    want = M.pick(bt["cand"], p)
    code = make(q, t, N)
    y = torch.from_numpy(bt["y"].copy()).cuda()
    for B in frame_counts(bt):
        same(code.correct_batch(y[:B], chase=p), want, B, (case, p, B))
    if p == 1:
        assert (want["status"][bt["low"]] == M.FRAME_LOCATOR).any()  # at -2 dB some frame has no candidate at all


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_model_batches_exercise_the_rules(case):
    """what makes the comparison above worth something, asserted on the model alone"""
    bt = batches(*case)
    cand, keep = bt["cand"], ~bt["low"]
    p6, p0 = M.pick(cand, 6), M.pick(cand, 0)
    assert (p6["winner"][keep] > 0).sum() >= 5
    several = [np.unique(cand["words"][f][cand["ok"][f]], axis=0).shape[0] > 1 for f in np.flatnonzero(keep)]
    # (two codewords of a t >= 15 code are 31 or more positions apart: six flips do not reach from one's sphere of radius
    #  t into another's in a batch of a hundred frames, so those codes show the first and the third property only)
    assert sum(several) >= 5 or case[1] >= 15
    differs = (p6["status"] != p0["status"]) | (p6["out"] != p0["out"]).any(axis=1)
    assert differs[keep].sum() >= 5
    fails = (p0["status"][: bt["sizes"][0]] != M.FRAME_OK).mean()
    assert 0.05 <= fails <= 0.35, fails  # hard decoding fails on a fair share of the AWGN frames, not on most


@pytest.mark.parametrize("tag", [cc.peterson_gorenstein_zierler_tag, cc.euklid_tag], ids=["pgz", "euklid"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_p0_is_hard_decoding_and_the_tag_does_not_matter(case, tag):
    import torch
    q, t, N, _ = case
    bt = batches(*case)
    y = torch.from_numpy(bt["y"].copy()).cuda()
    code = make(q, t, N, tag)
    got = {k: v.cpu().numpy() for k, v in code.correct_batch(y, chase=0).items()}
    hard = {k: v.cpu().numpy() for k, v in make(q, t, N, cc.peterson_gorenstein_zierler_tag).correct_batch(y).items()}
    ok = hard["status"] == M.FRAME_OK
    assert np.array_equal(got["status"] == M.FRAME_OK, ok) and ok.any() and not ok.all()
    assert np.array_equal(got["out"][ok], hard["out"][ok]) and np.array_equal(got["nerr"][ok], hard["nerr"][ok])
    z = M.hard(bt["y"])
    assert np.array_equal(got["out"][~ok], z[~ok]) and (got["nerr"][~ok] == -1).all()
    assert (got["status"][~ok] == M.FRAME_LOCATOR).all() and (got["metric"][~ok].view(np.uint32) == 0).all()
    same(code.correct_batch(y, chase=3), M.pick(bt["cand"], 3), y.shape[0], (case, "tag"))


def test_properties_against_H():
    import torch
    for case in (CASES[2], CASES[4], CASES[7]):
        q, t, N, _ = case
        bt = batches(*case)
        code = make(q, t, N)
        H = np.asarray(code.H(), np.int64)
        y = bt["y"]
        z = M.hard(y)
        res = {p: {k: v.cpu().numpy() for k, v in code.correct_batch(torch.from_numpy(y.copy()).cuda(), chase=p).items()}
               for p in (3, 6)}
        for p, r in res.items():
            ok = r["status"] == M.FRAME_OK
            assert ok.any() and set(np.unique(r["status"])) <= {M.FRAME_OK, M.FRAME_LOCATOR}
            assert not ((r["out"][ok].astype(np.int64) @ H.T) % 2).any()
            assert np.array_equal(M.metric(y, z, r["out"]).view(np.uint32), r["metric"].view(np.uint32))
            assert np.array_equal((r["out"] != z).sum(axis=1)[ok], r["nerr"][ok])
        both = (res[3]["status"] == M.FRAME_OK) & (res[6]["status"] == M.FRAME_OK)
        assert both.any() and (res[6]["metric"][both] <= res[3]["metric"][both]).all()  # the test sets nest
        assert ((res[3]["status"] == M.FRAME_OK) <= (res[6]["status"] == M.FRAME_OK)).all()


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
        "    for p in (0, 4, 6):\n"
        "        dev = {k: v.cpu().numpy() for k, v in code.correct_batch(torch.from_numpy(y.copy()).cuda(), chase=p).items()}\n"
        "        assert (dev['status'] == 0).any() and (dev['nerr'] > 0).any()\n"
        "        for src in (y, pinned):\n"
        "            host = code.correct_batch(src, chase=p)\n"
        "            assert sorted(host) == ['metric', 'nerr', 'out', 'status']\n"
        "            for k in host:\n"
        "                assert host[k].dtype == dev[k].dtype and np.array_equal(host[k].view(np.uint8), dev[k].view(np.uint8)), (p, k)\n"
        "        dec = code.decode_batch(y, chase=p)\n"
        "        assert np.array_equal(dec['out'], dev['out']) and np.array_equal(dec['msg'], code.extract_batch(dev['out']))\n"
        "print('CHASE HOST OK')\n" % (here, os.path.dirname(here)))
    env = dict(os.environ, CC_AMD_HOST_CHUNK_BYTES="40000")
    out = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "CHASE HOST OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


# ---- Monte-Carlo ----
def channel(code, ebno, seed, first, frames):
    import torch
    llr = torch.empty((frames, code.n), dtype=torch.float32, device="cuda")
    sent = torch.empty((frames, code.n), dtype=torch.uint8, device="cuda")
    capi.check(capi.lib().cc_awgn_llr_dev(code._h, float(ebno), seed, first, frames, 1, C.c_void_p(llr.data_ptr()),
                                          C.c_void_p(sent.data_ptr()), None), "cc_awgn_llr_dev")
    torch.cuda.synchronize()
    return llr, sent


def mc(code, p, ebno, seed, first, frames):
    return ChaseBackend(code, p, True).run(ebno, seed, first, frames).cpu().numpy()


def counted(out, status, sent, llr):
    """the counters of the frames given, by the definitions of the header"""
    wrong = (out != sent).sum(axis=1)
    failed = status != M.FRAME_OK
    c = np.zeros(capi.MC_NCOUNTERS, np.int64)
    c[capi.MC_FRAMES] = out.shape[0]
    c[capi.MC_WORD_ERRORS] = int((failed | (wrong > 0)).sum())
    c[capi.MC_BIT_ERRORS] = int(wrong.sum())
    c[capi.MC_FAILURES] = int(failed.sum())
    c[capi.MC_UNDETECTED] = int((~failed & (wrong > 0)).sum())
    c[capi.MC_CHANNEL_BIT_ERRORS] = int(((llr < 0) != (sent != 0)).sum())
    return c


def test_mc_counters_against_the_model_and_sharding():
    code = make(6, 3)
    seed, frames = 2024, 2048
    llr, sent = channel(code, 4.0, seed, 0, frames)
    y, s = llr.cpu().numpy(), sent.cpu().numpy()
    want = M.chase(M.decoder(6, 3), y, 4)
    expect = counted(want["out"], want["status"], s, y)
    got = mc(code, 4, 4.0, seed, 0, frames)
    assert np.array_equal(got, expect), (got[:8], expect[:8])
    assert expect[capi.MC_WORD_ERRORS] > 0 and got[capi.MC_ITER_SUM] == 0 and not got[capi.MC_ITER_HIST:].any()
    halves = mc(code, 4, 4.0, seed, 0, 1000) + mc(code, 4, 4.0, seed, 1000, frames - 1000)
    assert np.array_equal(halves, got)


def test_mc_across_a_chunk_boundary_equals_the_composition():
    import torch
    code = make(5, 3)
    seed, frames, p = 99, (1 << 20) + 4096, 2  # MC_CHUNK = 2^20
    got = mc(code, p, 3.0, seed, 0, frames)
    llr, sent = channel(code, 3.0, seed, 0, frames)
    res = code.correct_batch(llr, chase=p)
    wrong = (res["out"] != sent).sum(dim=1)
    failed = res["status"] != M.FRAME_OK
    expect = np.zeros(capi.MC_NCOUNTERS, np.int64)
    expect[capi.MC_FRAMES] = frames
    expect[capi.MC_WORD_ERRORS] = int((failed | (wrong > 0)).sum())
    expect[capi.MC_BIT_ERRORS] = int(wrong.sum())
    expect[capi.MC_FAILURES] = int(failed.sum())
    expect[capi.MC_UNDETECTED] = int((~failed & (wrong > 0)).sum())
    expect[capi.MC_CHANNEL_BIT_ERRORS] = int(((llr < 0) != (sent != 0)).sum())
    assert np.array_equal(got, expect), (got[:8], expect[:8])
    assert expect[capi.MC_WORD_ERRORS] > 0 and expect[capi.MC_UNDETECTED] > 0


def test_mc_chase_lowers_the_word_error_rate():
    code = make(6, 3)
    frames = 1 << 16
    hard, soft = mc(code, 0, 4.0, 5, 0, frames), mc(code, 4, 4.0, 5, 0, frames)
    assert hard[capi.MC_FRAMES] == soft[capi.MC_FRAMES] == frames
    assert hard[capi.MC_CHANNEL_BIT_ERRORS] == soft[capi.MC_CHANNEL_BIT_ERRORS] > 0  # the same channel
    assert soft[capi.MC_WORD_ERRORS] < hard[capi.MC_WORD_ERRORS]
