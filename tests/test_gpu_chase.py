"""GPU tests of Chase-II decoding: cc_correct_chase_batch(_dev) bit for bit against tests/chase_model.py
on out, nerr, status and metric; p = 0 against the hard decoder; host-pointer against device entry point; properties that
need nothing but H; and cc_mc_run_chase_dev against the model, against its own shards and against the composition of the
channel call, the decoder call and a count.  EDGE_CASES and the tests after test_host_pointers_equal_device_pointers
hold the kernel's layout boundaries: t = 1 and 4 .. 8, q = 3, lengths next to a multiple of 64, p = n, a wavefront's
second group of frames, denormal and near-overflow values, absent outputs and buffers at odd addresses."""
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

# The same columns.  t >= 4 takes the root search that reads lambda from LDS up to the wavefront's largest degree, with
# one (t = 4), a partial second (t = 5 .. 7) and two full (t = 8) reductions of four odd syndromes; t = 1 has a single
# syndrome in a reduction of four; n = 64 c and 64 c + 1 end a 64-position word of the flip masks; N = 5 and 6 allow p = n.
EDGE_CASES = [(6, 4, None, 3.0), (5, 5, None, 2.0), (7, 5, None, 3.5), (8, 4, None, 4.5), (6, 7, None, 3.5),
              (8, 8, None, 4.0),
              (3, 1, None, 3.0), (4, 1, None, 3.0), (8, 1, None, 5.0), (8, 1, 100, 5.0),
              (7, 3, 64, 4.0), (8, 3, 65, 4.0), (8, 3, 128, 4.5), (8, 3, 129, 4.5), (8, 2, 192, 5.0), (8, 3, 193, 5.0),
              (3, 1, 5, 3.0), (3, 1, 6, 3.0)]
ALL_CASES = CASES + EDGE_CASES
ALL_IDS = ["bch%d-t%d%s" % (q, t, "" if N is None else "-N%d" % N) for q, t, N, _ in ALL_CASES]


def perfect(case):
    """a full-length t = 1 code is a Hamming code: every word is within one position of a codeword, hard decoding never
    fails and no frame is without a candidate"""
    return case[1] == 1 and case[2] is None


def tiny(case):
    return case[2] is not None and case[2] <= 6


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
    big = t < 8
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
@pytest.mark.parametrize("case", ALL_CASES, ids=ALL_IDS)
def test_device_equals_model(case, p):
    import torch
    q, t, N, ebno = case
    bt = batches(*case)
    p = min(p, bt["dec"].n)  # a frame of five positions: p = 6 stands for p = n
    want = M.pick(bt["cand"], p)
    code = make(q, t, N)
    y = torch.from_numpy(bt["y"].copy()).cuda()
    for B in frame_counts(bt):
        same(code.correct_batch(y[:B], chase=p), want, B, (case, p, B))
    if p == 1 and not perfect(case) and not tiny(case):
        assert (want["status"][bt["low"]] == M.FRAME_LOCATOR).any()  # at -2 dB some frame has no candidate at all


@pytest.mark.parametrize("case", ALL_CASES, ids=ALL_IDS)
def test_model_batches_exercise_the_rules(case):
    """what makes the comparison above worth something, asserted on the model alone"""
    bt = batches(*case)
    cand, keep = bt["cand"], ~bt["low"]
    pn = min(6, bt["dec"].n)
    p6, p0 = M.pick(cand, pn), M.pick(cand, 0)
    assert (p6["winner"][keep] > 0).sum() >= 5
    several = [np.unique(cand["words"][f][cand["ok"][f]], axis=0).shape[0] > 1 for f in np.flatnonzero(keep)]
    # (two codewords of a t >= 15 code are 31 or more positions apart: six flips do not reach from one's sphere of radius
    #  t into another's in a batch of a hundred frames, so those codes show the first and the third property only; so
    #  does BCH(255,191) with t = 8, where they are 17 or more apart)
    assert sum(several) >= 5 or case[1] >= 15 or case[:3] == (8, 8, None)
    differs = (p6["status"] != p0["status"]) | (p6["out"] != p0["out"]).any(axis=1)
    assert differs[keep].sum() >= 5
    if perfect(case):
        assert (p0["status"] == M.FRAME_OK).all()
    elif tiny(case):
        # BCH(7,4) cut to N positions fails only where the Hamming decoder corrects a position it does not have; all
        # 2^N words are test patterns of p = N, codewords among them
        assert (p0["status"] != M.FRAME_OK).any() and (p6["status"] == M.FRAME_OK).all()
    else:
        fails = (p0["status"][: bt["sizes"][0]] != M.FRAME_OK).mean()
        assert 0.05 <= fails <= 0.35, fails  # hard decoding fails on a fair share of the AWGN frames, not on most


@pytest.mark.parametrize("tag", [cc.peterson_gorenstein_zierler_tag, cc.euklid_tag], ids=["pgz", "euklid"])
@pytest.mark.parametrize("case", ALL_CASES, ids=ALL_IDS)
def test_p0_is_hard_decoding_and_the_tag_does_not_matter(case, tag):
    import torch
    q, t, N, _ = case
    bt = batches(*case)
    y = torch.from_numpy(bt["y"].copy()).cuda()
    code = make(q, t, N, tag)
    got = {k: v.cpu().numpy() for k, v in code.correct_batch(y, chase=0).items()}
    hard = {k: v.cpu().numpy() for k, v in make(q, t, N, cc.peterson_gorenstein_zierler_tag).correct_batch(y).items()}
    ok = hard["status"] == M.FRAME_OK
    assert np.array_equal(got["status"] == M.FRAME_OK, ok)
    assert ok.all() if perfect(case) else ok.any() and not ok.all()
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


# ---- a wavefront's second group of frames ----
SECOND = [(4, 2, 3.0, 6), (4, 2, 3.0, 3), (5, 5, 2.0, 2), (6, 4, 3.0, 6)]


@pytest.mark.parametrize("q,t,ebno,p", SECOND, ids=["bch%d-t%d-p%d" % (q, t, p) for q, t, _, p in SECOND])
def test_second_visit_of_a_wavefront(q, t, ebno, p):
    """more than twice the frames one pass of the grid takes, so that every wavefront meets a second and some a third
    group in the LDS region (Y, SZ, LP, WM, the BM columns) that the group before has left"""
    import torch
    # launch_chase caps the grid at num_cus * 8 workgroups of 4 wavefronts
    W = 32 * torch.cuda.get_device_properties(0).multi_processor_count
    F = 64 >> p  # the kernel's frames per wavefront are never more: one pass takes W * F frames at the most
    B = 2 * W * F + 37 * F + 3
    dec = M.decoder(q, t)
    n = dec.n
    rng = np.random.default_rng(7000 + 100 * q + p)
    words = dec.encode(rng.integers(0, 2, (1024, dec.l)).astype(np.uint8))
    y = awgn_llr(rng, words[rng.integers(0, 1024, B)], dec.l / n, ebno)
    y[W * F - 2 * F: W * F + 2 * F] = quantised(rng, (4 * F, n))
    y = np.ascontiguousarray(y, np.float32)
    code = make(q, t)
    dev = torch.from_numpy(y).cuda()
    res = code.correct_batch(dev, chase=p)
    got = {k: v.cpu().numpy() for k, v in res.items()}

    # the model on a subset
    pick = np.zeros(B, bool)
    pick[::97] = True
    pick[W * F - 2 * F: W * F + 4 * F] = True
    pick[2 * W * F - 2 * F: 2 * W * F + 4 * F] = True
    pick[B - 1100:] = True
    idx = np.flatnonzero(pick)
    assert idx.size <= 5000
    want = M.chase(dec, y[idx], p)
    for k in ("out", "nerr", "status"):
        bad = (got[k][idx] != want[k]).reshape(idx.size, -1).any(axis=1)
        assert not bad.any(), (k, idx[bad][:8])
    assert np.array_equal(got["metric"][idx].view(np.uint32), want["metric"].view(np.uint32))
    later = idx >= W * F  # without these the comparison beyond the first pass proves nothing
    assert (want["winner"][later] > 0).sum() >= 5
    # (BCH(15,7) has no frame without a candidate at p = 6: for each of the 5005 sets of six positions, every one of the
    #  256 syndromes is moved onto that of a word within two positions of a codeword by some of the 64 patterns, found
    #  by enumeration.  BCH(63,39) at p = 6 shows the frame that leaves a zero winner mask with one frame per wavefront)
    assert (want["status"][later] == M.FRAME_LOCATOR).sum() >= 1 or (q, t, p) == (4, 2, 6)

    # no state carries from group to group: the call on a prefix and the call on the rest give the same
    head, tail = code.correct_batch(dev[: W * F], chase=p), code.correct_batch(dev[W * F:], chase=p)
    for k in ("out", "nerr", "status", "metric"):
        assert torch.equal(torch.cat([head[k], tail[k]]).view(torch.uint8), res[k].view(torch.uint8)), k

    # every frame: a codeword where the status says so, with the metric of the contract
    ok = got["status"] == M.FRAME_OK
    assert set(np.unique(got["status"])) <= {M.FRAME_OK, M.FRAME_LOCATOR} and ok.any()
    H = np.asarray(code.H(), np.int64)
    assert not ((got["out"][ok].astype(np.int64) @ H.T) % 2).any()
    z = M.hard(y)
    assert np.array_equal(got["out"][~ok], z[~ok]) and (got["nerr"][~ok] == -1).all()
    assert np.array_equal((got["out"] != z).sum(axis=1)[ok], got["nerr"][ok])
    assert np.array_equal(M.metric(y, z, got["out"]).view(np.uint32), got["metric"].view(np.uint32))


# ---- value ranges ----
TINY = np.finfo(np.float32).tiny
VALUE_CASES = [(6, 3, None, 4.0), (6, 4, None, 3.0)]  # the register and the LDS variant of the root search


def scaled(y, kind):
    with np.errstate(over="ignore"):
        small = (y * np.float32(1e-42)).astype(np.float32)
        large = np.clip((y * np.float32(1e38)).astype(np.float32), np.float32(-3e38), np.float32(3e38))
        large = large.astype(np.float32)
    if kind == "denormal":
        return small
    if kind == "top":
        return large
    mixed = large.copy()  # the frames that share a wavefront lie eighty orders of magnitude apart
    mixed[::2] = small[::2]
    return mixed


@functools.lru_cache(maxsize=None)
def value_batch(case, kind):
    """300 AWGN frames of the case, scaled, and constructed frames behind them; candidates of all 64 patterns"""
    q, t, N, ebno = case
    dec = M.decoder(q, t, N)
    n = dec.n
    rng = np.random.default_rng(500 + 10 * q + t)
    words = dec.encode(rng.integers(0, 2, (300, dec.l)).astype(np.uint8))
    y = scaled(awgn_llr(rng, words, dec.l / n, ebno), kind)
    extra = []
    if kind != "top":
        # codewords at the smallest magnitude there is: z is the codeword (nerr = 0) only if -1.4e-45 < 0 holds
        one = np.float32(1e-45)
        assert one > 0 and one == np.float32(2.0 ** -149)
        c10 = next(w for w in words if w[0] == 1 and w[n - 1] == 0)
        c01 = next(w for w in words if w[0] == 0 and w[n - 1] == 1)
        for c in (c10, c01):
            f = ((1.0 - 2.0 * c.astype(np.float32)) * np.float32(1e-42)).astype(np.float32)
            f[0], f[n - 1] = (-one, one) if c[0] else (one, -one)
            extra.append(f)
    if kind != "denormal":
        # all magnitudes 3e38, two errors beyond L_0 .. L_5 = 0 .. 5: every candidate differs from z in two or more
        # positions (the word sent in exactly the two, any other codeword in 2t + 1 - 2 or more), so every M is +inf
        f = ((1.0 - 2.0 * words[0].astype(np.float32)) * np.float32(3e38)).astype(np.float32)
        f[[10, 20]] *= np.float32(-1.0)
        extra.append(f)
    y = np.ascontiguousarray(np.concatenate([y, np.array(extra, np.float32)]), np.float32)
    assert np.isfinite(y).all()
    y.setflags(write=False)
    with np.errstate(over="ignore"):
        cand = M.candidates(dec, y)
    return dict(dec=dec, y=y, cand=cand, words=words)


@pytest.mark.parametrize("kind", ["denormal", "top", "mixed"])
@pytest.mark.parametrize("case", VALUE_CASES, ids=["bch6-t3", "bch6-t4"])
def test_model_value_batches_exercise_the_ranges(case, kind):
    """on the model alone: what a kernel that flushed denormals, or mishandled +inf, could not pass"""
    bt = value_batch(case, kind)
    y, cand, n = bt["y"], bt["cand"], bt["dec"].n
    p6, p0 = M.pick(cand, 6), M.pick(cand, 0)
    assert np.isfinite(y).all()
    if kind == "denormal":
        assert (np.abs(y) < TINY).all() and (y != 0).mean() > 0.99
        won = p6["metric"][p6["status"] == M.FRAME_OK]
        assert np.unique(won[won != 0]).size >= 50 and (won < TINY).all()
    if kind != "top":
        k = 300  # the two codewords at +-1.4e-45
        assert (cand["z"][k, 0], cand["z"][k, n - 1], cand["z"][k + 1, 0], cand["z"][k + 1, n - 1]) == (1, 0, 0, 1)
        for p_ in (p0, p6):
            assert (p_["status"][k: k + 2] == M.FRAME_OK).all() and (p_["nerr"][k: k + 2] == 0).all()
            assert np.array_equal(p_["out"][k: k + 2], cand["z"][k: k + 2])
    if kind != "denormal":
        inf = np.isinf(cand["M"]) & cand["ok"]
        assert (inf.sum(axis=1) >= 2).sum() >= 20
        assert not np.isnan(cand["M"]).any()
        last = y.shape[0] - 1
        for p_ in (p0, M.pick(cand, 3), p6):
            assert p_["status"][last] == M.FRAME_OK and np.isposinf(p_["metric"][last]) and p_["nerr"][last] == 2
            assert p_["winner"][last] == 0 and np.array_equal(p_["out"][last], bt["words"][0])
        assert cand["ok"][last].sum() >= 2 and np.isposinf(cand["M"][last][cand["ok"][last]]).all()  # a tie at +inf
    if kind == "mixed":
        assert (np.abs(y[:300:2]) < TINY).all() and (np.abs(y[1:300:2]) > 1e30).all()


@pytest.mark.parametrize("kind", ["denormal", "top", "mixed"])
@pytest.mark.parametrize("case", VALUE_CASES, ids=["bch6-t3", "bch6-t4"])
def test_device_equals_model_on_value_ranges(case, kind):
    import torch
    q, t, N, _ = case
    bt = value_batch(case, kind)
    assert np.isfinite(bt["y"]).all()
    code = make(q, t, N)
    y = torch.from_numpy(bt["y"].copy()).cuda()
    for p in (0, 3, 6):
        same(code.correct_batch(y, chase=p), M.pick(bt["cand"], p), y.shape[0], (case, kind, p))


# ---- optional outputs, buffers at odd addresses ----
GUARD, SENTINEL = 8, 0x5A


def guarded(torch, count, dtype):
    """count elements between two runs of GUARD elements, every byte SENTINEL"""
    size = torch.empty(0, dtype=dtype).element_size()
    whole = torch.full(((count + 2 * GUARD) * size,), SENTINEL, dtype=torch.uint8, device="cuda").view(dtype)
    return whole, whole[GUARD: GUARD + count]


def guards_intact(torch, whole):
    b = whole.view(torch.uint8)
    g = GUARD * whole.element_size()
    return bool((b[:g] == SENTINEL).all()) and bool((b[-g:] == SENTINEL).all())


def chase_dev(torch, code, llr, p, out, nerr, metric, status, B):
    ptr = lambda a: None if a is None else C.c_void_p(a.data_ptr())
    rc = capi.lib().cc_correct_chase_batch_dev(code._h, ptr(llr), p, ptr(out), ptr(nerr), ptr(metric), ptr(status), B, None)
    capi.check(rc, "cc_correct_chase_batch_dev")
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", [CASES[2], EDGE_CASES[3]], ids=["bch6-t3", "bch8-t4"])
def test_optional_outputs_and_offset_buffers(case):
    import torch
    q, t, N, _ = case
    assert (q, t) in ((6, 3), (8, 4))
    bt = batches(*case)
    B, p, n = 200, 3, bt["dec"].n
    code = make(q, t, N)
    y = torch.from_numpy(bt["y"][:B].copy()).cuda()
    full = code.correct_batch(y, chase=p)
    same(full, M.pick(bt["cand"], p), B, (case, "full"))
    kinds = dict(nerr=torch.int32, metric=torch.float32, status=torch.int32)
    for mask in range(8):
        passed = [k for i, k in enumerate(kinds) if (mask >> i) & 1]
        bufs = {k: guarded(torch, B, kinds[k]) for k in passed}
        out_whole, out = guarded(torch, B * n, torch.uint8)
        args = {k: bufs[k][1] if k in bufs else None for k in kinds}  # an output not passed has no buffer at all
        chase_dev(torch, code, y, p, out, args["nerr"], args["metric"], args["status"], B)
        assert torch.equal(out.view(B, n), full["out"]) and guards_intact(torch, out_whole), (mask, "out")
        for k in passed:
            assert torch.equal(bufs[k][1].view(torch.uint8), full[k].view(torch.uint8)), (mask, k)
            assert guards_intact(torch, bufs[k][0]), (mask, k)
    # llr one float and out one byte into larger allocations (rows of an odd n are misaligned anyway)
    llr_big = torch.zeros(B * n + 1, dtype=torch.float32, device="cuda")
    llr_big[1:] = y.reshape(-1)
    out_big = torch.full((B * n + 2,), SENTINEL, dtype=torch.uint8, device="cuda")
    llr, out = llr_big[1:], out_big[1: 1 + B * n]
    assert llr.data_ptr() % 8 == 4 and out.data_ptr() % 2 == 1
    nerr, status = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    metric = torch.empty(B, dtype=torch.float32, device="cuda")
    chase_dev(torch, code, llr, p, out, nerr, metric, status, B)
    assert int(out_big[0]) == SENTINEL and int(out_big[-1]) == SENTINEL
    want = {k: v.cpu().numpy() for k, v in full.items()}
    same(dict(out=out.view(B, n), nerr=nerr, status=status, metric=metric), want, B, (case, "offset"))


# ---- Monte-Carlo ----
def channel(code, ebno, seed, first, frames, random_codewords=True):
    import torch
    llr = torch.empty((frames, code.n), dtype=torch.float32, device="cuda")
    sent = torch.empty((frames, code.n), dtype=torch.uint8, device="cuda")
    capi.check(capi.lib().cc_awgn_llr_dev(code._h, float(ebno), seed, first, frames, int(random_codewords),
                                          C.c_void_p(llr.data_ptr()), C.c_void_p(sent.data_ptr()), None), "cc_awgn_llr_dev")
    torch.cuda.synchronize()
    return llr, sent


def mc(code, p, ebno, seed, first, frames, random_codewords=True):
    return ChaseBackend(code, p, random_codewords).run(ebno, seed, first, frames).cpu().numpy()


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


@pytest.mark.parametrize("random_codewords", [True, False], ids=["random", "zero"])
def test_mc_counters_of_a_t4_code_with_random_and_all_zero_words(random_codewords):
    code = make(6, 4)
    seed, frames, p, ebno = 4064, 2048, 3, 3.0
    llr, sent = channel(code, ebno, seed, 0, frames, random_codewords)
    y, s = llr.cpu().numpy(), sent.cpu().numpy()
    assert s.any() == random_codewords
    want = M.chase(M.decoder(6, 4), y, p)
    expect = counted(want["out"], want["status"], s, y)
    got = mc(code, p, ebno, seed, 0, frames, random_codewords)
    assert np.array_equal(got, expect), (got[:8], expect[:8])
    assert expect[capi.MC_WORD_ERRORS] > 0 and expect[capi.MC_FAILURES] > 0
    assert got[capi.MC_ITER_SUM] == 0 and not got[capi.MC_ITER_HIST:].any()
    halves = mc(code, p, ebno, seed, 0, 1000, random_codewords)
    halves = halves + mc(code, p, ebno, seed, 1000, frames - 1000, random_codewords)
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
