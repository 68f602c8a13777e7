"""GPU tests of GMD decoding: cc_correct_gmd_batch(_dev) bit for bit against tests/gmd_model.py on out,
nerr, status and metric; m = 1 against the hard decoder; host-pointer against device entry point; absent outputs and
buffers at odd addresses; a wavefront's second group of frames; cc_awgn_symbols_dev against the float64 channel model;
and cc_mc_run_gmd_dev against its own shards and against the composition of the channel call, the decoder call and a
count."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import capi
from channelcoding_amd.montecarlo import GmdBackend, shard
import gmd_model as M
from awgn_model import awgn_reference
from checkers import RS, Oracle
from test_discrete_host import rs_message_symbols
from test_gpu_mc import sigma_f32, tau

pytestmark = pytest.mark.gpu

# (q, t, N, mu): RS(7,3), RS(7,5), RS(15,9), RS(31,23), RS(63,47), RS(255,239), RS(255,223) (m = 17, the widest group),
# the two byte codes with first root alpha^0, RS(204,188), RS(255,239) cut to the 64-lane ownership edges, RS(7,3) at
# N = 2t + 1
CASES = [(3, 2, None, 1), (3, 1, None, 1), (4, 3, None, 1), (5, 4, None, 1), (6, 8, None, 1), (8, 8, None, 1),
         (8, 16, None, 1), (8, 16, None, 0), (8, 8, None, 0), (8, 8, 204, 1), (8, 8, 64, 1), (8, 8, 65, 1), (8, 8, 128, 1),
         (8, 8, 129, 1), (8, 8, 192, 1), (8, 8, 193, 1), (3, 2, 5, 1)]


def name(case):
    q, t, N, mu = case
    n = (1 << q) - 1 if N is None else N
    return "rs%d-%d%s" % (n, n - 2 * t, "" if mu == 1 else "-mu%d" % mu)


IDS = [name(c) for c in CASES]


def trial_counts(t):
    return sorted({1, min(2, t + 1), (t + 2) // 2, t + 1})  # (t + 2) // 2 = ceil((t + 1) / 2)


def make(q, t, N=None, mu=1, tag=cc.berlekamp_massey_tag):
    return cc.rs(q, cc.errors(t), tag(), mu=mu, **({} if N is None else {"n": N}))


TINY = np.finfo(np.float32).tiny


@functools.lru_cache(maxsize=None)
def batches(q, t, N, mu):
    """the frames of one code and the model's candidates of all t + 1 trials, made once.  261 general frames with
    0 .. 2t + 1 symbol errors (reliabilities low on the erroneous symbols in two frames of three, uninformative in the
    third), then 8 frames each with all reliabilities equal, all zero, denormal, and near FLT_MAX (M = +inf ties)"""
    dec = M.Decoder(q, t, N, mu)
    n = dec.n
    rng = np.random.default_rng(1000 * q + 10 * t + (N or 0) + 7 * mu)
    B = 261 + 32
    words = dec.encode(rng.integers(0, 1 << q, (B, dec.l)).astype(np.uint8))
    w = words.copy()
    r = np.abs(1.0 + 0.4 * rng.standard_normal((B, n))).astype(np.float32)
    r[:, ::7] = np.float32(0.5)  # equal keys in every frame
    for f in range(B):
        ne = min(int(rng.integers(0, 2 * t + 2)), n)
        pos = rng.choice(n, ne, replace=False)
        for p in pos:
            w[f, p] ^= int(rng.integers(1, 1 << q))
        if f % 3:
            r[f, pos] = (0.3 * rng.random(ne)).astype(np.float32)
            r[f, pos[::4]] = np.float32(0.0)
    r *= rng.choice(np.array([-1.0, 1.0], np.float32), r.shape)  # the sign is ignored
    r[261:269] = np.float32(0.75)
    r[269:277] = np.float32(0.0)
    r[269:273] = np.float32(-0.0)
    r[277:285] = (r[277:285] * np.float32(1e-42)).astype(np.float32)
    r[285:293] = np.float32(3e38) * np.sign(r[285:293])
    r = np.ascontiguousarray(r, np.float32)
    assert np.isfinite(r).all() and (np.abs(r[277:285]) < TINY).all()
    w.setflags(write=False)
    r.setflags(write=False)
    return dict(dec=dec, w=w, r=r, words=words, cand=M.candidates(dec, w, r))


def same(got, want, rows, what):
    for k in ("out", "nerr", "status"):
        assert np.array_equal(np.asarray(got[k].cpu()), want[k][:rows]), (what, k)
    assert np.array_equal(got["metric"].cpu().numpy().view(np.uint32), want["metric"][:rows].view(np.uint32)), (what, "metric")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_equals_model(case):
    import torch
    q, t, N, mu = case
    bt = batches(*case)
    code = make(q, t, N, mu)
    w, r = torch.from_numpy(bt["w"].copy()).cuda(), torch.from_numpy(bt["r"].copy()).cuda()
    total = w.shape[0]
    for m in trial_counts(t):
        want = M.pick(bt["cand"], m)
        F = M.frames_per_wave(2 * t, code.n, m)
        for B in sorted({1, F - 1, F, F + 1, 257, total} - {0}):
            same(code.correct_batch(w[:B], gmd=m, reliability=r[:B]), want, B, (case, m, B))
        if m == t + 1:
            assert (want["status"] == M.FRAME_OK).all()  # trial t decodes on erasures alone
            same(code.correct_batch(w, gmd=True, reliability=r), want, total, (case, "all"))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_model_batches_exercise_the_rules(case):
    """what makes the comparison above worth something, asserted on the model alone"""
    q, t, N, mu = case
    bt = batches(*case)
    cand = bt["cand"]
    full, one = M.pick(cand, t + 1), M.pick(cand, 1)
    assert (full["winner"] > 0).sum() >= 20 and (one["status"] == M.FRAME_LOCATOR).sum() >= 20
    assert (one["status"] == M.FRAME_OK).sum() >= 20
    if t > 1:
        assert np.unique(full["winner"]).size >= 3
    top = slice(285, 293)
    inf = np.isinf(cand["M"][top]) & cand["ok"][top]
    assert inf.any() and not np.isnan(cand["M"]).any()
    if t >= 3:  # (eight frames of a seven-symbol code need not hold one)
        assert (inf.sum(axis=1) >= 2).any()  # a tie at +inf, decided for the smallest tau
    den = full["metric"][277:285]
    assert (den < TINY).all() and (den > 0).any()  # a kernel that flushed denormals would report 0


@pytest.mark.parametrize("tag", [cc.peterson_gorenstein_zierler_tag, cc.euklid_tag], ids=["pgz", "euklid"])
@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[5], CASES[7], CASES[9], CASES[16]],
                         ids=[IDS[i] for i in (0, 2, 5, 7, 9, 16)])
def test_m1_is_hard_decoding_and_the_tag_does_not_matter(case, tag):
    import torch
    q, t, N, mu = case
    bt = batches(*case)
    w, r = torch.from_numpy(bt["w"].copy()).cuda(), torch.from_numpy(bt["r"].copy()).cuda()
    code = make(q, t, N, mu, tag)
    got = {k: v.cpu().numpy() for k, v in code.correct_batch(w, gmd=1, reliability=r).items()}
    hard = {k: v.cpu().numpy() for k, v in make(q, t, N, mu, cc.peterson_gorenstein_zierler_tag).correct_batch(w).items()}
    ok = hard["status"] == M.FRAME_OK
    assert np.array_equal(got["status"] == M.FRAME_OK, ok) and ok.any() and not ok.all()
    assert np.array_equal(got["out"][ok], hard["out"][ok]) and np.array_equal(got["nerr"][ok], hard["nerr"][ok])
    assert np.array_equal(got["out"][~ok], bt["w"][~ok]) and (got["nerr"][~ok] == -1).all()
    assert (got["status"][~ok] == M.FRAME_LOCATOR).all() and (got["metric"][~ok].view(np.uint32) == 0).all()
    m = (t + 2) // 2
    same(code.correct_batch(w, gmd=m, reliability=r), M.pick(bt["cand"], m), w.shape[0], (case, "tag"))


def test_host_pointers_equal_device_pointers():
    """numpy (pageable and page-locked) against torch, with the staging chunk forced small in a process of its own (the
    value is read once): 200 frames of n = 255 in chunks of 31"""
    here = os.path.dirname(os.path.abspath(__file__))
    script = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import numpy as np, torch\n"
        "import channelcoding_amd as cc\n"
        "rng = np.random.default_rng(5)\n"
        "for q, t, N, mu in ((8, 8, None, 0), (4, 3, 11, 1)):\n"
        "    code = cc.rs(q, cc.errors(t), cc.berlekamp_massey_tag(), mu=mu, **({} if N is None else {'n': N}))\n"
        "    w = np.asarray(code.encode_batch(rng.integers(0, 1 << q, (200, code.l)).astype(np.uint8))).copy()\n"
        "    r = np.abs(1.0 + 0.4 * rng.standard_normal((200, code.n))).astype(np.float32)\n"
        "    for f in range(200):\n"
        "        pos = rng.choice(code.n, int(rng.integers(0, 2 * t + 2)), replace=False)\n"
        "        w[f, pos] ^= rng.integers(1, 1 << q, pos.size).astype(np.uint8)\n"
        "        r[f, pos[: pos.size - f %% 3]] *= np.float32(0.2)\n"
        "    pw, pr = torch.from_numpy(w).pin_memory().numpy(), torch.from_numpy(r).pin_memory().numpy()\n"
        "    for m in (1, t // 2 + 1, True):\n"
        "        dev = code.correct_batch(torch.from_numpy(w.copy()).cuda(), gmd=m, reliability=torch.from_numpy(r.copy()).cuda())\n"
        "        dev = {k: v.cpu().numpy() for k, v in dev.items()}\n"
        "        assert (dev['status'] == 0).any() and (dev['nerr'] > 0).any()\n"
        "        for sw, sr in ((w, r), (pw, pr)):\n"
        "            host = code.correct_batch(sw, gmd=m, reliability=sr)\n"
        "            assert sorted(host) == ['metric', 'nerr', 'out', 'status']\n"
        "            for k in host:\n"
        "                assert host[k].dtype == dev[k].dtype and np.array_equal(host[k].view(np.uint8), dev[k].view(np.uint8)), (m, k)\n"
        "        dec = code.decode_batch(w, gmd=m, reliability=r)\n"
        "        assert np.array_equal(dec['out'], dev['out']) and np.array_equal(dec['msg'], code.extract_batch(dev['out']))\n"
        "    bad = w.copy(); bad[3, 2] = 255\n"
        "    if q < 8:\n"
        "        try:\n"
        "            code.correct_batch(bad, gmd=1, reliability=r); raise SystemExit('symbol outside the field accepted')\n"
        "        except cc.CcError as e:\n"
        "            assert e.status == cc.capi.ERR_NOT_IN_FIELD\n"
        "print('GMD HOST OK')\n" % (here, os.path.dirname(here)))
    env = dict(os.environ, CC_AMD_HOST_CHUNK_BYTES="40000")
    out = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "GMD HOST OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


# ---- a wavefront's second group of frames ----
SECOND = [(3, 2, None, 1, 3), (4, 3, None, 1, 4), (8, 8, None, 0, 9), (8, 16, None, 1, 17)]


@pytest.mark.parametrize("q,t,N,mu,m", SECOND, ids=["%s-m%d" % (name(c[:4]), c[4]) for c in SECOND])
def test_second_visit_of_a_wavefront(q, t, N, mu, m):
    """more than twice the frames one pass of the grid takes, so that every wavefront meets a second and some a third
    group in the LDS region (W, R, the E list, the BM columns) that the group before has left"""
    import torch
    # launch_gmd caps the grid at num_cus * 8 workgroups of 4 wavefronts
    W = 32 * torch.cuda.get_device_properties(0).multi_processor_count
    dec = M.Decoder(q, t, N, mu)
    n = dec.n
    F = M.frames_per_wave(2 * t, n, m)
    B = 2 * W * F + 37 * F + 3
    rng = np.random.default_rng(7000 + 100 * q + m)
    pool = 512
    words = dec.encode(rng.integers(0, 1 << q, (pool, dec.l)).astype(np.uint8))
    w = words[rng.integers(0, pool, B)].copy()
    r = np.abs(1.0 + 0.4 * rng.standard_normal((B, n))).astype(np.float32)
    K = min(2 * t + 1, n)  # 0 .. K symbol errors per frame at distinct positions, low reliabilities there in three of four
    ne = rng.integers(0, K + 1, B)
    pos = np.argpartition(rng.random((B, n), dtype=np.float32), K - 1, axis=1)[:, :K]
    hit, rows = np.arange(K)[None, :] < ne[:, None], np.arange(B)[:, None]
    w[rows, pos] ^= rng.integers(1, 1 << q, (B, K)).astype(np.uint8) * hit
    r[rows, pos] *= np.where(hit & (np.arange(B) % 4 != 0)[:, None], np.float32(0.2), np.float32(1.0))
    code = make(q, t, N, mu)
    dw, dr = torch.from_numpy(w).cuda(), torch.from_numpy(r).cuda()
    res = code.correct_batch(dw, gmd=m, reliability=dr)
    got = {k: v.cpu().numpy() for k, v in res.items()}

    # the model on a subset
    pick = np.zeros(B, bool)
    pick[:: max(97, B // 150)] = True
    pick[W * F - F: W * F + 2 * F] = True
    pick[2 * W * F - F: 2 * W * F + 2 * F] = True
    pick[B - (40 if t > 8 else 200):] = True
    idx = np.flatnonzero(pick)
    assert idx.size <= 1500
    want = M.gmd(dec, w[idx], r[idx], m)
    for k in ("out", "nerr", "status"):
        bad = (got[k][idx] != want[k]).reshape(idx.size, -1).any(axis=1)
        assert not bad.any(), (k, idx[bad][:8])
    assert np.array_equal(got["metric"][idx].view(np.uint32), want["metric"].view(np.uint32))
    later = idx >= W * F  # without these the comparison beyond the first pass proves nothing
    assert (want["winner"][later] > 0).sum() >= 5
    if m == t + 1:
        assert (got["status"] == M.FRAME_OK).all()

    # no state carries from group to group: the call on a prefix and the call on the rest give the same
    head = code.correct_batch(dw[: W * F], gmd=m, reliability=dr[: W * F])
    tail = code.correct_batch(dw[W * F:], gmd=m, reliability=dr[W * F:])
    for k in ("out", "nerr", "status", "metric"):
        assert torch.equal(torch.cat([head[k], tail[k]]).view(torch.uint8), res[k].view(torch.uint8)), k

    # every frame: a codeword where the status says so, with the metric and nerr of the contract
    ok = got["status"] == M.FRAME_OK
    assert set(np.unique(got["status"])) <= {M.FRAME_OK, M.FRAME_LOCATOR} and ok.any()
    chk = code.correct_batch(res["out"][torch.from_numpy(ok).cuda()])
    assert int((chk["status"] != 0).sum()) == 0 and int(chk["nerr"].sum()) == 0
    assert np.array_equal(got["out"][~ok], w[~ok]) and (got["nerr"][~ok] == -1).all()
    assert np.array_equal((got["out"] != w).sum(axis=1)[ok], got["nerr"][ok])
    step = max(1, B // 20000)
    assert np.array_equal(M.metric(r[::step], w[::step], got["out"][::step]).view(np.uint32),
                          got["metric"][::step].view(np.uint32))


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


def gmd_dev(torch, code, w, r, m, out, nerr, metric, status, B):
    ptr = lambda a: None if a is None else C.c_void_p(a.data_ptr())
    rc = capi.lib().cc_correct_gmd_batch_dev(code._h, ptr(w), ptr(r), m, ptr(out), ptr(nerr), ptr(metric), ptr(status), B, None)
    capi.check(rc, "cc_correct_gmd_batch_dev")
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", [CASES[2], CASES[8]], ids=[IDS[2], IDS[8]])
def test_optional_outputs_and_offset_buffers(case):
    import torch
    q, t, N, mu = case
    bt = batches(*case)
    B, m, n = 200, (t + 2) // 2, bt["dec"].n
    code = make(q, t, N, mu)
    w, r = torch.from_numpy(bt["w"][:B].copy()).cuda(), torch.from_numpy(bt["r"][:B].copy()).cuda()
    full = code.correct_batch(w, gmd=m, reliability=r)
    same(full, M.pick(bt["cand"], m), B, (case, "full"))
    kinds = dict(nerr=torch.int32, metric=torch.float32, status=torch.int32)
    for mask in range(8):
        passed = [k for i, k in enumerate(kinds) if (mask >> i) & 1]
        bufs = {k: guarded(torch, B, kinds[k]) for k in passed}
        out_whole, out = guarded(torch, B * n, torch.uint8)
        args = {k: bufs[k][1] if k in bufs else None for k in kinds}  # an output not passed has no buffer at all
        gmd_dev(torch, code, w, r, m, out, args["nerr"], args["metric"], args["status"], B)
        assert torch.equal(out.view(B, n), full["out"]) and guards_intact(torch, out_whole), (mask, "out")
        for k in passed:
            assert torch.equal(bufs[k][1].view(torch.uint8), full[k].view(torch.uint8)), (mask, k)
            assert guards_intact(torch, bufs[k][0]), (mask, k)
    # words and out one byte, rel one float into larger allocations (rows of an odd n are misaligned anyway)
    w_big = torch.zeros(B * n + 1, dtype=torch.uint8, device="cuda")
    w_big[1:] = w.reshape(-1)
    r_big = torch.zeros(B * n + 1, dtype=torch.float32, device="cuda")
    r_big[1:] = r.reshape(-1)
    out_big = torch.full((B * n + 2,), SENTINEL, dtype=torch.uint8, device="cuda")
    wo, ro, out = w_big[1:], r_big[1:], out_big[1: 1 + B * n]
    assert wo.data_ptr() % 2 == 1 and ro.data_ptr() % 8 == 4 and out.data_ptr() % 2 == 1
    nerr, status = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    metric = torch.empty(B, dtype=torch.float32, device="cuda")
    gmd_dev(torch, code, wo, ro, m, out, nerr, metric, status, B)
    assert int(out_big[0]) == SENTINEL and int(out_big[-1]) == SENTINEL
    want = {k: v.cpu().numpy() for k, v in full.items()}
    same(dict(out=out.view(B, n), nerr=nerr, status=status, metric=metric), want, B, (case, "offset"))


# ---- channel ----
def channel(code, ebno, seed, first, frames, random_cw=True):
    import torch
    w = torch.empty((frames, code.n), dtype=torch.uint8, device="cuda")
    rel = torch.empty((frames, code.n), dtype=torch.float32, device="cuda")
    sent = torch.empty((frames, code.n), dtype=torch.uint8, device="cuda")
    rc = capi.lib().cc_awgn_symbols_dev(code._h, float(ebno), seed, first, frames, int(random_cw), C.c_void_p(w.data_ptr()),
                                        C.c_void_p(rel.data_ptr()), C.c_void_p(sent.data_ptr()), None)
    capi.check(rc, "cc_awgn_symbols_dev")
    torch.cuda.synchronize()
    return w, rel, sent


def bits_of(sym, q):
    """(B, n) symbols -> (B, n q) bits, bit b of symbol i at i q + b"""
    return ((sym[:, :, None] >> np.arange(q, dtype=np.uint8)[None, None, :]) & 1).reshape(sym.shape[0], -1).astype(np.uint8)


def channel_model(code, ebno, seed, first, frames, sent):
    """y_ref (frames, n, q) float64 of the words sent, and the band"""
    sig = sigma_f32(code, ebno)
    y_ref = awgn_reference(code.n * code.q, sig, seed, first, frames, bits_of(sent, code.q))
    return y_ref.reshape(frames, code.n, code.q), tau(sig)


CHANNEL_CASES = [(3, 2, None, 1), (4, 3, None, 1), (5, 4, None, 1), (6, 8, None, 1), (7, 4, None, 1), (8, 16, None, 1),
                 (8, 8, 204, 0)]


@pytest.mark.parametrize("words", ["zero", "random"])
@pytest.mark.parametrize("case", CHANNEL_CASES, ids=[name(c) for c in CHANNEL_CASES])
def test_channel_equals_float64_model(case, words):
    q, t, N, mu = case
    code = make(q, t, N, mu)
    seed = (7 << 32) + 99
    for ebno, first, frames in ((3.0, (1 << 32) - 700, 1500), (6.0, (5 << 40) + 17, 300)):
        w, rel, sent = (a.cpu().numpy() for a in channel(code, ebno, seed, first, frames, words == "random"))
        if words == "zero":
            assert not sent.any()
        else:
            msgs = rs_message_symbols(seed, first, frames, code.l, q)
            if mu == 1:
                orc = Oracle(RS, q, t)
                full = np.zeros((frames, orc.l), np.uint8)
                full[:, : code.l] = msgs
                assert np.array_equal(sent, orc.encode(full)[:, : code.n])  # the oracle's encoding
            chk = code.correct_batch(sent)
            assert not chk["status"].any() and not chk["nerr"].any()
            assert np.array_equal(np.asarray(code.extract_batch(sent)), msgs)
        y_ref, band = channel_model(code, ebno, seed, first, frames, sent)
        rel_ref = np.abs(y_ref).min(axis=2)
        err = np.abs(rel.astype(np.float64) - rel_ref)
        assert err.max() <= band, (float(err.max()), band)
        assert (rel >= 0).all()
        sure = (np.abs(y_ref) > band).all(axis=2)
        w_ref = ((y_ref < 0).astype(np.uint32) << np.arange(q, dtype=np.uint32)).sum(axis=2).astype(np.uint8)
        assert np.array_equal(w[sure], w_ref[sure])
        assert (~sure).mean() <= 1e-3
    # a frame's draw depends only on (seed, global frame)
    import torch
    a = channel(code, 4.0, 5, 100, 300, True)
    b1, b2 = channel(code, 4.0, 5, 100, 123, True), channel(code, 4.0, 5, 223, 177, True)
    for x, y1, y2 in zip(a, b1, b2):
        assert torch.equal(x.view(torch.uint8), torch.cat([y1, y2]).view(torch.uint8))


# ---- Monte-Carlo ----
def mc(code, m, ebno, seed, first, frames, random_cw=True):
    return GmdBackend(code, m, random_cw).run(ebno, seed, first, frames).cpu().numpy()


def composed(code, m, ebno, seed, first, frames, random_cw=True):
    """the counters by their definition: channel call, decoder call and a comparison, on the device"""
    import torch
    w, rel, sent = channel(code, ebno, seed, first, frames, random_cw)
    res = code.correct_batch(w, gmd=m, reliability=rel)
    wrong = (res["out"] != sent).sum(dim=1)
    failed = res["status"] != M.FRAME_OK
    pop = torch.tensor([bin(v).count("1") for v in range(256)], dtype=torch.int64, device="cuda")
    expect = np.zeros(capi.MC_NCOUNTERS, np.int64)
    expect[capi.MC_FRAMES] = frames
    expect[capi.MC_WORD_ERRORS] = int((failed | (wrong > 0)).sum())
    expect[capi.MC_BIT_ERRORS] = int(wrong.sum())
    expect[capi.MC_FAILURES] = int(failed.sum())
    expect[capi.MC_UNDETECTED] = int((~failed & (wrong > 0)).sum())
    expect[capi.MC_CHANNEL_BIT_ERRORS] = int(pop[(w ^ sent).long()].sum())
    return expect, (w, rel, sent, res)


def test_mc_across_a_chunk_boundary_equals_the_composition_and_its_shards():
    code = make(4, 3)
    seed, first, frames, ebno = 99, (1 << 34) + 11, (1 << 20) + 4096, 5.0  # the chunk of the Monte-Carlo calls is 2^20
    for m in (2, True):
        got = mc(code, m, ebno, seed, first, frames)
        expect, _ = composed(code, m, ebno, seed, first, frames)
        assert np.array_equal(got, expect), (got[:8], expect[:8])
        assert expect[capi.MC_WORD_ERRORS] > 0 and got[capi.MC_ITER_SUM] == 0 and not got[capi.MC_ITER_HIST:].any()
        assert got[capi.MC_CHANNEL_ERASURES] == 0
        if m is True:
            assert got[capi.MC_FAILURES] == 0 and got[capi.MC_UNDETECTED] == got[capi.MC_WORD_ERRORS]
    total = np.zeros_like(got)
    for rank in range(3):
        lo, cnt = shard(frames, rank, 3)
        total += mc(code, True, ebno, seed, first + lo, cnt)
    assert np.array_equal(total, got)


@pytest.mark.parametrize("case,m,random_cw", [((4, 3, None, 1), 4, True), ((8, 8, 204, 0), 5, True), ((5, 4, None, 1), 2, False)],
                         ids=["rs15-9", "rs204-188-mu0", "rs31-23-zero"])
def test_mc_counters_against_the_models(case, m, random_cw):
    """the decoder's share against tests/gmd_model.py, the channel's bit errors by the band rule: the float64 model's
    hard decisions outside the band, the device's inside it"""
    q, t, N, mu = case
    code = make(q, t, N, mu)
    seed, first, frames, ebno = 31, 1 << 33, 1200 if q == 8 else 4000, 5.0
    got = mc(code, m, ebno, seed, first, frames, random_cw)
    expect, (w, rel, sent, res) = composed(code, m, ebno, seed, first, frames, random_cw)
    assert np.array_equal(got, expect), (got[:8], expect[:8])
    w, rel, sent = w.cpu().numpy(), rel.cpu().numpy(), sent.cpu().numpy()
    assert sent.any() == random_cw
    want = M.gmd(M.Decoder(q, t, N, mu), w, rel, m)
    same(res, want, frames, (case, "mc"))
    y_ref, band = channel_model(code, ebno, seed, first, frames, sent)
    y_ref = y_ref.reshape(frames, -1)
    inside, bits, dev = np.abs(y_ref) <= band, bits_of(sent, q) != 0, bits_of(w, q) != 0
    model = int((((y_ref < 0) != bits) & ~inside).sum()) + int(((dev != bits) & inside).sum())
    assert got[capi.MC_CHANNEL_BIT_ERRORS] == model == int((dev != bits).sum()) > 0


def test_mc_gmd_lowers_the_word_error_rate():
    code = make(4, 3)
    frames = 1 << 15
    hard, soft = mc(code, 1, 5.0, 5, 0, frames), mc(code, code.t + 1, 5.0, 5, 0, frames)
    assert hard[capi.MC_FRAMES] == soft[capi.MC_FRAMES] == frames
    assert hard[capi.MC_CHANNEL_BIT_ERRORS] == soft[capi.MC_CHANNEL_BIT_ERRORS] > 0  # the same channel
    assert soft[capi.MC_WORD_ERRORS] < hard[capi.MC_WORD_ERRORS]  # (the CPU model: 76 against 141 in 3000 frames)
