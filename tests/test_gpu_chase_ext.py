"""GPU tests of Chase decoding of extended BCH codes: cc_correct_chase_extended_batch(_dev) bit for bit
against tests/chase_ext_model.py -- out, nerr, status, metric and ext (compared as u32), hard output (ext NULL) and soft
output; the parity position at lane 63 and lane 0 of every position register; a wavefront's second group of frames;
absent outputs, guard elements and odd offsets; the host-pointer against the device entry point; the plain soft call on
the inner values; and cc.product_decode(extended=True) on device tensors against the model's loop."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import capi
import chase_ext_model as E
import chase_model as M
import chase_soft_model as S
from checkers import awgn_llr
from test_chase_ext_host import extended_product_batch
from test_chase_soft_host import ALPHA, BETA, P
from test_gpu_chase_soft import (SENTINEL, between_two_codewords, guarded, guards_intact, make, quantised, scaled,
                                 to_host)

pytestmark = pytest.mark.gpu

# (q, t, N, Eb/N0 found with the model on the CPU so that the batch below is not degenerate)
CASES = [(3, 1, None, 3.0),    # BCH(7,4) -> (8,4)
         (4, 2, None, 3.0),    # BCH(15,7) -> (16,7)
         (5, 1, None, 3.0),    # BCH(31,26) -> (32,26)
         (6, 1, None, 4.0),    # BCH(63,57) -> (64,57): the parity position is lane 63 of the first register
         (6, 2, None, 4.0),    # BCH(63,51) -> (64,51)
         (7, 2, None, 4.5),    # BCH(127,113) -> (128,113)
         (8, 3, None, 5.0),    # BCH(255,231) -> (256,231): the parity position is the last slot of the 4 x 64 mapping
         (8, 8, None, 4.0),    # BCH(255,191) -> (256,191): t = 8, the root search from the LDS column
         (6, 4, None, 3.0),    # BCH(63,39) -> (64,39): t = 4, the LDS column with one syndrome reduction
         # shortened GF(2^8) codes: the parity position on lane 63 and on lane 0 of each register
         (8, 3, 63, 4.0), (8, 3, 64, 4.0), (8, 3, 127, 4.5), (8, 3, 128, 4.5), (8, 3, 191, 5.0), (8, 3, 192, 5.0),
         (3, 1, 5, 3.0), (3, 1, 6, 3.0)]  # p = n
IDS = ["bch%d-t%d%s" % (q, t, "" if N is None else "-N%d" % N) for q, t, N, _ in CASES]
PS = (0, 1, 3, 6)
BETAS = (0.5, 0.0)


def frames_per_wave(code, p, soft):
    """F of launch_chase_extended, asked of the library: 64 >> p, fewer where LDS bounds it"""
    F = capi.lib().cc_chase_extended_frames_per_wavefront(code._h, p, int(soft))
    assert 1 <= F <= 64 >> p
    return F


def weak_parity(y):
    """every fifth frame: y_n is the smallest magnitude of the row, of either sign -- it must not be picked as L_0"""
    y = y.copy()
    rows = np.arange(2, y.shape[0], 5)
    least = np.abs(y[rows, :-1]).min(axis=1)
    y[rows, -1] = np.where(rows % 2 == 0, np.float32(0.25), np.float32(-0.25)) * least
    return y


@functools.lru_cache(maxsize=None)
def batches(q, t, N, ebno):
    """300 frames of n + 1 values of one code -- AWGN on extended codewords, quantised, -2 dB; for BCH(255,191) forty of
    the AWGN frames give way to frames between two codewords -- and the model's candidates for all 64 patterns, made once"""
    dec = M.decoder(q, t, N)
    rng = np.random.default_rng(3000 * q + 10 * t + (N or 0))
    sizes = (200, 50, 50)
    words = E.extend(dec.encode(rng.integers(0, 2, (sizes[0] + sizes[2], dec.l)).astype(np.uint8)))
    rate = dec.l / (dec.n + 1)
    y = np.concatenate([awgn_llr(rng, words[: sizes[0]], rate, ebno), quantised(rng, (sizes[1], dec.n + 1)),
                        awgn_llr(rng, words[sizes[0]:], rate, -2.0)])
    if (q, t, N) == (8, 8, None):  # spread over the groups of every F; the parity value of either sign, weak and strong
        y[3:163:4, : dec.n] = between_two_codewords(rng, dec, 40)
        y[3:163:4, dec.n] = rng.choice(np.array([-0.9, -0.07, 0.07, 0.9], np.float32), 40)
    y = np.ascontiguousarray(weak_parity(y), np.float32)
    y.setflags(write=False)
    return dict(dec=dec, y=y, cand=E.candidates(dec, y))


def same(got, want, rows, what, ext=True):
    got = to_host(got) if not isinstance(got["out"], np.ndarray) else got
    for k in ("out", "nerr", "status"):
        assert np.array_equal(got[k], want[k][:rows]), (what, k)
    assert np.array_equal(got["metric"].view(np.uint32), want["metric"][:rows].view(np.uint32)), (what, "metric")
    if ext:
        bad = np.argwhere(got["ext"].view(np.uint32) != want["ext"][:rows].view(np.uint32))
        assert bad.size == 0, (what, "ext", bad[:4].tolist())
    else:
        assert "ext" not in got, what


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_equals_model(case, p):
    import torch
    q, t, N, _ = case
    bt = batches(*case)
    n = bt["dec"].n
    p = min(p, n)  # a frame of five inner positions: p = 6 stands for p = n
    code = make(q, t, N)
    y = torch.from_numpy(bt["y"].copy()).cuda()
    total = y.shape[0]
    assert y.shape[1] == n + 1
    hard = M.pick(bt["cand"], p)
    F = frames_per_wave(code, p, False)
    for B in sorted({1, max(F - 1, 1), F + 1, total}):
        got = code.correct_batch(y[:B], chase=p, extended=True)
        assert sorted(got) == ["metric", "nerr", "out", "status"] and tuple(got["out"].shape) == (B, n + 1)
        same(got, hard, B, (case, p, "hard", B), ext=False)
    F = frames_per_wave(code, p, True)
    for beta in BETAS:
        want = S.soft(bt["cand"], p, beta)
        for B in sorted({1, max(F - 1, 1), F + 1, total}):
            got = code.correct_batch(y[:B], chase=p, soft=beta, extended=True)
            assert sorted(got) == ["ext", "metric", "nerr", "out", "status"] and got["ext"].dtype == torch.float32
            same(got, want, B, (case, p, beta, B))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_model_batches_are_not_degenerate(case):
    """what makes the comparison above worth something, asserted on the model alone over the four values of p together:
    the parity position with a competitor and without one, flipped by the winner and kept, frames without a candidate,
    winners other than pattern 0, and frames in which the parity value changes the inner word -- the plain model on the
    inner values picks another one.  The weakest value of a row is never a test position where it is y_n."""
    bt = batches(*case)
    dec, y, cand = bt["dec"], bt["y"], bt["cand"]
    n = dec.n
    weakest = np.abs(y).argmin(axis=1) == n
    assert weakest.sum() >= 50 and (cand["L"] < n).all()
    inner = M.candidates(dec, np.ascontiguousarray(y[:, :n]))
    with_, without, flipped, lost, late, moved = 0, 0, 0, 0, 0, 0
    for p in PS:
        r = S.soft(cand, min(p, n), 0.5)
        won = r["winner"] >= 0
        with_ += (r["has"][:, n] & won).sum()
        without += (~r["has"][:, n] & won).sum()
        flipped += (won & (r["out"][:, n] != cand["z"][:, n])).sum()
        lost += (~won).sum()
        late += (r["winner"] > 0).sum()
        plain = M.pick(inner, min(p, n))
        moved += (won & (plain["out"] != r["out"][:, :n]).any(axis=1)).sum()
        assert (r["ext"][~won].view(np.uint32) == 0).all()
        assert np.array_equal(r["out"][~won], cand["z"][~won])
    assert with_ >= 20 and without >= 20 and flipped >= 20 and late >= 5, (with_, without, flipped, late)
    assert lost >= 5 or (case[1] == 1 and case[2] is None), lost  # (a Hamming code has no frame without a candidate)
    # (the words of a heavily shortened code lie too far apart for one value to move the decision between them)
    assert moved >= 3 or case[2] is not None, moved


# ---- denormals, values near FLT_MAX ----
def parity_huge(y):
    """y_n at +-3.3e38 in every frame and position 0 as large in every third: a candidate that flips one of them has a
    metric near FLT_MAX, one that flips both has +inf -- ties at +inf go to the smallest j"""
    y = y.copy()
    y[:, -1] = np.where(y[:, -1] < 0, np.float32(-3.3e38), np.float32(3.3e38))
    y[::3, 0] = np.where(y[::3, 0] < 0, np.float32(-3.3e38), np.float32(3.3e38))
    return y


@pytest.mark.parametrize("kind", ["denormal", "parity_huge", "mixed"])
@pytest.mark.parametrize("case", [CASES[4], CASES[8], CASES[6]], ids=["bch6-t2", "bch6-t4", "bch8-t3"])
def test_denormal_and_huge_values(case, kind):
    """out, nerr, metric and status are the model's whatever the magnitudes, +inf among the metrics included; where every
    metric of a frame is finite ext is the model's as well -- a kernel that flushed denormals could not pass"""
    import torch
    q, t, N, _ = case
    bt = batches(*case)
    y_host = parity_huge(bt["y"]) if kind == "parity_huge" else scaled(bt["y"], kind)
    assert np.isfinite(y_host).all()
    if kind == "denormal":
        assert (np.abs(y_host) < np.finfo(np.float32).tiny).all() and (y_host != 0).mean() > 0.9
    code = make(q, t, N)
    y = torch.from_numpy(y_host.copy()).cuda()
    with np.errstate(over="ignore"):
        cand = E.candidates(bt["dec"], y_host)
    infinite = denormal_ext = 0
    for p in (0, 2, 6):
        with np.errstate(over="ignore", invalid="ignore"):
            want = S.soft(cand, p, 0.5)
        hard = code.correct_batch(y, chase=p, extended=True)
        soft = code.correct_batch(y, chase=p, soft=0.5, extended=True)
        same(hard, want, y.shape[0], (case, kind, p, "hard"), ext=False)
        got = to_host(soft)
        same({k: v for k, v in got.items() if k != "ext"}, want, y.shape[0], (case, kind, p), ext=False)
        finite = np.isfinite(np.where(cand["ok"][:, : 1 << p], cand["M"][:, : 1 << p], 0)).all(axis=1)
        infinite += (~finite).sum() + np.isinf(want["metric"]).sum()
        assert finite.all() if kind == "denormal" else finite.any()
        assert np.array_equal(got["ext"][finite].view(np.uint32), want["ext"][finite].view(np.uint32)), (kind, p)
        denormal_ext += (want["has"] & (want["ext"] != 0)).sum()
    # (the batch must hold what the kind is about: denormal differences in ext, infinite metrics)
    assert denormal_ext > 100 if kind == "denormal" else infinite > 0


# ---- a wavefront's second group of frames ----
def second_batch(W, q=5, t=2, ebno=3.0, p=3):
    """B frames of BCH(31,21) extended for a grid of W wavefronts, the subset the model decodes, and its answer on it"""
    dec = M.decoder(q, t)
    n = dec.n
    F = 64 >> p
    B = 2 * W * F + 37 * F + 3
    rng = np.random.default_rng(7300 + 100 * q + p)
    words = E.extend(dec.encode(rng.integers(0, 2, (1024, dec.l)).astype(np.uint8)))
    rate = dec.l / (n + 1)
    y = awgn_llr(rng, words[rng.integers(0, 1024, B)], rate, ebno)
    y[W * F - 2 * F: W * F + 2 * F] = quantised(rng, (4 * F, n + 1))
    low = np.arange(W * F + 5 * F, B, 11)  # frames at -2 dB among the later groups: some have no candidate
    y[low] = awgn_llr(rng, words[rng.integers(0, 1024, low.size)], rate, -2.0)
    y = np.ascontiguousarray(y, np.float32)
    pick = np.zeros(B, bool)
    pick[::397] = True
    pick[W * F - 2 * F: W * F + 4 * F] = True
    pick[2 * W * F - 2 * F: 2 * W * F + 4 * F] = True
    pick[B - 600:] = True
    idx = np.flatnonzero(pick)
    assert idx.size <= 3000
    want = E.chase_soft(dec, y[idx], p, 0.5)
    later = idx >= W * F  # without these the comparison beyond the first pass proves nothing
    assert (want["winner"][later] > 0).sum() >= 5 and want["has"][later][:, n].sum() >= 20
    assert (~want["has"][later][want["winner"][later] >= 0]).sum() >= 50
    return F, p, y, idx, want


def test_second_visit_of_a_wavefront():
    """more than twice the frames one pass of the grid takes, so that every wavefront meets a second and some a third
    group in the LDS region that the group before has left: its Y, K, M_D and the parity byte among the rest"""
    import torch
    W = 32 * torch.cuda.get_device_properties(0).multi_processor_count  # the grid is capped at 8 workgroups of 4 per CU
    F, p, y, idx, want = second_batch(W)
    B, w = y.shape
    code = make(5, 2)
    assert frames_per_wave(code, p, True) == F == frames_per_wave(code, p, False)  # one pass takes exactly W F frames
    assert B > 2 * W * F
    dev = torch.from_numpy(y).cuda()
    res = code.correct_batch(dev, chase=p, soft=0.5, extended=True)
    got = to_host(res)
    same({k: v[idx] for k, v in got.items()}, want, idx.size, "second visit")
    hard = code.correct_batch(dev, chase=p, extended=True)
    for k in ("out", "nerr", "status", "metric"):
        assert torch.equal(hard[k].view(torch.uint8), res[k].view(torch.uint8)), k

    # no state carries from group to group: the call on a prefix and the call on the rest give the same
    head = code.correct_batch(dev[: W * F], chase=p, soft=0.5, extended=True)
    tail = code.correct_batch(dev[W * F:], chase=p, soft=0.5, extended=True)
    for k in ("out", "ext", "nerr", "status", "metric"):
        assert torch.equal(torch.cat([head[k], tail[k]]).view(torch.uint8), res[k].view(torch.uint8)), k

    # every OK frame has even weight; every frame without a candidate is z with +0.0f throughout ext
    lost = got["status"] == M.FRAME_LOCATOR
    assert set(np.unique(got["status"])) <= {M.FRAME_OK, M.FRAME_LOCATOR}
    assert lost[W * F:].sum() >= 1 and (~lost).sum() > B // 2
    assert (got["out"][~lost].sum(axis=1) % 2 == 0).all()
    assert (got["ext"][lost].view(np.uint32) == 0).all()
    assert np.array_equal(got["out"][lost], (y[lost] < 0).astype(np.uint8))
    assert np.isfinite(got["ext"]).all()


# ---- optional outputs, guard elements, buffers at odd addresses ----
def ext_dev(torch, code, llr, p, beta, out, ext, nerr, metric, status, B):
    ptr = lambda a: None if a is None else C.c_void_p(a.data_ptr())
    rc = capi.lib().cc_correct_chase_extended_batch_dev(code._h, ptr(llr), p, C.c_float(beta), ptr(out), ptr(ext),
                                                        ptr(nerr), ptr(metric), ptr(status), B, None)
    capi.check(rc, "cc_correct_chase_extended_batch_dev")
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", [CASES[4], CASES[8]], ids=["bch6-t2", "bch6-t4"])
def test_optional_outputs_guards_and_offset_buffers(case):
    import torch
    q, t, N, _ = case
    bt = batches(*case)
    B, p, w = 200, 3, bt["dec"].n + 1
    code = make(q, t, N)
    y = torch.from_numpy(bt["y"][:B].copy()).cuda()
    full = code.correct_batch(y, chase=p, soft=0.5, extended=True)
    same(full, S.soft(bt["cand"], p, 0.5), B, (case, "full"))
    kinds = dict(nerr=torch.int32, metric=torch.float32, status=torch.int32)
    for mask in range(8):
        for soft in (True, False):
            passed = [k for i, k in enumerate(kinds) if (mask >> i) & 1]
            bufs = {k: guarded(torch, B, kinds[k]) for k in passed}
            out_whole, out = guarded(torch, B * w, torch.uint8)
            ext_whole, ext = guarded(torch, B * w, torch.float32)
            args = {k: bufs[k][1] if k in bufs else None for k in kinds}  # an output not passed has no buffer at all
            # (the hard output reads no beta: a NaN must not matter)
            ext_dev(torch, code, y, p, 0.5 if soft else float("nan"), out, ext if soft else None, args["nerr"],
                    args["metric"], args["status"], B)
            assert torch.equal(out.view(B, w), full["out"]) and guards_intact(torch, out_whole), (mask, soft, "out")
            if soft:
                assert torch.equal(ext.view(B, w).view(torch.uint8), full["ext"].view(torch.uint8)), (mask, "ext")
            else:
                assert bool((ext.view(torch.uint8) == SENTINEL).all()), (mask, "ext untouched")
            assert guards_intact(torch, ext_whole), (mask, soft, "ext")
            for k in passed:
                assert torch.equal(bufs[k][1].view(torch.uint8), full[k].view(torch.uint8)), (mask, soft, k)
                assert guards_intact(torch, bufs[k][0]), (mask, soft, k)
    # llr and ext one float, out one byte into larger allocations
    llr_big = torch.zeros(B * w + 1, dtype=torch.float32, device="cuda")
    llr_big[1:] = y.reshape(-1)
    ext_big = torch.full((B * w + 2,), 7.0, dtype=torch.float32, device="cuda")
    out_big = torch.full((B * w + 2,), SENTINEL, dtype=torch.uint8, device="cuda")
    llr, ext, out = llr_big[1:], ext_big[1: 1 + B * w], out_big[1: 1 + B * w]
    assert llr.data_ptr() % 8 == 4 and ext.data_ptr() % 8 == 4 and out.data_ptr() % 2 == 1
    nerr, status = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    metric = torch.empty(B, dtype=torch.float32, device="cuda")
    ext_dev(torch, code, llr, p, 0.5, out, ext, nerr, metric, status, B)
    assert int(out_big[0]) == SENTINEL and int(out_big[-1]) == SENTINEL
    assert float(ext_big[0]) == 7.0 and float(ext_big[-1]) == 7.0
    got = dict(out=out.view(B, w), ext=ext.view(B, w), nerr=nerr, status=status, metric=metric)
    same(got, to_host(full), B, (case, "offset"))


def test_host_pointers_equal_device_pointers():
    """numpy (pageable and page-locked) against torch, with the staging chunk forced small in a process of its own (the
    value is read once): 200 frames of 256 values in chunks of 39; hard and soft output; decode_batch on top"""
    here = os.path.dirname(os.path.abspath(__file__))
    script = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import numpy as np, torch\n"
        "import channelcoding_amd as cc\n"
        "rng = np.random.default_rng(6)\n"
        "for q, t, N in ((8, 3, None), (6, 3, 50)):\n"
        "    code = cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag(), **({} if N is None else {'n': N}))\n"
        "    y = (1.0 + 0.6 * rng.standard_normal((200, code.n + 1))).astype(np.float32)\n"
        "    pinned = torch.from_numpy(y).pin_memory().numpy()\n"
        "    for p, beta in ((0, 0.5), (4, None), (4, 0.25), (6, 0.0)):\n"
        "        kw = dict(chase=p, extended=True, **({} if beta is None else {'soft': beta}))\n"
        "        keys = ['metric', 'nerr', 'out', 'status'] + ([] if beta is None else ['ext'])\n"
        "        dev = {k: v.cpu().numpy() for k, v in code.correct_batch(torch.from_numpy(y.copy()).cuda(), **kw).items()}\n"
        "        assert sorted(dev) == sorted(keys) and (dev['status'] == 0).any() and (dev['nerr'] > 0).any()\n"
        "        for src in (y, pinned):\n"
        "            host = code.correct_batch(src, **kw)\n"
        "            assert sorted(host) == sorted(keys)\n"
        "            for k in host:\n"
        "                assert host[k].dtype == dev[k].dtype and host[k].shape == dev[k].shape, (p, k)\n"
        "                assert np.array_equal(host[k].view(np.uint8), dev[k].view(np.uint8)), (p, k)\n"
        "        dec = code.decode_batch(y, **kw)\n"
        "        assert np.array_equal(dec['out'], dev['out'])\n"
        "        assert np.array_equal(dec['msg'], code.extract_batch(cc.unextend(dev['out'])))\n"
        "        assert dec['msg'].shape == (200, code.l)\n"
        "print('CHASE EXTENDED HOST OK')\n" % (here, os.path.dirname(here)))
    env = dict(os.environ, CC_AMD_HOST_CHUNK_BYTES="40000")
    out = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "CHASE EXTENDED HOST OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


@pytest.mark.parametrize("case", [CASES[4], CASES[6], CASES[8]], ids=["bch6-t2", "bch8-t3", "bch6-t4"])
def test_zero_at_the_parity_position_leaves_the_inner_decision_to_the_plain_call(case):
    """|y_n| = +0.0f adds nothing to any metric: the inner n columns of out, the metric and the status are those of
    cc_correct_chase_soft_batch_dev on the inner values"""
    import torch
    q, t, N, _ = case
    bt = batches(*case)
    n = bt["dec"].n
    yh = bt["y"].copy()
    yh[:, n] = np.float32(0.0)
    code = make(q, t, N)
    y = torch.from_numpy(yh).cuda()
    inner = y[:, :n].contiguous()
    flips = 0
    for p in (0, 3, 6):
        plain = code.correct_batch(inner, chase=p, soft=0.5)
        for soft in (None, 0.5):
            got = code.correct_batch(y, chase=p, extended=True, **({} if soft is None else {"soft": soft}))
            assert torch.equal(got["out"][:, :n], plain["out"]), (case, p, soft)
            assert torch.equal(got["status"], plain["status"]), (case, p, soft)
            assert torch.equal(got["metric"].view(torch.int32), plain["metric"].view(torch.int32)), (case, p, soft)
            ok = got["status"] == 0
            assert bool((got["out"][ok].sum(dim=1) % 2 == 0).all())
            flips += int((got["nerr"][ok] - plain["nerr"][ok]).sum())  # z_n = 0: the parity bit of an odd inner word
            assert bool(((got["nerr"] - plain["nerr"] == got["out"][:, n].to(torch.int32)) | ~ok).all())
    assert flips > 50


# ---- product decoding ----
def test_product_decode_on_device_tensors_equals_the_model_loop():
    """eBCH(16,11) rows x eBCH(32,26) columns, 64 blocks of 32 x 16 values"""
    import torch
    rows, cols, sent, y = extended_product_batch(4, 1, 5, 1, 3.0, 64, 2017)
    assert y.shape == (64, 32, 16)
    r, c = make(4, 1), make(5, 1)
    steps = E.product_decode(rows, cols, y, P, ALPHA, BETA)
    dev = torch.from_numpy(y.copy()).cuda()
    for halves in (1, 2, 3, 4):
        got = cc.product_decode(r, c, dev, P, ALPHA[:halves], BETA[:halves], extended=True)
        want = steps[halves - 1]
        assert sorted(got) == ["ext", "out", "status"] and got["out"].shape == (64, 32, 16)
        assert np.array_equal(got["out"].cpu().numpy(), want["out"]), halves
        assert np.array_equal(got["status"].cpu().numpy(), want["status"]), halves
        bad = np.argwhere(got["ext"].cpu().numpy().view(np.uint32) != want["ext"].view(np.uint32))
        assert bad.size == 0, (halves, bad[:4].tolist())
    # the numpy route through the host-pointer entry point is the same loop
    host = cc.product_decode(r, c, np.asarray(y), P, ALPHA, BETA, extended=True)
    assert np.array_equal(host["out"], steps[-1]["out"])
    assert np.array_equal(host["ext"].view(np.uint32), steps[-1]["ext"].view(np.uint32))
    errors = [int((s["out"] != sent).any(axis=(1, 2)).sum()) for s in steps]
    assert errors[-1] < errors[0]  # and it does what it is for
