"""GPU tests of the soft-aided staircase decoder (cc_staircase_decode_sr): the device byte for byte and int
for int against tests/staircase_sr_model.py under the buffer contract of tests/guarded_buffers.py (guard elements around
every output, the least alignment of every buffer, every subset of the optional outputs absent, two poisons around the
input); host against device pointers in small staging chunks; a stream of the caller's own; the channel of values against
cc_awgn_staircase_dev's signs and cc_awgn_product_dev's draws; the Monte-Carlo counters against channel + model + count.

The batches are those of tests/test_staircase_sr_host.py (CASES, SCHEDULES and SWEEP there;
test_model_batches_are_not_degenerate holds what they are chosen for).  The tiles are those of
tests/test_gpu_staircase.py, the smallest at which each mapping of the kernel can go wrong -- m7, m8e, m15, m16e (several
steps in a wavefront, one and two syndromes), m31, m32e (the widest one-register lines), m63, m64e (the four-register
kernel; W = 2 has empty odd half-passes), m127, m128e (two wavefronts per step, rows of five dwords) -- and m128e_t15_w4,
which asks for more LDS than the default limit of a workgroup.  Each runs under the schedules rising to infinity,
constant, non-monotone, (0, 0, inf, inf), I = 1, fifteen distinct weights at I = 8 (four level planes) and 130
half-passes (the levels travel through the workspace pool)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import capi
import staircase_model as SM
import staircase_sr_model as SR
from guarded_buffers import check_call
from test_staircase_sr_host import (CASES, INF, SCHEDULES, SWEEP_SCHEDULES, SWEEP_TILES, SWEEP_WINDOWS, batch, case, channel,
                                    model, sweep_case, sweep_lengths)

pytestmark = pytest.mark.gpu


def handle(q, t, N=None):
    kw = {} if N is None else {"n": N}
    return cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag(), **kw)


def code_of(name, iters, blocks=None):
    (q, t, N), extended, W, L = CASES[name][:4]
    return cc.staircase_code(handle(q, t, N), L if blocks is None else blocks, W, iters, extended=extended)


def decode_checked(sc, y, weights, want, what=""):
    """cc_staircase_decode_sr_dev under the buffer contract: every subset of (nflip, status) absent in turn"""
    B = y.shape[0]
    desc = sc._sc()
    w = np.array(weights, np.float32)

    def call(p):
        return capi.lib().cc_staircase_decode_sr_dev(C.byref(desc), w.ctypes.data_as(C.c_void_p), p["y"], p["out"], p["nflip"],
                                                     p["status"], B, p["stream"])

    check_call(call, {"y": np.ascontiguousarray(y)}, {"out": (np.uint8, y.size), "nflip": (np.int32, B), "status": (np.int32, B)},
               want, optional=("nflip", "status"), what=what)


def on_device(sc, y, weights):
    import torch
    return {k: v.cpu().numpy() for k, v in sc.correct_sr_batch(torch.from_numpy(np.array(y)).cuda(), weights).items()}


def same(got, want, what):
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)


@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_model(name, schedule):
    y = batch(name, schedule)
    w = SCHEDULES[schedule]
    decode_checked(code_of(name, len(w) // 2, y.shape[1]), y, w, model(name, schedule)[0], what=(name, schedule))


@pytest.mark.parametrize("W", SWEEP_WINDOWS)
@pytest.mark.parametrize("tile", sorted(SWEEP_TILES))
def test_every_window_iteration_count_and_stream_length(tile, W):
    (q, t, N), extended, _ = SWEEP_TILES[tile]
    code = handle(q, t, N)
    for I, w in SWEEP_SCHEDULES.items():
        for L in sweep_lengths(W):
            y, want = sweep_case(tile, W, I, L)
            same(on_device(cc.staircase_code(code, L, W, I, extended=extended), y, w), want, (tile, W, I, L))


@pytest.mark.parametrize("name", ["m7", "m16e", "m63", "m128e"])
def test_special_values(name):
    """-0.0, NaN, +inf and -inf planted in y, and |y| set to exactly a weight of the schedule at a fiftieth of the
    positions: ties, which revert"""
    dec, extended, sent, y = case(name)
    y = np.array(y)
    rng = np.random.default_rng(3)
    flat = y.reshape(-1)
    for v in (-0.0, np.nan, np.inf, -np.inf):
        flat[rng.integers(0, flat.size, max(4, flat.size // 500))] = v
    w = (0.5, 0.9, 1.3, INF)
    for tie in w[:3]:
        at = rng.integers(0, flat.size, flat.size // 150)
        flat[at] = np.where(flat[at] < 0, -tie, tie).astype(np.float32)
    W = CASES[name][2]
    trace = []
    want = SR.decode(dec, y, w, W, 2, extended, trace)
    assert sum(int(r["reverted"].sum()) for r in trace) > 0 and want["nflip"].max() > 0
    decode_checked(code_of(name, 2), y, w, want, what=name)


@pytest.mark.parametrize("B", [1, 2])
def test_one_and_two_streams(B):
    for name in ("m8e", "m31", "m64e", "m127"):
        y = case(name)[3][:B]
        want = {k: v[:B] for k, v in model(name, "rising")[0].items()}
        same(on_device(code_of(name, 2), y, SCHEDULES["rising"]), want, (name, B))


def test_python_calls_on_both_sides_and_an_empty_batch():
    import torch
    name = "m16e"
    dec, extended, sent, y = case(name)
    w = SCHEDULES["nonmonotone"]
    want = model(name, "nonmonotone")[0]
    sc = code_of(name, 3)
    same(on_device(sc, y, w), want, name)
    host = sc.decode_sr_batch(np.array(y), w)
    same(host, want, name)
    assert np.array_equal(host["msg"], SM.extract(dec, want["out"], extended))
    desc = sc._sc()
    fw = (C.c_float * 6)(*w)
    assert capi.lib().cc_staircase_decode_sr_dev(C.byref(desc), fw, None, None, None, None, 0, None) == capi.OK
    assert capi.lib().cc_staircase_decode_sr(C.byref(desc), fw, None, None, None, None, 0) == capi.OK
    assert capi.lib().cc_awgn_staircase_values_dev(C.byref(desc), 3.0, 1, 0, 0, 1, None, None, None) == capi.OK
    counters = torch.zeros(capi.MC_NCOUNTERS, dtype=torch.int64, device="cuda")
    assert capi.lib().cc_mc_run_staircase_sr_dev(C.byref(desc), fw, 3.0, 1, 0, 0, 1, C.c_void_p(counters.data_ptr()), None) == capi.OK
    assert capi.lib().cc_mc_run_staircase_sr_dev(C.byref(desc), fw, 3.0, 1, 0, 4, 1, None, None) == capi.ERR_INVALID_ARGUMENT
    assert not counters.any()
    # a window that does not fit is refused on a handle with a device too
    big = cc.staircase_code(handle(8, 2), 3, 16, 2, extended=True)
    with pytest.raises(cc.CcError) as e:
        big.correct_sr_batch(torch.zeros((1, 3, 128, 128), device="cuda"), SCHEDULES["rising"])
    assert e.value.status == capi.ERR_UNSUPPORTED


def test_a_stream_of_the_callers_own():
    import torch
    name = "m32e"
    y = torch.from_numpy(np.array(case(name)[3])).cuda()
    sc = code_of(name, 2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = sc.correct_sr_batch(y, SCHEDULES["rising"])
    side.synchronize()
    same({k: v.cpu().numpy() for k, v in got.items()}, model(name, "rising")[0], name)


@pytest.mark.parametrize("tile,W,L", [("m7", 3, 5), ("m8e", 4, 4)])
def test_second_and_third_stream_of_a_workgroup(tile, W, L):
    """twice as many streams as the largest grid has workgroups and 77 more: a workgroup decodes a second and a third
    stream over the tiles, planes, states and copies of the one before.  The model decodes a prefix, a stretch around an
    odd cut and the suffix; the two parts, decoded on their own, equal the whole"""
    import torch
    (q, t, N), extended, p = SWEEP_TILES[tile]
    dec = SM.decoder(q, t, N)
    cap = 8 * torch.cuda.get_device_properties(0).multi_processor_count
    B = 2 * cap + 77
    rng = np.random.default_rng(77)
    few = channel(dec, extended, L, p, 256, 77)[1]
    y = few[rng.integers(0, 256, B)]
    y = (y * rng.uniform(0.5, 1.5, y.shape)).astype(np.float32)  # the same hard decisions, other reliabilities
    w = SWEEP_SCHEDULES[2]
    cut = (cap + cap // 3) | 1
    pick = np.unique(np.concatenate([np.arange(40), np.arange(cut - 20, cut + 20), np.arange(B - 40, B)]))
    want = SR.decode(dec, y[pick], w, W, 2, extended)
    late = pick >= cap
    assert late.sum() >= 80 and set(want["status"][late].tolist()) == {SR.FRAME_OK, SR.FRAME_NOT_CONVERGED}
    sc = cc.staircase_code(handle(q, t, N), L, W, 2, extended=extended)
    yd = torch.from_numpy(y).cuda()
    whole = {k: v.cpu().numpy() for k, v in sc.correct_sr_batch(yd, w).items()}
    same({k: v[pick] for k, v in whole.items()}, want, (tile, "whole"))
    for lo, hi in ((0, cut), (cut, B)):
        part = {k: v.cpu().numpy() for k, v in sc.correct_sr_batch(yd[lo:hi], w).items()}
        same(part, {k: v[lo:hi] for k, v in whole.items()}, (tile, lo))


def run_child(script, env, marker):
    here = os.path.dirname(os.path.abspath(__file__))
    head = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n" % (here, os.path.dirname(here))
    out = subprocess.run([sys.executable, "-c", head + script], env=dict(os.environ, **env), capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0 and marker in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_host_pointers_equal_device_pointers_in_small_staging_chunks():
    """the staging chunk forced small in a process of its own (the value is read once): 70 streams of 5 x 31 x 31 floats in
    chunks of 16 and 300 of 6 x 8 x 8, pageable and page-locked memory"""
    run_child(
        "import numpy as np, torch\n"
        "import channelcoding_amd as cc\n"
        "rng = np.random.default_rng(8)\n"
        "mk = lambda q, t, **kw: cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag(), **kw)\n"
        "W = (0.5, 0.9, 1.3, float('inf'))\n"
        "for sc, B, s in ((cc.staircase_code(mk(6, 2, n=62), 5, 3, 2), 70, 0.47), (cc.staircase_code(mk(4, 1), 6, 4, 2, extended=True), 300, 0.58)):\n"
        "    sent = sc.encode_batch(rng.integers(0, 2, (B, sc.blocks, sc.m, sc.k_b)).astype(np.uint8))\n"
        "    y = ((1.0 - 2.0 * sent) + s * rng.standard_normal(sent.shape)).astype(np.float32)\n"
        "    pinned = torch.from_numpy(y.copy()).pin_memory().numpy()\n"
        "    dev = {k: v.cpu().numpy() for k, v in sc.correct_sr_batch(torch.from_numpy(y.copy()).cuda(), W).items()}\n"
        "    assert dev['nflip'].any() and len(set(dev['status'].tolist())) == 2\n"
        "    for src in (y, pinned):\n"
        "        host = sc.correct_sr_batch(src, W)\n"
        "        for k in dev:\n"
        "            assert host[k].dtype == dev[k].dtype and np.array_equal(host[k], dev[k]), k\n"
        "print('STAIRCASE SR HOST OK')\n", {"CC_AMD_HOST_CHUNK_BYTES": str(16 * 5 * 31 * 31 * 4)}, "STAIRCASE SR HOST OK")


def test_channel_values_have_the_signs_of_the_hard_channel_and_the_draws_of_the_product_channel():
    """y of cc_awgn_staircase_values_dev: (y < 0) is what cc_awgn_staircase_dev writes, byte for byte, the streams sent
    are the same, and value v of stream g is cc_awgn_product_dev's draw for value v of block g, rescaled to the staircase's
    sigma (tests/test_gpu_staircase.py holds the same for the hard channel)"""
    import torch
    sc = cc.staircase_code(handle(4, 1, 14), 9, 3, 1)  # 9 * 49 = 441 = 21 * 21 values per stream
    pc = cc.product_code(handle(5, 1, 21), handle(5, 1, 21))
    assert pc.n == sc.n
    for first, streams in ((0, 6), (5, 3)):
        noise = (pc.channel(2.5, 99, first, streams)["y"].cpu().numpy().reshape(streams, -1) - 1.0) / np.float32(pc.sigma(2.5))
        sigma = np.float32(sc.sigma(2.5))
        for rc in (False, True):
            soft, hard = sc.channel(2.5, 99, first, streams, rc, values=True), sc.channel(2.5, 99, first, streams, rc)
            assert set(soft) == {"y", "sent"} and soft["y"].dtype == torch.float32 and soft["y"].shape == hard["z"].shape
            assert torch.equal(soft["sent"], hard["sent"]) and bool(soft["sent"].any()) == rc
            assert torch.equal((soft["y"] < 0).to(torch.uint8), hard["z"])
            centre = 1.0 - 2.0 * soft["sent"].cpu().numpy().reshape(streams, -1).astype(np.float32)
            assert np.allclose(soft["y"].cpu().numpy().reshape(streams, -1), centre + sigma * noise, rtol=0, atol=2e-6)
        if first == 5:  # the streams of a later call are those of the first at the same global index
            assert torch.equal(soft["y"][:1], first_y[5:6])
        else:
            first_y = soft["y"]


# ---- Monte-Carlo ----
def counted(want, sent, y, L, W):
    """the counters of the streams given, by the definitions of the header: over the blocks 1 .. L_c, the channel's flips
    from the signs of y"""
    B = sent.shape[0]
    Lc = SM.counted_blocks(L, W)
    wrong = (want["out"][:, :Lc] != sent[:, :Lc]).reshape(B, -1).sum(axis=1)
    failed = want["status"] != SM.FRAME_OK
    c = np.zeros(capi.MC_NCOUNTERS, np.int64)
    c[capi.MC_FRAMES] = B
    c[capi.MC_WORD_ERRORS] = int((failed | (wrong > 0)).sum())
    c[capi.MC_BIT_ERRORS] = int(wrong.sum())
    c[capi.MC_FAILURES] = int(failed.sum())
    c[capi.MC_UNDETECTED] = int((~failed & (wrong > 0)).sum())
    c[capi.MC_CHANNEL_BIT_ERRORS] = int((SR.hard(y)[:, :Lc] != sent[:, :Lc]).sum())
    return c


def mc(sc, w, ebno, seed, first, streams, random_codewords=True):
    from channelcoding_amd.montecarlo import StaircaseSrBackend
    return StaircaseSrBackend(sc, w, random_codewords).run(ebno, seed, first, streams).cpu().numpy()


@pytest.mark.parametrize("q,t,N,extended,L,W,ebno,streams", [(4, 1, 14, False, 9, 4, 4.0, 256), (5, 2, None, True, 3, 4, 3.0, 96)],
                         ids=["m7_L9_W4", "m16e_L3_W4"])
@pytest.mark.parametrize("random_codewords", [True, False], ids=["random", "zero"])
def test_mc_counters_against_channel_model_and_count(q, t, N, extended, L, W, ebno, streams, random_codewords):
    """two codes, one with L >= W (six counted blocks of nine) and one with a stream shorter than the window (all three
    counted); the counters lie between guard elements; two adjacent ranges of unequal size sum to the whole"""
    import torch
    from guarded_buffers import guarded, guards_intact
    dec = SM.decoder(q, t, N)
    w = SCHEDULES["rising"]
    sc = cc.staircase_code(handle(q, t, N), L, W, 2, extended=extended)
    seed, first = 2026, (1 << 33) + 5
    ch = sc.channel(ebno, seed, first, streams, random_codewords, values=True)
    y, sent = ch["y"].cpu().numpy(), ch["sent"].cpu().numpy()
    assert bool(sent.any()) == random_codewords
    want = SR.decode(dec, y, w, W, 2, extended)
    expect = counted(want, sent, y, L, W)
    print(expect[:8])
    assert expect[capi.MC_WORD_ERRORS] > 0 and expect[capi.MC_FAILURES] > 0 and expect[capi.MC_BIT_ERRORS] > 0
    assert 0 < expect[capi.MC_CHANNEL_BIT_ERRORS] and (L < W or expect[capi.MC_CHANNEL_BIT_ERRORS] < (SR.hard(y) != sent).sum())
    assert not expect[capi.MC_ITER_SUM] and not expect[capi.MC_ITER_HIST:].any()
    wc, counters = guarded(torch, capi.MC_NCOUNTERS, np.int64)
    counters.zero_()
    desc = sc._sc()
    fw = (C.c_float * 4)(*w)
    rc = capi.lib().cc_mc_run_staircase_sr_dev(C.byref(desc), fw, ebno, seed, first, streams, int(random_codewords),
                                               C.c_void_p(counters.data_ptr()), None)
    capi.check(rc, "cc_mc_run_staircase_sr_dev")
    torch.cuda.synchronize()
    assert guards_intact(torch, wc, counters)
    got = counters.cpu().numpy()
    assert np.array_equal(got, expect), (got, expect)
    cut = streams // 3
    shards = mc(sc, w, ebno, seed, first, cut, random_codewords) + mc(sc, w, ebno, seed, first + cut, streams - cut, random_codewords)
    assert np.array_equal(shards, expect)


def test_mc_counters_across_a_chunk_boundary():
    """the chunk of the product routes forced small in a process of its own (the value is read once): 100 streams of
    6 x 8 x 8 in chunks of ten; counters = channel + decode call + count"""
    run_child(
        "import numpy as np, torch\n"
        "import channelcoding_amd as cc\n"
        "from channelcoding_amd import capi\n"
        "from channelcoding_amd.montecarlo import StaircaseSrBackend\n"
        "W = (0.5, 0.9, 1.3, float('inf'))\n"
        "sc = cc.staircase_code(cc.primitive_bch(4, cc.errors(1), cc.berlekamp_massey_tag()), 6, 3, 2, extended=True)\n"
        "seed, first, B, ebno = 7, 1000, 100, 3.5\n"
        "ch = sc.channel(ebno, seed, first, B, True, values=True)\n"
        "one = torch.cat([sc.channel(ebno, seed, first + g, 1, True, values=True)['y'] for g in (0, 9, 10, 11, 99)])\n"
        "assert torch.equal(one, ch['y'][[0, 9, 10, 11, 99]])\n"
        "res = sc.correct_sr_batch(ch['y'], W)\n"
        "Lc = 4\n"
        "wrong = (res['out'][:, :Lc] != ch['sent'][:, :Lc]).reshape(B, -1).sum(dim=1).cpu().numpy()\n"
        "failed = res['status'].cpu().numpy() != 0\n"
        "c = np.zeros(capi.MC_NCOUNTERS, np.int64)\n"
        "c[capi.MC_FRAMES], c[capi.MC_BIT_ERRORS], c[capi.MC_FAILURES] = B, wrong.sum(), failed.sum()\n"
        "c[capi.MC_WORD_ERRORS], c[capi.MC_UNDETECTED] = (failed | (wrong > 0)).sum(), (~failed & (wrong > 0)).sum()\n"
        "c[capi.MC_CHANNEL_BIT_ERRORS] = int(((ch['y'][:, :Lc] < 0).to(torch.uint8) != ch['sent'][:, :Lc]).sum())\n"
        "got = StaircaseSrBackend(sc, W, True).run(ebno, seed, first, B).cpu().numpy()\n"
        "assert np.array_equal(got, c) and c[capi.MC_FAILURES] > 0 and c[capi.MC_FAILURES] < B, (got, c)\n"
        "print('STAIRCASE SR MC OK')\n", {"CC_AMD_PRODUCT_MC_CHUNK_VALUES": str(10 * 6 * 64)}, "STAIRCASE SR MC OK")
