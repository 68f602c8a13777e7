"""GPU tests of the staircase calls (cc_staircase): the sliding-window decoder on the device byte for byte
and int for int against tests/staircase_model.py under the buffer contract of tests/guarded_buffers.py (guard elements
around every output, the least alignment of every buffer, each optional output absent in turn, two poisons around the
input); in place; host against device pointers in small staging chunks; encode and extract against the model; the
channel against cc_awgn_product_dev's draws.

The batches are those of tests/test_staircase_host.py (CASES and SWEEP there; test_model_batches_are_not_degenerate holds
what they are chosen for).  The tiles, the smallest at which each mapping of the kernel can go wrong:
  m7, m8e          BCH(14,10) and eBCH(16,11): the lines-of-64-bits kernel, several steps in one wavefront, a block side
                   that is no multiple of anything; through every window 2, 3, 4, 16, 1 .. 3 iterations and the stream
                   lengths L < W - 1 (one position, a short window), L = W - 1, L = W (the first slide) and L = 2W + 1
                   (the ring wraps twice)
  m15, m16e        q = 5, t = 2: two syndromes per line, lines of 30 / 32 bits
  m31, m32e        lines of 62 / 64 bits: the widest the one-register kernel takes, a step is half a wavefront
  m63, m64e        the four-register kernel; a step is exactly one wavefront of lines (63: one lane short); W = 2 has
                   empty odd half-passes
  m127, m128e      two wavefronts per step, the second one lane short at 127; rows of five dwords, four in use
  m128e_t15_w16    t = 15 next to sixteen blocks of 128 x 128: more LDS than the default limit of a workgroup, eight steps
                   per half-pass in four trips of 256 lanes
Past the first stream of a workgroup: twice the largest grid (8 workgroups per compute unit) and 77 more streams, so that
every workgroup decodes a second and 77 a third stream over the ring, states and columns of the one before."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import capi
import staircase_model as SM
from guarded_buffers import check_call
from test_staircase_host import (CASES, SWEEP_ITERS, SWEEP_STREAMS, SWEEP_TILES, SWEEP_WINDOWS, case, make_batch,
                                 sweep_case, sweep_lengths)

pytestmark = pytest.mark.gpu


def handle(q, t, N=None):
    kw = {} if N is None else {"n": N}
    return cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag(), **kw)


def code_of(name, **replace):
    (q, t, N), extended, W, I, L = CASES[name][:5]
    kw = dict(blocks=L, window=W, iters=I)
    kw.update(replace)
    return cc.staircase_code(handle(q, t, N), extended=extended, **kw)


def decode_checked(sc, z, want, in_place=False, what=""):
    """cc_staircase_decode_dev under the buffer contract: every subset of (nflip, status) absent in turn"""
    B = z.shape[0]
    desc = sc._sc()

    def call(p):
        return capi.lib().cc_staircase_decode_dev(C.byref(desc), p["in"], p["out"], p["nflip"], p["status"], B, p["stream"])

    check_call(call, {"in": np.ascontiguousarray(z)}, {"out": (np.uint8, z.size), "nflip": (np.int32, B), "status": (np.int32, B)},
               want, optional=("nflip", "status"), in_place={"out": "in"} if in_place else None, what=what)


def decode_plain(sc, z):
    import torch
    out, nflip, status = sc.correct_batch(torch.from_numpy(np.array(z)).cuda())
    return dict(out=out.cpu().numpy(), nflip=nflip.cpu().numpy(), status=status.cpu().numpy())


def same(got, want, what):
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_model(name):
    dec, extended, sent, z, want, _ = case(name)
    decode_checked(code_of(name), z, want, what=name)


@pytest.mark.parametrize("name", ["m7", "m16e", "m63", "m128e"])
def test_in_place(name):
    dec, extended, sent, z, want, _ = case(name)
    decode_checked(code_of(name), z, want, in_place=True, what=name)


@pytest.mark.parametrize("W", SWEEP_WINDOWS)
@pytest.mark.parametrize("tile", sorted(SWEEP_TILES))
def test_every_window_iteration_count_and_stream_length(tile, W):
    (q, t, N), extended, _ = SWEEP_TILES[tile]
    code = handle(q, t, N)
    for I in SWEEP_ITERS:
        for L in sweep_lengths(W):
            z, want = sweep_case(tile, W, I, L)
            sc = cc.staircase_code(code, L, W, I, extended=extended)
            same(decode_plain(sc, z), want, (tile, W, I, L))


@pytest.mark.parametrize("B", [1, 2])
def test_one_and_two_streams(B):
    for name in ("m8e", "m31", "m64e", "m127"):
        dec, extended, sent, z, want, _ = case(name)
        same(decode_plain(code_of(name), z[:B]), {k: v[:B] for k, v in want.items()}, (name, B))


@pytest.mark.parametrize("name", ["m7", "m8e", "m32e", "m63", "m128e"])
def test_a_zero_stream_and_a_code_stream_are_left_alone(name):
    sent = case(name)[2]
    z = np.stack([np.zeros_like(sent[0]), sent[0], sent[1]])
    for W, I in ((2, 1), (3, 2), (16, 3)):
        got = decode_plain(code_of(name, window=W, iters=I), z)
        assert np.array_equal(got["out"], z) and not got["nflip"].any() and not got["status"].any(), (name, W, I)


@pytest.mark.parametrize("tile,W,I,L", [("m7", 3, 2, 5), ("m8e", 4, 1, 4)])
def test_second_and_third_stream_of_a_workgroup(tile, W, I, L):
    """twice as many streams as the largest grid has workgroups and 77 more: the model decodes a prefix, a stretch around
    an odd cut past the first trip and the suffix; the two parts, decoded on their own (as other workgroups' first, second
    or third stream), equal the whole"""
    import torch
    (q, t, N), extended, p = SWEEP_TILES[tile]
    dec = SM.decoder(q, t, N)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cap = 8 * cus
    B = 2 * cap + 77
    rng = np.random.default_rng(77)
    few = make_batch(dec, extended, L, 0.0, 256, 77)[0]
    z = few[rng.integers(0, 256, B)]
    z = z ^ (rng.random(z.shape) < p).astype(np.uint8)
    cut = (cap + cap // 3) | 1
    pick = np.unique(np.concatenate([np.arange(50), np.arange(cut - 25, cut + 25), np.arange(B - 50, B)]))
    want = SM.decode(dec, z[pick], W, I, extended)
    late = pick >= cap
    assert late.sum() >= 100 and set(want["status"][late].tolist()) == {SM.FRAME_OK, SM.FRAME_NOT_CONVERGED}
    sc = cc.staircase_code(handle(q, t, N), L, W, I, extended=extended)
    zd = torch.from_numpy(z).cuda()
    whole = [v.cpu().numpy() for v in sc.correct_batch(zd)]
    whole = dict(out=whole[0], nflip=whole[1], status=whole[2])
    same({k: v[pick] for k, v in whole.items()}, want, (tile, "whole"))
    for lo, hi in ((0, cut), (cut, B)):
        part = [v.cpu().numpy() for v in sc.correct_batch(zd[lo:hi])]
        same(dict(out=part[0], nflip=part[1], status=part[2]), {k: v[lo:hi] for k, v in whole.items()}, (tile, lo))


def test_python_calls_on_both_sides_and_an_empty_batch():
    import torch
    name = "m16e"
    dec, extended, sent, z, want, _ = case(name)
    sc = code_of(name)
    dev = sc.correct_batch(torch.from_numpy(np.array(z)).cuda())
    host = sc.correct_batch(np.array(z))
    for got in (dict(zip(("out", "nflip", "status"), (v.cpu().numpy() for v in dev))), dict(zip(("out", "nflip", "status"), host))):
        same(got, want, name)
    msg, nflip, status = sc.decode_batch(np.array(z))
    assert np.array_equal(msg, SM.extract(dec, want["out"], extended)) and np.array_equal(nflip, want["nflip"])
    bad = np.array(z)
    bad[3, 2, 1, 0] = 2  # a value that is no bit: the host form refuses it
    with pytest.raises(cc.CcError) as e:
        sc.correct_batch(bad)
    assert e.value.status == capi.ERR_NOT_IN_FIELD
    desc = sc._sc()
    assert capi.lib().cc_staircase_decode_dev(C.byref(desc), None, None, None, None, 0, None) == capi.OK
    assert capi.lib().cc_staircase_decode(C.byref(desc), None, None, None, None, 0) == capi.OK
    assert capi.lib().cc_staircase_encode_batch_dev(C.byref(desc), None, None, 0, None) == capi.OK
    assert capi.lib().cc_awgn_staircase_dev(C.byref(desc), 3.0, 1, 0, 0, 1, None, None, None) == capi.OK


@pytest.mark.parametrize("q,t,N,extended,L", [(4, 1, 14, False, 5), (4, 1, None, True, 4), (6, 2, 62, False, 3),
                                               (7, 2, None, True, 3), (8, 2, 254, False, 2), (8, 15, None, True, 2)])
def test_encode_and_extract_equal_the_model(q, t, N, extended, L):
    import torch
    dec = SM.decoder(q, t, N)
    sc = cc.staircase_code(handle(q, t, N), L, 2, 1, extended=extended)
    rng = np.random.default_rng(11)
    B = 5
    msg = rng.integers(0, 2, (B, L, sc.m, sc.k_b)).astype(np.uint8)
    want = SM.encode(dec, msg, extended)
    desc = sc._sc()

    def enc(p):
        return capi.lib().cc_staircase_encode_batch_dev(C.byref(desc), p["msg"], p["cw"], B, p["stream"])

    def ext(p):
        return capi.lib().cc_staircase_extract_batch_dev(C.byref(desc), p["cw"], p["msg"], B, p["stream"])

    check_call(enc, {"msg": msg}, {"cw": (np.uint8, want.size)}, {"cw": want}, what="encode")
    check_call(ext, {"cw": want}, {"msg": (np.uint8, msg.size)}, {"msg": msg}, what="extract")
    assert np.array_equal(sc.encode_batch(msg), want) and np.array_equal(sc.extract_batch(want), msg)  # the host forms
    assert np.array_equal(sc.extract_batch(sc.encode_batch(torch.from_numpy(msg).cuda())).cpu().numpy(), msg)


def test_channel_equals_the_product_channel_re_indexed():
    """value v of stream g is what cc_awgn_product_dev draws for value v of block g at the same sigma: a product code
    whose block has as many values as a stream and the same rate would give y, and z = (y < 0).  No product has both in
    general, so the draws are taken at the product's own sigma and rescaled: y = s (1 - 2 sent) + sigma noise."""
    import torch
    code = handle(4, 1, 14)
    sc = cc.staircase_code(code, 9, 3, 1)  # 9 * 49 = 441 = 21 * 21 values per stream
    pc = cc.product_code(handle(5, 1, 21), handle(5, 1, 21))
    assert pc.n == sc.n
    for first, streams in ((0, 6), (5, 3)):
        zero = sc.channel(2.5, 99, first, streams)
        y = pc.channel(2.5, 99, first, streams)["y"].cpu().numpy().reshape(streams, -1)
        noise = (y - 1.0) / np.float32(pc.sigma(2.5))
        assert not zero["sent"].any()
        rnd = sc.channel(2.5, 99, first, streams, random_codewords=True)
        sent = rnd["sent"].cpu().numpy()
        assert (SM.status(SM.decoder(4, 1, 14), sent, False) == SM.FRAME_OK).all() and sent.any()
        sigma = np.float32(sc.sigma(2.5))
        for got, s in ((zero["z"], np.zeros_like(sent)), (rnd["z"], sent)):
            centre = 1.0 - 2.0 * s.reshape(streams, -1).astype(np.float32)
            want = (centre + sigma * noise) < 0
            differ = got.cpu().numpy().reshape(streams, -1) != want
            # (the rescaling rounds: a value within a few ulp of zero may fall on the other side)
            assert differ.sum() <= 1 and not (differ & (np.abs(centre + sigma * noise) > 1e-5)).any()
        if first == 5:  # the streams of a later call are those of the first at the same global index
            assert torch.equal(rnd["sent"][:1], first_sent[5:6]) and torch.equal(rnd["z"][:1], first_z[5:6])
        else:
            first_sent, first_z = rnd["sent"], rnd["z"]
    # the messages are those of frame g of a code with l = L m k_b
    msg = sc.extract_batch(first_sent).cpu().numpy()
    assert 0.3 < msg.mean() < 0.7


def run_child(script, env, marker):
    here = os.path.dirname(os.path.abspath(__file__))
    head = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n" % (here, os.path.dirname(here))
    out = subprocess.run([sys.executable, "-c", head + script], env=dict(os.environ, **env), capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0 and marker in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_host_pointers_equal_device_pointers_in_small_staging_chunks():
    """the staging chunk forced small in a process of its own (the value is read once): 70 streams of 5 x 31 x 31 in
    chunks of 16 and 300 of 6 x 8 x 8, pageable and page-locked memory, separate buffers and in place"""
    run_child(
        "import ctypes as C\n"
        "import numpy as np, torch\n"
        "import channelcoding_amd as cc\n"
        "from channelcoding_amd import capi\n"
        "rng = np.random.default_rng(8)\n"
        "mk = lambda q, t, **kw: cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag(), **kw)\n"
        "vp = lambda a: a.ctypes.data_as(C.c_void_p)\n"
        "for sc, B, p in ((cc.staircase_code(mk(6, 2, n=62), 5, 3, 2), 70, 0.02), (cc.staircase_code(mk(4, 1), 6, 4, 2, extended=True), 300, 0.04)):\n"
        "    sent = sc.encode_batch(rng.integers(0, 2, (B, sc.blocks, sc.m, sc.k_b)).astype(np.uint8))\n"
        "    z = sent ^ (rng.random(sent.shape) < p).astype(np.uint8)\n"
        "    pinned = torch.from_numpy(z.copy()).pin_memory().numpy()\n"
        "    dev = [v.cpu().numpy() for v in sc.correct_batch(torch.from_numpy(z.copy()).cuda())]\n"
        "    assert dev[1].any() and len(set(dev[2].tolist())) == 2\n"
        "    for src in (z, pinned):\n"
        "        host = sc.correct_batch(src)\n"
        "        for h, d in zip(host, dev):\n"
        "            assert h.dtype == d.dtype and np.array_equal(h, d)\n"
        "    buf = z.copy()\n"
        "    desc = sc._sc()\n"
        "    status = np.zeros(B, np.int32)\n"
        "    rc = capi.lib().cc_staircase_decode(C.byref(desc), vp(buf), vp(buf), None, vp(status), B)\n"
        "    assert rc == 0 and np.array_equal(buf, dev[0]) and np.array_equal(status, dev[2])\n"
        "print('STAIRCASE HOST OK')\n", {"CC_AMD_HOST_CHUNK_BYTES": str(16 * 5 * 31 * 31)}, "STAIRCASE HOST OK")


# ---- Monte-Carlo ----
def counted(want, sent, z, L, W):
    """the counters of the streams given, by the definitions of the header: over the blocks 1 .. L_c"""
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
    c[capi.MC_CHANNEL_BIT_ERRORS] = int((z[:, :Lc] != sent[:, :Lc]).sum())
    return c


def mc(sc, ebno, seed, first, streams, random_codewords=True):
    from channelcoding_amd.montecarlo import StaircaseBackend
    return StaircaseBackend(sc, random_codewords).run(ebno, seed, first, streams).cpu().numpy()


@pytest.mark.parametrize("q,t,N,extended,L,W,I,ebno,streams", [(4, 1, 14, False, 9, 4, 2, 5.0, 256), (5, 2, None, True, 3, 4, 2, 4.0, 96)],
                         ids=["m7_L9_W4", "m16e_L3_W4"])
@pytest.mark.parametrize("random_codewords", [True, False], ids=["random", "zero"])
def test_mc_counters_against_channel_model_and_count(q, t, N, extended, L, W, I, ebno, streams, random_codewords):
    """two codes, one with L >= W (six counted blocks of nine) and one with a stream shorter than the window (all three
    counted); the counters lie between guard elements; two shards of unequal size sum to the whole"""
    import torch
    from guarded_buffers import guarded, guards_intact
    dec = SM.decoder(q, t, N)
    sc = cc.staircase_code(handle(q, t, N), L, W, I, extended=extended)
    seed, first = 2026, (1 << 33) + 5
    ch = sc.channel(ebno, seed, first, streams, random_codewords)
    z, sent = ch["z"].cpu().numpy(), ch["sent"].cpu().numpy()
    assert bool(sent.any()) == random_codewords
    want = SM.decode(dec, z, W, I, extended)
    expect = counted(want, sent, z, L, W)
    assert expect[capi.MC_WORD_ERRORS] > 0 and expect[capi.MC_FAILURES] > 0 and expect[capi.MC_BIT_ERRORS] > 0
    assert 0 < expect[capi.MC_CHANNEL_BIT_ERRORS] and (L < W or expect[capi.MC_CHANNEL_BIT_ERRORS] < (z != sent).sum())
    assert not expect[capi.MC_ITER_SUM] and not expect[capi.MC_ITER_HIST:].any()
    wc, counters = guarded(torch, capi.MC_NCOUNTERS, np.int64)
    counters.zero_()
    desc = sc._sc()
    rc = capi.lib().cc_mc_run_staircase_dev(C.byref(desc), ebno, seed, first, streams, int(random_codewords),
                                            C.c_void_p(counters.data_ptr()), None)
    capi.check(rc, "cc_mc_run_staircase_dev")
    torch.cuda.synchronize()
    assert guards_intact(torch, wc, counters)
    got = counters.cpu().numpy()
    assert np.array_equal(got, expect), (got, expect)
    cut = streams // 3
    shards = mc(sc, ebno, seed, first, cut, random_codewords) + mc(sc, ebno, seed, first + cut, streams - cut, random_codewords)
    assert np.array_equal(shards, expect)
    assert capi.lib().cc_mc_run_staircase_dev(C.byref(desc), ebno, seed, first, 0, 1, C.c_void_p(counters.data_ptr()), None) == capi.OK
    assert capi.lib().cc_mc_run_staircase_dev(C.byref(desc), ebno, seed, first, 4, 1, None, None) == capi.ERR_INVALID_ARGUMENT


def test_mc_counters_across_a_chunk_boundary():
    """the chunk of the product routes forced small in a process of its own (the value is read once): 100 streams of
    6 x 8 x 8 in chunks of ten, the channel call in the same chunks; counters = channel + decode call + count"""
    run_child(
        "import numpy as np, torch\n"
        "import channelcoding_amd as cc\n"
        "from channelcoding_amd import capi\n"
        "from channelcoding_amd.montecarlo import StaircaseBackend\n"
        "sc = cc.staircase_code(cc.primitive_bch(4, cc.errors(1), cc.berlekamp_massey_tag()), 6, 3, 2, extended=True)\n"
        "seed, first, B, ebno = 7, 1000, 100, 4.5\n"
        "ch = sc.channel(ebno, seed, first, B, True)\n"
        "one = torch.cat([sc.channel(ebno, seed, first + g, 1, True)['z'] for g in (0, 9, 10, 11, 99)])\n"
        "assert torch.equal(one, ch['z'][[0, 9, 10, 11, 99]])\n"
        "out, nflip, status = sc.correct_batch(ch['z'])\n"
        "Lc = 4\n"
        "wrong = (out[:, :Lc] != ch['sent'][:, :Lc]).reshape(B, -1).sum(dim=1).cpu().numpy()\n"
        "failed = status.cpu().numpy() != 0\n"
        "c = np.zeros(capi.MC_NCOUNTERS, np.int64)\n"
        "c[capi.MC_FRAMES], c[capi.MC_BIT_ERRORS], c[capi.MC_FAILURES] = B, wrong.sum(), failed.sum()\n"
        "c[capi.MC_WORD_ERRORS], c[capi.MC_UNDETECTED] = (failed | (wrong > 0)).sum(), (~failed & (wrong > 0)).sum()\n"
        "c[capi.MC_CHANNEL_BIT_ERRORS] = int((ch['z'][:, :Lc] != ch['sent'][:, :Lc]).sum())\n"
        "got = StaircaseBackend(sc, True).run(ebno, seed, first, B).cpu().numpy()\n"
        "assert np.array_equal(got, c) and c[capi.MC_FAILURES] > 0 and c[capi.MC_FAILURES] < B, (got, c)\n"
        "print('STAIRCASE MC OK')\n", {"CC_AMD_PRODUCT_MC_CHUNK_VALUES": str(10 * 6 * 64)}, "STAIRCASE MC OK")
