"""GPU tests of iterated hard-decision decoding of product codes (cc_product_decode_hard): the device byte
for byte and int for int against tests/product_hard_model.py after 1, 2, 3 and 8 half-iterations, with guard elements
around every output; in place; outputs left out one at a time; odd byte offsets; host against device pointers in small
staging chunks; every hard tag; the Monte-Carlo counters against channel + model + count, sharded and chunked.

The batches are those of tests/test_product_hard_host.py (CASES there; test_model_batches_are_not_degenerate holds what
they are chosen for).  The shapes, the smallest at which each mapping of the kernel can go wrong:
  7_4x7_4 (grid stride)     several blocks per workgroup, more blocks than the grid has wavefronts
  15_11x15_7                15 x 15, one dword per row, different t per side; B = 1, 2, 67
  e16_11xe32_26             two fields, extended, non-square
  s40_22x15_7               ragged dwords (40 bits in two), the shortened rule
  63_45x63_45               t = 3, one wavefront at 63 lines
  e64_51xe64_51             exactly 64 lines
  127_113x15_11             the first workgroup-per-block shape: 127 column lines, a half-filled second wavefront
  e256_239xe8_4 and its turn  256 lines of 8 bits, 8 lines of 256
  255_239x255_239           bit index no multiple of 32
  e256_239xe256_239 (_noisy)  the full block, converging and not
  255_131x15_11             2t = 32 on one side: the largest Berlekamp-Massey columns
  255_131x255_239           2t = 32 next to a block of 255 lines: more LDS than the default limit of a workgroup
Past the first block of a workgroup (TRIPS there, sized from the device's compute units) and past 8 half-iterations
(LONG there):
  127_113x7_4 and its turn  twice the largest grid of the workgroup-per-block kernel and 77 more: a second and a third
                            block in the same LDS, wavefronts without a line
  63_45x63_45 (trips)       the same for a wavefront of the other kernel, 63 of 64 lanes, t = 3
  15_11x15_11 (long)        56, 57 and 60 half-iterations, blocks in a cycle with `last` = halves; in the Monte-Carlo
                            route the last histogram slot at 55 and 60, and three blocks per wavefront of the count"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import capi
from channelcoding_amd.montecarlo import ProductHardBackend
import product_hard_model as PH
from test_gpu_chase_soft import GUARD, SENTINEL, guarded, guards_intact  # noqa: F401
from test_product_hard_host import (CASES, HALVES, LONG_HALVES, TRIP_HALVES, TRIPS, case, encode_blocks, long_case,
                                    long_outputs, model_outputs, trips_batch, trips_batch_is_not_degenerate)

pytestmark = pytest.mark.gpu

TAGS = {"bm": cc.berlekamp_massey_tag, "pgz": cc.peterson_gorenstein_zierler_tag, "euklid": cc.euklid_tag}


def handle(q, t, N=None, tag="bm"):
    kw = {} if N is None else {"n": N}
    return cc.primitive_bch(q, cc.errors(t), TAGS[tag](), **kw)


def product_of(name, tag="bm"):
    r, c, extended = CASES[name][:3]
    return cc.product_code(handle(*r, tag=tag), handle(*c, tag=tag), extended=extended)


def ptr(a):
    return None if a is None else C.c_void_p(a.data_ptr())


def decode_dev(pc, z, halves, in_place=False, leave_out=()):
    """cc_product_decode_hard_dev itself on the host array z (B, n2, n1), every output between guard elements"""
    import torch
    desc = pc._pc_hard(halves)
    B = z.shape[0]
    wi, zin = guarded(torch, B * pc.n, torch.uint8)
    zin.copy_(torch.from_numpy(np.array(z)).cuda().reshape(-1))
    wo, out = guarded(torch, B * pc.n, torch.uint8)
    small = {k: guarded(torch, B, torch.int32) for k in ("nflip", "last", "status")}
    args = {k: (None if k in leave_out else ptr(v[1])) for k, v in small.items()}
    rc = capi.lib().cc_product_decode_hard_dev(C.byref(desc), ptr(zin), ptr(zin if in_place else out), args["nflip"],
                                               args["last"], args["status"], B, None)
    capi.check(rc, "cc_product_decode_hard_dev")
    torch.cuda.synchronize()
    assert guards_intact(torch, wi) and guards_intact(torch, wo) and all(guards_intact(torch, v[0]) for v in small.values())
    if in_place:
        assert bool((wo == SENTINEL).all())
    else:
        assert np.array_equal(zin.cpu().numpy().reshape(z.shape), z)
    for k in leave_out:
        assert bool((small[k][0].view(torch.uint8) == SENTINEL).all()), k
    got = {k: v[1].cpu().numpy() for k, v in small.items() if k not in leave_out}
    got["out"] = (zin if in_place else out).cpu().numpy().reshape(z.shape)
    return got


def same(got, want, what):
    for k in got:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)


@pytest.mark.parametrize("halves", [1, 2, 3, HALVES])
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_model(name, halves):
    z = case(name)[4]
    same(decode_dev(product_of(name), z, halves), model_outputs(name, halves), (name, halves))


@pytest.mark.parametrize("B", [1, 2])
def test_one_and_two_blocks(B):
    for name in ("15_11x15_7", "e64_51xe64_51", "127_113x15_11"):
        z = case(name)[4][:B]
        for halves in (2, HALVES):
            same(decode_dev(product_of(name), z, halves), model_outputs(name, halves, slice(0, B)), (name, B, halves))


def test_grid_stride_and_several_blocks_per_workgroup():
    """BCH(7,4)^2 with more blocks than the largest grid has wavefronts (8 workgroups of four per compute unit): every
    wavefront makes several trips.  The model decodes a prefix, a stretch around a cut and a suffix; the two parts,
    decoded on their own, equal the whole."""
    import torch
    pc = product_of_codes((3, 1, None), (3, 1, None), False)
    dec = PH.decoder(3, 1)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 3 * 4 * 8 * cus + 77
    rng = np.random.default_rng(77)
    few = encode_blocks(dec, dec, rng.integers(0, 2, (256, 4, 4)).astype(np.uint8), False)
    sent = few[rng.integers(0, 256, B)]
    z = sent ^ (rng.random(sent.shape) < 0.12).astype(np.uint8)
    cut = 12345
    pick = np.concatenate([np.arange(40), np.arange(cut - 20, cut + 20), np.arange(B - 40, B)])
    want = PH.decode(dec, dec, z[pick], 5, False)
    assert len(set(want["last"].tolist())) >= 3 and (want["status"] != 0).any() and (want["status"] == 0).any()
    whole = pc.correct_hard_batch(torch.from_numpy(z).cuda(), 5)
    whole = {k: v.cpu().numpy() for k, v in whole.items()}
    same({k: v[pick] for k, v in whole.items()}, want, "whole")
    for lo, hi in ((0, cut), (cut, B)):
        part = pc.correct_hard_batch(torch.from_numpy(z[lo:hi]).cuda(), 5)
        same({k: v.cpu().numpy() for k, v in part.items()}, {k: v[lo:hi] for k, v in whole.items()}, lo)


def product_of_codes(r, c, extended, tag="bm"):
    return cc.product_code(handle(*r, tag=tag), handle(*c, tag=tag), extended=extended)


def whole_equals_model_and_parts_equal_whole(name):
    """a batch of tests/test_product_hard_host.py's TRIPS at this device's grid: the whole call against the model on the
    picked blocks, and the blocks before and from the odd cut, decoded on their own (as other workgroups' first, second
    or third block), against the whole"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    batch = trips_batch(name, cus)
    trips_batch_is_not_degenerate(name, batch)
    r, c = TRIPS[name][:2]
    pc = product_of_codes(r + (None,), c + (None,), False)
    z, pick, cut = batch["z"], batch["pick"], batch["cut"]
    assert z.shape[0] > 2 * batch["cap"] and z.shape[1:] == (pc.n2, pc.n1)
    zd = torch.from_numpy(z).cuda()
    whole = {k: v.cpu().numpy() for k, v in pc.correct_hard_batch(zd, TRIP_HALVES).items()}
    same({k: v[pick] for k, v in whole.items()}, batch["want"], (name, "whole"))
    for lo, hi in ((0, cut), (cut, z.shape[0])):
        part = pc.correct_hard_batch(zd[lo:hi], TRIP_HALVES)
        same({k: v.cpu().numpy() for k, v in part.items()}, {k: v[lo:hi] for k, v in whole.items()}, (name, lo))


@pytest.mark.parametrize("name", ["127_113x7_4", "7_4x127_113"])
def test_second_and_third_block_of_a_workgroup(name):
    """the workgroup-per-block kernel with twice as many blocks as its largest grid (8 workgroups per compute unit) and
    77 more: every workgroup decodes a second block, and 77 a third, over the X, X0, ctl, line states and
    Berlekamp-Massey columns of the one before.  7 x 127 leaves two of the four wavefronts without a line in either pass,
    three in the row pass, and the second one lane short in the column pass; 127 x 7 is its turn."""
    whole_equals_model_and_parts_equal_whole(name)


def test_second_and_third_block_of_a_wavefront_at_full_width():
    """the wavefront-per-block kernel at 63 lines of t = 3 with twice as many blocks as the largest grid has wavefronts
    and 77 more: 63 of 64 lanes have a line, the Berlekamp-Massey columns are six deep, and a wavefront meets all of it
    again from the block before"""
    whole_equals_model_and_parts_equal_whole("63_45x63_45")


@pytest.mark.parametrize("halves", LONG_HALVES)
def test_many_half_iterations(halves):
    """BCH(15,11)^2 through 56, 57 and 60 half-iterations: blocks in a cycle change up to the last pass (`last` ==
    halves, far above the 8 of the other tests), settled blocks stop early; separate buffers and in place"""
    dec, z, xs = long_case()
    want = long_outputs(halves)
    assert (want["last"] == halves).sum() >= 5 and (want["last"] <= 8).sum() >= 5
    pc = product_of_codes((4, 1, None), (4, 1, None), False)
    same(decode_dev(pc, z, halves), want, (halves, "separate"))
    same(decode_dev(pc, z, halves, in_place=True), want, (halves, "in place"))


@pytest.mark.parametrize("name", ["15_11x15_7", "e16_11xe32_26", "255_239x255_239"])
def test_in_place_and_outputs_left_out_one_at_a_time(name):
    z = case(name)[4]
    pc = product_of(name)
    for halves in (3, HALVES):
        want = model_outputs(name, halves)
        same(decode_dev(pc, z, halves, in_place=True), want, (name, halves, "in place"))
        for k in ("nflip", "last", "status"):
            same(decode_dev(pc, z, halves, leave_out=(k,)), want, (name, halves, k))
        same(decode_dev(pc, z, halves, leave_out=("nflip", "last", "status")), want, (name, halves, "none"))


@pytest.mark.parametrize("name", ["15_11x15_7", "s40_22x15_7", "127_113x15_11"])
def test_buffers_at_odd_offsets(name):
    import torch
    z = case(name)[4][:5]
    pc = product_of(name)
    B, N = z.shape[0], pc.n
    base = torch.zeros(B * N + 3, dtype=torch.uint8, device="cuda")
    zin = base[3:]
    zin.copy_(torch.from_numpy(np.array(z)).cuda().reshape(-1))
    for halves in (2, HALVES):
        wo, out = guarded(torch, B * N + 1, torch.uint8)
        small = {k: guarded(torch, B + 1, torch.int32) for k in ("nflip", "last", "status")}
        desc = pc._pc_hard(halves)
        rc = capi.lib().cc_product_decode_hard_dev(C.byref(desc), ptr(zin), ptr(out[1:]), ptr(small["nflip"][1][1:]),
                                                   ptr(small["last"][1][1:]), ptr(small["status"][1][1:]), B, None)
        capi.check(rc, "cc_product_decode_hard_dev")
        torch.cuda.synchronize()
        assert guards_intact(torch, wo) and all(guards_intact(torch, v[0]) for v in small.values())
        assert int(out[0]) == SENTINEL and all(int(v[1].view(torch.uint8)[0]) == SENTINEL for v in small.values())
        got = {k: v[1][1:].cpu().numpy() for k, v in small.items()}
        got["out"] = out[1:].cpu().numpy().reshape(z.shape)
        same(got, model_outputs(name, halves, slice(0, 5)), (name, halves))


@pytest.mark.parametrize("name", ["15_11x15_7", "s40_22x15_7", "e64_51xe64_51"])
def test_every_hard_tag_gives_the_same_bytes(name):
    z = case(name)[4]
    want = model_outputs(name, HALVES)
    for tag in TAGS:
        same(decode_dev(product_of(name, tag), z, HALVES), want, (name, tag))


@pytest.mark.parametrize("name", ["15_11x15_7", "e16_11xe32_26", "e256_239xe8_4", "255_239x255_239"])
def test_a_zero_block_and_a_code_block_are_left_alone(name):
    sent = case(name)[3]
    z = np.stack([np.zeros_like(sent[0]), sent[0], sent[1]])
    for halves in (1, 2, HALVES):
        got = decode_dev(product_of(name), z, halves)
        assert np.array_equal(got["out"], z)
        for k in ("nflip", "last", "status"):
            assert not got[k].any(), (name, halves, k)


def test_python_calls_on_both_sides_and_an_empty_batch():
    import torch
    name = "e16_11xe32_26"
    rows, cols, extended, sent, z, xs, _ = case(name)
    pc = product_of(name)
    want = model_outputs(name, 6)
    dev = pc.correct_hard_batch(torch.from_numpy(np.array(z)).cuda(), 6)
    host = pc.correct_hard_batch(z, 6)
    assert list(dev) == list(host) == ["out", "nflip", "last", "status"]
    same({k: v.cpu().numpy() for k, v in dev.items()}, want, "device")
    same(host, want, "host")
    dec = pc.decode_hard_batch(z, 6)
    assert list(dec) == ["out", "nflip", "last", "status", "msg"] and dec["msg"].shape == (z.shape[0], pc.k2, pc.k1)
    assert np.array_equal(dec["msg"], pc.extract_batch(want["out"]))
    # a value that is no bit: the host form refuses it, as cc_correct_hard_batch does
    bad = z.copy()
    bad[3, 2, 1] = 2
    with pytest.raises(cc.CcError) as e:
        pc.correct_hard_batch(bad, 6)
    assert e.value.status == capi.ERR_NOT_IN_FIELD
    desc = pc._pc_hard(3)
    assert capi.lib().cc_product_decode_hard_dev(C.byref(desc), None, None, None, None, None, 0, None) == capi.OK
    assert capi.lib().cc_product_decode_hard(C.byref(desc), None, None, None, None, None, 0) == capi.OK
    counters = torch.zeros(capi.MC_NCOUNTERS, dtype=torch.int64, device="cuda")
    assert capi.lib().cc_mc_run_product_hard_dev(C.byref(desc), 3.0, 1, 0, 0, 1, ptr(counters), None) == capi.OK
    assert not counters.any()


def test_handles_on_different_devices_are_refused():
    """refusal 4 of the header needs a handle with a device: after what the Chase call refuses for either handle, before
    the overlap"""
    import torch
    on = handle(4, 1)
    off = cc.primitive_bch(4, cc.errors(1), cc.berlekamp_massey_tag(), device=capi.DEVICE_NONE)
    z = torch.zeros((2, 15, 15), dtype=torch.uint8, device="cuda")
    for rows, cols in ((on, off), (off, on)):
        pc = cc.product_code(rows, cols)
        with pytest.raises(cc.CcError) as e:
            pc.correct_hard_batch(z, 2)
        assert e.value.status == capi.ERR_INVALID_ARGUMENT
    with pytest.raises(cc.CcError) as e:
        cc.product_code(on, cc.rs(4, cc.errors(2), cc.berlekamp_massey_tag(), device=capi.DEVICE_NONE)).correct_hard_batch(z, 2)
    assert e.value.status == capi.ERR_UNSUPPORTED


def run_child(script, env, marker):
    here = os.path.dirname(os.path.abspath(__file__))
    head = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n" % (here, os.path.dirname(here))
    out = subprocess.run([sys.executable, "-c", head + script], env=dict(os.environ, **env), capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0 and marker in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_host_pointers_equal_device_pointers_in_small_staging_chunks():
    """the staging chunk forced small in a process of its own (the value is read once): 70 blocks of 63 x 63 in chunks
    of 16 and 300 of 16 x 32, pageable and page-locked memory, separate buffers and in place"""
    run_child(
        "import ctypes as C\n"
        "import numpy as np, torch\n"
        "import channelcoding_amd as cc\n"
        "from channelcoding_amd import capi\n"
        "rng = np.random.default_rng(8)\n"
        "mk = lambda q, t: cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag())\n"
        "vp = lambda a: a.ctypes.data_as(C.c_void_p)\n"
        "for pc, B, p in ((cc.product_code(mk(6, 3), mk(6, 3)), 70, 0.04), (cc.product_code(mk(4, 1), mk(5, 1), extended=True), 300, 0.04)):\n"
        "    sent = pc.encode_batch(rng.integers(0, 2, (B, pc.k2, pc.k1)).astype(np.uint8))\n"
        "    z = sent ^ (rng.random(sent.shape) < p).astype(np.uint8)\n"
        "    pinned = torch.from_numpy(z.copy()).pin_memory().numpy()\n"
        "    for halves in (1, 6):\n"
        "        dev = {k: v.cpu().numpy() for k, v in pc.correct_hard_batch(torch.from_numpy(z.copy()).cuda(), halves).items()}\n"
        "        assert dev['nflip'].any() and (halves == 1 or len(set(dev['last'].tolist())) > 1)\n"
        "        for src in (z, pinned):\n"
        "            host = pc.correct_hard_batch(src, halves)\n"
        "            for k in dev:\n"
        "                assert host[k].dtype == dev[k].dtype and np.array_equal(host[k], dev[k]), (halves, k)\n"
        "        buf = z.copy()\n"
        "        desc = pc._pc_hard(halves)\n"
        "        last = np.zeros(B, np.int32)\n"
        "        rc = capi.lib().cc_product_decode_hard(C.byref(desc), vp(buf), vp(buf), None, vp(last), None, B)\n"
        "        assert rc == 0 and np.array_equal(buf, dev['out']) and np.array_equal(last, dev['last'])\n"
        "print('PRODUCT HARD HOST OK')\n", {"CC_AMD_HOST_CHUNK_BYTES": str(16 * 63 * 63)}, "PRODUCT HARD HOST OK")


# ---- Monte-Carlo ----
def counted(res, sent, y):
    """the counters of the blocks given, by the definitions of the header"""
    B = sent.shape[0]
    wrong = (res["out"] != sent).reshape(B, -1).sum(axis=1)
    failed = res["status"] != PH.FRAME_OK
    c = np.zeros(capi.MC_NCOUNTERS, np.int64)
    c[capi.MC_FRAMES] = B
    c[capi.MC_WORD_ERRORS] = int((failed | (wrong > 0)).sum())
    c[capi.MC_BIT_ERRORS] = int(wrong.sum())
    c[capi.MC_FAILURES] = int(failed.sum())
    c[capi.MC_UNDETECTED] = int((~failed & (wrong > 0)).sum())
    c[capi.MC_CHANNEL_BIT_ERRORS] = int(((y < 0) != (sent != 0)).sum())
    c[capi.MC_ITER_SUM] = int(res["last"].sum())
    for v in res["last"]:
        c[capi.MC_ITER_HIST + min(int(v), 55)] += 1
    return c


def mc(pc, halves, ebno, seed, first, blocks, random_codewords=True):
    return ProductHardBackend(pc, halves, random_codewords).run(ebno, seed, first, blocks).cpu().numpy()


@pytest.mark.parametrize("q,t,extended,ebno,blocks", [(4, 1, False, 4.5, 512), (5, 1, True, 4.0, 128)],
                         ids=["15_11x15_11", "e32_26xe32_26"])
@pytest.mark.parametrize("random_codewords", [True, False], ids=["random", "zero"])
def test_mc_counters_against_channel_model_and_count(q, t, extended, ebno, blocks, random_codewords):
    pc = product_of_codes((q, t, None), (q, t, None), extended)
    dec = PH.decoder(q, t)
    seed, first = 2026, (1 << 33) + 5
    ch = pc.channel(ebno, seed, first, blocks, random_codewords)
    y, sent = ch["y"].cpu().numpy(), ch["sent"].cpu().numpy()
    assert bool(sent.any()) == random_codewords
    z = (y < 0).astype(np.uint8)
    xs = PH.steps(dec, dec, z, 6, extended)
    for halves in (6, 3):
        want = PH.outputs(dec, dec, z, xs, halves, extended)
        expect = counted(want, sent, y)
        got = mc(pc, halves, ebno, seed, first, blocks, random_codewords)
        assert np.array_equal(got, expect), (halves, got, expect)
        assert expect[capi.MC_WORD_ERRORS] > 0 and expect[capi.MC_ITER_SUM] > 0
        assert np.count_nonzero(expect[capi.MC_ITER_HIST:]) >= (3 if halves == 6 else 2) and expect[capi.MC_ITER_HIST:].sum() == blocks
    assert expect[capi.MC_FAILURES] > 0
    cut = blocks // 3
    shards = mc(pc, 6, ebno, seed, first, cut, random_codewords) + mc(pc, 6, ebno, seed, first + cut, blocks - cut, random_codewords)
    assert np.array_equal(shards, mc(pc, 6, ebno, seed, first, blocks, random_codewords))


def mc_between_guards(pc, halves, ebno, seed, first, blocks, random_codewords):
    """cc_mc_run_product_hard_dev itself, the 64 counters between guard elements: a histogram slot past the last would
    land in them"""
    import torch
    wc, counters = guarded(torch, capi.MC_NCOUNTERS, torch.int64)
    counters.zero_()
    desc = pc._pc_hard(halves)
    rc = capi.lib().cc_mc_run_product_hard_dev(C.byref(desc), ebno, seed, first, blocks, int(random_codewords), ptr(counters), None)
    capi.check(rc, "cc_mc_run_product_hard_dev")
    torch.cuda.synchronize()
    assert guards_intact(torch, wc)
    return counters.cpu().numpy()


@pytest.mark.parametrize("random_codewords", [True, False], ids=["random", "zero"])
def test_mc_counters_at_and_beyond_the_last_histogram_slot(random_codewords):
    """BCH(15,11)^2 at an Eb/N0 where a fifth of the blocks end in a cycle (chosen with the model on awgn_model's channel
    values): after 60 half-iterations those blocks have `last` = 60 and share the last slot, 55, of the histogram with
    nothing else, while CC_MC_ITER_SUM takes the 60; after 55 the same blocks have `last` = 55, the slot's own value.
    The counters lie between guard elements."""
    pc = product_of_codes((4, 1, None), (4, 1, None), False)
    dec = PH.decoder(4, 1)
    seed, first, ebno, blocks = 2026, (1 << 33) + 5, 3.5, 512
    ch = pc.channel(ebno, seed, first, blocks, random_codewords)
    y, sent = ch["y"].cpu().numpy(), ch["sent"].cpu().numpy()
    assert bool(sent.any()) == random_codewords
    z = (y < 0).astype(np.uint8)
    xs = PH.steps(dec, dec, z, 60, False)
    top = capi.MC_ITER_HIST + 55
    assert top + 1 == capi.MC_NCOUNTERS
    for halves in (60, 55):
        want = PH.outputs(dec, dec, z, xs, halves, False)
        expect = counted(want, sent, y)
        print(halves, "half-iterations: blocks in the last slot", expect[top], "sum of last", expect[capi.MC_ITER_SUM])
        assert (want["last"] == halves).sum() >= 5 and expect[top] == (want["last"] >= 55).sum() > 0
        assert expect[capi.MC_ITER_HIST: top + 1].sum() == blocks and np.count_nonzero(expect[capi.MC_ITER_HIST:]) >= 3
        if halves > 55:
            assert expect[capi.MC_ITER_SUM] > 55 * expect[top]  # the sum is not clamped
        got = mc_between_guards(pc, halves, ebno, seed, first, blocks, random_codewords)
        assert np.array_equal(got, expect), (halves, got, expect)
        assert np.array_equal(mc(pc, halves, ebno, seed, first, blocks, random_codewords), expect)


@pytest.mark.parametrize("random_codewords", [True, False], ids=["random", "zero"])
def test_mc_count_of_several_blocks_per_wavefront(random_codewords):
    """BCH(7,4)^2 with three times as many blocks as the count kernel's largest grid has wavefronts (8 workgroups of four
    per compute unit) and 77 more, one chunk: every wavefront sums three or four blocks in registers before its atomics.
    Want = the composition on the device (the decode call is held to the model by the tests above): channel, hard
    decisions, the decode call, the counter definitions.  Three shards of unequal size sum to the whole."""
    import torch
    pc = product_of_codes((3, 1, None), (3, 1, None), False)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    blocks = 3 * 32 * cus + 77
    assert blocks * pc.n < 1 << 24  # one chunk
    seed, first, ebno, halves = 2028, (1 << 33) + 5, 3.0, 5
    ch = pc.channel(ebno, seed, first, blocks, random_codewords)
    assert bool(ch["sent"].any()) == random_codewords
    res = pc.correct_hard_batch((ch["y"] < 0).to(torch.uint8), halves)
    wrong = (res["out"] != ch["sent"]).reshape(blocks, -1).sum(dim=1)
    failed = res["status"] != 0
    want = np.zeros(capi.MC_NCOUNTERS, np.int64)
    want[capi.MC_FRAMES] = blocks
    want[capi.MC_WORD_ERRORS] = int((failed | (wrong > 0)).sum())
    want[capi.MC_BIT_ERRORS] = int(wrong.sum())
    want[capi.MC_FAILURES] = int(failed.sum())
    want[capi.MC_UNDETECTED] = int((~failed & (wrong > 0)).sum())
    want[capi.MC_CHANNEL_BIT_ERRORS] = int(((ch["y"] < 0) != (ch["sent"] != 0)).sum())
    want[capi.MC_ITER_SUM] = int(res["last"].sum())
    want[capi.MC_ITER_HIST:] = torch.bincount(res["last"].clamp(max=55).long(), minlength=56).cpu().numpy()
    print("counters", want[:7], "histogram", want[capi.MC_ITER_HIST: capi.MC_ITER_HIST + halves + 1])
    assert want[capi.MC_WORD_ERRORS] > 0 and want[capi.MC_FAILURES] > 0 and want[capi.MC_UNDETECTED] > 0
    assert np.count_nonzero(want[capi.MC_ITER_HIST:]) >= 3 and want[capi.MC_ITER_HIST:].sum() == blocks
    got = mc_between_guards(pc, halves, ebno, seed, first, blocks, random_codewords)
    assert np.array_equal(got, want), (got, want)
    a, b = blocks // 5, blocks // 2 + 1
    shards = sum(mc(pc, halves, ebno, seed, first + lo, hi - lo, random_codewords) for lo, hi in ((0, a), (a, b), (b, blocks)))
    assert np.array_equal(shards, want)


def test_mc_across_a_chunk_boundary_equals_the_composition():
    """chunks of 100 blocks (the value is read once, so in a process of its own): 512 blocks cross five boundaries"""
    run_child(
        "import numpy as np, torch\n"
        "import channelcoding_amd as cc\n"
        "from channelcoding_amd import capi\n"
        "from channelcoding_amd.montecarlo import ProductHardBackend\n"
        "mk = lambda q, t: cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag())\n"
        "pc = cc.product_code(mk(5, 3), mk(5, 3))\n"
        "for rc in (True, False):\n"
        "    got = ProductHardBackend(pc, 5, rc).run(5.0, 31, 7, 512).cpu().numpy()\n"
        "    ch = pc.channel(5.0, 31, 7, 512, rc)\n"
        "    res = pc.correct_hard_batch((ch['y'] < 0).to(torch.uint8), 5)\n"
        "    wrong = (res['out'] != ch['sent']).reshape(512, -1).sum(dim=1)\n"
        "    failed = res['status'] != 0\n"
        "    want = np.zeros(capi.MC_NCOUNTERS, np.int64)\n"
        "    want[capi.MC_FRAMES] = 512\n"
        "    want[capi.MC_WORD_ERRORS] = int((failed | (wrong > 0)).sum())\n"
        "    want[capi.MC_BIT_ERRORS] = int(wrong.sum())\n"
        "    want[capi.MC_FAILURES] = int(failed.sum())\n"
        "    want[capi.MC_UNDETECTED] = int((~failed & (wrong > 0)).sum())\n"
        "    want[capi.MC_CHANNEL_BIT_ERRORS] = int(((ch['y'] < 0) != (ch['sent'] != 0)).sum())\n"
        "    want[capi.MC_ITER_SUM] = int(res['last'].sum())\n"
        "    for v in res['last'].cpu().tolist():\n"
        "        want[capi.MC_ITER_HIST + min(v, 55)] += 1\n"
        "    assert np.array_equal(got, want), (got, want)\n"
        "    assert want[capi.MC_WORD_ERRORS] > 0 and want[capi.MC_FAILURES] > 0 and want[capi.MC_ITER_SUM] > 0\n"
        "print('PRODUCT HARD MC OK')\n", {"CC_AMD_PRODUCT_MC_CHUNK_VALUES": str(100 * 961)}, "PRODUCT HARD MC OK")
