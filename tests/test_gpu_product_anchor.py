"""GPU tests of anchor decoding of product codes (cc_product_decode_anchor): the device byte for byte and int
for int against tests/product_anchor_model.py under guarded_buffers.check_call -- guard elements around every output,
every buffer at its least alignment, each optional output absent in turn, two poisons around the input -- at delta = 1,
2, 3 and 2^31 after 1, 2, 3, 8 and 16 half-iterations; in place; zero and code blocks; host against device pointers in
small staging chunks; the Monte-Carlo counters against channel + model + count, sharded and chunked.

The batches are those of tests/test_product_hard_host.py (CASES there; tests/test_gpu_product_hard.py says what each shape
is there for, tests/test_product_anchor_host.py what they hold for this decoder): 15 x 15 with t = 1 against t = 2 at B =
1, 2 and 67; 16 x 32 extended over two fields; 40 x 15 shortened; 63 x 63 and 64 x 64, the last one-wavefront shape; 127
x 15, 256 x 8 and 8 x 256; 255 x 255 and 256 x 256; 2t = 32 against 15 lines and against 255, which asks for the LDS
attribute.  Past the first block of a workgroup: the TRIPS shapes there with 2 * 8 * CUs + 77 blocks, the first trip made
of blocks that backtrack, so that a second and a third block meet the flags, counters and records of the one before.  56
and 57 half-iterations on BCH(15,11)^2: the early stop against the model's full run."""
import ctypes as C

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import capi
from channelcoding_amd.montecarlo import ProductAnchorBackend
import product_anchor_model as PA
import product_hard_model as PH
from guarded_buffers import check_call
from test_gpu_product_hard import counted, product_of, product_of_codes, run_child
from test_product_anchor_host import (DELTAS, HALVES, LONG_DELTA, LONG_HALVES, SMALL, TRIP_DELTA, TRIP_HALVES, long_case,
                                      model_outputs, trips_batch, trips_batch_is_not_degenerate)
from test_product_hard_host import CASES, TRIPS, case

pytestmark = pytest.mark.gpu


def decode_dev(pc, z, delta, halves, want, optional=(), in_place=False, what=""):
    """cc_product_decode_anchor_dev itself on the host array z (B, n2, n1) under the buffer contract; want: the model's
    outputs"""
    desc = pc._pc_hard(halves)
    B = z.shape[0]

    def call(p):
        return capi.lib().cc_product_decode_anchor_dev(C.byref(desc), delta, p["in"], p["out"], p["nflip"], p["last"], p["status"],
                                                       p["nback"], p["nconf"], B, p["stream"])

    outputs = {"out": (np.uint8, z.size)}
    outputs.update({k: (np.int32, B) for k in SMALL})
    expected = {k: want[k] for k in outputs}
    return check_call(call, {"in": np.ascontiguousarray(z).reshape(-1)}, outputs, expected, optional=optional,
                      in_place={"out": "in"} if in_place else None, what=str((what, delta, halves)))


@pytest.mark.parametrize("delta", DELTAS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_model(name, delta):
    """every setting with all outputs under both poisons; each optional output absent in turn after 3 and 8
    half-iterations"""
    z = case(name)[4]
    pc = product_of(name)
    for halves in HALVES:
        decode_dev(pc, z, delta, halves, model_outputs(name, delta, halves), optional=SMALL if halves in (3, 8) and delta == 2 else (),
                   what=name)


@pytest.mark.parametrize("B", [1, 2])
def test_one_and_two_blocks(B):
    for name in ("15_11x15_7", "e64_51xe64_51", "127_113x15_11"):
        z = case(name)[4][:B]
        for delta in (1, 2):
            for halves in (2, 8):
                decode_dev(product_of(name), z, delta, halves, model_outputs(name, delta, halves, slice(0, B)), what=(name, B))


def same(got, want, what):
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)


def whole_equals_model_and_parts_equal_whole(name):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    batch = trips_batch(name, cus)
    trips_batch_is_not_degenerate(name, batch)
    r, c = TRIPS[name][:2]
    pc = product_of_codes(r + (None,), c + (None,), False)
    z, pick, cut = batch["z"], batch["pick"], batch["cut"]
    assert z.shape[0] > 2 * batch["cap"] and z.shape[1:] == (pc.n2, pc.n1)
    zd = torch.from_numpy(z).cuda()
    whole = {k: v.cpu().numpy() for k, v in pc.correct_anchor_batch(zd, TRIP_DELTA, TRIP_HALVES).items()}
    same({k: v[pick] for k, v in whole.items()}, batch["want"], (name, "whole"))
    for lo, hi in ((0, cut), (cut, z.shape[0])):
        part = pc.correct_anchor_batch(zd[lo:hi], TRIP_DELTA, TRIP_HALVES)
        same({k: v.cpu().numpy() for k, v in part.items()}, {k: v[lo:hi] for k, v in whole.items()}, (name, lo))


@pytest.mark.parametrize("name", sorted(TRIPS))
def test_second_and_third_block_over_the_state_of_the_one_before(name):
    """twice as many blocks as the largest grid holds and 77 more: every workgroup (wavefront) decodes a second block, and
    77 a third, in the LDS of a block that left anchor flags, hold flags, records and counts behind.  The whole call
    against the model on the picked blocks; the blocks before and from an odd cut, decoded on their own as other
    workgroups' first, second or third block, against the whole."""
    whole_equals_model_and_parts_equal_whole(name)


@pytest.mark.parametrize("halves", LONG_HALVES)
def test_many_half_iterations_and_the_early_stop(halves):
    """the device's early stop against the model, which runs every pass: blocks where two passes change no bit and a
    later one does (tests/test_product_anchor_host.py asserts that the batch has them), ending on a row and on a column
    pass; separate buffers and in place"""
    dec, z, run, _ = long_case()
    want = PA.outputs(dec, dec, z, run, halves, False)
    pc = product_of_codes((4, 1, None), (4, 1, None), False)
    decode_dev(pc, z, LONG_DELTA, halves, want, what="long")
    decode_dev(pc, z, LONG_DELTA, halves, want, in_place=True, what="long in place")


@pytest.mark.parametrize("name", ["15_11x15_7", "e16_11xe32_26", "255_239x255_239"])
def test_in_place(name):
    z = case(name)[4]
    for delta, halves in ((1, 3), (2, 8), (3, 16)):
        decode_dev(product_of(name), z, delta, halves, model_outputs(name, delta, halves), in_place=True, what=(name, "in place"))


@pytest.mark.parametrize("name", ["15_11x15_7", "e16_11xe32_26", "e256_239xe8_4", "255_239x255_239"])
def test_a_zero_block_and_a_code_block_are_left_alone(name):
    sent = case(name)[3]
    z = np.stack([np.zeros_like(sent[0]), sent[0], sent[1]])
    want = dict(out=z, **{k: np.zeros(3, np.int32) for k in SMALL})
    for halves in (1, 2, 8):
        decode_dev(product_of(name), z, 1, halves, want, what=(name, "code blocks"))


def test_python_calls_on_both_sides_and_an_empty_batch():
    import torch
    name = "e16_11xe32_26"
    z = case(name)[4]
    pc = product_of(name)
    want = model_outputs(name, 2, 6)
    dev = pc.correct_anchor_batch(torch.from_numpy(np.array(z)).cuda(), 2, 6)
    host = pc.correct_anchor_batch(z, 2, 6)
    assert list(dev) == list(host) == ["out"] + list(SMALL)
    same({k: v.cpu().numpy() for k, v in dev.items()}, want, "device")
    same(host, want, "host")
    dec = pc.decode_anchor_batch(z, 2, 6)
    assert list(dec) == ["out"] + list(SMALL) + ["msg"] and np.array_equal(dec["msg"], pc.extract_batch(want["out"]))
    bad = z.copy()
    bad[3, 2, 1] = 2
    with pytest.raises(cc.CcError) as e:
        pc.correct_anchor_batch(bad, 2, 6)
    assert e.value.status == capi.ERR_NOT_IN_FIELD
    desc = pc._pc_hard(3)
    lib = capi.lib()
    assert lib.cc_product_decode_anchor_dev(C.byref(desc), 2, None, None, None, None, None, None, None, 0, None) == capi.OK
    assert lib.cc_product_decode_anchor(C.byref(desc), 2, None, None, None, None, None, None, None, 0) == capi.OK
    counters = torch.zeros(capi.MC_NCOUNTERS, dtype=torch.int64, device="cuda")
    assert lib.cc_mc_run_product_anchor_dev(C.byref(desc), 2, 3.0, 1, 0, 0, 1, C.c_void_p(counters.data_ptr()), None) == capi.OK
    assert not counters.any()


def test_host_pointers_equal_device_pointers_in_small_staging_chunks():
    """the staging chunk forced small in a process of its own (the value is read once): 70 blocks of 63 x 63 in chunks of
    16 and 300 of 16 x 32, pageable and page-locked memory, all outputs, some absent, and in place"""
    run_child(
        "import ctypes as C\n"
        "import numpy as np, torch\n"
        "import channelcoding_amd as cc\n"
        "from channelcoding_amd import capi\n"
        "rng = np.random.default_rng(8)\n"
        "mk = lambda q, t: cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag())\n"
        "vp = lambda a: a.ctypes.data_as(C.c_void_p)\n"
        "for pc, B, p in ((cc.product_code(mk(6, 3), mk(6, 3)), 70, 0.045), (cc.product_code(mk(4, 1), mk(5, 1), extended=True), 300, 0.05)):\n"
        "    sent = pc.encode_batch(rng.integers(0, 2, (B, pc.k2, pc.k1)).astype(np.uint8))\n"
        "    z = sent ^ (rng.random(sent.shape) < p).astype(np.uint8)\n"
        "    pinned = torch.from_numpy(z.copy()).pin_memory().numpy()\n"
        "    for delta, halves in ((1, 1), (1, 6), (2, 6)):\n"
        "        dev = {k: v.cpu().numpy() for k, v in pc.correct_anchor_batch(torch.from_numpy(z.copy()).cuda(), delta, halves).items()}\n"
        "        assert dev['nflip'].any() and (halves == 1 or (dev['nconf'].any() and len(set(dev['last'].tolist())) > 1))\n"
        "        for src in (z, pinned):\n"
        "            host = pc.correct_anchor_batch(src, delta, halves)\n"
        "            for k in dev:\n"
        "                assert host[k].dtype == dev[k].dtype and np.array_equal(host[k], dev[k]), (halves, k)\n"
        "        buf = z.copy()\n"
        "        desc = pc._pc_hard(halves)\n"
        "        last, nconf = np.zeros(B, np.int32), np.zeros(B, np.int32)\n"
        "        rc = capi.lib().cc_product_decode_anchor(C.byref(desc), delta, vp(buf), vp(buf), None, vp(last), None, None, vp(nconf), B)\n"
        "        assert rc == 0 and np.array_equal(buf, dev['out']) and np.array_equal(last, dev['last'])\n"
        "        assert np.array_equal(nconf, dev['nconf'])\n"
        "    assert dev['nback'].any()\n"
        "print('PRODUCT ANCHOR HOST OK')\n", {"CC_AMD_HOST_CHUNK_BYTES": str(16 * 63 * 63)}, "PRODUCT ANCHOR HOST OK")


# ---- Monte-Carlo ----
def mc(pc, delta, halves, ebno, seed, first, blocks, random_codewords=True):
    return ProductAnchorBackend(pc, delta, halves, random_codewords).run(ebno, seed, first, blocks).cpu().numpy()


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
    for delta in (1, 2):
        run = PA.steps(dec, dec, z, 6, delta, extended)
        for halves in (6, 3):
            want = PA.outputs(dec, dec, z, run, halves, extended)
            expect = counted(want, sent, y)
            got = mc(pc, delta, halves, ebno, seed, first, blocks, random_codewords)
            assert np.array_equal(got, expect), (delta, halves, got, expect)
            assert expect[capi.MC_WORD_ERRORS] > 0 and expect[capi.MC_ITER_SUM] > 0 and want["nconf"].any()
            assert expect[capi.MC_ITER_HIST:].sum() == blocks
        assert want["nback"].any() or delta > 1
        cut = blocks // 3
        shards = mc(pc, delta, 6, ebno, seed, first, cut, random_codewords) \
            + mc(pc, delta, 6, ebno, seed, first + cut, blocks - cut, random_codewords)
        assert np.array_equal(shards, mc(pc, delta, 6, ebno, seed, first, blocks, random_codewords))


def test_mc_across_a_chunk_boundary_equals_the_composition():
    """chunks of 100 blocks (the value is read once, so in a process of its own): 512 blocks cross five boundaries"""
    run_child(
        "import numpy as np, torch\n"
        "import channelcoding_amd as cc\n"
        "from channelcoding_amd import capi\n"
        "from channelcoding_amd.montecarlo import ProductAnchorBackend\n"
        "mk = lambda q, t: cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag())\n"
        "pc = cc.product_code(mk(5, 3), mk(5, 3))\n"
        "for rc in (True, False):\n"
        "    got = ProductAnchorBackend(pc, 2, 5, rc).run(5.0, 31, 7, 512).cpu().numpy()\n"
        "    ch = pc.channel(5.0, 31, 7, 512, rc)\n"
        "    res = pc.correct_anchor_batch((ch['y'] < 0).to(torch.uint8), 2, 5)\n"
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
        "    assert want[capi.MC_WORD_ERRORS] > 0 and want[capi.MC_FAILURES] > 0 and res['nconf'].any()\n"
        "print('PRODUCT ANCHOR MC OK')\n", {"CC_AMD_PRODUCT_MC_CHUNK_VALUES": str(100 * 961)}, "PRODUCT ANCHOR MC OK")
